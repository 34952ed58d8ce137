// mesh_expose.hip -- which triangles an outside view can see (csrc/pvd_hip_mesh_expose.h): an any-hit query from S points of every
// triangle along D directions, over the workspace pvd_mesh_ray_build leaves (csrc/mesh_ray.hip, csrc/mesh_tri_grid.h) and with the
// walk and the watertight test of csrc/mesh_ray_walk.h, which the first-hit cast uses too.
//
// k_mx_expose    one wave per triangle, kWaves triangles per workgroup; lanes are directions, 64 at a time, in a loop over the points
//                and the chunks of directions.  The sample point and the side test are in unfused float64; a lane walks until its
//                first hit or out of the grid, then the outside list.  The four counts are ballots and population counts: no LDS; one
//                integer atomicAdd per wave and nonzero total.  The rays exist in registers only.
// All lanes of a wave start in the same cell (the triangle's own), so the first cells' records are the same addresses across the wave;
// the walks diverge from there.  What bounds it: the latency of the dependent loads start[c] -> list[s] -> packed[j] of a lane that
// steps from cell to cell, and the float64 rate of the test (about 40 float64 operations per record).
#include "block_scan.h"
#include "mesh_ray_walk.h"

#include "pvd_hip_mesh_expose.h"

namespace {

using namespace pvd;
using namespace pvd::tgrid;
using namespace pvd::mray;

struct AnyHit {  // the walk's visitor: is some valid triangle other than `self` hit with 0 <= t < +inf
    Ray r;
    int32_t self;
    bool hit;

    PVD_HD void test(const float4 *__restrict__ packed, uint32_t j) {
#pragma clang fp contract(off)
        const float4 q0 = packed[3 * (size_t)j], q1 = packed[3 * (size_t)j + 1], q2 = packed[3 * (size_t)j + 2];
        const int32_t idx = (int32_t)f2u(q2.y);
        if (idx < 0 || idx == self) return;  // an invalid triangle; the ray's own one, by index
        Crossing x;
        if (!crossing(q0, q1, q2, r, x)) return;
        if (x.t >= 0.0 && x.t < (double)INFINITY) hit = true;  // false for NaN
    }
    PVD_HD bool found() const { return hit; }
    PVD_HD bool settled(double) const { return hit; }
};

constexpr double kThird = 1.0 / 3.0, kTwoThirds = 2.0 / 3.0, kSixth = 1.0 / 6.0;

__global__ __launch_bounds__(kThreads) void k_mx_expose(const float *__restrict__ dirs, uint32_t D, uint32_t S, uint32_t tri0, uint32_t tri1,
                                                       uint32_t T, uint32_t G, uint32_t pairs, const uint32_t *__restrict__ header,
                                                       const uint32_t *__restrict__ start, const uint32_t *__restrict__ list,
                                                       const uint32_t *__restrict__ outside, const float4 *__restrict__ packed,
                                                       int32_t *__restrict__ counts, unsigned long long *__restrict__ totals) {
#pragma clang fp contract(off)
    const uint32_t lane = threadIdx.x & (kWave - 1), row = blockIdx.x * kWaves + threadIdx.x / kWave;
    if (row >= tri1 - tri0) return;  // the whole wave
    const uint32_t f = tri0 + row;   // < tri1 <= T
    const float4 q0 = packed[3 * (size_t)f], q1 = packed[3 * (size_t)f + 1], q2 = packed[3 * (size_t)f + 2];
    const bool valid = (int32_t)f2u(q2.y) >= 0;
    uint32_t front_cast = 0, front_esc = 0, back_cast = 0, back_esc = 0;
    if (valid) {
        const double a[3] = {(double)q0.x, (double)q0.y, (double)q0.z}, b[3] = {(double)q0.w, (double)q1.x, (double)q1.y};
        const double c[3] = {(double)q1.z, (double)q1.w, (double)q2.x};
        const double e[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, g[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
        const double n[3] = {e[1] * g[2] - e[2] * g[1], e[2] * g[0] - e[0] * g[2], e[0] * g[1] - e[1] * g[0]};
        for (uint32_t p = 0; p < S; ++p) {
            const double wa = p == 0 ? kThird : (p == 1 ? kTwoThirds : kSixth), wb = p == 0 ? kThird : (p == 2 ? kTwoThirds : kSixth);
            const double wc = p == 0 ? kThird : (p == 3 ? kTwoThirds : kSixth);
            float of[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) of[k] = (float)((wa * a[k] + wb * b[k]) + wc * c[k]);
            const bool point_ok = finite3(of[0], of[1], of[2]);
            const double o[3] = {(double)of[0], (double)of[1], (double)of[2]};
            for (uint32_t base = 0; base < D; base += kWave) {  // the trip count is the wave's: the ballots below see every lane
                const uint32_t i = base + lane;
                bool cast = false, front = false, escaped = false;
                if (point_ok && i < D) {
                    const float dx = dirs[3 * (size_t)i], dy = dirs[3 * (size_t)i + 1], dz = dirs[3 * (size_t)i + 2];
                    if (finite3(dx, dy, dz) && !(dx == 0.0f && dy == 0.0f && dz == 0.0f)) {
                        const double d[3] = {(double)dx, (double)dy, (double)dz};
                        const double s = (n[0] * d[0] + n[1] * d[1]) + n[2] * d[2];
                        if (s > 0.0 || s < 0.0) {  // false for NaN
                            cast = true;
                            front = s > 0.0;
                            AnyHit vis;
                            vis.r = ray_of(o, d);
                            vis.self = (int32_t)f;
                            vis.hit = false;
                            walk(o, d, T, G, header, start, list, outside, packed, pairs, 0.0, (double)INFINITY, vis);
                            escaped = !vis.hit;
                        }
                    }
                }
                front_cast += (uint32_t)__popcll(__ballot(cast && front));
                front_esc += (uint32_t)__popcll(__ballot(cast && front && escaped));
                back_cast += (uint32_t)__popcll(__ballot(cast && !front));
                back_esc += (uint32_t)__popcll(__ballot(cast && !front && escaped));
            }
        }
    }
    if (lane == 0) {
        int32_t *out = counts + 4 * (size_t)row;
        out[0] = (int32_t)front_cast;
        out[1] = (int32_t)front_esc;
        out[2] = (int32_t)back_cast;
        out[3] = (int32_t)back_esc;
        if (valid) {
            if (front_cast + back_cast) atomicAdd(&totals[0], (unsigned long long)(front_cast + back_cast));
            if (front_esc + back_esc) atomicAdd(&totals[1], (unsigned long long)(front_esc + back_esc));
            if (front_esc) atomicAdd(&totals[2], 1ull);
            if (back_esc) atomicAdd(&totals[3], 1ull);
            if (!(front_esc + back_esc)) atomicAdd(&totals[4], 1ull);
        }
    }
}

}  // namespace

extern "C" {

int pvd_mesh_expose(const float *dirs, uint32_t D, uint32_t S, uint32_t tri0, uint32_t tri1, uint32_t T, uint32_t G, uint64_t pairs,
                    const void *workspace, size_t workspace_bytes, int32_t *counts, uint64_t *totals, pvd_stream_t stream) {
    if (D < 1 || D > PVD_MESH_EXPOSE_MAX_D || (S != 1 && S != 4)) return PVD_ERR_UNSUPPORTED;
    const int rc = check_args<3>(T, G, pairs, workspace, workspace_bytes);
    if (rc != PVD_OK) return rc;
    if (!(tri0 <= tri1 && tri1 <= T)) return PVD_ERR_INVALID;
    if (tri0 == tri1) return PVD_OK;
    if (!dirs || !counts || !totals) return PVD_ERR_INVALID;
    const Layout l = layout<3>(T, G, pairs);
    const char *ws = (const char *)workspace;
    hipLaunchKernelGGL(k_mx_expose, dim3(div_up(tri1 - tri0, kWaves)), dim3(kThreads), 0, (hipStream_t)stream, dirs, D, S, tri0, tri1, T, G,
                       (uint32_t)pairs, (const uint32_t *)ws, (const uint32_t *)(ws + l.start), (const uint32_t *)(ws + l.pairs),
                       (const uint32_t *)(ws + l.outside), (const float4 *)(ws + l.packed), counts, (unsigned long long *)totals);
    return check_launch();
}

}  // extern "C"
