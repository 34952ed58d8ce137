// mesh_project.hip -- colour for surface points from posed images (csrc/pvd_hip_mesh_project.h): the views are projected onto the
// points, tested for facing, frame and occlusion, and blended; over the workspace pvd_mesh_ray_build leaves (csrc/mesh_ray.hip,
// csrc/mesh_tri_grid.h) and with the walk and the watertight test of csrc/mesh_ray_walk.h, which the first-hit cast and the exposure
// query use too.
//
// k_mp_integrate  ONE LANE PER POINT, consecutive lanes take consecutive points (the texels of an atlas row, the vertices in the
//                 mesher's order): a wave's rays to a camera are near-parallel, start in neighbouring cells and gather neighbouring
//                 pixels.  The lane keeps p, u and its four accumulators in registers through the views of the call; v is uniform, so
//                 the sixteen numbers of a view's camera are scalar loads that the whole wave shares.  The float32 tests come first
//                 and the float64 walk last: a lane whose view was skipped idles while its neighbours walk.  No LDS, no atomics; the
//                 accumulators are written back only where some view of the call reached the point.
// k_mp_finalize   one lane per point and pass of a grid-stride walk; the two totals: ballots per wave, summed in scalar registers over
//                 the walk, then one integer atomic per wave and total from lane 0.
// Every float32 operation is a single one in the order of the header; nothing is fused (the build's -ffp-contract=off, and the pragma
// below for a build without it).
#include "block_scan.h"
#include "mesh_ray_walk.h"

#include "pvd_hip_mesh_project.h"

namespace {

using namespace pvd;
using namespace pvd::tgrid;
using namespace pvd::mray;

constexpr float kFltMax = 3.402823466e+38f;
// The finalize pass walks the points with at most this many workgroups (8 per CU): its totals are same-address atomics, one per wave
// and total (as k_tsdf_finalize: profiles/mesh_tsdf.txt).
constexpr uint32_t kFinalizeBlocks = 2048;

struct F3 {
    float x, y, z;
};

struct Blocker {  // the walk's visitor: is some valid triangle hit with 0 <= t < 1 -- between the offset point and the camera
    Ray r;
    bool hit;

    PVD_HD void test(const float4 *__restrict__ packed, uint32_t j) {
#pragma clang fp contract(off)
        const float4 q0 = packed[3 * (size_t)j], q1 = packed[3 * (size_t)j + 1], q2 = packed[3 * (size_t)j + 2];
        if ((int32_t)f2u(q2.y) < 0) return;  // an invalid triangle
        Crossing x;
        if (!crossing(q0, q1, q2, r, x)) return;
        if (x.t >= 0.0 && x.t < 1.0) hit = true;  // false for NaN
    }
    PVD_HD bool found() const { return hit; }
    PVD_HD bool settled(double) const { return hit; }
};

__device__ __forceinline__ bool finite_f3(const F3 &a) { return finite3(a.x, a.y, a.z); }

__global__ __launch_bounds__(kThreads) void k_mp_integrate(const F3 *__restrict__ points, const F3 *__restrict__ normals, uint32_t N,
                                                          const F3 *__restrict__ color, const float *__restrict__ weight,
                                                          const float *__restrict__ poses, const float *__restrict__ intrinsics, uint32_t V,
                                                          uint32_t H, uint32_t W, uint32_t T, uint32_t G, uint32_t pairs,
                                                          const uint32_t *__restrict__ header, const uint32_t *__restrict__ start,
                                                          const uint32_t *__restrict__ list, const uint32_t *__restrict__ outside,
                                                          const float4 *__restrict__ packed, float cos_min, uint32_t power, float bias,
                                                          bool both, bool best, F3 *__restrict__ acc_c, float *__restrict__ acc_w) {
#pragma clang fp contract(off)
    const uint64_t n = (uint64_t)blockIdx.x * kThreads + threadIdx.x;  // 64 bits: N may be close to 2^32
    if (n >= N) return;
    const F3 p = points[n], nr = normals[n];
    const float L = sqrtf((nr.x * nr.x + nr.y * nr.y) + nr.z * nr.z);
    if (!(finite_f3(p) && finite_f3(nr) && L > 0.0f && L <= kFltMax)) return;  // takes no part
    const F3 u = {nr.x / L, nr.y / L, nr.z / L};
    const float x_hi = (float)W - 0.5f, y_hi = (float)H - 0.5f;
    float aw = acc_w[n];
    F3 ac = acc_c[n];
    bool touched = false;
    for (uint32_t v = 0; v < V; ++v) {
        const float *M = poses + 16 * (size_t)v;  // uniform: scalar loads
        const float *K = intrinsics + 4 * (size_t)v;
        const float ox = M[3], oy = M[7], oz = M[11];
        // 1. distance
        const float ex = ox - p.x, ey = oy - p.y, ez = oz - p.z;
        const float r = sqrtf((ex * ex + ey * ey) + ez * ez);
        if (!(r > 0.0f)) continue;
        // 2. facing
        float c = ((u.x * ex + u.y * ey) + u.z * ez) / r;
        float s = 1.0f;
        if (both) {
            if (c < 0.0f) s = -1.0f;
            c = fabsf(c);
        }
        if (!(c > cos_min)) continue;
        // 3. projection
        const float dx = p.x - ox, dy = p.y - oy, dz = p.z - oz;
        const float qz = (M[2] * dx + M[6] * dy) + M[10] * dz;
        if (!(qz > 0.0f)) continue;
        const float qx = (M[0] * dx + M[4] * dy) + M[8] * dz;
        const float qy = (M[1] * dx + M[5] * dy) + M[9] * dz;
        const float x = (K[0] * qx) / qz + K[2];
        const float y = (K[1] * qy) / qz + K[3];
        // 4. in frame
        if (!(x >= 0.5f && x <= x_hi && y >= 0.5f && y <= y_hi)) continue;
        // 5. texel: 0 <= a <= W - 1 and 0 <= b <= H - 1 by the test above, so i is 0 .. W - 2 and j is 0 .. H - 2
        const float a = x - 0.5f, b = y - 0.5f;
        const uint32_t i = umin((uint32_t)(int)floorf(a), W - 2u), j = umin((uint32_t)(int)floorf(b), H - 2u);
        const float f = a - (float)i, g = b - (float)j;
        // 6. bilinear colour
        const float f1 = 1.0f - f, g1 = 1.0f - g;
        const float m00 = f1 * g1, m10 = f * g1, m01 = f1 * g, m11 = f * g;
        const size_t pix = ((size_t)v * H + j) * W + i;
        const F3 I00 = color[pix], I10 = color[pix + 1], I01 = color[pix + W], I11 = color[pix + W + 1];
        if (!(finite_f3(I00) && finite_f3(I10) && finite_f3(I01) && finite_f3(I11))) continue;
        const F3 C = {((m00 * I00.x + m10 * I10.x) + m01 * I01.x) + m11 * I11.x, ((m00 * I00.y + m10 * I10.y) + m01 * I01.y) + m11 * I11.y,
                      ((m00 * I00.z + m10 * I10.z) + m01 * I01.z) + m11 * I11.z};
        // 7. view weight
        float w = 1.0f;
        for (uint32_t k = 0; k < power; ++k) w = w * c;
        if (weight) {
            const float wp = ((m00 * weight[pix] + m10 * weight[pix + 1]) + m01 * weight[pix + W]) + m11 * weight[pix + W + 1];
            if (!(wp > 0.0f && wp <= kFltMax)) continue;
            w = w * wp;
        }
        // 8. occlusion
        const float sb = s * bias;
        const float sx = p.x + sb * u.x, sy = p.y + sb * u.y, sz = p.z + sb * u.z;
        if (T != 0 && finite3(sx, sy, sz) && finite3(ox, oy, oz)) {
            const double o2[3] = {(double)sx, (double)sy, (double)sz};
            const double D[3] = {(double)ox - o2[0], (double)oy - o2[1], (double)oz - o2[2]};
            if (!(D[0] == 0.0 && D[1] == 0.0 && D[2] == 0.0)) {
                Blocker vis;
                vis.r = ray_of(o2, D);
                vis.hit = false;
                walk(o2, D, T, G, header, start, list, outside, packed, pairs, 0.0, 1.0, vis);
                if (vis.hit) continue;
            }
        }
        // 9. accumulate
        if (best) {
            if (w > aw) {
                aw = w;
                ac = C;
                touched = true;
            }
        } else {
            aw = aw + w;
            ac.x = ac.x + w * C.x;
            ac.y = ac.y + w * C.y;
            ac.z = ac.z + w * C.z;
            touched = true;
        }
    }
    if (touched) {
        acc_w[n] = aw;
        acc_c[n] = ac;
    }
}

__global__ __launch_bounds__(kThreads) void k_mp_finalize(const F3 *__restrict__ acc_c, const float *__restrict__ acc_w, uint32_t N,
                                                         float min_weight, bool best, F3 *__restrict__ colors, uint8_t *__restrict__ seen,
                                                         unsigned long long *__restrict__ totals) {
#pragma clang fp contract(off)
    // a grid-stride walk: the wave's first index is a multiple of 64 and the stride is one, so `first < N` is the same in every lane of
    // a wave and the ballots see whole waves (the index is 64 bits wide: N may be close to 2^32)
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint64_t stride = (uint64_t)gridDim.x * kThreads;
    unsigned long long n_seen = 0, n_not = 0;
    for (uint64_t first = (uint64_t)blockIdx.x * kThreads + (threadIdx.x - lane); first < N; first += stride) {
        const uint64_t n = first + lane;
        const bool live = n < N;
        bool is_seen = false;
        if (live) {
            const float w = acc_w[n];
            is_seen = w >= min_weight;  // false for NaN
            if (is_seen) {
                const F3 a = acc_c[n];
                const F3 q = best ? a : F3{a.x / w, a.y / w, a.z / w};
                colors[n] = {fminf(fmaxf(q.x, 0.0f), 1.0f), fminf(fmaxf(q.y, 0.0f), 1.0f), fminf(fmaxf(q.z, 0.0f), 1.0f)};
            }
            seen[n] = is_seen ? 1 : 0;
        }
        n_seen += __popcll(__ballot(is_seen));
        n_not += __popcll(__ballot(live && !is_seen));
    }
    if (lane == 0) {
        if (n_seen) atomicAdd(&totals[0], n_seen);
        if (n_not) atomicAdd(&totals[1], n_not);
    }
}

bool side_ok(uint32_t s) { return s >= 2 && s <= PVD_MESH_PROJECT_MAX_SIDE; }
bool mode_ok(uint32_t m) { return m == PVD_MESH_PROJECT_MODE_BLEND || m == PVD_MESH_PROJECT_MODE_BEST; }

}  // namespace

extern "C" {

int pvd_mesh_project_integrate(const float *points, const float *normals, uint32_t N, const float *color, const float *weight,
                               const float *poses, const float *intrinsics, uint32_t V, uint32_t H, uint32_t W, uint32_t T, uint32_t G,
                               uint64_t pairs, const void *workspace, size_t workspace_bytes, float cos_min, uint32_t power, float bias,
                               uint32_t sides, uint32_t mode, float *acc_c, float *acc_w, pvd_stream_t stream) {
    if (!side_ok(W) || !side_ok(H) || power > PVD_MESH_PROJECT_MAX_POWER || !mode_ok(mode) ||
        !(sides == PVD_MESH_PROJECT_SIDES_FRONT || sides == PVD_MESH_PROJECT_SIDES_BOTH))
        return PVD_ERR_UNSUPPORTED;
    if (!(cos_min >= 0.0f && cos_min < 1.0f)) return PVD_ERR_INVALID;  // false for NaN
    if (!(bias >= 0.0f && bias <= kFltMax)) return PVD_ERR_INVALID;
    const int rc = check_args<3>(T, G, pairs, workspace, workspace_bytes);
    if (rc != PVD_OK) return rc;
    if (N == 0 || V == 0) return PVD_OK;
    if (!points || !normals || !color || !poses || !intrinsics || !acc_c || !acc_w) return PVD_ERR_INVALID;
    const Layout l = layout<3>(T, G, pairs);
    const char *ws = (const char *)workspace;
    hipLaunchKernelGGL(k_mp_integrate, dim3((uint32_t)(((uint64_t)N + kThreads - 1) / kThreads)), dim3(kThreads), 0, (hipStream_t)stream, (const F3 *)points,
                       (const F3 *)normals, N, (const F3 *)color, weight, poses, intrinsics, V, H, W, T, G, (uint32_t)pairs,
                       (const uint32_t *)ws, (const uint32_t *)(ws + l.start), (const uint32_t *)(ws + l.pairs),
                       (const uint32_t *)(ws + l.outside), (const float4 *)(ws + l.packed), cos_min, power, bias,
                       sides == PVD_MESH_PROJECT_SIDES_BOTH, mode == PVD_MESH_PROJECT_MODE_BEST, (F3 *)acc_c, acc_w);
    return check_launch();
}

int pvd_mesh_project_finalize(const float *acc_c, const float *acc_w, uint32_t N, float min_weight, uint32_t mode, float *colors,
                              uint8_t *seen, int64_t *totals, pvd_stream_t stream) {
    if (!mode_ok(mode)) return PVD_ERR_UNSUPPORTED;
    if (!(min_weight > 0.0f && min_weight <= kFltMax)) return PVD_ERR_INVALID;
    if (N == 0) return PVD_OK;
    if (!acc_c || !acc_w || !colors || !seen || !totals) return PVD_ERR_INVALID;
    const hipStream_t st = (hipStream_t)stream;
    const int rc = check_memset(hipMemsetAsync(totals, 0, 2 * sizeof(int64_t), st));
    if (rc != PVD_OK) return rc;
    hipLaunchKernelGGL(k_mp_finalize, dim3(umin((uint32_t)(((uint64_t)N + kThreads - 1) / kThreads), kFinalizeBlocks)), dim3(kThreads), 0, st, (const F3 *)acc_c, acc_w, N,
                       min_weight, mode == PVD_MESH_PROJECT_MODE_BEST, (F3 *)colors, seen, (unsigned long long *)totals);
    return check_launch();
}

}  // extern "C"
