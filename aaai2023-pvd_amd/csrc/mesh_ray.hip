// mesh_ray.hip -- the first hit of many rays on a triangle mesh (include/pvd_hip_mesh_ray.h): a uniform grid over the triangles'
// dilated bounding boxes, built on the device (csrc/mesh_tri_grid.h, three binned axes: k_tg_count<3>, k_tg_bin<3>, the scan of
// csrc/block_scan.h, k_tg_fill<3>), and a 3D-DDA walk per ray with the watertight test in unfused float64.
//
// k_mr_cast      one lane per ray: clip, walk, outside list.  No LDS, no atomics.
// The order of the pairs inside a cell depends on the run; the cast's (t, index) minimum does not.
#include "mesh_ray_walk.h"

namespace {

using namespace pvd;
using namespace pvd::tgrid;  // the workspace's layout and its build
using namespace pvd::mray;   // the test and the walk: shared with csrc/mesh_expose.hip

// ------------------------------------------------------------------------------------------------------- the first hit
struct Best {
    double t;     // the best t so far (starts at t_max)
    int32_t tri;  // its triangle (-1: none yet)
    double v, w;  // V / det, W / det of the best
};

struct FirstHit {  // the walk's visitor (csrc/mesh_ray_walk.h): the smallest (t, index) over [t_min, t_max)
    Ray r;
    double t_min, t_max;
    Best best;

    // record j of the packed array against the ray: include/pvd_hip_mesh_ray.h, steps 3 .. 8 and "Result"
    PVD_HD void test(const float4 *__restrict__ packed, uint32_t j) {
#pragma clang fp contract(off)
        const float4 q0 = packed[3 * (size_t)j], q1 = packed[3 * (size_t)j + 1], q2 = packed[3 * (size_t)j + 2];
        const int32_t idx = (int32_t)f2u(q2.y);
        if (idx < 0) return;  // an invalid triangle
        Crossing x;
        if (!crossing(q0, q1, q2, r, x)) return;
        if (!(x.t >= t_min && x.t < t_max)) return;  // false for NaN
        if (x.t < best.t || (x.t == best.t && best.tri >= 0 && idx < best.tri)) {  // best.t <= t_max throughout
            best.t = x.t;
            best.tri = idx;
            best.v = x.V / x.det;
            best.w = x.W / x.det;
        }
    }
    PVD_HD bool found() const { return false; }  // a later triangle may be nearer
    PVD_HD bool settled(double t_exit) const { return best.tri >= 0 && best.t < t_exit * (1.0 - 0x1p-30); }
};

// the search of one valid ray
PVD_HD void cast_ray(const double o[3], const double d[3], uint32_t T, uint32_t G, const uint32_t *__restrict__ header,
                     const uint32_t *__restrict__ start, const uint32_t *__restrict__ list, const uint32_t *__restrict__ outside,
                     const float4 *__restrict__ packed, uint32_t pairs, double t_min, double t_max, Best &best) {
    FirstHit vis;
    vis.r = ray_of(o, d);
    vis.t_min = t_min;
    vis.t_max = t_max;
    vis.best.t = t_max;
    vis.best.tri = -1;
    vis.best.v = vis.best.w = 0.0;
    walk(o, d, T, G, header, start, list, outside, packed, pairs, t_min, t_max, vis);
    best = vis.best;
}

__global__ __launch_bounds__(kThreads) void k_mr_cast(const float *__restrict__ origins, const float *__restrict__ dirs, uint32_t N, uint32_t T,
                                                     uint32_t G, uint32_t pairs, const uint32_t *__restrict__ header,
                                                     const uint32_t *__restrict__ start, const uint32_t *__restrict__ list,
                                                     const uint32_t *__restrict__ outside, const float4 *__restrict__ packed, float t_min,
                                                     float t_max, float *__restrict__ out_t, int32_t *__restrict__ out_tri,
                                                     float *__restrict__ out_bary) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= N) return;
    const float ox = origins[3 * (size_t)i], oy = origins[3 * (size_t)i + 1], oz = origins[3 * (size_t)i + 2];
    const float dx = dirs[3 * (size_t)i], dy = dirs[3 * (size_t)i + 1], dz = dirs[3 * (size_t)i + 2];
    if (!finite3(ox, oy, oz) || !finite3(dx, dy, dz) || (dx == 0.0f && dy == 0.0f && dz == 0.0f)) {
        out_t[i] = u2f(0x7fc00000u);
        out_tri[i] = -1;
        out_bary[2 * (size_t)i] = 0.0f;
        out_bary[2 * (size_t)i + 1] = 0.0f;
        return;
    }
    const double o[3] = {(double)ox, (double)oy, (double)oz}, d[3] = {(double)dx, (double)dy, (double)dz};
    Best best;
    cast_ray(o, d, T, G, header, start, list, outside, packed, pairs, (double)t_min, (double)t_max, best);
    const bool hit = best.tri >= 0;
    out_t[i] = hit ? (float)best.t : t_max;
    out_tri[i] = hit ? best.tri : -1;
    out_bary[2 * (size_t)i] = hit ? (float)best.v : 0.0f;
    out_bary[2 * (size_t)i + 1] = hit ? (float)best.w : 0.0f;
}

}  // namespace

extern "C" {

size_t pvd_mesh_ray_workspace_bytes(uint32_t T, uint32_t G, uint64_t pairs) { return in_range<3>(T, G, pairs) ? layout<3>(T, G, pairs).total : 0; }

int pvd_mesh_ray_count(const float *vertices, uint32_t V, const int32_t *triangles, uint32_t T, const float *bmin3, const float *bmax3,
                       uint32_t G, uint64_t *totals, pvd_stream_t stream) {
    if (!bmin3 || !bmax3 || !totals || (T && !triangles) || (T && V && !vertices)) return PVD_ERR_INVALID;
    if (!in_range<3>(T, G, 0)) return PVD_ERR_UNSUPPORTED;
    return count<3>(vertices, V, triangles, T, bmin3, bmax3, G, totals, (hipStream_t)stream);
}

int pvd_mesh_ray_build(const float *vertices, uint32_t V, const int32_t *triangles, uint32_t T, const float *bmin3, const float *bmax3,
                       uint32_t G, uint64_t pairs, void *workspace, size_t workspace_bytes, pvd_stream_t stream) {
    if (!bmin3 || !bmax3 || (T && !triangles) || (T && V && !vertices)) return PVD_ERR_INVALID;
    const int rc = check_args<3>(T, G, pairs, workspace, workspace_bytes);
    if (rc != PVD_OK) return rc;
    return build<3>(vertices, V, triangles, T, bmin3, bmax3, G, pairs, workspace, (hipStream_t)stream);
}

int pvd_mesh_ray_cast(const float *origins, const float *dirs, uint32_t N, uint32_t T, uint32_t G, uint64_t pairs, const void *workspace,
                      size_t workspace_bytes, float t_min, float t_max, float *t, int32_t *tri, float *bary, pvd_stream_t stream) {
    if (!(t_min >= 0.0f && t_min < INFINITY) || !(t_max > t_min)) return PVD_ERR_INVALID;  // false for NaN
    const int rc = check_args<3>(T, G, pairs, workspace, workspace_bytes);
    if (rc != PVD_OK) return rc;
    if (N == 0) return PVD_OK;
    if (!origins || !dirs || !t || !tri || !bary) return PVD_ERR_INVALID;
    const Layout l = layout<3>(T, G, pairs);
    const char *ws = (const char *)workspace;
    hipLaunchKernelGGL(k_mr_cast, dim3(div_up(N, kThreads)), dim3(kThreads), 0, (hipStream_t)stream, origins, dirs, N, T, G, (uint32_t)pairs,
                       (const uint32_t *)ws, (const uint32_t *)(ws + l.start), (const uint32_t *)(ws + l.pairs),
                       (const uint32_t *)(ws + l.outside), (const float4 *)(ws + l.packed), t_min, t_max, t, tri, bary);
    return check_launch();
}

}  // extern "C"
