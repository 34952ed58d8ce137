// mesh_ray.hip -- the first hit of many rays on a triangle mesh (include/pvd_hip_mesh_ray.h): a uniform grid over the triangles'
// dilated bounding boxes, built on the device, and a 3D-DDA walk per ray with the watertight test in unfused float64.
//
// k_mr_count     one lane per triangle: validity, inside / outside, the number of cells of its range; one integer atomicAdd per
//                wave on each of the two 64-bit totals.
// k_mr_bin       one lane per triangle: the packed record (index -1: invalid), one integer atomicAdd per cell of its range on the
//                cell's count, or a slot of the outside list.
// k_blocksum, k_scan, k_offsets   (csrc/block_scan.h) the per-cell counts -> the cell starts and fill cursors; the
//                total (the number of pairs) to start[C] and to the header.
// k_mr_fill      one lane per triangle: per cell of its range a slot from the cell's cursor (integer atomicAdd), its index into it.
// k_mr_cast      one lane per ray: clip, walk, outside list.  No LDS, no atomics.
// No workgroup waits on another one of the same launch, and no loop retries an atomic.  The order of the pairs inside a cell depends
// on the run; the cast's (t, index) minimum does not.
#include "block_scan.h"
#include "mesh_ray_walk.h"

namespace {

using namespace pvd;
using namespace pvd::mray;  // the workspace's layout, the box, the test and the walk: shared with csrc/mesh_expose.hip

static_assert(kCellsPerSum == (size_t)kThreads, "the layout's partial sums are those of k_blocksum");

enum : int { kInvalid = 0, kInside = 1, kOutside = 2 };

// the class of triangle t and, for an inside one, its range of cells k0 .. k1 per axis
PVD_HD int classify(const float *__restrict__ vertices, uint32_t V, const int32_t *__restrict__ triangles, uint32_t t, const Box &box,
                    uint32_t G, int k0[3], int k1[3], float corners[9]) {
    const int32_t ia = triangles[3 * (size_t)t], ib = triangles[3 * (size_t)t + 1], ic = triangles[3 * (size_t)t + 2];
    if (!((uint32_t)ia < V && (uint32_t)ib < V && (uint32_t)ic < V)) return kInvalid;  // a negative index is a large unsigned one
    const float *pa = vertices + 3 * (size_t)ia, *pb = vertices + 3 * (size_t)ib, *pc = vertices + 3 * (size_t)ic;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        corners[q] = pa[q];
        corners[3 + q] = pb[q];
        corners[6 + q] = pc[q];
    }
    if (!(finite3(corners[0], corners[1], corners[2]) && finite3(corners[3], corners[4], corners[5]) &&
          finite3(corners[6], corners[7], corners[8])))
        return kInvalid;
    bool inside = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double mn = (double)fminf(corners[a], fminf(corners[3 + a], corners[6 + a]));
        const double mx = (double)fmaxf(corners[a], fmaxf(corners[3 + a], corners[6 + a]));
        if (!box.flat[a] && !(box.lo[a] <= mn && mx <= box.hi[a])) inside = false;
        k0[a] = cell_axis(box, a, mn - box.eps[a], G);
        k1[a] = cell_axis(box, a, mx + box.eps[a], G);
    }
    return inside ? kInside : kOutside;
}

// a triangle's range holds at most 2^24 cells and a wave 64 triangles: the wave's sum fits 32 bits, the totals are 64 bits wide
__global__ __launch_bounds__(kThreads) void k_mr_count(const float *__restrict__ vertices, uint32_t V, const int32_t *__restrict__ triangles,
                                                      uint32_t T, const float *__restrict__ bmin3, const float *__restrict__ bmax3, uint32_t G,
                                                      unsigned long long *__restrict__ totals) {
    const uint32_t t = blockIdx.x * kThreads + threadIdx.x;
    uint32_t cells = 0, out = 0;
    if (t < T) {
        int k0[3], k1[3];
        float c[9];
        const int cls = classify(vertices, V, triangles, t, box_of(bmin3, bmax3, G), G, k0, k1, c);
        if (cls == kInside) cells = (uint32_t)(k1[0] - k0[0] + 1) * (uint32_t)(k1[1] - k0[1] + 1) * (uint32_t)(k1[2] - k0[2] + 1);
        out = cls == kOutside ? 1u : 0u;
    }
    cells = wave_sum(cells);
    out = wave_sum(out);
    if ((threadIdx.x & (kWave - 1)) == 0) {
        if (cells) atomicAdd(&totals[0], (unsigned long long)cells);
        if (out) atomicAdd(&totals[1], (unsigned long long)out);
    }
}

// the grid has at least one workgroup, so that the box reaches the header when T == 0 too
__global__ __launch_bounds__(kThreads) void k_mr_bin(const float *__restrict__ vertices, uint32_t V, const int32_t *__restrict__ triangles,
                                                    uint32_t T, const float *__restrict__ bmin3, const float *__restrict__ bmax3, uint32_t G,
                                                    uint32_t *__restrict__ header, uint32_t *__restrict__ cursor,
                                                    uint32_t *__restrict__ outside, float4 *__restrict__ packed) {
    const uint32_t t = blockIdx.x * kThreads + threadIdx.x;
    if (t < 3) {
        header[1 + t] = f2u(bmin3[t]);
        header[4 + t] = f2u(bmax3[t]);
    }
    if (t >= T) return;
    int k0[3], k1[3];
    float c[9] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    const int cls = classify(vertices, V, triangles, t, box_of(bmin3, bmax3, G), G, k0, k1, c);
    float4 *o = packed + 3 * (size_t)t;
    o[0] = make_float4(c[0], c[1], c[2], c[3]);
    o[1] = make_float4(c[4], c[5], c[6], c[7]);
    o[2] = make_float4(c[8], u2f(cls == kInvalid ? 0xffffffffu : t), 0.0f, 0.0f);
    if (cls == kInside) {
        for (int x = k0[0]; x <= k1[0]; ++x)
            for (int y = k0[1]; y <= k1[1]; ++y)
                for (int z = k0[2]; z <= k1[2]; ++z) atomicAdd(&cursor[((uint32_t)x * G + (uint32_t)y) * G + (uint32_t)z], 1u);
    } else if (cls == kOutside) {
        const uint32_t slot = atomicAdd(&header[0], 1u);
        if (slot < T) outside[slot] = t;  // (always: at most T triangles are outside)
    }
}

__global__ __launch_bounds__(kThreads) void k_mr_fill(const float *__restrict__ vertices, uint32_t V, const int32_t *__restrict__ triangles,
                                                     uint32_t T, const uint32_t *__restrict__ header, uint32_t G, uint32_t pairs,
                                                     uint32_t *__restrict__ cursor, uint32_t *__restrict__ list) {
    const uint32_t t = blockIdx.x * kThreads + threadIdx.x;
    if (t >= T) return;
    int k0[3], k1[3];
    float c[9];
    // the same box, bit for bit, as k_mr_bin read: the ranges agree with the counts
    if (classify(vertices, V, triangles, t, box_of((const float *)(header + 1), (const float *)(header + 4), G), G, k0, k1, c) != kInside) return;
    for (int x = k0[0]; x <= k1[0]; ++x)
        for (int y = k0[1]; y <= k1[1]; ++y)
            for (int z = k0[2]; z <= k1[2]; ++z) {
                const uint32_t slot = atomicAdd(&cursor[((uint32_t)x * G + (uint32_t)y) * G + (uint32_t)z], 1u);
                if (slot < pairs) list[slot] = t;  // a `pairs` below the true total loses pairs and stays inside the workspace
            }
}

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

size_t pvd_mesh_ray_workspace_bytes(uint32_t T, uint32_t G, uint64_t pairs) { return in_range(T, G, pairs) ? layout(T, G, pairs).total : 0; }

int pvd_mesh_ray_count(const float *vertices, uint32_t V, const int32_t *triangles, uint32_t T, const float *bmin3, const float *bmax3,
                       uint32_t G, uint64_t *totals, pvd_stream_t stream) {
    if (!bmin3 || !bmax3 || !totals || (T && !triangles) || (T && V && !vertices)) return PVD_ERR_INVALID;
    if (!in_range(T, G, 0)) return PVD_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    int rc;
    if ((rc = check_memset(hipMemsetAsync(totals, 0, 16, st))) != PVD_OK) return rc;
    if (T == 0) return PVD_OK;
    hipLaunchKernelGGL(k_mr_count, dim3(div_up(T, kThreads)), dim3(kThreads), 0, st, vertices, V, triangles, T, bmin3, bmax3, G,
                       (unsigned long long *)totals);
    return check_launch();
}

int pvd_mesh_ray_build(const float *vertices, uint32_t V, const int32_t *triangles, uint32_t T, const float *bmin3, const float *bmax3,
                       uint32_t G, uint64_t pairs, void *workspace, size_t workspace_bytes, pvd_stream_t stream) {
    if (!bmin3 || !bmax3 || (T && !triangles) || (T && V && !vertices)) return PVD_ERR_INVALID;
    int rc = check_args(T, G, pairs, workspace, workspace_bytes);
    if (rc != PVD_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    const Layout l = layout(T, G, pairs);
    const uint32_t C = G * G * G, NB = div_up(C, kThreads), TB = T ? div_up(T, kThreads) : 1u;
    char *ws = (char *)workspace;
    uint32_t *header = (uint32_t *)ws, *start = (uint32_t *)(ws + l.start), *cursor = (uint32_t *)(ws + l.cursor);
    uint32_t *bsum = (uint32_t *)(ws + l.bsum), *outside = (uint32_t *)(ws + l.outside), *list = (uint32_t *)(ws + l.pairs);
    float4 *packed = (float4 *)(ws + l.packed);
    if ((rc = check_memset(hipMemsetAsync(header, 0, kHeaderBytes, st))) != PVD_OK) return rc;
    if ((rc = check_memset(hipMemsetAsync(cursor, 0, 4 * (size_t)C, st))) != PVD_OK) return rc;
    hipLaunchKernelGGL(k_mr_bin, dim3(TB), dim3(kThreads), 0, st, vertices, V, triangles, T, bmin3, bmax3, G, header, cursor, outside, packed);
    if ((rc = check_launch()) != PVD_OK) return rc;
    hipLaunchKernelGGL(k_blocksum<uint32_t>, dim3(NB), dim3(kThreads), 0, st, cursor, C, bsum);
    if ((rc = check_launch()) != PVD_OK) return rc;
    hipLaunchKernelGGL(k_scan<uint32_t>, dim3(1), dim3(kScanThreads), 0, st, bsum, NB, start + C, header + 7);
    if ((rc = check_launch()) != PVD_OK) return rc;
    hipLaunchKernelGGL(k_offsets<uint32_t>, dim3(NB), dim3(kThreads), 0, st, cursor, C, bsum, start);
    if ((rc = check_launch()) != PVD_OK) return rc;
    if (T == 0) return PVD_OK;
    hipLaunchKernelGGL(k_mr_fill, dim3(TB), dim3(kThreads), 0, st, vertices, V, triangles, T, header, G, (uint32_t)pairs, cursor, list);
    return check_launch();
}

int pvd_mesh_ray_cast(const float *origins, const float *dirs, uint32_t N, uint32_t T, uint32_t G, uint64_t pairs, const void *workspace,
                      size_t workspace_bytes, float t_min, float t_max, float *t, int32_t *tri, float *bary, pvd_stream_t stream) {
    if (!(t_min >= 0.0f && t_min < INFINITY) || !(t_max > t_min)) return PVD_ERR_INVALID;  // false for NaN
    const int rc = check_args(T, G, pairs, workspace, workspace_bytes);
    if (rc != PVD_OK) return rc;
    if (N == 0) return PVD_OK;
    if (!origins || !dirs || !t || !tri || !bary) return PVD_ERR_INVALID;
    const Layout l = layout(T, G, pairs);
    const char *ws = (const char *)workspace;
    hipLaunchKernelGGL(k_mr_cast, dim3(div_up(N, kThreads)), dim3(kThreads), 0, (hipStream_t)stream, origins, dirs, N, T, G, (uint32_t)pairs,
                       (const uint32_t *)ws, (const uint32_t *)(ws + l.start), (const uint32_t *)(ws + l.pairs),
                       (const uint32_t *)(ws + l.outside), (const float4 *)(ws + l.packed), t_min, t_max, t, tri, bary);
    return check_launch();
}

}  // extern "C"
