// mesh_tri_grid.h -- the uniform grid over the triangles' dilated bounding boxes, built on the device, once: a CSR of (cell, triangle)
// pairs plus an outside list and the packed records ("Grid" of include/pvd_hip_mesh_ray.h and of include/pvd_hip_mesh_winding.h).
// D is the number of binned axes: 3 for the ray cast (csrc/mesh_ray.hip, csrc/mesh_expose.hip through csrc/mesh_ray_walk.h), 2 (x and y)
// for the winding numbers (csrc/mesh_winding.hip).  The two differ in the cell index, the limit on G and one word of the record.
//
// k_tg_count<D>  one lane per triangle: validity, inside / outside, the number of cells of its range; one integer atomicAdd per
//                wave on each of the two 64-bit totals.
// k_tg_bin<D>    one lane per triangle: the packed record (index -1: invalid; for D = 2 the directions of its three edges), one integer
//                atomicAdd per cell of its range on the cell's count, or a slot of the outside list.
// k_blocksum, k_scan, k_offsets   (csrc/block_scan.h) the per-cell counts -> the cell starts and fill cursors; the
//                total (the number of pairs) to start[C] and to the header.
// k_tg_fill<D>   one lane per triangle: per cell of its range a slot from the cell's cursor (integer atomicAdd), its index into it.
// No workgroup waits on another one of the same launch, and no loop retries an atomic.  The order of the pairs inside a cell and of
// the outside list depends on the run.
// Everything is defined here (the library is built without relocatable device code): each translation unit gets its own copy.
#pragma once

#include "block_scan.h"
#include "mesh_grid.h"

#include "../../include/pvd_hip_mesh_ray.h"
#include "../../include/pvd_hip_mesh_winding.h"

namespace pvd {
namespace tgrid {

constexpr uint32_t kMaxT = 0x7fffffffu;
constexpr uint64_t kMaxPairs = 0x7fffffffull;
template <int D>
constexpr uint32_t kMaxG = D == 3 ? PVD_MESH_RAY_MAX_G : PVD_MESH_WINDING_MAX_G;

// header words (uint32): 0 = outside triangles (the list's cursor), 1..3 = bmin, 4..6 = bmax (float bits), 7 = pairs; 64 bytes in all
constexpr size_t kHeaderBytes = 64;
constexpr size_t kCellsPerSum = 256;  // cells per partial sum of the build's scan
static_assert(kCellsPerSum == (size_t)kThreads, "the layout's partial sums are those of k_blocksum");

struct Layout {  // byte offsets into the workspace; the 16-byte records first, so that a 16-byte aligned workspace aligns them
    size_t packed, start, cursor, bsum, outside, pairs, total;
};

template <int D>
inline Layout layout(uint32_t T, uint32_t G, uint64_t pairs) {
    const size_t C = (size_t)G * G * (D == 3 ? G : 1u), NB = (C + kCellsPerSum - 1) / kCellsPerSum;
    Layout l;
    l.packed = kHeaderBytes;
    l.start = l.packed + 48 * (size_t)T;
    l.cursor = l.start + 4 * (C + 1);
    l.bsum = l.cursor + 4 * C;
    l.outside = l.bsum + 4 * NB;
    l.pairs = l.outside + 4 * (size_t)T;
    l.total = l.pairs + 4 * (size_t)pairs;
    return l;
}

template <int D>
inline bool in_range(uint32_t T, uint32_t G, uint64_t pairs) {
    return G >= 1 && G <= kMaxG<D> && T <= kMaxT && pairs <= kMaxPairs;
}

template <int D>
inline int check_args(uint32_t T, uint32_t G, uint64_t pairs, const void *workspace, size_t workspace_bytes) {
    if (!workspace || ((uintptr_t)workspace & 15u)) return PVD_ERR_INVALID;
    if (!in_range<D>(T, G, pairs)) return PVD_ERR_UNSUPPORTED;
    if (workspace_bytes < layout<D>(T, G, pairs).total) return PVD_ERR_INVALID;
    return PVD_OK;
}

// the pure parts (box, ranges) are PVD_HD, __host__ __device__: a CPU build can walk the same code
template <int D>
struct Box {  // per binned axis: flat (one layer from -inf to +inf), the bounds, the cell size and its inverse, the dilation eps
    bool flat[D];
    double lo[D], hi[D], h[D], inv_h[D], eps[D];
};

template <int D>
PVD_HD Box<D> box_of(const float *__restrict__ bmin3, const float *__restrict__ bmax3, uint32_t G) {
    Box<D> b;
#pragma unroll
    for (int a = 0; a < D; ++a) {
        const double lo = (double)bmin3[a], hi = (double)bmax3[a];
        const double ext = hi - lo;
        const bool ok = ext > 0.0 && ext < (double)INFINITY;  // false for NaN
        b.flat[a] = !ok;
        b.lo[a] = ok ? lo : 0.0;
        b.hi[a] = ok ? hi : 0.0;
        b.h[a] = ok ? ext / (double)G : 0.0;
        b.inv_h[a] = ok ? (double)G / ext : 0.0;
        b.eps[a] = ok ? 0x1p-20 * ext : 0.0;
    }
    return b;
}

enum : int { kInvalid = 0, kInside = 1, kOutside = 2 };

// the class of triangle t, for an inside one its range of cells k0 .. k1 per axis, and the directions of its edges: bit 0 = (b, c)
// runs from the lower to the higher index, bit 1 = (c, a), bit 2 = (a, b)
template <int D>
PVD_HD int classify(const float *__restrict__ vertices, uint32_t V, const int32_t *__restrict__ triangles, uint32_t t, const Box<D> &box,
                    uint32_t G, int k0[D], int k1[D], float corners[9], uint32_t &dirs) {
    const int32_t ia = triangles[3 * (size_t)t], ib = triangles[3 * (size_t)t + 1], ic = triangles[3 * (size_t)t + 2];
    if (!((uint32_t)ia < V && (uint32_t)ib < V && (uint32_t)ic < V)) return kInvalid;  // a negative index is a large unsigned one
    dirs = (ib < ic ? 1u : 0u) | (ic < ia ? 2u : 0u) | (ia < ib ? 4u : 0u);
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
    for (int a = 0; a < D; ++a) {
        const double mn = (double)fminf(corners[a], fminf(corners[3 + a], corners[6 + a]));
        const double mx = (double)fmaxf(corners[a], fmaxf(corners[3 + a], corners[6 + a]));
        if (!box.flat[a] && !(box.lo[a] <= mn && mx <= box.hi[a])) inside = false;
        k0[a] = cell_axis(box, a, mn - box.eps[a], G);
        k1[a] = cell_axis(box, a, mx + box.eps[a], G);
    }
    return inside ? kInside : kOutside;
}

// f(cell) for every cell of the range k0 .. k1, the last axis fastest
template <int D, typename F>
PVD_HD void for_cells(const int k0[D], const int k1[D], uint32_t G, F f) {
    for (int x = k0[0]; x <= k1[0]; ++x)
        for (int y = k0[1]; y <= k1[1]; ++y) {
            const uint32_t c = (uint32_t)x * G + (uint32_t)y;
            if constexpr (D == 2) {
                f(c);
            } else {
                for (int z = k0[2]; z <= k1[2]; ++z) f(c * G + (uint32_t)z);
            }
        }
}

// Templates in an unnamed namespace: a translation unit gets a kernel, in its own code object, only where it launches it.
namespace {

// a triangle's range holds at most 2^24 cells (2^20 for two axes) and a wave 64 triangles: the wave's sum fits 32 bits, the totals
// are 64 bits wide
template <int D>
__global__ __launch_bounds__(kThreads) void k_tg_count(const float *__restrict__ vertices, uint32_t V, const int32_t *__restrict__ triangles,
                                                      uint32_t T, const float *__restrict__ bmin3, const float *__restrict__ bmax3, uint32_t G,
                                                      unsigned long long *__restrict__ totals) {
    const uint32_t t = blockIdx.x * kThreads + threadIdx.x;
    uint32_t cells = 0, out = 0;
    if (t < T) {
        int k0[D], k1[D];
        float c[9];
        uint32_t dirs;
        const int cls = classify<D>(vertices, V, triangles, t, box_of<D>(bmin3, bmax3, G), G, k0, k1, c, dirs);
        if (cls == kInside) {
            cells = 1;
#pragma unroll
            for (int a = 0; a < D; ++a) cells *= (uint32_t)(k1[a] - k0[a] + 1);
        }
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
template <int D>
__global__ __launch_bounds__(kThreads) void k_tg_bin(const float *__restrict__ vertices, uint32_t V, const int32_t *__restrict__ triangles,
                                                    uint32_t T, const float *__restrict__ bmin3, const float *__restrict__ bmax3, uint32_t G,
                                                    uint32_t *__restrict__ header, uint32_t *__restrict__ cursor,
                                                    uint32_t *__restrict__ outside, float4 *__restrict__ packed) {
    const uint32_t t = blockIdx.x * kThreads + threadIdx.x;
    if (t < 3) {
        header[1 + t] = f2u(bmin3[t]);
        header[4 + t] = f2u(bmax3[t]);
    }
    if (t >= T) return;
    int k0[D], k1[D];
    float c[9] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    uint32_t dirs = 0;
    const int cls = classify<D>(vertices, V, triangles, t, box_of<D>(bmin3, bmax3, G), G, k0, k1, c, dirs);
    float4 *o = packed + 3 * (size_t)t;
    o[0] = make_float4(c[0], c[1], c[2], c[3]);
    o[1] = make_float4(c[4], c[5], c[6], c[7]);
    o[2] = make_float4(c[8], u2f(cls == kInvalid ? 0xffffffffu : t), D == 2 ? u2f(dirs) : 0.0f, 0.0f);
    if (cls == kInside) {
        for_cells<D>(k0, k1, G, [&](uint32_t cell) { atomicAdd(&cursor[cell], 1u); });
    } else if (cls == kOutside) {
        const uint32_t slot = atomicAdd(&header[0], 1u);
        if (slot < T) outside[slot] = t;  // (always: at most T triangles are outside)
    }
}

template <int D>
__global__ __launch_bounds__(kThreads) void k_tg_fill(const float *__restrict__ vertices, uint32_t V, const int32_t *__restrict__ triangles,
                                                     uint32_t T, const uint32_t *__restrict__ header, uint32_t G, uint32_t pairs,
                                                     uint32_t *__restrict__ cursor, uint32_t *__restrict__ list) {
    const uint32_t t = blockIdx.x * kThreads + threadIdx.x;
    if (t >= T) return;
    int k0[D], k1[D];
    float c[9];
    uint32_t dirs;
    // the same box, bit for bit, as k_tg_bin read: the ranges agree with the counts
    const Box<D> box = box_of<D>((const float *)(header + 1), (const float *)(header + 4), G);
    if (classify<D>(vertices, V, triangles, t, box, G, k0, k1, c, dirs) != kInside) return;
    for_cells<D>(k0, k1, G, [&](uint32_t cell) {
        const uint32_t slot = atomicAdd(&cursor[cell], 1u);
        if (slot < pairs) list[slot] = t;  // a `pairs` below the true total loses pairs and stays inside the workspace
    });
}

}  // namespace

// ------------------------------------------------------------------------- the host side of pvd_mesh_{ray,winding}_{count,build}
// totals[0 .. 1] <- (pairs, outside triangles); the arguments are checked by the caller
template <int D>
inline int count(const float *vertices, uint32_t V, const int32_t *triangles, uint32_t T, const float *bmin3, const float *bmax3, uint32_t G,
                 uint64_t *totals, hipStream_t st) {
    const int rc = check_memset(hipMemsetAsync(totals, 0, 16, st));
    if (rc != PVD_OK || T == 0) return rc;
    hipLaunchKernelGGL(k_tg_count<D>, dim3(div_up(T, kThreads)), dim3(kThreads), 0, st, vertices, V, triangles, T, bmin3, bmax3, G,
                       (unsigned long long *)totals);
    return check_launch();
}

// the whole workspace of layout<D>(T, G, pairs); the arguments are checked by the caller
template <int D>
inline int build(const float *vertices, uint32_t V, const int32_t *triangles, uint32_t T, const float *bmin3, const float *bmax3, uint32_t G,
                 uint64_t pairs, void *workspace, hipStream_t st) {
    const Layout l = layout<D>(T, G, pairs);
    const uint32_t C = G * G * (D == 3 ? G : 1u), NB = div_up(C, kThreads), TB = T ? div_up(T, kThreads) : 1u;
    char *ws = (char *)workspace;
    uint32_t *header = (uint32_t *)ws, *start = (uint32_t *)(ws + l.start), *cursor = (uint32_t *)(ws + l.cursor);
    uint32_t *bsum = (uint32_t *)(ws + l.bsum), *outside = (uint32_t *)(ws + l.outside), *list = (uint32_t *)(ws + l.pairs);
    float4 *packed = (float4 *)(ws + l.packed);
    int rc;
    if ((rc = check_memset(hipMemsetAsync(header, 0, kHeaderBytes, st))) != PVD_OK) return rc;
    if ((rc = check_memset(hipMemsetAsync(cursor, 0, 4 * (size_t)C, st))) != PVD_OK) return rc;
    hipLaunchKernelGGL(k_tg_bin<D>, dim3(TB), dim3(kThreads), 0, st, vertices, V, triangles, T, bmin3, bmax3, G, header, cursor, outside, packed);
    if ((rc = check_launch()) != PVD_OK) return rc;
    hipLaunchKernelGGL(k_blocksum<uint32_t>, dim3(NB), dim3(kThreads), 0, st, cursor, C, bsum);
    if ((rc = check_launch()) != PVD_OK) return rc;
    hipLaunchKernelGGL(k_scan<uint32_t>, dim3(1), dim3(kScanThreads), 0, st, bsum, NB, start + C, header + 7);
    if ((rc = check_launch()) != PVD_OK) return rc;
    hipLaunchKernelGGL(k_offsets<uint32_t>, dim3(NB), dim3(kThreads), 0, st, cursor, C, bsum, start);
    if ((rc = check_launch()) != PVD_OK) return rc;
    if (T == 0) return PVD_OK;
    hipLaunchKernelGGL(k_tg_fill<D>, dim3(TB), dim3(kThreads), 0, st, vertices, V, triangles, T, header, G, (uint32_t)pairs, cursor, list);
    return check_launch();
}

}  // namespace tgrid
}  // namespace pvd
