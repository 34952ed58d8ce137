// mesh_simplify.hip -- uniform-grid vertex clustering of a triangle mesh (include/pvd_hip_mesh_simplify.h): every sum is a sum of
// integers, so the outputs do not depend on the order in which the atomics land.
//
// count phase
// k_ms_cells     one lane per vertex: its cell (all-ones for a vertex that is not valid), kept for the three kernels that need it.
// k_ms_tris      one lane per triangle: the survive flag, and a plain store of 1 into the flag word of each of its three cells
//                (every writer of a word stores the same value).
// k_blocksum, k_scan   (csrc/block_scan.h) the sums of the flags per workgroup (cells, then triangles) and their scan; the
//                total to totals_dev.
// k_ms_offsets   one lane per word: the flag becomes its exclusive rank (the cell's new index, the triangle's output row), all-ones
//                where the flag was 0.
// emit phase
// k_ms_gather    one lane per vertex: vertex_map, and 64-bit integer atomicAdd of (1, q, attributes) into the kept cell's row.
// k_ms_finish    one lane per new vertex: the means, mapped back into the box.
// k_ms_remap     one lane per triangle: a survivor writes its remapped row at its rank.
// The count -> one-workgroup scan -> offsets shape of csrc/block_scan.h: no workgroup waits on another one of the same launch, and
// no loop retries an atomic.
#include "block_scan.h"
#include "mesh_quant.h"

#include "../../include/pvd_hip_mesh_simplify.h"

namespace {

using namespace pvd;

constexpr uint32_t kNone = 0xffffffffu;
constexpr uint32_t kMaxN = 0x7fffffffu;  // V and T
constexpr int kMaxK = PVD_MESH_SIMPLIFY_MAX_K;

struct Layout {  // byte offsets into the workspace; the 8-byte records first
    size_t acc, vcell, cidx, cbsum, trow, tbsum, total;
};

inline size_t cells_of(uint32_t G) { return (size_t)G * G * G; }
inline size_t max_new(uint32_t V, uint32_t G) { return cells_of(G) < (size_t)V ? cells_of(G) : (size_t)V; }

inline Layout layout(uint32_t V, uint32_t T, uint32_t G, uint32_t K) {
    const size_t C = cells_of(G);
    Layout l;
    l.acc = 0;
    l.vcell = l.acc + 8 * (size_t)(4 + K) * max_new(V, G);
    l.cidx = l.vcell + 4 * (size_t)V;
    l.cbsum = l.cidx + 4 * C;
    l.trow = l.cbsum + 4 * ((C + kThreads - 1) / kThreads);
    l.tbsum = l.trow + 4 * (size_t)T;
    l.total = l.tbsum + 4 * (((size_t)T + kThreads - 1) / kThreads);
    return l;
}

inline bool in_limits(uint32_t V, uint32_t T, uint32_t G, uint32_t K) {
    return G >= 1 && G <= PVD_MESH_SIMPLIFY_MAX_G && K <= (uint32_t)kMaxK && V <= kMaxN && T <= kMaxN;
}

// Box, box_of and quantise (q_a) are in mesh_quant.h, finite1 in mesh_grid.h

PVD_HD uint32_t cell_axis(int64_t q, uint32_t G) {
    const uint32_t k = (uint32_t)(((uint64_t)q * G) >> 30);
    return k < G - 1 ? k : G - 1;
}

// llrint(clamp(v, -1, 1) * 2^30); 0 for a value that is not finite
PVD_HD int64_t quantise_attr(float v) {
    if (!finite1(v)) return 0;
    return (int64_t)llrint(fmin(1.0, fmax(-1.0, (double)v)) * 0x1p30);
}

__global__ __launch_bounds__(kThreads) void k_ms_cells(const float *__restrict__ vertices, uint32_t V, const float *__restrict__ bmin3,
                                                      const float *__restrict__ bmax3, uint32_t G, uint32_t *__restrict__ vcell) {
    const uint32_t v = blockIdx.x * kThreads + threadIdx.x;
    if (v >= V) return;
    const float x = vertices[3 * (size_t)v], y = vertices[3 * (size_t)v + 1], z = vertices[3 * (size_t)v + 2];
    uint32_t cell = kNone;
    if (finite1(x) && finite1(y) && finite1(z)) {
        const Box b = box_of(bmin3, bmax3);
        cell = (cell_axis(quantise(b, 0, x), G) * G + cell_axis(quantise(b, 1, y), G)) * G + cell_axis(quantise(b, 2, z), G);
    }
    vcell[v] = cell;
}

// C: the number of cells, a bound on what is read from vcell (a damaged workspace stays inside itself)
__global__ __launch_bounds__(kThreads) void k_ms_tris(const int32_t *__restrict__ triangles, uint32_t T, uint32_t V,
                                                     const uint32_t *__restrict__ vcell, uint32_t C, uint32_t *__restrict__ cflag,
                                                     uint32_t *__restrict__ trow) {
    const uint32_t t = blockIdx.x * kThreads + threadIdx.x;
    if (t >= T) return;
    const int32_t ia = triangles[3 * (size_t)t], ib = triangles[3 * (size_t)t + 1], ic = triangles[3 * (size_t)t + 2];
    uint32_t survives = 0;
    if ((uint32_t)ia < V && (uint32_t)ib < V && (uint32_t)ic < V) {  // a negative index is a large unsigned one
        const uint32_t ca = vcell[ia], cb = vcell[ib], cc = vcell[ic];
        if (ca < C && cb < C && cc < C && ca != cb && cb != cc && ca != cc) {  // kNone is not below C
            survives = 1;
            cflag[ca] = 1u;
            cflag[cb] = 1u;
            cflag[cc] = 1u;
        }
    }
    trow[t] = survives;
}

// flag (0 / 1) -> its exclusive rank where it was 1, kNone where it was 0; in place, each lane its own word
__global__ __launch_bounds__(kThreads) void k_ms_offsets(uint32_t *__restrict__ flag, uint32_t N, const uint32_t *__restrict__ bsum) {
    __shared__ uint32_t wtot[kWaves];
    const uint32_t c = blockIdx.x * kThreads + threadIdx.x;
    const uint32_t n = c < N ? flag[c] : 0u;
    const uint32_t rank = bsum[blockIdx.x] + block_exclusive(n, wtot);
    if (c < N) flag[c] = n ? rank : kNone;
}

// acc: per new vertex 4 + K words of 64 bits -- n, S_x, S_y, S_z, A_0 .. A_{K-1}.  Two's complement: the unsigned add is the signed one.
__global__ __launch_bounds__(kThreads) void k_ms_gather(const float *__restrict__ vertices, uint32_t V, const float *__restrict__ attrs,
                                                       uint32_t K, const float *__restrict__ bmin3, const float *__restrict__ bmax3,
                                                       const uint32_t *__restrict__ vcell, const uint32_t *__restrict__ cidx, uint32_t C,
                                                       uint32_t Vn, unsigned long long *__restrict__ acc, int32_t *__restrict__ vertex_map) {
    const uint32_t v = blockIdx.x * kThreads + threadIdx.x;
    if (v >= V) return;
    const uint32_t cell = vcell[v];
    const uint32_t nv = cell < C ? cidx[cell] : kNone;
    if (nv >= Vn) {  // kNone included; a rank at or above Vn cannot come out of the count phase
        vertex_map[v] = -1;
        return;
    }
    vertex_map[v] = (int32_t)nv;
    const Box b = box_of(bmin3, bmax3);
    unsigned long long *row = acc + (size_t)(4 + K) * nv;
    atomicAdd(row, 1ull);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        if (!b.flat[a]) atomicAdd(row + 1 + a, (unsigned long long)quantise(b, a, vertices[3 * (size_t)v + a]));
    }
    for (uint32_t j = 0; j < K; ++j) {
        const int64_t q = quantise_attr(attrs[(size_t)K * v + j]);
        if (q != 0) atomicAdd(row + 4 + j, (unsigned long long)q);
    }
}

__global__ __launch_bounds__(kThreads) void k_ms_finish(const unsigned long long *__restrict__ acc, uint32_t Vn, uint32_t K,
                                                       const float *__restrict__ bmin3, const float *__restrict__ bmax3,
                                                       float *__restrict__ out_vertices, float *__restrict__ out_attrs) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= Vn) return;
    const Box b = box_of(bmin3, bmax3);
    const unsigned long long *row = acc + (size_t)(4 + K) * i;
    const double n = (double)row[0];  // at least 1: a kept cell holds a corner of a surviving triangle
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        out_vertices[3 * (size_t)i + a] = b.flat[a] ? bmin3[a] : (float)(b.lo[a] + ((double)(int64_t)row[1 + a] / n) * (b.ext[a] * 0x1p-30));
    }
    for (uint32_t j = 0; j < K; ++j) out_attrs[(size_t)K * i + j] = (float)(((double)(int64_t)row[4 + j] / n) * 0x1p-30);
}

__global__ __launch_bounds__(kThreads) void k_ms_remap(const int32_t *__restrict__ triangles, uint32_t T, uint32_t V,
                                                      const uint32_t *__restrict__ vcell, const uint32_t *__restrict__ cidx, uint32_t C,
                                                      const uint32_t *__restrict__ trow, uint32_t Tn, int32_t *__restrict__ out_triangles) {
    const uint32_t t = blockIdx.x * kThreads + threadIdx.x;
    if (t >= T) return;
    const uint32_t row = trow[t];
    if (row >= Tn) return;  // kNone included
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const uint32_t i = (uint32_t)triangles[3 * (size_t)t + q];  // a survivor's indices are below V; the checks hold for any workspace
        const uint32_t cell = i < V ? vcell[i] : kNone;
        out_triangles[3 * (size_t)row + q] = cell < C ? (int32_t)cidx[cell] : -1;
    }
}

int check_args(uint32_t V, uint32_t T, uint32_t G, uint32_t K, const void *workspace, size_t workspace_bytes) {
    if (!workspace || ((uintptr_t)workspace & 15u)) return PVD_ERR_INVALID;
    if (!in_limits(V, T, G, K)) return PVD_ERR_UNSUPPORTED;
    if (workspace_bytes < layout(V, T, G, K).total) return PVD_ERR_INVALID;
    return PVD_OK;
}

// blocksum -> scan -> offsets over the N flags at `flag`
int scan_flags(uint32_t *flag, uint32_t N, uint32_t *bsum, int32_t *total, hipStream_t st) {
    const uint32_t NB = div_up(N, kThreads);
    int rc;
    if (NB) {
        hipLaunchKernelGGL(k_blocksum<uint32_t>, dim3(NB), dim3(kThreads), 0, st, flag, N, bsum);
        if ((rc = check_launch()) != PVD_OK) return rc;
    }
    // NB == 0: the total 0.  The total is at most 2^31 - 1 triangles or 2^27 cells: the unsigned word is the signed one.
    hipLaunchKernelGGL(k_scan<uint32_t>, dim3(1), dim3(kScanThreads), 0, st, bsum, NB, (uint32_t *)total, (uint32_t *)total);
    if ((rc = check_launch()) != PVD_OK) return rc;
    if (NB) {
        hipLaunchKernelGGL(k_ms_offsets, dim3(NB), dim3(kThreads), 0, st, flag, N, bsum);
        if ((rc = check_launch()) != PVD_OK) return rc;
    }
    return PVD_OK;
}

}  // namespace

extern "C" {

size_t pvd_mesh_simplify_workspace_bytes(uint32_t V, uint32_t T, uint32_t G, uint32_t K) {
    return in_limits(V, T, G, K) ? layout(V, T, G, K).total : 0;
}

int pvd_mesh_simplify_count(const float *vertices, uint32_t V, const int32_t *triangles, uint32_t T, const float *bmin3,
                            const float *bmax3, uint32_t G, uint32_t K, void *workspace, size_t workspace_bytes, int32_t *totals_dev,
                            pvd_stream_t stream) {
    if (!bmin3 || !bmax3 || !totals_dev || (T && !triangles) || (V && !vertices)) return PVD_ERR_INVALID;
    int rc = check_args(V, T, G, K, workspace, workspace_bytes);
    if (rc != PVD_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    const Layout l = layout(V, T, G, K);
    const uint32_t C = G * G * G;
    char *ws = (char *)workspace;
    uint32_t *vcell = (uint32_t *)(ws + l.vcell), *cidx = (uint32_t *)(ws + l.cidx);
    uint32_t *cbsum = (uint32_t *)(ws + l.cbsum), *trow = (uint32_t *)(ws + l.trow), *tbsum = (uint32_t *)(ws + l.tbsum);
    if ((rc = check_memset(hipMemsetAsync(cidx, 0, 4 * (size_t)C, st))) != PVD_OK) return rc;
    if (V) {
        hipLaunchKernelGGL(k_ms_cells, dim3(div_up(V, kThreads)), dim3(kThreads), 0, st, vertices, V, bmin3, bmax3, G, vcell);
        if ((rc = check_launch()) != PVD_OK) return rc;
    }
    if (T) {
        hipLaunchKernelGGL(k_ms_tris, dim3(div_up(T, kThreads)), dim3(kThreads), 0, st, triangles, T, V, vcell, C, cidx, trow);
        if ((rc = check_launch()) != PVD_OK) return rc;
    }
    if ((rc = scan_flags(cidx, C, cbsum, totals_dev + 0, st)) != PVD_OK) return rc;
    return scan_flags(trow, T, tbsum, totals_dev + 1, st);
}

int pvd_mesh_simplify_emit(const float *vertices, uint32_t V, const int32_t *triangles, uint32_t T, const float *attrs, uint32_t K,
                           const float *bmin3, const float *bmax3, uint32_t G, void *workspace, size_t workspace_bytes,
                           float *out_vertices, uint32_t Vn, float *out_attrs, int32_t *out_triangles, uint32_t Tn, int32_t *vertex_map,
                           pvd_stream_t stream) {
    if (!bmin3 || !bmax3 || (T && !triangles) || (V && (!vertices || !vertex_map))) return PVD_ERR_INVALID;
    int rc = check_args(V, T, G, K, workspace, workspace_bytes);
    if (rc != PVD_OK) return rc;
    if ((size_t)Vn > max_new(V, G) || Tn > T) return PVD_ERR_INVALID;
    if ((V && K && !attrs) || (Vn && (!out_vertices || (K && !out_attrs))) || (Tn && !out_triangles)) return PVD_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const Layout l = layout(V, T, G, K);
    const uint32_t C = G * G * G;
    char *ws = (char *)workspace;
    const uint32_t *vcell = (const uint32_t *)(ws + l.vcell), *cidx = (const uint32_t *)(ws + l.cidx);
    const uint32_t *trow = (const uint32_t *)(ws + l.trow);
    unsigned long long *acc = (unsigned long long *)(ws + l.acc);
    if (V == 0) return PVD_OK;  // then Vn == 0 and Tn == 0
    if (Vn && (rc = check_memset(hipMemsetAsync(acc, 0, 8 * (size_t)(4 + K) * Vn, st))) != PVD_OK) return rc;
    hipLaunchKernelGGL(k_ms_gather, dim3(div_up(V, kThreads)), dim3(kThreads), 0, st, vertices, V, attrs, K, bmin3, bmax3, vcell, cidx, C,
                       Vn, acc, vertex_map);
    if ((rc = check_launch()) != PVD_OK) return rc;
    if (Vn) {
        hipLaunchKernelGGL(k_ms_finish, dim3(div_up(Vn, kThreads)), dim3(kThreads), 0, st, acc, Vn, K, bmin3, bmax3, out_vertices, out_attrs);
        if ((rc = check_launch()) != PVD_OK) return rc;
    }
    if (Tn) {
        hipLaunchKernelGGL(k_ms_remap, dim3(div_up(T, kThreads)), dim3(kThreads), 0, st, triangles, T, V, vcell, cidx, C, trow, Tn,
                           out_triangles);
        if ((rc = check_launch()) != PVD_OK) return rc;
    }
    return PVD_OK;
}

}  // extern "C"
