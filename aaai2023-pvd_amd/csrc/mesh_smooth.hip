// mesh_smooth.hip -- Taubin lambda|mu smoothing of a triangle mesh (include/pvd_hip_mesh_smooth.h): every sum is a sum of integers,
// so the outputs do not depend on the order in which the atomics of the build land, and the passes use none.
//
// build
// k_sm_quant     one lane per vertex: its 16-byte row (q_x, q_y, q_z, flags), zeros and no valid flag for a vertex that is not valid.
// k_sm_count     one lane per triangle: a valid one adds 2 to the row size of each of its corners (32-bit integer atomicAdd).
// k_sm_blocksum  one lane per vertex: the sum (64-bit) and the largest of the workgroup's 256 row sizes.
// k_sm_scan      ONE workgroup: the exclusive scan of those sums in place (scan_sums, csrc/block_scan.h) and the largest of the
//                maxima; the total and the largest row to totals_dev, the total also behind the last row offset.
// k_sm_offsets   one lane per vertex: its 64-bit row offset, and its index appended to the list of long rows (one atomic counter)
//                when it is movable and its row is longer than kLongRow.
// k_sm_fill      one lane per triangle: a valid one takes two slots of each corner's row by an atomicSub of 2 on the row size -- the
//                cursor runs from the row's end to its start -- and stores the other two corners there.
// run
// k_sm_pass      ONE launch per pass, a pure gather.  Each lane first serves the vertex of its global index: a vertex that is not
//                movable is copied, a row of at most kLongRow entries is summed by the lane.  Then the workgroup's waves take long rows
//                from the list, one wave per row, grid-strided: the lanes stride the row, and three int64 partial sums are reduced
//                across the 64 lanes.  A long row is written by that wave's lane 0 alone.
// k_sm_out       one lane per vertex: a movable vertex mapped back into the box, any other one its input bits.
// The count -> one-workgroup scan -> offsets shape of csrc/block_scan.h, over 64-bit sums: no workgroup waits on another one of the
// same launch, and no loop retries an atomic.  The dependency between two passes is the launch boundary.
#include "block_scan.h"
#include "mesh_quant.h"

#include "../../include/pvd_hip_mesh_smooth.h"

namespace {

using namespace pvd;

constexpr uint32_t kMaxN = 0x7fffffffu;  // V and T
// A movable row of more than kLongRow entries is summed by a whole wavefront, any other one by a single lane.  One wave stride is 64
// entries; a closed manifold mesh has rows of about 12.  Not A/B-measured: profiles/mesh_smooth.txt says what was.
constexpr uint32_t kLongRow = 64;
constexpr uint32_t kValid = 1u, kPinned = 2u;  // the flag word of a vertex row
constexpr int32_t kOne = 1 << 30;

struct Layout {  // byte offsets into the workspace; the 16-byte rows first, then the 8-byte words, then the 4-byte ones
    size_t q0, qa, qb, off, bsum, cnt, longs, bmax, adj, nlong, total;
};

inline Layout layout(uint32_t V, uint32_t T) {
    const size_t NB = ((size_t)V + kThreads - 1) / kThreads;
    Layout l;
    l.q0 = 0;
    l.qa = l.q0 + 16 * (size_t)V;
    l.qb = l.qa + 16 * (size_t)V;
    l.off = l.qb + 16 * (size_t)V;
    l.bsum = l.off + 8 * ((size_t)V + 1);
    l.cnt = l.bsum + 8 * NB;
    l.longs = l.cnt + 4 * (size_t)V;
    l.bmax = l.longs + 4 * (size_t)V;
    l.adj = l.bmax + 4 * NB;
    l.nlong = l.adj + 24 * (size_t)T;
    l.total = l.nlong + 16;
    return l;
}

inline bool in_limits(uint32_t V, uint32_t T) { return V <= kMaxN && T <= kMaxN; }

__global__ __launch_bounds__(kThreads) void k_sm_quant(const float *__restrict__ vertices, uint32_t V, const float *__restrict__ bmin3,
                                                      const float *__restrict__ bmax3, const uint8_t *__restrict__ pinned,
                                                      int4 *__restrict__ q0) {
    const uint32_t v = blockIdx.x * kThreads + threadIdx.x;
    if (v >= V) return;
    const float x = vertices[3 * (size_t)v], y = vertices[3 * (size_t)v + 1], z = vertices[3 * (size_t)v + 2];
    int4 row = make_int4(0, 0, 0, 0);
    if (finite1(x) && finite1(y) && finite1(z)) {
        const Box b = box_of(bmin3, bmax3);
        row.x = (int32_t)quantise(b, 0, x);
        row.y = (int32_t)quantise(b, 1, y);
        row.z = (int32_t)quantise(b, 2, z);
        row.w = (int32_t)(kValid | ((pinned && pinned[v]) ? kPinned : 0u));
    }
    q0[v] = row;
}

// the three corners of triangle t when it is valid; no index is used before it is checked against V
__device__ __forceinline__ bool valid_triangle(const int32_t *__restrict__ triangles, uint32_t t, uint32_t V, const int4 *__restrict__ q0,
                                               uint32_t &ia, uint32_t &ib, uint32_t &ic) {
    ia = (uint32_t)triangles[3 * (size_t)t];  // a negative index is a large unsigned one
    ib = (uint32_t)triangles[3 * (size_t)t + 1];
    ic = (uint32_t)triangles[3 * (size_t)t + 2];
    if (ia >= V || ib >= V || ic >= V || ia == ib || ib == ic || ia == ic) return false;
    return ((uint32_t)q0[ia].w & (uint32_t)q0[ib].w & (uint32_t)q0[ic].w & kValid) != 0u;
}

__global__ __launch_bounds__(kThreads) void k_sm_count(const int32_t *__restrict__ triangles, uint32_t T, uint32_t V,
                                                      const int4 *__restrict__ q0, uint32_t *__restrict__ cnt) {
    const uint32_t t = blockIdx.x * kThreads + threadIdx.x;
    if (t >= T) return;
    uint32_t ia, ib, ic;
    if (!valid_triangle(triangles, t, V, q0, ia, ib, ic)) return;
    atomicAdd(cnt + ia, 2u);
    atomicAdd(cnt + ib, 2u);
    atomicAdd(cnt + ic, 2u);
}

__global__ __launch_bounds__(kThreads) void k_sm_blocksum(const uint32_t *__restrict__ cnt, uint32_t V, uint64_t *__restrict__ bsum,
                                                         uint32_t *__restrict__ bmax) {
    __shared__ uint64_t red[kWaves];
    __shared__ uint32_t big[kWaves];
    const uint32_t v = blockIdx.x * kThreads + threadIdx.x;
    const uint32_t n = v < V ? cnt[v] : 0u;
    const uint64_t a = block_sum((uint64_t)n, red);
    const uint32_t b = block_max(n, big);
    if (threadIdx.x == 0) {
        bsum[blockIdx.x] = a;
        bmax[blockIdx.x] = b;
    }
}

// one workgroup; sums [NB] -> exclusive scan in place; (total, largest row) to totals, the total to *last_off
__global__ __launch_bounds__(kScanThreads) void k_sm_scan(uint64_t *__restrict__ bsum, const uint32_t *__restrict__ bmax, uint32_t NB,
                                                         int64_t *__restrict__ totals, uint64_t *__restrict__ last_off) {
    __shared__ uint32_t wbig[kScanWaves];
    const uint64_t total = scan_sums(bsum, NB);
    uint32_t big = 0;
    for (uint32_t i = threadIdx.x; i < NB; i += kScanThreads) big = bmax[i] > big ? bmax[i] : big;  // (no barrier in this loop)
    big = block_max(big, wbig);
    if (threadIdx.x == 0) {
        totals[0] = (int64_t)total;  // at most 6 (2^31 - 1)
        totals[1] = (int64_t)big;
        *last_off = total;
    }
}

__global__ __launch_bounds__(kThreads) void k_sm_offsets(const uint32_t *__restrict__ cnt, uint32_t V, const uint64_t *__restrict__ bsum,
                                                        const int4 *__restrict__ q0, uint64_t *__restrict__ off,
                                                        uint32_t *__restrict__ longs, uint32_t *__restrict__ nlong) {
    __shared__ uint64_t wtot[kWaves];
    const uint32_t v = blockIdx.x * kThreads + threadIdx.x;
    const uint32_t n = v < V ? cnt[v] : 0u;
    const uint64_t at = bsum[blockIdx.x] + block_exclusive((uint64_t)n, wtot);
    if (v >= V) return;
    off[v] = at;
    if (n > kLongRow && ((uint32_t)q0[v].w & (kValid | kPinned)) == kValid) longs[atomicAdd(nlong, 1u)] = v;  // at most V of them
}

// E: 6 T, the room of adj -- a bound on what is written (a damaged workspace stays inside itself)
__global__ __launch_bounds__(kThreads) void k_sm_fill(const int32_t *__restrict__ triangles, uint32_t T, uint32_t V,
                                                     const int4 *__restrict__ q0, const uint64_t *__restrict__ off,
                                                     uint32_t *__restrict__ cnt, uint64_t E, uint32_t *__restrict__ adj) {
    const uint32_t t = blockIdx.x * kThreads + threadIdx.x;
    if (t >= T) return;
    uint32_t c[3];
    if (!valid_triangle(triangles, t, V, q0, c[0], c[1], c[2])) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const uint32_t left = atomicSub(cnt + c[k], 2u);  // the slots of this row not yet taken; the count phase made it >= 2
        const uint64_t at = off[c[k]] + (uint64_t)left - 2u;
        if (left >= 2u && at + 2u <= E) {
            adj[at] = c[(k + 1) % 3];
            adj[at + 1] = c[(k + 2) % 3];
        }
    }
}

// q + llrint(w (S / n - q)), clamped; every operation rounded on its own (-ffp-contract=off)
__device__ __forceinline__ int32_t moved(int32_t q, int64_t S, double n, double w) {
    const int64_t r = (int64_t)q + (int64_t)llrint(w * ((double)S / n - (double)q));
    return (int32_t)(r < 0 ? 0 : (r > kOne ? kOne : r));
}

__global__ __launch_bounds__(kThreads) void k_sm_pass(const int4 *__restrict__ src, int4 *__restrict__ dst, uint32_t V,
                                                     const uint64_t *__restrict__ off, const uint32_t *__restrict__ adj,
                                                     const uint32_t *__restrict__ longs, const uint32_t *__restrict__ nlong, double w) {
    const uint32_t v = blockIdx.x * kThreads + threadIdx.x;
    if (v < V) {
        const int4 me = src[v];
        const uint64_t lo = off[v], n = off[v + 1] - lo;
        const bool movable = ((uint32_t)me.w & (kValid | kPinned)) == kValid && n > 0;
        if (!movable) {
            dst[v] = me;
        } else if (n <= kLongRow) {
            int64_t sx = 0, sy = 0, sz = 0;
            for (uint32_t k = 0; k < (uint32_t)n; ++k) {
                const uint32_t j = adj[lo + k];
                if (j < V) {  // always, for a workspace build left
                    const int4 o = src[j];
                    sx += o.x;
                    sy += o.y;
                    sz += o.z;
                }
            }
            const double nd = (double)n;
            dst[v] = make_int4(moved(me.x, sx, nd, w), moved(me.y, sy, nd, w), moved(me.z, sz, nd, w), me.w);
        }
    }
    // the long rows: one wave per row
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint32_t nl = *nlong < V ? *nlong : V;
    for (uint32_t i = blockIdx.x * kWaves + threadIdx.x / kWave; i < nl; i += gridDim.x * kWaves) {  // wave-uniform
        const uint32_t r = longs[i];
        if (r >= V) continue;  // never, for a workspace build left
        const uint64_t lo = off[r], n = off[r + 1] - lo;
        int64_t sx = 0, sy = 0, sz = 0;
        for (uint64_t k = lane; k < n; k += kWave) {
            const uint32_t j = adj[lo + k];
            if (j < V) {
                const int4 o = src[j];
                sx += o.x;
                sy += o.y;
                sz += o.z;
            }
        }
        sx = (int64_t)wave_sum((uint64_t)sx);  // two's complement: the unsigned sum is the signed one
        sy = (int64_t)wave_sum((uint64_t)sy);
        sz = (int64_t)wave_sum((uint64_t)sz);
        if (lane == 0 && n > kLongRow) {
            const int4 me = src[r];
            const double nd = (double)n;
            dst[r] = make_int4(moved(me.x, sx, nd, w), moved(me.y, sy, nd, w), moved(me.z, sz, nd, w), me.w);
        }
    }
}

// q == nullptr: iterations == 0, every vertex gets its input bits
__global__ __launch_bounds__(kThreads) void k_sm_out(const uint32_t *__restrict__ vertex_bits, uint32_t V, const int4 *__restrict__ q,
                                                    const uint64_t *__restrict__ off, const float *__restrict__ bmin3,
                                                    const float *__restrict__ bmax3, uint32_t *__restrict__ out_bits) {
    const uint32_t v = blockIdx.x * kThreads + threadIdx.x;
    if (v >= V) return;
    bool movable = false;
    int4 me = make_int4(0, 0, 0, 0);
    if (q) {
        me = q[v];
        movable = ((uint32_t)me.w & (kValid | kPinned)) == kValid && off[v + 1] > off[v];
    }
    if (!movable) {
#pragma unroll
        for (int a = 0; a < 3; ++a) out_bits[3 * (size_t)v + a] = vertex_bits[3 * (size_t)v + a];
        return;
    }
    const Box b = box_of(bmin3, bmax3);
    const int32_t qs[3] = {me.x, me.y, me.z};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float x = b.flat[a] ? bmin3[a] : (float)(b.lo[a] + (double)qs[a] * (b.ext[a] * 0x1p-30));
        out_bits[3 * (size_t)v + a] = __float_as_uint(x);
    }
}

int check_args(uint32_t V, uint32_t T, const void *workspace, size_t workspace_bytes) {
    if (!workspace || ((uintptr_t)workspace & 15u)) return PVD_ERR_INVALID;
    if (!in_limits(V, T)) return PVD_ERR_UNSUPPORTED;
    if (workspace_bytes < layout(V, T).total) return PVD_ERR_INVALID;
    return PVD_OK;
}

bool weight_ok(double w) { return w >= -1.0 && w <= 1.0; }  // false for NaN

}  // namespace

extern "C" {

size_t pvd_mesh_smooth_workspace_bytes(uint32_t V, uint32_t T) { return in_limits(V, T) ? layout(V, T).total : 0; }

int pvd_mesh_smooth_build(const float *vertices, uint32_t V, const int32_t *triangles, uint32_t T, const float *bmin3,
                          const float *bmax3, const uint8_t *pinned, void *workspace, size_t workspace_bytes, int64_t *totals_dev,
                          pvd_stream_t stream) {
    if (!in_limits(V, T)) return PVD_ERR_UNSUPPORTED;
    if (V == 0) return PVD_OK;
    if (!vertices || !bmin3 || !bmax3 || !totals_dev || (T && !triangles)) return PVD_ERR_INVALID;
    int rc = check_args(V, T, workspace, workspace_bytes);
    if (rc != PVD_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    const Layout l = layout(V, T);
    char *ws = (char *)workspace;
    int4 *q0 = (int4 *)(ws + l.q0);
    uint64_t *off = (uint64_t *)(ws + l.off), *bsum = (uint64_t *)(ws + l.bsum);
    uint32_t *cnt = (uint32_t *)(ws + l.cnt), *longs = (uint32_t *)(ws + l.longs), *bmax = (uint32_t *)(ws + l.bmax);
    uint32_t *adj = (uint32_t *)(ws + l.adj), *nlong = (uint32_t *)(ws + l.nlong);
    const uint32_t NB = div_up(V, kThreads);
    if ((rc = check_memset(hipMemsetAsync(cnt, 0, 4 * (size_t)V, st))) != PVD_OK) return rc;
    if ((rc = check_memset(hipMemsetAsync(nlong, 0, 16, st))) != PVD_OK) return rc;
    hipLaunchKernelGGL(k_sm_quant, dim3(NB), dim3(kThreads), 0, st, vertices, V, bmin3, bmax3, pinned, q0);
    if ((rc = check_launch()) != PVD_OK) return rc;
    if (T) {
        hipLaunchKernelGGL(k_sm_count, dim3(div_up(T, kThreads)), dim3(kThreads), 0, st, triangles, T, V, q0, cnt);
        if ((rc = check_launch()) != PVD_OK) return rc;
    }
    hipLaunchKernelGGL(k_sm_blocksum, dim3(NB), dim3(kThreads), 0, st, cnt, V, bsum, bmax);
    if ((rc = check_launch()) != PVD_OK) return rc;
    hipLaunchKernelGGL(k_sm_scan, dim3(1), dim3(kScanThreads), 0, st, bsum, bmax, NB, totals_dev, off + V);
    if ((rc = check_launch()) != PVD_OK) return rc;
    hipLaunchKernelGGL(k_sm_offsets, dim3(NB), dim3(kThreads), 0, st, cnt, V, bsum, q0, off, longs, nlong);
    if ((rc = check_launch()) != PVD_OK) return rc;
    if (T) {
        hipLaunchKernelGGL(k_sm_fill, dim3(div_up(T, kThreads)), dim3(kThreads), 0, st, triangles, T, V, q0, off, cnt, 6 * (uint64_t)T, adj);
        if ((rc = check_launch()) != PVD_OK) return rc;
    }
    return PVD_OK;
}

int pvd_mesh_smooth_run(const float *vertices, uint32_t V, uint32_t T, const float *bmin3, const float *bmax3, void *workspace,
                        size_t workspace_bytes, double lambda, double mu, uint32_t iterations, float *out_vertices,
                        pvd_stream_t stream) {
    if (!in_limits(V, T)) return PVD_ERR_UNSUPPORTED;
    if (!weight_ok(lambda) || !weight_ok(mu) || iterations > PVD_MESH_SMOOTH_MAX_ITERATIONS) return PVD_ERR_INVALID;
    if (V == 0) return PVD_OK;
    if (!vertices || !bmin3 || !bmax3 || !out_vertices) return PVD_ERR_INVALID;
    int rc = check_args(V, T, workspace, workspace_bytes);
    if (rc != PVD_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    const Layout l = layout(V, T);
    char *ws = (char *)workspace;
    const int4 *q0 = (const int4 *)(ws + l.q0);
    int4 *buf[2] = {(int4 *)(ws + l.qa), (int4 *)(ws + l.qb)};
    const uint64_t *off = (const uint64_t *)(ws + l.off);
    const uint32_t *longs = (const uint32_t *)(ws + l.longs), *adj = (const uint32_t *)(ws + l.adj);
    const uint32_t *nlong = (const uint32_t *)(ws + l.nlong);
    const uint32_t NB = div_up(V, kThreads);
    const int4 *src = q0;  // what build left is only read
    for (uint32_t p = 0; p < 2 * iterations; ++p) {
        int4 *dst = buf[p & 1u];
        hipLaunchKernelGGL(k_sm_pass, dim3(NB), dim3(kThreads), 0, st, src, dst, V, off, adj, longs, nlong, (p & 1u) ? mu : lambda);
        if ((rc = check_launch()) != PVD_OK) return rc;
        src = dst;
    }
    hipLaunchKernelGGL(k_sm_out, dim3(NB), dim3(kThreads), 0, st, (const uint32_t *)vertices, V, iterations ? src : (const int4 *)nullptr, off,
                       bmin3, bmax3, (uint32_t *)out_vertices);
    return check_launch();
}

}  // extern "C"
