// mesh_atex.hip -- the area-adaptive texture atlas of csrc/pvd_hip_mesh_atex.h: a cell edge per triangle from the texel density asked
// for, the triangles of a class packed into a band of the image in the order of their index, and inside a band the atlas of
// include/pvd_hip_mesh_tex.h with the rank in place of the triangle index.
//
// k_ax_classify  one lane per triangle: three indices, nine floats, the class; the class (<< 28) into slot[f]; the workgroup's five class
//                counts and its capped count from ONE 64-bit block_sum (six fields of 10 bits: a workgroup has 256 triangles).
// k_ax_scan      one workgroup: scan_sums over the six arrays of workgroup sums side by side; the six totals to the caller.
// k_ax_slots     one lane per triangle: its rank inside the workgroup from ONE 64-bit block_exclusive (five fields of 12 bits) plus the
//                workgroup's scanned sum; slot[f] = c << 28 | rank, order[base_c + rank] = f with base_c from the totals of the scan.
// k_ax_points    one lane per texel of a band of image rows, as k_mt_points: the class from y, the owner from order[], then
//                atlas::texel_point (csrc/mesh_atlas.h), the same arithmetic.
// k_ax_sample    one lane per hit: slot[tri], atlas::footprint_of with the class's S, C and the rank, y0 on the two rows, atlas::blend.
// Integer sums only and no atomics: the same bits from run to run.  Every float operation is a single float32 one in the order of the
// header; nothing is fused (the build's -ffp-contract=off, and the pragmas below for a build without it).
#include "block_scan.h"
#include "mesh_atlas.h"

#include "pvd_hip_mesh_atex.h"

namespace {

using namespace pvd;
using namespace pvd::atlas;

constexpr int kClasses = PVD_MESH_ATEX_CLASSES;
constexpr int kSums = PVD_MESH_ATEX_TOTALS;  // the five classes and the capped
constexpr uint32_t kRankMask = 0x0fffffffu;

struct AtexLayout {  // passed to the kernels by value
    uint32_t Wt, Ht;
    uint32_t y0[kClasses], rows[kClasses], C[kClasses], count[kClasses], base[kClasses];
};

// the layout of the header, or PVD_ERR_UNSUPPORTED
int layout_of(const uint32_t counts[5], AtexLayout &l) {
    uint64_t area = 0, total = 0;
    for (int c = 0; c < kClasses; ++c) {
        const uint64_t cells = (uint64_t)(counts[c] / 2u) + (counts[c] & 1u), S = 4u << c;
        area += cells * S * S;
        l.count[c] = counts[c];
        l.base[c] = (uint32_t)total;  // total <= 2^28 here or the function fails below
        total += counts[c];
    }
    if (total > PVD_MESH_ATEX_MAX_T) return PVD_ERR_UNSUPPORTED;
    uint64_t Wt = 64;
    while (Wt * Wt < area && Wt <= PVD_MESH_ATEX_MAX_SIDE) Wt += 64;
    if (Wt > PVD_MESH_ATEX_MAX_SIDE) return PVD_ERR_UNSUPPORTED;
    uint64_t y = 0;
    for (int c = 0; c < kClasses; ++c) {
        const uint64_t cells = (uint64_t)(counts[c] / 2u) + (counts[c] & 1u), S = 4u << c, C = Wt / S;
        const uint64_t rows = (cells + C - 1) / C;
        l.C[c] = (uint32_t)C;
        l.rows[c] = (uint32_t)rows;
        l.y0[c] = (uint32_t)y;
        y += rows * S;
        if (y > PVD_MESH_ATEX_MAX_SIDE) return PVD_ERR_UNSUPPORTED;
    }
    l.Wt = (uint32_t)Wt;
    l.Ht = y ? (uint32_t)y : 4u;
    return PVD_OK;
}

// NULL counts, the layout's errors, then counts that disagree with T
int layout_for(const uint32_t counts[5], uint32_t T, AtexLayout &l) {
    if (!counts) return PVD_ERR_INVALID;
    const int rc = layout_of(counts, l);
    if (rc != PVD_OK) return rc;
    return l.base[kClasses - 1] + l.count[kClasses - 1] == T ? PVD_OK : PVD_ERR_INVALID;
}

size_t sums_bytes(uint32_t T) { return (((size_t)kSums * div_up(T, kThreads) * sizeof(uint32_t)) + 15u) & ~(size_t)15u; }

__device__ __forceinline__ float len2(float ax, float ay, float az, float bx, float by, float bz) {
#pragma clang fp contract(off)
    const float ux = bx - ax, uy = by - ay, uz = bz - az;
    return (ux * ux + uy * uy) + uz * uz;
}

__global__ __launch_bounds__(kThreads) void k_ax_classify(const float *__restrict__ vertices, uint32_t V, const int32_t *__restrict__ triangles,
                                                         uint32_t T, float rho2, uint32_t max_class, uint32_t NB,
                                                         uint32_t *__restrict__ slot, uint32_t *__restrict__ bsum) {
#pragma clang fp contract(off)
    __shared__ unsigned long long red[kWaves];
    const uint32_t f = blockIdx.x * kThreads + threadIdx.x;
    unsigned long long mine = 0;  // field l: bits 10 l .. 10 l + 9
    if (f < T) {
        uint32_t c = 0, capped = 0;
        const int32_t ia = triangles[3 * (size_t)f], ib = triangles[3 * (size_t)f + 1], ic = triangles[3 * (size_t)f + 2];
        if ((uint32_t)ia < V && (uint32_t)ib < V && (uint32_t)ic < V) {
            const float *pa = vertices + 3 * (size_t)ia, *pb = vertices + 3 * (size_t)ib, *pc = vertices + 3 * (size_t)ic;
            const float ax = pa[0], ay = pa[1], az = pa[2], bx = pb[0], by = pb[1], bz = pb[2], gx = pc[0], gy = pc[1], gz = pc[2];
            if (finite3(ax, ay, az) && finite3(bx, by, bz) && finite3(gx, gy, gz)) {
                const float dAB = len2(ax, ay, az, bx, by, bz), dAC = len2(ax, ay, az, gx, gy, gz), dBC = len2(bx, by, bz, gx, gy, gz);
                const float L2 = fmaxf(fmaxf(dAB, dAC), dBC);
                const float q = L2 * rho2;
                const uint32_t c0 = (q > 1.0f ? 1u : 0u) + (q > 25.0f ? 1u : 0u) + (q > 169.0f ? 1u : 0u) + (q > 841.0f ? 1u : 0u);
                c = umin(c0, max_class);
                capped = (c0 > max_class || q > 3721.0f) ? 1u : 0u;
            }
        }
        slot[f] = c << 28;
        mine = (1ull << (10 * c)) | ((unsigned long long)capped << (10 * kClasses));
    }
    const unsigned long long all = block_sum(mine, red);  // a barrier: every thread is here
    if (threadIdx.x == 0) {
#pragma unroll
        for (int l = 0; l < kSums; ++l) bsum[(size_t)l * NB + blockIdx.x] = (uint32_t)(all >> (10 * l)) & 1023u;
    }
}

__global__ __launch_bounds__(kScanThreads) void k_ax_scan(uint32_t *__restrict__ bsum, uint32_t NB, uint32_t *__restrict__ totals) {
    uint32_t *const arrays[kSums] = {bsum, bsum + NB, bsum + 2 * (size_t)NB, bsum + 3 * (size_t)NB, bsum + 4 * (size_t)NB, bsum + 5 * (size_t)NB};
    uint32_t total[kSums];
    // six arrays, not five: the capped count rides along for its TOTAL only (a sum without atomics); its scanned sums are written back
    // like the others' and nothing reads them
    scan_sums(arrays, NB, total);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int l = 0; l < kSums; ++l) totals[l] = total[l];
    }
}

__global__ __launch_bounds__(kThreads) void k_ax_slots(uint32_t T, uint32_t NB, const uint32_t *__restrict__ bsum,
                                                      const uint32_t *__restrict__ totals, uint32_t *__restrict__ slot,
                                                      uint32_t *__restrict__ order) {
    __shared__ unsigned long long wtot[kWaves];
    const uint32_t f = blockIdx.x * kThreads + threadIdx.x;
    const uint32_t c = f < T ? slot[f] >> 28 : 0u;  // k_ax_classify's: 0 .. 4
    const unsigned long long before = block_exclusive(f < T ? 1ull << (12 * c) : 0ull, wtot);  // a barrier; field l: bits 12 l .. 12 l + 11
    if (f >= T) return;
    const uint32_t rank = bsum[(size_t)c * NB + blockIdx.x] + ((uint32_t)(before >> (12 * c)) & 4095u);
    uint32_t base = 0;
#pragma unroll
    for (uint32_t l = 0; l + 1 < (uint32_t)kClasses; ++l) base += l < c ? totals[l] : 0u;
    slot[f] = c << 28 | rank;
    order[base + rank] = f;  // base + rank < T: the ranks of a class are 0 .. count_c - 1
}

__global__ __launch_bounds__(kThreads) void k_ax_points(const float *__restrict__ vertices, uint32_t V, const int32_t *__restrict__ triangles,
                                                       uint32_t T, const float *__restrict__ normals, const uint32_t *__restrict__ order,
                                                       AtexLayout l, uint32_t row0, F3 *__restrict__ out_x, F3 *__restrict__ out_n) {
#pragma clang fp contract(off)
    const uint32_t x = blockIdx.x * kThreads + threadIdx.x;
    if (x >= l.Wt) return;
    const uint32_t r = blockIdx.y, y = row0 + r;
    uint32_t c = 0;  // the band of y: the last class that has rows and starts at or before y (uniform over the workgroup)
#pragma unroll
    for (uint32_t b = 1; b < (uint32_t)kClasses; ++b) c = (l.rows[b] && y >= l.y0[b]) ? b : c;
    const uint32_t sh = c + 2, S = 1u << sh, yy = y - l.y0[c];  // y >= y0[c]: y0[0] = 0
    const uint32_t cx = x >> sh, cy = yy >> sh, i = x - (cx << sh), j = yy - (cy << sh);
    const uint32_t k = cy * l.C[c] + cx;  // < rows * C <= 2^24
    const bool lower = i + j <= S - 1;
    const uint32_t rank = 2u * k + (lower ? 0u : 1u);
    const uint32_t p = lower ? i : S - 1 - i, q = lower ? j : S - 1 - j;
    const float nan = u2f(0x7fc00000u);
    F3 X = {nan, nan, nan}, N = {nan, nan, nan};
    if (rank < l.count[c]) {  // base + rank < T: the counts sum to T
        const uint32_t f = order[l.base[c] + rank];
        if (f < T) texel_point(vertices, V, triangles, normals, f, p, q, S, X, N);
    }
    const size_t e = (size_t)r * l.Wt + x;  // inside the band: r < row1 - row0, x < Wt
    out_x[e] = X;
    out_n[e] = N;
}

__global__ __launch_bounds__(kThreads) void k_ax_sample(const F3 *__restrict__ texture, uint32_t T, const uint32_t *__restrict__ slot,
                                                       AtexLayout l, const int32_t *__restrict__ tri, const float *__restrict__ bary,
                                                       uint32_t N, const float *__restrict__ bg3, F3 *__restrict__ color) {
#pragma clang fp contract(off)
    const uint32_t r = blockIdx.x * kThreads + threadIdx.x;
    if (r >= N) return;
    const int32_t f = tri[r];
    F3 out = {bg3[0], bg3[1], bg3[2]};
    if (f >= 0 && (uint32_t)f < T) {
        const uint32_t s = slot[f], c = s >> 28, rank = s & kRankMask;
        if (c < (uint32_t)kClasses && rank < l.count[c]) {  // so that the cell lies inside the band, whatever slot holds
            const float beta = bary[2 * (size_t)r], gamma = bary[2 * (size_t)r + 1];
            Footprint p = footprint_of(rank, beta, gamma, 4u << c, l.C[c]);
            p.ya += l.y0[c];
            p.yb += l.y0[c];
            out = blend(texture[(size_t)p.ya * l.Wt + p.xa], texture[(size_t)p.ya * l.Wt + p.xb], texture[(size_t)p.yb * l.Wt + p.xa],
                        texture[(size_t)p.yb * l.Wt + p.xb], p);
        }
    }
    color[r] = out;
}

}  // namespace

#define PVD_AX_LAUNCH(kernel, blocks, threads, ...)                                     \
    do {                                                                                \
        hipLaunchKernelGGL(kernel, dim3(blocks), dim3(threads), 0, st, __VA_ARGS__);    \
        if ((rc = check_launch()) != PVD_OK) return rc;                                 \
    } while (0)

extern "C" {

size_t pvd_mesh_atex_workspace_bytes(uint32_t T) {
    if (T > PVD_MESH_ATEX_MAX_T) return 0;
    const size_t n = sums_bytes(T);
    return n ? n : 16;
}

int pvd_mesh_atex_build(const float *vertices, uint32_t V, const int32_t *triangles, uint32_t T, float density, uint32_t max_class,
                        void *workspace, size_t workspace_bytes, uint32_t *slot, uint32_t *order, uint32_t *totals_dev, pvd_stream_t stream) {
    if (T > PVD_MESH_ATEX_MAX_T || max_class >= (uint32_t)kClasses) return PVD_ERR_UNSUPPORTED;
    const float rho2 = density * density;
    if (!(density > 0.0f) || !(rho2 > 0.0f) || !finite1(rho2)) return PVD_ERR_INVALID;
    if (!totals_dev) return PVD_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    if (T == 0) return check_memset(hipMemsetAsync(totals_dev, 0, kSums * sizeof(uint32_t), st));
    if ((V && !vertices) || !triangles || !slot || !order) return PVD_ERR_INVALID;
    if (!workspace || ((uintptr_t)workspace & 15u) || workspace_bytes < sums_bytes(T)) return PVD_ERR_INVALID;
    int rc;
    const uint32_t NB = div_up(T, kThreads);
    uint32_t *bsum = (uint32_t *)workspace;  // [6][NB]
    PVD_AX_LAUNCH(k_ax_classify, NB, kThreads, vertices, V, triangles, T, rho2, max_class, NB, slot, bsum);
    PVD_AX_LAUNCH(k_ax_scan, 1, kScanThreads, bsum, NB, totals_dev);
    PVD_AX_LAUNCH(k_ax_slots, NB, kThreads, T, NB, (const uint32_t *)bsum, (const uint32_t *)totals_dev, slot, order);
    return PVD_OK;
}

int pvd_mesh_atex_layout(const uint32_t counts[5], uint32_t out[]) {
    if (!counts || !out) return PVD_ERR_INVALID;
    AtexLayout l;
    const int rc = layout_of(counts, l);
    if (rc != PVD_OK) return rc;
    out[0] = l.Wt;
    out[1] = l.Ht;
    for (int c = 0; c < kClasses; ++c) {
        out[2 + c] = l.y0[c];
        out[2 + kClasses + c] = l.rows[c];
        out[2 + 2 * kClasses + c] = l.C[c];
    }
    return PVD_OK;
}

int pvd_mesh_atex_points(const float *vertices, uint32_t V, const int32_t *triangles, uint32_t T, const float *normals,
                         const uint32_t counts[5], const uint32_t *order, uint32_t row0, uint32_t row1, float *x, float *n,
                         pvd_stream_t stream) {
    AtexLayout l;
    const int rc = layout_for(counts, T, l);
    if (rc != PVD_OK) return rc;
    if (row0 > row1 || row1 > l.Ht) return PVD_ERR_INVALID;
    if (row0 == row1) return PVD_OK;
    if ((T && (!triangles || !order)) || (T && V && !vertices) || !x || !n) return PVD_ERR_INVALID;
    // rows of a band: at most 16384, below the limit of 65535 on gridDim.y
    hipLaunchKernelGGL(k_ax_points, dim3(div_up(l.Wt, kThreads), row1 - row0), dim3(kThreads), 0, (hipStream_t)stream, vertices, V, triangles,
                       T, normals, order, l, row0, (F3 *)x, (F3 *)n);
    return check_launch();
}

int pvd_mesh_atex_sample(const float *texture, uint32_t T, const uint32_t counts[5], const uint32_t *slot, const int32_t *tri,
                         const float *bary, uint32_t N, const float *bg3, float *color, pvd_stream_t stream) {
    AtexLayout l;
    const int rc = layout_for(counts, T, l);
    if (rc != PVD_OK) return rc;
    if (N == 0) return PVD_OK;
    if (!texture || (T && !slot) || !tri || !bary || !bg3 || !color) return PVD_ERR_INVALID;
    hipLaunchKernelGGL(k_ax_sample, dim3(div_up(N, kThreads)), dim3(kThreads), 0, (hipStream_t)stream, (const F3 *)texture, T, slot, l, tri,
                       bary, N, bg3, (F3 *)color);
    return check_launch();
}

}  // extern "C"
