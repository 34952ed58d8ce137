// mesh_tex.hip -- a per-triangle texture atlas in closed form (include/pvd_hip_mesh_tex.h): the surface point and normal of every texel,
// and the bilinear lookup of a baked texture at the (tri, bary) of a ray cast.
//
// k_mt_points    one lane per texel of a band of image rows, consecutive lanes along x (blockIdx.y is the row): the owner from integer
//                arithmetic, its three indices and corners (the lanes of a cell share them: one cache line per wave and corner), the
//                weights, six floats out as two 12-byte stores.  A pure store stream of 24 B per texel.  No LDS, no atomics.
// k_mt_sample    one lane per ray: four 12-byte gathers out of the triangle's own cell (their addresses and the bilinear mix:
//                csrc/mesh_atlas.h, shared with csrc/mesh_shtex.hip).  No LDS, no atomics.
// Every float operation is a single float32 one in the order of the header; nothing is fused (the build's -ffp-contract=off, and the
// pragma below for a build without it).
#include "mesh_atlas.h"

#include "../../include/pvd_hip_mesh_tex.h"

namespace {

using namespace pvd;
using namespace pvd::atlas;

constexpr int kThreads = 256;

struct TexLayout {
    uint32_t C, rows, Wt, Ht;
};

// the layout of the header, or PVD_ERR_UNSUPPORTED
int layout_of(uint32_t T, uint32_t S, TexLayout &l) {
    if (S < PVD_MESH_TEX_MIN_S || S > PVD_MESH_TEX_MAX_S) return PVD_ERR_UNSUPPORTED;
    const uint64_t cells = (uint64_t)(T / 2u) + (T & 1u);
    uint64_t C = 1;
    // the smallest C >= 1 with C * C >= cells, in integers: a bisection over 1 .. 2^16 (cells < 2^32)
    uint64_t lo = 1, hi = 65536;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) / 2;
        if (mid * mid >= cells)
            hi = mid;
        else
            lo = mid + 1;
    }
    C = lo;
    const uint64_t rows = cells ? (cells + C - 1) / C : 1;
    if (C * S > PVD_MESH_TEX_MAX_SIDE || rows * S > PVD_MESH_TEX_MAX_SIDE) return PVD_ERR_UNSUPPORTED;
    l.C = (uint32_t)C;
    l.rows = (uint32_t)rows;
    l.Wt = (uint32_t)(C * S);
    l.Ht = (uint32_t)(rows * S);
    return PVD_OK;
}

__global__ __launch_bounds__(kThreads) void k_mt_points(const float *__restrict__ vertices, uint32_t V, const int32_t *__restrict__ triangles,
                                                       uint32_t T, const float *__restrict__ normals, uint32_t S, uint32_t C, uint32_t Wt,
                                                       uint32_t row0, F3 *__restrict__ out_x, F3 *__restrict__ out_n) {
#pragma clang fp contract(off)
    const uint32_t x = blockIdx.x * kThreads + threadIdx.x;
    if (x >= Wt) return;
    const uint32_t r = blockIdx.y, y = row0 + r;
    const uint32_t cx = x / S, cy = y / S, i = x - cx * S, j = y - cy * S;
    const uint32_t k = cy * C + cx;  // < C * C <= 2^24
    const bool lower = i + j <= S - 1;
    const uint32_t f = 2u * k + (lower ? 0u : 1u);
    const uint32_t p = lower ? i : S - 1 - i, q = lower ? j : S - 1 - j;
    const float nan = u2f(0x7fc00000u);
    F3 X = {nan, nan, nan}, N = {nan, nan, nan};
    if (f < T) texel_point(vertices, V, triangles, normals, f, p, q, S, X, N);  // csrc/mesh_atlas.h
    const size_t e = (size_t)r * Wt + x;  // inside the band: r < row1 - row0, x < Wt
    out_x[e] = X;
    out_n[e] = N;
}

__global__ __launch_bounds__(kThreads) void k_mt_sample(const F3 *__restrict__ texture, uint32_t T, uint32_t S, uint32_t C, uint32_t Wt,
                                                       const int32_t *__restrict__ tri, const float *__restrict__ bary, uint32_t N,
                                                       const float *__restrict__ bg3, F3 *__restrict__ color) {
#pragma clang fp contract(off)
    const uint32_t r = blockIdx.x * kThreads + threadIdx.x;
    if (r >= N) return;
    const int32_t f = tri[r];
    F3 out = {bg3[0], bg3[1], bg3[2]};
    if (f >= 0 && (uint32_t)f < T) {
        const float beta = bary[2 * (size_t)r], gamma = bary[2 * (size_t)r + 1];
        const Footprint p = footprint_of((uint32_t)f, beta, gamma, S, C);
        out = blend(texture[(size_t)p.ya * Wt + p.xa], texture[(size_t)p.ya * Wt + p.xb], texture[(size_t)p.yb * Wt + p.xa],
                    texture[(size_t)p.yb * Wt + p.xb], p);
    }
    color[r] = out;
}

}  // namespace

extern "C" {

int pvd_mesh_tex_layout(uint32_t T, uint32_t S, uint32_t out[4]) {
    if (!out) return PVD_ERR_INVALID;
    TexLayout l;
    const int rc = layout_of(T, S, l);
    if (rc != PVD_OK) return rc;
    out[0] = l.C;
    out[1] = l.rows;
    out[2] = l.Wt;
    out[3] = l.Ht;
    return PVD_OK;
}

int pvd_mesh_tex_points(const float *vertices, uint32_t V, const int32_t *triangles, uint32_t T, const float *normals, uint32_t S,
                        uint32_t row0, uint32_t row1, float *x, float *n, pvd_stream_t stream) {
    TexLayout l;
    const int rc = layout_of(T, S, l);
    if (rc != PVD_OK) return rc;
    if (row0 > row1 || row1 > l.Ht) return PVD_ERR_INVALID;
    if (row0 == row1) return PVD_OK;
    if ((T && !triangles) || (T && V && !vertices) || !x || !n) return PVD_ERR_INVALID;
    // rows of a band: at most 16384, below the limit of 65535 on gridDim.y
    hipLaunchKernelGGL(k_mt_points, dim3(div_up(l.Wt, kThreads), row1 - row0), dim3(kThreads), 0, (hipStream_t)stream, vertices, V, triangles,
                       T, normals, S, l.C, l.Wt, row0, (F3 *)x, (F3 *)n);
    return check_launch();
}

int pvd_mesh_tex_sample(const float *texture, uint32_t T, uint32_t S, const int32_t *tri, const float *bary, uint32_t N, const float *bg3,
                        float *color, pvd_stream_t stream) {
    TexLayout l;
    const int rc = layout_of(T, S, l);
    if (rc != PVD_OK) return rc;
    if (N == 0) return PVD_OK;
    if (!texture || !tri || !bary || !bg3 || !color) return PVD_ERR_INVALID;
    hipLaunchKernelGGL(k_mt_sample, dim3(div_up(N, kThreads)), dim3(kThreads), 0, (hipStream_t)stream, (const F3 *)texture, T, S, l.C, l.Wt, tri,
                       bary, N, bg3, (F3 *)color);
    return check_launch();
}

}  // extern "C"
