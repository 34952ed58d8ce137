// mesh_shtex.hip -- a view-dependent texture atlas (pvd_hip_mesh_shtex.h): K = L * L spherical-harmonics coefficients per channel and
// texel on the atlas of include/pvd_hip_mesh_tex.h; the basis, the mirrored query directions of the bake, the projection of the
// queried colours onto the basis, and the lookup at the (tri, bary, dir) of a ray cast.
//
// k_st_basis<L>    one lane per direction: three loads, K stores of one row.
// k_st_dirs        one lane per normal, consecutive lanes along M; the lane keeps n, s' inputs and q and runs through the J fitting
//                  directions (wave-uniform loads of U): one 12-byte store per direction, each of them along M.
// k_st_project<L>  one lane per texel: the K x 3 accumulators stay in registers through the J directions of the batch; rgb[j] is read
//                  as one 12-byte load per lane along M, the K entries of P's column are wave-uniform.  The lane then stores its own
//                  K * 12 contiguous bytes (and loads them first where the batch is not the first).
// k_st_sample<L>   ONE LANE PER RAY, as k_mt_sample (the four texels and the bilinear mix: csrc/mesh_atlas.h, shared with it): the lane
//                  evaluates the basis of its direction once (K registers) and folds each of its four texels, K * 12 contiguous
//                  bytes (192 at L = 4, moved as wide loads), into three numbers as they arrive.
//                  Several lanes per ray would put the K-term sums, which the header orders, across lanes and buy nothing that
//                  neighbouring rays of a wave -- which hit the same and neighbouring cells -- do not already share in the cache;
//                  profiles/mesh_shtex.txt has the measured time next to a copy of the bytes the hits touch.
// No LDS, no atomics.  Every float operation is a single float32 one in the order of the header; nothing is fused (the build's
// -ffp-contract=off, and the pragma below for a build without it).
#include "mesh_atlas.h"

#include "pvd_hip_mesh_shtex.h"

namespace {

using namespace pvd;
using namespace pvd::atlas;

constexpr int kThreads = 256;

template <int L>
struct __attribute__((packed, aligned(4))) Texel {  // the K x 3 floats of a texel, moved as wide accesses
    float v[3 * L * L];
};

// Y[0 .. L*L) of the header, operation for operation
template <int L>
__device__ __forceinline__ void sh_basis(float x, float y, float z, float (&Y)[L * L]) {
#pragma clang fp contract(off)
    Y[0] = 0.282094806f;
    if constexpr (L > 1) {
        Y[1] = -0.488602519f * y;
        Y[2] = 0.488602519f * z;
        Y[3] = -0.488602519f * x;
    }
    if constexpr (L > 2) {
        const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
        Y[4] = 1.09254849f * xy;
        Y[5] = -1.09254849f * yz;
        Y[6] = 0.946174681f * zz - 0.31539157f;
        Y[7] = -1.09254849f * xz;
        Y[8] = 0.546274245f * (xx - yy);
        if constexpr (L > 3) {
            Y[9] = -0.590043604f * (y * (3.0f * xx - yy));
            Y[10] = 2.89061141f * (xy * z);
            Y[11] = (0.457045794f - 2.28522897f * zz) * y;
            Y[12] = (1.86588168f * zz - 1.11952901f) * z;
            Y[13] = (0.457045794f - 2.28522897f * zz) * x;
            Y[14] = 1.44530571f * (z * (xx - yy));
            Y[15] = -0.590043604f * (x * (xx - 3.0f * yy));
        }
    }
}

template <int L>
__global__ __launch_bounds__(kThreads) void k_st_basis(const F3 *__restrict__ dirs, uint32_t N, float *__restrict__ out) {
    constexpr int K = L * L;
    const uint32_t r = blockIdx.x * kThreads + threadIdx.x;
    if (r >= N) return;
    const F3 d = dirs[r];
    float Y[K];
    sh_basis<L>(d.x, d.y, d.z, Y);
#pragma unroll
    for (int k = 0; k < K; ++k) out[(size_t)r * K + k] = Y[k];
}

__global__ __launch_bounds__(kThreads) void k_st_dirs(const F3 *__restrict__ n, uint32_t M, const float *__restrict__ U, uint32_t J,
                                                     F3 *__restrict__ d) {
#pragma clang fp contract(off)
    const uint32_t t = blockIdx.x * kThreads + threadIdx.x;
    if (t >= M) return;
    const F3 nn = n[t];
    const float q = (nn.x * nn.x + nn.y * nn.y) + nn.z * nn.z;
    const bool q_ok = q > 0.0f && q <= 3.402823466e+38f;  // finite and positive; false for a NaN
    for (uint32_t j = 0; j < J; ++j) {
        const float ux = U[3 * (size_t)j], uy = U[3 * (size_t)j + 1], uz = U[3 * (size_t)j + 2];
        const float s = (ux * nn.x + uy * nn.y) + uz * nn.z;
        F3 o = {ux, uy, uz};
        if (s > 0.0f && q_ok) {
            const float r = (2.0f * s) / q;
            o.x = ux - r * nn.x;
            o.y = uy - r * nn.y;
            o.z = uz - r * nn.z;
        }
        d[(size_t)j * M + t] = o;
    }
}

template <int L>
__global__ __launch_bounds__(kThreads) void k_st_project(const F3 *__restrict__ rgb, const float *__restrict__ Pcols, uint32_t J, uint32_t M,
                                                        Texel<L> *__restrict__ coef, uint32_t first) {
#pragma clang fp contract(off)
    constexpr int K = L * L;
    const uint32_t t = blockIdx.x * kThreads + threadIdx.x;
    if (t >= M) return;
    Texel<L> acc;
    if (first) {
#pragma unroll
        for (int e = 0; e < 3 * K; ++e) acc.v[e] = 0.0f;
    } else {
        acc = coef[t];
    }
    for (uint32_t j = 0; j < J; ++j) {
        const F3 c = rgb[(size_t)j * M + t];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const float p = Pcols[(size_t)k * J + j];
            acc.v[3 * k] = acc.v[3 * k] + p * c.x;
            acc.v[3 * k + 1] = acc.v[3 * k + 1] + p * c.y;
            acc.v[3 * k + 2] = acc.v[3 * k + 2] + p * c.z;
        }
    }
    coef[t] = acc;
}

// the K-term sum of one texel and channel, k ascending
template <int L>
__device__ __forceinline__ F3 fold(const Texel<L> &c, const float (&Y)[L * L]) {
#pragma clang fp contract(off)
    F3 o = {c.v[0] * Y[0], c.v[1] * Y[0], c.v[2] * Y[0]};
#pragma unroll
    for (int k = 1; k < L * L; ++k) {
        o.x = o.x + c.v[3 * k] * Y[k];
        o.y = o.y + c.v[3 * k + 1] * Y[k];
        o.z = o.z + c.v[3 * k + 2] * Y[k];
    }
    return o;
}

__device__ __forceinline__ float unit_clamp(float c) { return fminf(fmaxf(c, 0.0f), 1.0f); }  // fmaxf(NaN, 0) = 0

template <int L>
__global__ __launch_bounds__(kThreads) void k_st_sample(const Texel<L> *__restrict__ texture, uint32_t T, uint32_t S, uint32_t C, uint32_t Wt,
                                                       const int32_t *__restrict__ tri, const float *__restrict__ bary,
                                                       const F3 *__restrict__ dirs, uint32_t N, const float *__restrict__ bg3,
                                                       F3 *__restrict__ color) {
#pragma clang fp contract(off)
    const uint32_t r = blockIdx.x * kThreads + threadIdx.x;
    if (r >= N) return;
    const int32_t f = tri[r];
    F3 out = {bg3[0], bg3[1], bg3[2]};
    if (f >= 0 && (uint32_t)f < T) {
        const float beta = bary[2 * (size_t)r], gamma = bary[2 * (size_t)r + 1];
        const Footprint p = footprint_of((uint32_t)f, beta, gamma, S, C);
        const F3 d = dirs[r];
        float Y[L * L];
        sh_basis<L>(d.x, d.y, d.z, Y);
        out = blend(fold<L>(texture[(size_t)p.ya * Wt + p.xa], Y), fold<L>(texture[(size_t)p.ya * Wt + p.xb], Y),
                    fold<L>(texture[(size_t)p.yb * Wt + p.xa], Y), fold<L>(texture[(size_t)p.yb * Wt + p.xb], Y), p);
        out = {unit_clamp(out.x), unit_clamp(out.y), unit_clamp(out.z)};
    }
    color[r] = out;
}

bool bands_ok(uint32_t L) { return L >= 1 && L <= PVD_MESH_SHTEX_MAX_L; }

}  // namespace

extern "C" {

int pvd_mesh_shtex_basis(const float *dirs, uint32_t N, uint32_t L, float *out, pvd_stream_t stream) {
    if (!bands_ok(L)) return PVD_ERR_UNSUPPORTED;
    if (N == 0) return PVD_OK;
    if (!dirs || !out) return PVD_ERR_INVALID;
    const dim3 grid(div_up(N, kThreads)), block(kThreads);
    const hipStream_t st = (hipStream_t)stream;
    switch (L) {
        case 1: hipLaunchKernelGGL(k_st_basis<1>, grid, block, 0, st, (const F3 *)dirs, N, out); break;
        case 2: hipLaunchKernelGGL(k_st_basis<2>, grid, block, 0, st, (const F3 *)dirs, N, out); break;
        case 3: hipLaunchKernelGGL(k_st_basis<3>, grid, block, 0, st, (const F3 *)dirs, N, out); break;
        default: hipLaunchKernelGGL(k_st_basis<4>, grid, block, 0, st, (const F3 *)dirs, N, out); break;
    }
    return check_launch();
}

int pvd_mesh_shtex_dirs(const float *n, uint32_t M, const float *U, uint32_t J, float *d, pvd_stream_t stream) {
    if (M == 0 || J == 0) return PVD_OK;
    if (!n || !U || !d) return PVD_ERR_INVALID;
    hipLaunchKernelGGL(k_st_dirs, dim3(div_up(M, kThreads)), dim3(kThreads), 0, (hipStream_t)stream, (const F3 *)n, M, U, J, (F3 *)d);
    return check_launch();
}

int pvd_mesh_shtex_project(const float *rgb, const float *Pcols, uint32_t L, uint32_t J, uint32_t M, float *coef, uint32_t first,
                           pvd_stream_t stream) {
    if (!bands_ok(L)) return PVD_ERR_UNSUPPORTED;
    if (M == 0 || J == 0) return PVD_OK;
    if (!rgb || !Pcols || !coef) return PVD_ERR_INVALID;
    const dim3 grid(div_up(M, kThreads)), block(kThreads);
    const hipStream_t st = (hipStream_t)stream;
    const F3 *c = (const F3 *)rgb;
    switch (L) {
        case 1: hipLaunchKernelGGL(k_st_project<1>, grid, block, 0, st, c, Pcols, J, M, (Texel<1> *)coef, first); break;
        case 2: hipLaunchKernelGGL(k_st_project<2>, grid, block, 0, st, c, Pcols, J, M, (Texel<2> *)coef, first); break;
        case 3: hipLaunchKernelGGL(k_st_project<3>, grid, block, 0, st, c, Pcols, J, M, (Texel<3> *)coef, first); break;
        default: hipLaunchKernelGGL(k_st_project<4>, grid, block, 0, st, c, Pcols, J, M, (Texel<4> *)coef, first); break;
    }
    return check_launch();
}

int pvd_mesh_shtex_sample(const float *texture, uint32_t T, uint32_t S, uint32_t L, const int32_t *tri, const float *bary,
                          const float *dirs, uint32_t N, const float *bg3, float *color, pvd_stream_t stream) {
    uint32_t lay[4];  // (C, rows, Wt, Ht)
    const int rc = pvd_mesh_tex_layout(T, S, lay);
    if (rc != PVD_OK) return rc;
    if (!bands_ok(L)) return PVD_ERR_UNSUPPORTED;
    if (N == 0) return PVD_OK;
    if (!texture || !tri || !bary || !dirs || !bg3 || !color) return PVD_ERR_INVALID;
    const dim3 grid(div_up(N, kThreads)), block(kThreads);
    const hipStream_t st = (hipStream_t)stream;
    const F3 *d = (const F3 *)dirs;
    F3 *o = (F3 *)color;
    switch (L) {
        case 1: hipLaunchKernelGGL(k_st_sample<1>, grid, block, 0, st, (const Texel<1> *)texture, T, S, lay[0], lay[2], tri, bary, d, N, bg3, o); break;
        case 2: hipLaunchKernelGGL(k_st_sample<2>, grid, block, 0, st, (const Texel<2> *)texture, T, S, lay[0], lay[2], tri, bary, d, N, bg3, o); break;
        case 3: hipLaunchKernelGGL(k_st_sample<3>, grid, block, 0, st, (const Texel<3> *)texture, T, S, lay[0], lay[2], tri, bary, d, N, bg3, o); break;
        default: hipLaunchKernelGGL(k_st_sample<4>, grid, block, 0, st, (const Texel<4> *)texture, T, S, lay[0], lay[2], tri, bary, d, N, bg3, o); break;
    }
    return check_launch();
}

}  // extern "C"
