// metrics.hip -- SSIM + mean squared error of image pairs in one fused pass (include/pvd_hip_metrics.h).
//
// reference: compute_ssim, distill_mutual/utils.py:219-300 (10 depthwise conv2d + ~25 elementwise launches and, in
// Trainer.evaluate, two .item() read-backs for max_val per view) and PSNRMeter.update, utils.py:491-529.
//
// k_metrics_max    (only for max_val <= 0) up to 256 workgroups, one partial maximum over both batches each, into the workspace.
// k_ssim<FS>       one workgroup of 256 threads per (image, 32 x 32 output tile), looping over the channels.  Per channel the tile
//                  and its FS - 1 halo of both images go to LDS (zeros outside the image), the five moments are blurred along W
//                  out of LDS into LDS (8 outputs per thread from a sliding register window), then along H in registers (4
//                  outputs per thread), and the pixel formula runs in registers.  LDS per workgroup at FS = 15: 2 x 46 x 47 x 4 B
//                  of pixels + 5 x 46 x 33 x 4 B of row-blurred moments = 47.7 KB, i.e. three workgroups per CU.  Row pitches are
//                  odd (47 / 33 floats), which puts the 8-output segments of the W pass on distinct banks.
// k_metrics_final  one workgroup per image adds that image's per-tile partial sums in a fixed order, in double.
// No float atomics: the result does not depend on the order in which workgroups run.
#include "pvd_device.h"

#include "../../include/pvd_hip_metrics.h"

namespace {

using namespace pvd;

constexpr int kTile = PVD_METRICS_TILE;
constexpr int kMaxFilter = PVD_METRICS_MAX_FILTER;
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr uint32_t kWsHeader = 4;       // [0] max_val used, [1..3] unused
constexpr uint32_t kMaxPartials = 256;  // partial maxima, at workspace[kWsHeader ..]
constexpr uint32_t kWsSums = kWsHeader + kMaxPartials;

struct Taps {
    float w[kMaxFilter];
};

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_down(v, o, kWave);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) v = fmaxf(v, __shfl_down(v, o, kWave));
    return v;
}

// max over the workgroup, returned to every thread (red: kWaves floats of LDS)
__device__ __forceinline__ float block_max(float v, float *red) {
    v = wave_max(v);
    if ((threadIdx.x & (kWave - 1)) == 0) red[threadIdx.x / kWave] = v;
    __syncthreads();
    float m = red[0];
#pragma unroll
    for (int i = 1; i < kWaves; ++i) m = fmaxf(m, red[i]);
    __syncthreads();
    return m;
}

// n4 float4 + the floats from 4 n4 to n of each image (n4 = 0 when a pointer is not 16-byte aligned)
__global__ __launch_bounds__(kThreads) void k_metrics_max(const float *__restrict__ img0, const float *__restrict__ img1, uint64_t n,
                                                         uint64_t n4, float *__restrict__ ws) {
    __shared__ float red[kWaves];
    float m = -INFINITY;
    const uint64_t stride = (uint64_t)gridDim.x * kThreads;
    const uint64_t first = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    for (int k = 0; k < 2; ++k) {
        const float *img = k ? img1 : img0;
        const float4 *v4 = reinterpret_cast<const float4 *>(img);
        for (uint64_t i = first; i < n4; i += stride) {
            const float4 v = v4[i];
            m = fmaxf(fmaxf(m, fmaxf(v.x, v.y)), fmaxf(v.z, v.w));
        }
        for (uint64_t i = 4 * n4 + first; i < n; i += stride) m = fmaxf(m, img[i]);
    }
    m = block_max(m, red);
    if (threadIdx.x == 0) ws[kWsHeader + blockIdx.x] = m;
}

template <int FS>
__global__ __launch_bounds__(kThreads) void k_ssim(const float *__restrict__ img0, const float *__restrict__ img1, uint32_t H, uint32_t W,
                                                   uint32_t C, uint32_t tiles_x, uint32_t ntiles, Taps taps, float k1, float k2,
                                                   float max_val, uint32_t n_max_partials, float *__restrict__ ws,
                                                   float *__restrict__ ssim_map) {
    constexpr int HALF = FS / 2;
    constexpr int TH = kTile + FS - 1;  // staged rows and columns
    constexpr int PITCH = TH | 1;       // odd: the W pass's (row, 8-column segment) starts fall on distinct banks
    constexpr int RBP = kTile + 1;      // odd as well, for the W pass's stores
    constexpr int SEG = 8;              // outputs per thread in the W pass
    constexpr int NSEG = kTile / SEG;
    constexpr int ROWS = 4;             // outputs per thread in the H pass (kThreads / kTile = 8 row groups of 4)
    static_assert(TH * NSEG <= kThreads, "the W pass is one round");
    static_assert((kThreads / kTile) * ROWS == kTile, "the H pass covers the tile");

    __shared__ float s_img[2][TH * PITCH];
    __shared__ float s_rb[5][TH * RBP];
    __shared__ float s_red[2][kWaves];

    const uint32_t t = threadIdx.x;
    const uint32_t b = blockIdx.x / ntiles;
    const uint32_t tile = blockIdx.x - b * ntiles;
    const int y0 = (int)(tile / tiles_x) * kTile, x0 = (int)(tile % tiles_x) * kTile;

    if (n_max_partials) max_val = block_max(t < n_max_partials ? ws[kWsHeader + t] : -INFINITY, s_red[0]);
    if (blockIdx.x == 0 && t == 0) ws[0] = max_val;
    const float c1 = (k1 * max_val) * (k1 * max_val), c2 = (k2 * max_val) * (k2 * max_val);

    float sum_map = 0.0f, sum_sq = 0.0f;
    for (uint32_t c = 0; c < C; ++c) {
        // ---- stage the tile + halo of both images, zeros outside
        for (int i = (int)t; i < TH * TH; i += kThreads) {
            const int r = i / TH, col = i - r * TH;
            const int gy = y0 - HALF + r, gx = x0 - HALF + col;
            float a = 0.0f, v = 0.0f;
            if (gy >= 0 && gy < (int)H && gx >= 0 && gx < (int)W) {
                const size_t idx = (((size_t)b * H + (uint32_t)gy) * W + (uint32_t)gx) * C + c;
                a = img0[idx];
                v = img1[idx];
            }
            s_img[0][r * PITCH + col] = a;
            s_img[1][r * PITCH + col] = v;
        }
        __syncthreads();

        // ---- blur along W: thread (row r, segment s) -> 8 outputs of each of the five moments
        if (t < TH * NSEG) {
            const int r = (int)t / NSEG, s = (int)t % NSEG;
            float a[SEG + FS - 1], v[SEG + FS - 1];
#pragma unroll
            for (int j = 0; j < SEG + FS - 1; ++j) {
                a[j] = s_img[0][r * PITCH + s * SEG + j];
                v[j] = s_img[1][r * PITCH + s * SEG + j];
            }
#pragma unroll
            for (int m = 0; m < 5; ++m) {
                float p[SEG + FS - 1];
#pragma unroll
                for (int j = 0; j < SEG + FS - 1; ++j)
                    p[j] = m == 0 ? a[j] : m == 1 ? v[j] : m == 2 ? a[j] * a[j] : m == 3 ? v[j] * v[j] : a[j] * v[j];
#pragma unroll
                for (int j = 0; j < SEG; ++j) {
                    float acc = 0.0f;
#pragma unroll
                    for (int k = 0; k < FS; ++k) acc = fmaf(taps.w[k], p[j + k], acc);
                    s_rb[m][r * RBP + s * SEG + j] = acc;
                }
            }
        }
        __syncthreads();

        // ---- blur along H in registers: thread (column x, row group g) -> 4 pixels
        const int x = (int)t % kTile, g = (int)t / kTile;
        float mo[5][ROWS];
#pragma unroll
        for (int m = 0; m < 5; ++m) {
            float p[ROWS + FS - 1];
#pragma unroll
            for (int j = 0; j < ROWS + FS - 1; ++j) p[j] = s_rb[m][(g * ROWS + j) * RBP + x];
#pragma unroll
            for (int i = 0; i < ROWS; ++i) {
                float acc = 0.0f;
#pragma unroll
                for (int k = 0; k < FS; ++k) acc = fmaf(taps.w[k], p[i + k], acc);
                mo[m][i] = acc;
            }
        }
        // ---- the pixel formula, utils.py:279-298, operation by operation
        const int gx = x0 + x;
#pragma unroll
        for (int i = 0; i < ROWS; ++i) {
            const int gy = y0 + g * ROWS + i;
            if (gy < (int)H && gx < (int)W) {
                const float mu0 = mo[0][i], mu1 = mo[1][i];
                const float mu00 = mu0 * mu0, mu11 = mu1 * mu1, mu01 = mu0 * mu1;
                const float s00 = fmaxf(mo[2][i] - mu00, 0.0f), s11 = fmaxf(mo[3][i] - mu11, 0.0f);
                float s01 = mo[4][i] - mu01;
                const float sgn = s01 > 0.0f ? 1.0f : s01 < 0.0f ? -1.0f : 0.0f;
                s01 = sgn * fminf(sqrtf(s00 * s11), fabsf(s01));
                const float numer = (2.0f * mu01 + c1) * (2.0f * s01 + c2);
                const float denom = (mu00 + mu11 + c1) * (s00 + s11 + c2);
                const float val = numer / denom;
                sum_map += val;
                if (ssim_map) ssim_map[(((size_t)b * H + (uint32_t)gy) * W + (uint32_t)gx) * C + c] = val;
                const int at = (HALF + g * ROWS + i) * PITCH + HALF + x;
                const float d = s_img[0][at] - s_img[1][at];
                sum_sq += d * d;
            }
        }
        __syncthreads();  // the next channel overwrites s_img / s_rb
    }

    // ---- one partial per (image, tile): wave, then workgroup, in a fixed order
    sum_map = wave_sum(sum_map);
    sum_sq = wave_sum(sum_sq);
    if ((t & (kWave - 1)) == 0) {
        s_red[0][t / kWave] = sum_map;
        s_red[1][t / kWave] = sum_sq;
    }
    __syncthreads();
    if (t == 0) {
        float a = s_red[0][0], q = s_red[1][0];
#pragma unroll
        for (int i = 1; i < kWaves; ++i) {
            a += s_red[0][i];
            q += s_red[1][i];
        }
        ws[kWsSums + 2 * (size_t)blockIdx.x] = a;
        ws[kWsSums + 2 * (size_t)blockIdx.x + 1] = q;
    }
}

__global__ __launch_bounds__(kThreads) void k_metrics_final(const float *__restrict__ ws, uint32_t ntiles, double count,
                                                           float *__restrict__ ssim, float *__restrict__ mse) {
    __shared__ double red[2][kThreads];
    const float *part = ws + kWsSums + 2 * (size_t)blockIdx.x * ntiles;
    double a = 0.0, q = 0.0;
    for (uint32_t i = threadIdx.x; i < ntiles; i += kThreads) {
        a += (double)part[2 * (size_t)i];
        q += (double)part[2 * (size_t)i + 1];
    }
    red[0][threadIdx.x] = a;
    red[1][threadIdx.x] = q;
    __syncthreads();
    for (int o = kThreads / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            red[0][threadIdx.x] += red[0][threadIdx.x + o];
            red[1][threadIdx.x] += red[1][threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        ssim[blockIdx.x] = (float)(red[0][0] / count);
        mse[blockIdx.x] = (float)(red[1][0] / count);
    }
}

template <int FS>
void launch_ssim(uint32_t grid, hipStream_t stream, const float *img0, const float *img1, uint32_t H, uint32_t W, uint32_t C, uint32_t tiles_x,
                 uint32_t ntiles, const Taps &taps, float k1, float k2, float max_val, uint32_t n_max_partials, float *ws, float *ssim_map) {
    hipLaunchKernelGGL(k_ssim<FS>, dim3(grid), dim3(kThreads), 0, stream, img0, img1, H, W, C, tiles_x, ntiles, taps, k1, k2, max_val,
                       n_max_partials, ws, ssim_map);
}

// tiles per image; 0 if B * tiles does not fit a launch
uint64_t tile_count(uint32_t B, uint32_t H, uint32_t W, uint32_t *tiles_x) {
    const uint64_t tx = ((uint64_t)W + kTile - 1) / kTile, ty = ((uint64_t)H + kTile - 1) / kTile;
    *tiles_x = (uint32_t)tx;
    const uint64_t n = tx * ty;
    return (n * B > 0x7fffffffull) ? 0 : n;
}

}  // namespace

extern "C" {

int pvd_image_metrics_workspace_floats(uint32_t B, uint32_t H, uint32_t W, uint32_t C) {
    (void)C;
    uint32_t tx;
    const uint64_t ntiles = tile_count(B, H, W, &tx);
    if (B && H && W && !ntiles) return PVD_ERR_UNSUPPORTED;
    const uint64_t n = kWsSums + 2 * ntiles * B;
    return n > 0x7fffffffull ? PVD_ERR_UNSUPPORTED : (int)n;
}

int pvd_image_metrics(const float *img0, const float *img1, uint32_t B, uint32_t H, uint32_t W, uint32_t C, const float *taps_host,
                      uint32_t filter_size, float k1, float k2, float max_val, float *workspace, float *ssim, float *mse, float *ssim_map,
                      pvd_stream_t stream) {
    if (B == 0) return PVD_OK;
    if (!img0 || !img1 || !taps_host || !workspace || !ssim || !mse || H == 0 || W == 0) return PVD_ERR_INVALID;
    if (C == 0 || C > 4 || (filter_size & 1u) == 0 || filter_size > (uint32_t)kMaxFilter) return PVD_ERR_UNSUPPORTED;
    if (H > 0x3fffffffu || W > 0x3fffffffu) return PVD_ERR_UNSUPPORTED;  // pixel coordinates are ints in the kernel
    uint32_t tiles_x;
    const uint64_t ntiles = tile_count(B, H, W, &tiles_x);
    if (!ntiles || pvd_image_metrics_workspace_floats(B, H, W, C) < 0) return PVD_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    Taps taps;
    for (uint32_t k = 0; k < (uint32_t)kMaxFilter; ++k) taps.w[k] = k < filter_size ? taps_host[k] : 0.0f;

    uint32_t n_max = 0;
    if (!(max_val > 0.0f)) {
        const uint64_t n = (uint64_t)B * H * W * C;
        const bool aligned = (((uintptr_t)img0 | (uintptr_t)img1) & 15u) == 0;
        const uint64_t n4 = aligned ? n / 4 : 0;
        const uint64_t work = aligned ? (n + 3) / 4 : n;
        uint64_t blocks = (work + kThreads - 1) / kThreads;
        n_max = (uint32_t)(blocks > kMaxPartials ? kMaxPartials : blocks);
        hipLaunchKernelGGL(k_metrics_max, dim3(n_max), dim3(kThreads), 0, st, img0, img1, n, n4, workspace);
        const int rc = check_launch();
        if (rc != PVD_OK) return rc;
    }
    const uint32_t grid = (uint32_t)(ntiles * B);
#define PVD_SSIM_CASE(FS)                                                                                                              \
    case FS:                                                                                                                           \
        launch_ssim<FS>(grid, st, img0, img1, H, W, C, tiles_x, (uint32_t)ntiles, taps, k1, k2, max_val, n_max, workspace, ssim_map); \
        break;
    switch (filter_size) {
        PVD_SSIM_CASE(1)
        PVD_SSIM_CASE(3)
        PVD_SSIM_CASE(5)
        PVD_SSIM_CASE(7)
        PVD_SSIM_CASE(9)
        PVD_SSIM_CASE(11)
        PVD_SSIM_CASE(13)
        PVD_SSIM_CASE(15)
        default:
            return PVD_ERR_UNSUPPORTED;
    }
#undef PVD_SSIM_CASE
    int rc = check_launch();
    if (rc != PVD_OK) return rc;
    hipLaunchKernelGGL(k_metrics_final, dim3(B), dim3(kThreads), 0, st, workspace, (uint32_t)ntiles, (double)H * W * C, ssim, mse);
    return check_launch();
}

}  // extern "C"
