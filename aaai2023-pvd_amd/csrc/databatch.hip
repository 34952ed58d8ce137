// databatch.hip -- training batches drawn on the device from a resident uint8 image stack (include/pvd_hip_data.h).
//
// reference: NeRFDataset.collate, distill_mutual/provider.py:278-308 -> get_rays with its error_map branch
// (distill_mutual/utils.py:324-404, :357-381), the random background and alpha blend of train_step (utils.py:987-995) and the
// error-map feedback at its end (utils.py:1120-1129): ~20 elementwise launches, two gathers and a multinomial per step.
//
// k_draw_cells    (error-map mode) ONE workgroup of 1024 lanes draws N distinct cells of the view's row by the exponential race:
//                 lane t owns cells 16 t .. 16 t + 15 and keeps their keys in registers; the N-th largest key is found by a radix
//                 select on the key bits (four passes over 8-bit digits, one 256-bin histogram in LDS), the winners are written in
//                 ascending cell order through a prefix scan over the lanes.  LDS: 1 KB of histogram + a few words.
// k_image_batch   one lane per ray: pixel id (uniform, or the jittered pixel of its cell), the pixel's bytes, blend, ray, near/far.
//                 The last workgroup to finish advances the state, as k_make_ray_batch does; k_draw_cells only reads it.
// k_error_update  one lane per ray: the EMA of the squared error into the ray's cell.
#include "rays.h"

#include "../../include/pvd_hip_data.h"

namespace {

using namespace pvd;

constexpr uint32_t kBlock = 256;
constexpr uint32_t kDrawLanes = 1024;
constexpr uint32_t kDrawWaves = kDrawLanes / kWave;
constexpr uint32_t kPerLane = 16;  // kDrawLanes * kPerLane = PVD_DATA_MAX_GRID^2
static_assert(kDrawLanes * kPerLane == PVD_DATA_MAX_GRID * PVD_DATA_MAX_GRID, "one key per cell of the largest grid");
constexpr uint64_t kGolden = 0x9E3779B97F4A7C15ull;

__device__ __forceinline__ uint32_t view_of(const int32_t *__restrict__ order, long long pos, uint32_t V) {
    const uint32_t p = (uint32_t)((unsigned long long)pos % V);
    return order ? (uint32_t)order[p] % V : p;  // (% V: an order the caller filled wrongly must not send a load out of the stack)
}

// inclusive scan over the wave
__device__ __forceinline__ uint32_t wave_scan(uint32_t v, uint32_t lane) {
#pragma unroll
    for (uint32_t o = 1; o < (uint32_t)kWave; o <<= 1) {
        const uint32_t u = __shfl_up(v, o, kWave);
        if (lane >= o) v += u;
    }
    return v;
}

__global__ void __launch_bounds__(kDrawLanes) k_draw_cells(const float *__restrict__ error_map, const int32_t *__restrict__ order,
                                                           uint32_t V, const long long *__restrict__ state, uint64_t seed, uint32_t G,
                                                           uint32_t N, int64_t *__restrict__ inds_coarse, float *__restrict__ keys_out) {
    __shared__ uint32_t hist[256];
    __shared__ uint32_t wave_tot[kDrawWaves];
    __shared__ uint32_t s_digit, s_above;
    const uint32_t t = threadIdx.x, lane = t & (kWave - 1), wave = t / kWave;
    const uint32_t view = view_of(order, state[0], V);
    const long long batch = state[1];
    const float *__restrict__ w = error_map + (size_t)view * G;
    const uint32_t c0 = t * kPerLane;
    if (t == 0) { s_digit = 0; s_above = 0; }

    // key + 1 as an unsigned word orders like the key (keys are >= 0 or +inf); 0 marks a cell past the grid
    uint32_t uk[kPerLane];
    Pcg32 rng;
    rng.seed(seed + kGolden * (uint64_t)(batch + 1), 2);
    rng.advance(c0);  // (cell c takes draw c of the stream)
#pragma unroll
    for (uint32_t i = 0; i < kPerLane; i++) {
        const uint32_t c = c0 + i;
        const float u = rng.next_float();
        uk[i] = 0;
        if (c < G) {
            const float wc = w[c];
            const float e = 0.0f - logf(1.0f - u);  // (not a negation: u == 0 gives e = +0 and the key +inf, not -inf)
            const float key = wc > 0.0f ? wc / e : 0.0f;
            if (keys_out) keys_out[c] = key;
            uk[i] = __float_as_uint(key) + 1u;
        }
    }

    // radix select: after the passes `prefix` is the N-th largest word and `want` of the words equal to it are taken
    uint32_t prefix = 0, mask = 0, want = N;
#pragma unroll 1
    for (int shift = 24; shift >= 0; shift -= 8) {
        if (t < 256) hist[t] = 0;
        __syncthreads();
#pragma unroll
        for (uint32_t i = 0; i < kPerLane; i++)
            if (uk[i] != 0 && (uk[i] & mask) == prefix) atomicAdd(&hist[(uk[i] >> shift) & 255u], 1u);
        __syncthreads();
        if (wave == 0) {
            // lane l holds bins 4 l .. 4 l + 3; suffix sums over the lanes find the bin the want-th largest word falls in
            const uint32_t h0 = hist[4 * lane], h1 = hist[4 * lane + 1], h2 = hist[4 * lane + 2], h3 = hist[4 * lane + 3];
            const uint32_t mine = h0 + h1 + h2 + h3;
            uint32_t suf = mine;
#pragma unroll
            for (uint32_t o = 1; o < (uint32_t)kWave; o <<= 1) {
                const uint32_t u = __shfl_down(suf, o, kWave);
                if (lane + o < (uint32_t)kWave) suf += u;
            }
            uint32_t above = suf - mine;  // words in the bins above this lane's
            if (above < want && want <= suf) {
                const uint32_t h[4] = {h0, h1, h2, h3};
                uint32_t d = 0;
#pragma unroll
                for (int b = 3; b >= 0; b--) {
                    if (above + h[b] >= want) { d = (uint32_t)b; break; }
                    above += h[b];
                }
                s_digit = 4 * lane + d;
                s_above = above;
            }
        }
        __syncthreads();
        prefix |= s_digit << shift;
        mask |= 255u << shift;
        want -= s_above;
    }

    // compaction in cell order: position of a winner = winners before it
    uint32_t n_gt = 0, n_eq = 0;
#pragma unroll
    for (uint32_t i = 0; i < kPerLane; i++) {
        n_gt += uk[i] > prefix;
        n_eq += uk[i] == prefix;
    }
    const uint32_t packed = n_gt | (n_eq << 16);  // (both <= 16384 over the whole workgroup)
    const uint32_t incl = wave_scan(packed, lane);
    if (lane == kWave - 1) wave_tot[wave] = incl;
    __syncthreads();
    uint32_t before = incl - packed;
    for (uint32_t k = 0; k < wave; k++) before += wave_tot[k];
    uint32_t gt_before = before & 0xffffu, eq_before = before >> 16;
#pragma unroll
    for (uint32_t i = 0; i < kPerLane; i++) {
        const bool gt = uk[i] > prefix, eq = uk[i] == prefix;
        if (gt || (eq && eq_before < want)) {
            const uint32_t pos = gt_before + (eq_before < want ? eq_before : want);
            if (pos < N) inds_coarse[pos] = (int64_t)(c0 + i);
        }
        gt_before += gt;
        eq_before += eq;
    }
}

template <int C>
__global__ void __launch_bounds__(kBlock) k_image_batch(const uint8_t *__restrict__ images, const float *__restrict__ poses,
                                                        const int32_t *__restrict__ order, uint32_t V, uint32_t H, uint32_t W,
                                                        long long *__restrict__ state, uint64_t seed, float fx, float fy, float cx,
                                                        float cy, uint32_t N, const float *__restrict__ aabb, float min_near,
                                                        uint32_t g, const int64_t *__restrict__ cells, int32_t *__restrict__ view_out,
                                                        int64_t *__restrict__ inds, float *__restrict__ rays_o, float *__restrict__ rays_d,
                                                        float *__restrict__ gt, float *__restrict__ bg, float *__restrict__ nears,
                                                        float *__restrict__ fars) {
    const uint32_t n = blockIdx.x * kBlock + threadIdx.x;
    const long long pos = state[0], batch = state[1];
    const uint32_t view = view_of(order, pos, V);
    if (n == 0) view_out[0] = (int32_t)view;
    if (n < N) {
        Pcg32 rng;
        rng.seed(seed + kGolden * (uint64_t)(batch + 1));
        rng.advance(8ull * n);
        const uint32_t d0 = rng.next();
        const float u1 = rng.next_float(), u2 = rng.next_float();
        int64_t k;
        if (cells) {
            // reference: get_rays' error_map branch, utils.py:357-381 (float32, every operation rounded)
            const uint32_t G = g * g;
            uint32_t c = (uint32_t)cells[n];
            if (c >= G) c = G - 1;
            const float sx = (float)((double)H / (double)g), sy = (float)((double)W / (double)g);
            const float fr = (float)(c / g) * sx + u1 * sx, fc = (float)(c % g) * sy + u2 * sy;
            int64_t row = (int64_t)fr, col = (int64_t)fc;
            if (row > (int64_t)H - 1) row = (int64_t)H - 1;
            if (col > (int64_t)W - 1) col = (int64_t)W - 1;
            k = row * (int64_t)W + col;
        } else {
            k = (int64_t)(((uint64_t)d0 * (uint64_t)(H * W)) >> 32);  // uniform in [0, H*W)
        }
        inds[n] = k;
        const uint8_t *__restrict__ px = images + ((size_t)view * H * W + (size_t)k) * C;
        const float r0 = (float)px[0] / 255.0f, r1 = (float)px[1] / 255.0f, r2 = (float)px[2] / 255.0f;
        float *__restrict__ out = gt + 3 * (size_t)n;
        if (C == 4) {
            // reference: training_target, utils.py:987-995: gt = rgb * a + bg * (1 - a)
            const float a = (float)px[3] / 255.0f, na = 1.0f - a;
            const float b0 = rng.next_float(), b1 = rng.next_float(), b2 = rng.next_float();
            bg[3 * (size_t)n] = b0; bg[3 * (size_t)n + 1] = b1; bg[3 * (size_t)n + 2] = b2;
            out[0] = r0 * a + b0 * na; out[1] = r1 * a + b1 * na; out[2] = r2 * a + b2 * na;
        } else {
            out[0] = r0; out[1] = r1; out[2] = r2;
        }
        float o[3], d[3];
        ray_of_pixel(poses + 16 * (size_t)view, fx, fy, cx, cy, k, W, o, d);
#pragma unroll
        for (int r = 0; r < 3; r++) { rays_o[3 * (size_t)n + r] = o[r]; rays_d[3 * (size_t)n + r] = d[r]; }
        near_far_of(o, d, aabb, min_near, nears[n], fars[n]);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        __threadfence();
        const unsigned long long done = atomicAdd(reinterpret_cast<unsigned long long *>(state + 2), 1ull);
        if (done == gridDim.x - 1) {  // every workgroup has read the state
            state[0] = (long long)(((unsigned long long)pos + 1ull) % V);
            state[1] = batch + 1;
            state[2] = 0;
        }
    }
}

// reference: train_step's error-map update, utils.py:1120-1129
__global__ void __launch_bounds__(kBlock) k_error_update(float *__restrict__ error_map, uint32_t G, const int32_t *__restrict__ view,
                                                         const int64_t *__restrict__ cells, const float *__restrict__ pred,
                                                         const float *__restrict__ gt, uint32_t N) {
    const uint32_t n = blockIdx.x * kBlock + threadIdx.x;
    if (n >= N) return;
    const int64_t c = cells[n];
    if (c < 0 || c >= (int64_t)G) return;
    const float d0 = pred[3 * (size_t)n] - gt[3 * (size_t)n], d1 = pred[3 * (size_t)n + 1] - gt[3 * (size_t)n + 1],
                d2 = pred[3 * (size_t)n + 2] - gt[3 * (size_t)n + 2];
    const float err = ((d0 * d0 + d1 * d1) + d2 * d2) / 3.0f;
    float *__restrict__ cell = error_map + (size_t)(uint32_t)view[0] * G + (size_t)c;
    *cell = 0.1f * *cell + 0.9f * err;
}

}  // namespace

#define PVD_REQUIRE(cond) \
    do { if (!(cond)) return PVD_ERR_INVALID; } while (0)

extern "C" {

int pvd_image_batch(const uint8_t *images, const float *poses, const int32_t *order, uint32_t V, uint32_t H, uint32_t W, uint32_t C,
                    int64_t *state, uint64_t seed, float fx, float fy, float cx, float cy, uint32_t N, const float *aabb,
                    float min_near, const float *error_map, uint32_t g, int32_t *view_out, int64_t *inds, int64_t *inds_coarse,
                    float *rays_o, float *rays_d, float *gt, float *bg, float *nears, float *fars, float *keys_out,
                    pvd_stream_t stream) {
    if (N == 0) return PVD_OK;
    PVD_REQUIRE(images && poses && state && aabb && view_out && inds && rays_o && rays_d && gt && nears && fars);
    PVD_REQUIRE(V > 0 && H > 0 && W > 0 && (uint64_t)H * W < (1ull << 32));
    PVD_REQUIRE((C == 3 || C == 4) && (C == 3 || bg));
    if (error_map) {
        if (g == 0 || g > PVD_DATA_MAX_GRID) return PVD_ERR_UNSUPPORTED;
        PVD_REQUIRE(inds_coarse && N <= g * g);
        hipLaunchKernelGGL(k_draw_cells, dim3(1), dim3(kDrawLanes), 0, (hipStream_t)stream, error_map, order, V, (const long long *)state,
                           seed, g * g, N, inds_coarse, keys_out);
        const int rc = check_launch();
        if (rc != PVD_OK) return rc;
    }
    const int64_t *cells = error_map ? inds_coarse : nullptr;
    if (C == 4)
        hipLaunchKernelGGL(k_image_batch<4>, dim3(div_up(N, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, images, poses, order, V, H, W,
                           (long long *)state, seed, fx, fy, cx, cy, N, aabb, min_near, g, cells, view_out, inds, rays_o, rays_d, gt, bg,
                           nears, fars);
    else
        hipLaunchKernelGGL(k_image_batch<3>, dim3(div_up(N, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, images, poses, order, V, H, W,
                           (long long *)state, seed, fx, fy, cx, cy, N, aabb, min_near, g, cells, view_out, inds, rays_o, rays_d, gt, bg,
                           nears, fars);
    return check_launch();
}

int pvd_error_map_update(float *error_map, uint32_t g, const int32_t *view, const int64_t *inds_coarse, const float *pred,
                         const float *gt, uint32_t N, pvd_stream_t stream) {
    if (N == 0) return PVD_OK;
    PVD_REQUIRE(error_map && view && inds_coarse && pred && gt && g > 0);
    hipLaunchKernelGGL(k_error_update, dim3(div_up(N, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, error_map, g * g, view, inds_coarse,
                       pred, gt, N);
    return check_launch();
}

}  // extern "C"
