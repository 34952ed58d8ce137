// mesh_tsdf.hip -- depth-map fusion into a truncated signed distance volume (pvd_hip_mesh_tsdf.h): the integration of V views into
// the accumulators of an R^3 lattice, the division that makes the field, and the trilinear colour lookup at mesh vertices.
//
// k_tsdf_integrate<COLOR, WEIGHT>   ONE LANE PER VOXEL, z fastest: a wave is 64 neighbours of a z column (or the end of one and the
//                  start of the next), so its accumulator loads and stores are contiguous, and the pixels its lanes gather from a view
//                  are neighbours on a short image segment.  The lane keeps p and its two (five with colour) accumulators in registers
//                  through the views of the call; v is uniform, so the sixteen numbers of a view's camera are scalar loads that the
//                  whole wave shares -- nothing is staged in LDS and the views are not chunked.  The accumulators are written back
//                  only where some view of the call reached the voxel.
// k_tsdf_finalize  one lane per voxel and pass of a grid-stride walk; the three totals: ballots per wave, summed in scalar registers over
//                  the walk, then one integer atomic per wave and total from lane 0.
// k_tsdf_sample    one lane per point: eight gathers of a weight and, where it is observed, of its three colour sums.
// Every float operation is a single float32 one in the order of the header; nothing is fused (the build's -ffp-contract=off, and the
// pragma below for a build without it).
#include "pvd_device.h"

#include "pvd_hip_mesh_tsdf.h"

namespace {

using namespace pvd;

constexpr int kThreads = 256;
constexpr float kFltMax = 3.402823466e+38f;
// The finalize pass walks the volume with at most this many workgroups (8 per CU): its three totals are same-address atomics, one per
// wave and total, and a wave per 64 voxels spent more time on them than on the volume (profiles/mesh_tsdf.txt).
constexpr uint32_t kFinalizeBlocks = 2048;

struct F3 {
    float x, y, z;
};

// coordinate n of an axis of the lattice (include/pvd_hip_mesh_winding.h, "Lattice")
__device__ __forceinline__ float lattice_coord(uint32_t n, float r1, float d, float lo) {
#pragma clang fp contract(off)
    const float f = (float)n / r1;
    const float g = f * d;
    return g + lo;
}

template <bool COLOR, bool WEIGHT>
__global__ __launch_bounds__(kThreads) void k_tsdf_integrate(const float *__restrict__ depth, const F3 *__restrict__ color,
                                                            const float *__restrict__ weight, const float *__restrict__ poses,
                                                            const float *__restrict__ intrinsics, uint32_t V, uint32_t H, uint32_t W,
                                                            uint32_t R, uint32_t voxels, const float *__restrict__ bmin3,
                                                            const float *__restrict__ bmax3, float tau, float *__restrict__ acc_d,
                                                            float *__restrict__ acc_w, F3 *__restrict__ acc_c) {
#pragma clang fp contract(off)
    const uint32_t n = blockIdx.x * kThreads + threadIdx.x;
    if (n >= voxels) return;
    const uint32_t k = n % R, ij = n / R, j = ij % R, i = ij / R;
    const float r1 = (float)(R - 1);
    const float lo_x = bmin3[0], lo_y = bmin3[1], lo_z = bmin3[2];
    const float px = lattice_coord(i, r1, bmax3[0] - lo_x, lo_x);
    const float py = lattice_coord(j, r1, bmax3[1] - lo_y, lo_y);
    const float pz = lattice_coord(k, r1, bmax3[2] - lo_z, lo_z);
    const float fW = (float)W, fH = (float)H, neg_tau = -tau;
    float ad = acc_d[n], aw = acc_w[n];
    F3 ac = {0.0f, 0.0f, 0.0f};
    if constexpr (COLOR) ac = acc_c[n];
    bool touched = false;
    for (uint32_t v = 0; v < V; ++v) {
        const float *M = poses + 16 * (size_t)v;  // uniform: scalar loads
        const float *K = intrinsics + 4 * (size_t)v;
        const float dx = px - M[3], dy = py - M[7], dz = pz - M[11];
        const float qz = (M[2] * dx + M[6] * dy) + M[10] * dz;
        if (!(qz > 0.0f)) continue;
        const float qx = (M[0] * dx + M[4] * dy) + M[8] * dz;
        const float qy = (M[1] * dx + M[5] * dy) + M[9] * dz;
        const float x = (K[0] * qx) / qz + K[2];
        const float y = (K[1] * qy) / qz + K[3];
        if (!(x >= 0.0f && x < fW && y >= 0.0f && y < fH)) continue;
        const uint32_t pi = (uint32_t)(int)floorf(x), pj = (uint32_t)(int)floorf(y);  // 0 .. W - 1, 0 .. H - 1 by the test above
        const size_t pix = ((size_t)v * H + pj) * W + pi;
        const float D = depth[pix];
        if (!(D > 0.0f)) continue;
        const float r = sqrtf((dx * dx + dy * dy) + dz * dz);
        const float s = D - r;
        if (!(s >= neg_tau)) continue;
        const float t = fminf(s / tau, 1.0f);
        float w = 1.0f;
        if constexpr (WEIGHT) {
            w = weight[pix];
            if (!(w > 0.0f && w <= kFltMax)) continue;
        }
        ad = ad + w * t;
        aw = aw + w;
        if constexpr (COLOR) {
            const F3 c = color[pix];
            ac.x = ac.x + w * c.x;
            ac.y = ac.y + w * c.y;
            ac.z = ac.z + w * c.z;
        }
        touched = true;
    }
    if (touched) {
        acc_d[n] = ad;
        acc_w[n] = aw;
        if constexpr (COLOR) acc_c[n] = ac;
    }
}

__global__ __launch_bounds__(kThreads) void k_tsdf_finalize(const float *__restrict__ acc_d, const float *__restrict__ acc_w, uint32_t voxels,
                                                           float min_weight, float unknown, float *__restrict__ field,
                                                           unsigned long long *__restrict__ totals) {
#pragma clang fp contract(off)
    // a grid-stride walk: the wave's first index is a multiple of 64 and the stride is one, so `first < voxels` is the same in every
    // lane of a wave and the ballots see whole waves; the counts stay in scalar registers until the wave is done (voxels <= 2^30 and
    // the stride is 2^19 at most: the index does not wrap)
    const uint32_t lane = threadIdx.x & (kWave - 1), stride = gridDim.x * kThreads;
    unsigned long long n_seen = 0, n_in = 0, n_not = 0;
    for (uint32_t first = blockIdx.x * kThreads + (threadIdx.x - lane); first < voxels; first += stride) {
        const uint32_t n = first + lane;
        const bool live = n < voxels;
        bool seen = false, inside = false;
        if (live) {
            const float w = acc_w[n];
            seen = w >= min_weight;
            float f = unknown;
            if (seen) {
                f = fmaxf(fminf(acc_d[n] / w, 1.0f), -1.0f);
                inside = f <= 0.0f;
            }
            field[n] = f;
        }
        n_seen += __popcll(__ballot(seen));
        n_in += __popcll(__ballot(inside));
        n_not += __popcll(__ballot(live && !seen));
    }
    if (lane == 0) {
        if (n_seen) atomicAdd(&totals[0], n_seen);
        if (n_in) atomicAdd(&totals[1], n_in);
        if (n_not) atomicAdd(&totals[2], n_not);
    }
}

__global__ __launch_bounds__(kThreads) void k_tsdf_sample(const F3 *__restrict__ acc_c, const float *__restrict__ acc_w, uint32_t R,
                                                         const float *__restrict__ bmin3, const float *__restrict__ bmax3, float min_weight,
                                                         const F3 *__restrict__ points, uint32_t N, F3 *__restrict__ colors) {
#pragma clang fp contract(off)
    const uint32_t row = blockIdx.x * kThreads + threadIdx.x;
    if (row >= N) return;
    const F3 P = points[row];
    const float r1 = (float)(R - 1);
    const float Pa[3] = {P.x, P.y, P.z};
    uint32_t base[3];
    float f[3], g[3];
    bool in_box = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float lo = bmin3[a];
        const float u = (Pa[a] - lo) / (bmax3[a] - lo) * r1;
        const bool ok = u >= 0.0f && u <= r1;  // false for a NaN: a point that is not finite is outside
        in_box = in_box && ok;
        const uint32_t cell = ok ? min((uint32_t)(int)floorf(u), R - 2u) : 0u;
        base[a] = cell;
        f[a] = u - (float)cell;
        g[a] = 1.0f - f[a];
    }
    F3 out = {0.0f, 0.0f, 0.0f};
    if (in_box) {
        float m_sum = 0.0f;
        F3 c_sum = {0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int code = 0; code < 8; ++code) {
            const int a = code >> 2, b = (code >> 1) & 1, c = code & 1;
            const size_t n = ((size_t)(base[0] + a) * R + (base[1] + b)) * R + (base[2] + c);
            const float w = acc_w[n];
            if (!(w >= min_weight)) continue;
            const float m = ((a ? f[0] : g[0]) * (b ? f[1] : g[1])) * (c ? f[2] : g[2]);
            const F3 s = acc_c[n];
            m_sum = m_sum + m;
            c_sum.x = c_sum.x + m * (s.x / w);
            c_sum.y = c_sum.y + m * (s.y / w);
            c_sum.z = c_sum.z + m * (s.z / w);
        }
        if (m_sum > 0.0f)
            out = {fminf(fmaxf(c_sum.x / m_sum, 0.0f), 1.0f), fminf(fmaxf(c_sum.y / m_sum, 0.0f), 1.0f),
                   fminf(fmaxf(c_sum.z / m_sum, 0.0f), 1.0f)};
    }
    colors[row] = out;
}

bool lattice_ok(uint32_t R) { return R >= 2 && R <= PVD_MESH_TSDF_MAX_R; }
bool positive_finite(float x) { return x > 0.0f && x <= kFltMax; }

}  // namespace

extern "C" {

int pvd_mesh_tsdf_integrate(const float *depth, const float *color, const float *weight, const float *poses, const float *intrinsics,
                            uint32_t V, uint32_t H, uint32_t W, uint32_t R, const float *bmin3, const float *bmax3, float tau,
                            float *acc_d, float *acc_w, float *acc_c, pvd_stream_t stream) {
    if (!lattice_ok(R) || H < 1 || H > PVD_MESH_TSDF_MAX_SIDE || W < 1 || W > PVD_MESH_TSDF_MAX_SIDE) return PVD_ERR_UNSUPPORTED;
    if (!positive_finite(tau)) return PVD_ERR_INVALID;
    if (V == 0) return PVD_OK;
    if (!depth || !poses || !intrinsics || !bmin3 || !bmax3 || !acc_d || !acc_w) return PVD_ERR_INVALID;
    const uint32_t voxels = R * R * R;
    const dim3 grid(div_up(voxels, kThreads)), block(kThreads);
    const hipStream_t st = (hipStream_t)stream;
    const F3 *c = (const F3 *)color;
    F3 *ac = (F3 *)acc_c;
    const bool with_color = color && acc_c;
#define PVD_TSDF_LAUNCH(COLOR, WEIGHT)                                                                                                    \
    hipLaunchKernelGGL((k_tsdf_integrate<COLOR, WEIGHT>), grid, block, 0, st, depth, c, weight, poses, intrinsics, V, H, W, R, voxels, bmin3, \
                       bmax3, tau, acc_d, acc_w, ac)
    if (with_color && weight) PVD_TSDF_LAUNCH(true, true);
    else if (with_color) PVD_TSDF_LAUNCH(true, false);
    else if (weight) PVD_TSDF_LAUNCH(false, true);
    else PVD_TSDF_LAUNCH(false, false);
#undef PVD_TSDF_LAUNCH
    return check_launch();
}

int pvd_mesh_tsdf_finalize(const float *acc_d, const float *acc_w, uint32_t R, float min_weight, float unknown, float *field,
                           int64_t *totals, pvd_stream_t stream) {
    if (!lattice_ok(R)) return PVD_ERR_UNSUPPORTED;
    if (!positive_finite(min_weight) || !(unknown >= -kFltMax && unknown <= kFltMax)) return PVD_ERR_INVALID;
    if (!acc_d || !acc_w || !field || !totals) return PVD_ERR_INVALID;
    const hipStream_t st = (hipStream_t)stream;
    const int rc = check_memset(hipMemsetAsync(totals, 0, 3 * sizeof(int64_t), st));
    if (rc != PVD_OK) return rc;
    const uint32_t voxels = R * R * R;
    hipLaunchKernelGGL(k_tsdf_finalize, dim3(min(div_up(voxels, kThreads), kFinalizeBlocks)), dim3(kThreads), 0, st, acc_d, acc_w, voxels, min_weight, unknown, field,
                       (unsigned long long *)totals);
    return check_launch();
}

int pvd_mesh_tsdf_sample_color(const float *acc_c, const float *acc_w, uint32_t R, const float *bmin3, const float *bmax3,
                               float min_weight, const float *points, uint32_t N, float *colors, pvd_stream_t stream) {
    if (!lattice_ok(R)) return PVD_ERR_UNSUPPORTED;
    if (!positive_finite(min_weight)) return PVD_ERR_INVALID;
    if (N == 0) return PVD_OK;
    if (!acc_c || !acc_w || !bmin3 || !bmax3 || !points || !colors) return PVD_ERR_INVALID;
    hipLaunchKernelGGL(k_tsdf_sample, dim3(div_up(N, kThreads)), dim3(kThreads), 0, (hipStream_t)stream, (const F3 *)acc_c, acc_w, R, bmin3,
                       bmax3, min_weight, (const F3 *)points, N, (F3 *)colors);
    return check_launch();
}

}  // extern "C"
