// block_scan.h -- the one copy of the count -> workgroup sums -> one-workgroup scan -> offsets pattern that csrc/mesh.hip,
// mesh_dist.hip, mesh_simplify.hip, mesh_ray.hip and mesh_smooth.hip are built on, and of the wave reductions under it
// (csrc/components.hip uses those too).
//
//   count      per item, the caller's own kernel (or a memset and atomics)
//   blocksum   one lane per item: block_sum -> the sum of the workgroup's kThreads items
//   scan       ONE workgroup of kScanThreads: scan_sums -> the sums become their exclusive scan, in place, plus the total
//   offsets    one lane per item: block_exclusive + the workgroup's scanned sum -> the item's offset
//
// Reduce-then-scan in separate launches: no workgroup waits on another one of the same launch, nothing here is atomic, and every
// sum is a sum of integers, so no result depends on the order in which workgroups run.  The library is built without relocatable
// device code, so everything is defined here: every translation unit gets its own copy of what it uses.
//
// Every function that has a barrier inside says so; all threads of the workgroup must reach it (no early return before it).
#pragma once

#include <type_traits>

#include "pvd_device.h"

namespace pvd {

constexpr int kThreads = 256;  // per workgroup of the per-item kernels
constexpr int kWaves = kThreads / kWave;
constexpr int kScanThreads = 1024;  // of the one scanning workgroup
constexpr int kScanWaves = kScanThreads / kWave;
constexpr int kScanItems = 8;  // sums per thread and chunk
constexpr uint32_t kScanChunk = kScanThreads * kScanItems;  // 8192 sums per chunk

// ---------------------------------------------------------------------------------------------------------------- one wave
// T: uint32_t or uint64_t; the 64-bit shuffles are those of unsigned long long
template <typename T>
using shfl_t = std::conditional_t<sizeof(T) == 8, unsigned long long, T>;

// the sum over the wave, in lane 0
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
    static_assert(std::is_unsigned<T>::value, "wrap-around sums");
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) v += (T)__shfl_down((shfl_t<T>)v, o, kWave);
    return v;
}
// the maximum over the wave, in lane 0
template <typename T>
__device__ __forceinline__ T wave_max(T v) {
    static_assert(std::is_unsigned<T>::value, "unsigned order");
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
        const T w = (T)__shfl_down((shfl_t<T>)v, o, kWave);
        v = w > v ? w : v;
    }
    return v;
}
// inclusive scan over the wave
template <typename T>
__device__ __forceinline__ T wave_scan(T v) {
    static_assert(std::is_unsigned<T>::value, "wrap-around sums");
    const uint32_t lane = threadIdx.x & (kWave - 1);
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
        const T w = (T)__shfl_up((shfl_t<T>)v, o, kWave);
        if (lane >= (uint32_t)o) v += w;
    }
    return v;
}

// ----------------------------------------------------------------------------------------------------------- one workgroup
// `red` is LDS of the caller, one word per wave of the workgroup; a second call in the same kernel takes a second array.
// One barrier each.

// the sum of the waves' values s (read from lane 0 of each wave), in thread 0
template <typename T, int W>
__device__ __forceinline__ T block_sum_of_waves(T s, T (&red)[W]) {
    if ((threadIdx.x & (kWave - 1)) == 0) red[threadIdx.x / kWave] = s;
    __syncthreads();
    T a = 0;
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 0; w < W; ++w) a += red[w];
    }
    return a;
}
// the sum of v over the workgroup, in thread 0
template <typename T, int W>
__device__ __forceinline__ T block_sum(T v, T (&red)[W]) {
    return block_sum_of_waves(wave_sum(v), red);
}
// the maximum of v over the workgroup, in thread 0
template <typename T, int W>
__device__ __forceinline__ T block_max(T v, T (&red)[W]) {
    v = wave_max(v);
    if ((threadIdx.x & (kWave - 1)) == 0) red[threadIdx.x / kWave] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < W; ++w) v = red[w] > v ? red[w] : v;
    }
    return v;
}
// this thread's exclusive prefix of v within the workgroup
template <typename T, int W>
__device__ __forceinline__ T block_exclusive(T v, T (&wtot)[W]) {
    const uint32_t lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const T in = wave_scan(v);
    if (lane == kWave - 1) wtot[wave] = in;
    __syncthreads();
    T before = 0;
#pragma unroll
    for (uint32_t w = 0; w < (uint32_t)W; ++w) {
        if (w < wave) before += wtot[w];
    }
    return before + (in - v);
}

// ------------------------------------------------------------------------------------------- the scan of the workgroup sums
// ONE workgroup of kScanThreads; L arrays of NB sums each, walked side by side (one pass over both for a kernel that scans two
// things, as csrc/mesh.hip does) in chunks of kScanChunk with a running carry: each array becomes its exclusive scan, in place,
// and total[l] is the sum of array l, in every thread.  Two barriers per chunk.
template <typename T, int L>
__device__ __forceinline__ void scan_sums(T *const (&sums)[L], uint32_t NB, T (&total)[L]) {
    __shared__ T wtot[L][kScanWaves];
    const uint32_t t = threadIdx.x, lane = t & (kWave - 1), wave = t / kWave;
    T carry[L] = {};
    for (uint32_t base = 0; base < NB; base += kScanChunk) {  // the trip count is the same for every thread
        const uint32_t first = base + t * kScanItems;
        T a[L][kScanItems], sa[L] = {}, ia[L];
#pragma unroll
        for (int q = 0; q < kScanItems; ++q) {
#pragma unroll
            for (int l = 0; l < L; ++l) {
                a[l][q] = first + q < NB ? sums[l][first + q] : 0u;
                sa[l] += a[l][q];
            }
        }
#pragma unroll
        for (int l = 0; l < L; ++l) {
            ia[l] = wave_scan(sa[l]);
            if (lane == kWave - 1) wtot[l][wave] = ia[l];
        }
        __syncthreads();
        T before[L] = {}, all[L] = {};
#pragma unroll
        for (uint32_t w = 0; w < (uint32_t)kScanWaves; ++w) {
#pragma unroll
            for (int l = 0; l < L; ++l) {
                const T x = wtot[l][w];
                if (w < wave) before[l] += x;
                all[l] += x;
            }
        }
        __syncthreads();  // wtot is rewritten by the next chunk
#pragma unroll
        for (int l = 0; l < L; ++l) {
            T e = carry[l] + before[l] + (ia[l] - sa[l]);
#pragma unroll
            for (int q = 0; q < kScanItems; ++q) {
                if (first + q < NB) sums[l][first + q] = e;
                e += a[l][q];
            }
            carry[l] += all[l];
        }
    }
#pragma unroll
    for (int l = 0; l < L; ++l) total[l] = carry[l];
}
// one array
template <typename T>
__device__ __forceinline__ T scan_sums(T *sums, uint32_t NB) {
    T *const one[1] = {sums};
    T total[1];
    scan_sums(one, NB, total);
    return total[0];
}

// ------------------------------------------------------------------------------------ the three kernels over plain counts
// Templates in an unnamed namespace: a translation unit gets a kernel, in its own code object, only where it launches it.
namespace {

// one lane per item: the sum of the workgroup's kThreads counts
template <typename T>
__global__ __launch_bounds__(kThreads) void k_blocksum(const T *__restrict__ count, uint32_t N, T *__restrict__ bsum) {
    __shared__ T red[kWaves];
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    const T a = block_sum(i < N ? count[i] : (T)0, red);
    if (threadIdx.x == 0) bsum[blockIdx.x] = a;
}

// one workgroup; sums [NB] -> exclusive scan in place; the total to *total_a and *total_b (which may be one word)
template <typename T>
__global__ __launch_bounds__(kScanThreads) void k_scan(T *__restrict__ bsum, uint32_t NB, T *total_a, T *total_b) {
    const T total = scan_sums(bsum, NB);
    if (threadIdx.x == 0) {
        *total_a = total;
        *total_b = total;
    }
}

// one lane per item: exclusive scan of the counts inside the workgroup + the workgroup's base -> the item's start, and the same
// value in place of the count (a fill pass takes its slots from there)
template <typename T>
__global__ __launch_bounds__(kThreads) void k_offsets(T *__restrict__ cursor, uint32_t N, const T *__restrict__ bsum, T *__restrict__ start) {
    __shared__ T wtot[kWaves];
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    const T at = bsum[blockIdx.x] + block_exclusive(i < N ? cursor[i] : (T)0, wtot);
    if (i < N) {
        start[i] = at;
        cursor[i] = at;
    }
}

}  // namespace

}  // namespace pvd
