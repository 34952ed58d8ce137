// components.hip -- connected components of the inside set of a density volume (include/pvd_hip_components.h): lock-free union-find
// with `labels` as the parent array, over the 14-neighbour connectivity of the mesher's Kuhn split; sizes and statistics in integers.
//
// reference: distill_mutual/network.py:601 ("lots of noisy outliers in hashnerf"); extract_geometry, distill_mutual/utils.py:442-488.
//
// Invariant of the parent array, from the first launch on: for an inside point p, 0 <= labels[p] <= p and labels[p] is a point of
// p's component; labels[p] == p marks a root; outside points hold -1 and are never written again.  Parents only ever get smaller.
//
// k_cc_init     one lane per lattice point (k fastest): labels[p] = the first point of p's run of inside points along k inside its
//               wave (the local merge: a ballot, no memory traffic), -1 outside; sizes[p] = 0; the statistics are zeroed.
// k_cc_merge    one lane per lattice point: union(p, p + d) for the seven directions d, skipping the edges that other edges imply.
// k_cc_flatten  one lane per lattice point: labels[p] = root of p; sizes[root] += points, runs of equal labels along k merged in
//               the wave and the waves' leading runs merged in the workgroup first; components and inside points counted.
// k_cc_largest  packed 64-bit maximum of (size, ~label) over the roots; k_cc_unpack turns it into {size, label}.
// k_cc_filter   out = field, thresh at the points of dropped components; kept components and points counted.
// A kernel boundary is the only thing that makes one phase's plain stores visible to the next phase.  Inside k_cc_merge a parent is
// only ever taken from an agent-scope relaxed atomic load or from the value an atomicMin returned.  No loop waits for a store of
// another lane or workgroup: every loop below states why each trip lowers an index or leaves.
#include "block_scan.h"

#include "../../include/pvd_hip_components.h"

namespace {

using namespace pvd;

constexpr int kFlatThreads = 1024;
constexpr int kFlatWaves = kFlatThreads / kWave;

// the seven directions in the slot order of pvd_hip_mesh.h
constexpr int kDirs[7][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}, {1, 1, 0}, {1, 0, 1}, {0, 1, 1}, {1, 1, 1}};

__device__ __forceinline__ int32_t load_parent(int32_t *labels, int32_t x) {
    return __hip_atomic_load(labels + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Root of x as far as this lane can tell.  Terminates: a parent is <= its point, so every trip either finds labels[x] == x and
// leaves, or replaces x by a strictly smaller index; x >= 0 bounds the trips by the start value.  Nothing is waited for.
__device__ __forceinline__ int32_t find_root(int32_t *labels, int32_t x) {
    for (;;) {
        const int32_t p = load_parent(labels, x);
        if (p == x) return x;
        x = p;
    }
}

// Join the components of a and b.  Each trip looks at two roots-as-seen a != b and tries to hang the larger one, hi, under the
// smaller one, lo, with one atomicMin.  If hi was still a root the two trees are one and the lane leaves.  If not, hi had got
// a parent `old` < hi meanwhile (from another lane); labels[hi] is now min(old, lo) -- still a smaller point of the same
// component -- and what remains to be joined is old's tree and lo's, so hi is replaced by root(old) <= old < hi.
// Terminates: in every trip that does not leave, max(a, b) is replaced by a strictly smaller index >= 0, and the other one is
// kept, so a + b strictly falls; the lane never re-reads a value to see whether someone else has changed it.
__device__ __forceinline__ void unite(int32_t *labels, int32_t a, int32_t b) {
    a = find_root(labels, a);
    b = find_root(labels, b);
    while (a != b) {
        const int32_t hi = a > b ? a : b, lo = a > b ? b : a;
        const int32_t old = atomicMin(labels + hi, lo);
        if (old == hi) return;
        a = find_root(labels, old);
        b = lo;
    }
}

__global__ __launch_bounds__(kThreads) void k_cc_init(const float *__restrict__ u, uint32_t R, uint32_t N, float thresh,
                                                     int32_t *__restrict__ labels, uint32_t *__restrict__ sizes,
                                                     uint32_t *__restrict__ stats) {
    const uint32_t n = blockIdx.x * kThreads + threadIdx.x, lane = threadIdx.x & (kWave - 1);
    if (n < 4) stats[n] = 0u;
    const bool in = n < N && u[n] > thresh;
    // a lane starts a run when it is not joined to the lane before it: one of the two is outside, or a new k-row begins
    const uint64_t inside = __ballot(in);
    const bool row_start = n % R == 0;
    const bool joined = lane > 0 && in && ((inside >> (lane - 1)) & 1ull) && !row_start;
    const uint64_t starts = __ballot(!joined);                     // bit 0 is always set
    const uint64_t upto = starts & (~0ull >> (kWave - 1 - lane));  // the starts at or below this lane
    const uint32_t first = 63u - (uint32_t)__clzll((long long)upto);
    if (n < N) {
        labels[n] = in ? (int32_t)(n - lane + first) : -1;
        sizes[n] = 0u;
    }
}

__global__ __launch_bounds__(kThreads) void k_cc_merge(const float *__restrict__ u, uint32_t R, uint32_t N, float thresh,
                                                      int32_t *labels) {
    const uint32_t n = blockIdx.x * kThreads + threadIdx.x;
    if (n >= N) return;
    const int32_t i = (int32_t)(n / (R * R)), r = (int32_t)(n - (uint32_t)i * R * R), j = r / (int32_t)R, k = r - j * (int32_t)R;
    const int32_t Ri = (int32_t)R;
    // the field is read-only in this launch: plain loads
    auto in = [&](int32_t dx, int32_t dy, int32_t dz) -> bool {
        const int32_t ii = i + dx, jj = j + dy, kk = k + dz;
        if (ii >= Ri || jj >= Ri || kk < 0 || kk >= Ri) return false;
        return u[((uint32_t)ii * R + (uint32_t)jj) * R + (uint32_t)kk] > thresh;
    };
    if (!in(0, 0, 0)) return;
    const int32_t p = (int32_t)n;
    // The k-edge p -> p + 1: k_cc_init has joined the runs inside a wave, so only the last lane of a wave has one left.
    if ((n & (kWave - 1)) == kWave - 1 && in(0, 0, 1)) unite(labels, p, p + 1);
    // An edge p -> q in another direction is implied, and skipped, when p - 1 and q - 1 (one step back along k) are both inside:
    // p ~ p - 1 and q ~ q - 1 by k-edges, and p - 1 ~ q - 1 is the same direction's edge one step back, which is either made or
    // implied in turn -- the chain ends at the first point of the row at the latest.  Only the surface does unions.
    const bool back = in(0, 0, -1);
#pragma unroll
    for (int32_t c = 0; c < 4; ++c) {
        const int32_t dx = c >> 1, dy = c & 1;
        const bool qm = in(dx, dy, -1), q0 = c == 0 ? true : in(dx, dy, 0), qp = in(dx, dy, 1);
        const int32_t q = p + (dx * Ri + dy) * Ri;
        if (c != 0 && q0 && !(back && qm)) unite(labels, p, q);
        if (c != 0 && qp && !(back && q0)) unite(labels, p, q + 1);
    }
}

// Plain loads of labels: every value this launch stores into labels[x] is the root of x, and every value the launches before
// left there is an ancestor of x in a forest that no longer changes shape, so a stale read (the old parent where another
// workgroup has already stored the root) is benign: the walk passes through ancestors only and ends at the root, whose own
// entry never changes.  Terminates as find_root does: every trip lowers x or leaves.
__device__ __forceinline__ int32_t walk_root(const int32_t *labels, int32_t x) {
    for (;;) {
        const int32_t p = labels[x];
        if (p == x) return x;
        x = p;
    }
}

__global__ __launch_bounds__(kFlatThreads) void k_cc_flatten(int32_t *labels, uint32_t N, uint32_t *__restrict__ sizes,
                                                            uint32_t *__restrict__ stats) {
    __shared__ int32_t lead_root[kFlatWaves];
    __shared__ uint32_t lead_len[kFlatWaves], n_roots[kFlatWaves], n_inside[kFlatWaves];
    const uint32_t n = blockIdx.x * kFlatThreads + threadIdx.x, lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    int32_t root = -1;
    if (n < N) {
        const int32_t p = labels[n];  // own entry: written by this lane alone in this launch
        if (p >= 0) {
            root = walk_root(labels, p);
            if (root != p) labels[n] = root;
        }
    }
    // runs of equal labels along k inside the wave: one add per run, not per point (the giant component of a real scene would
    // put millions of increments on one address)
    const int32_t before = __shfl_up(root, 1, kWave);
    const bool head = lane == 0 || root != before;
    const uint64_t heads = __ballot(head);
    const uint64_t above = lane == kWave - 1 ? 0ull : heads >> (lane + 1);
    const uint32_t len = above ? (uint32_t)__ffsll((long long)above) : kWave - lane;  // to the next head, or to the wave's end
    if (head && lane > 0 && root >= 0) atomicAdd(sizes + root, len);
    const uint64_t roots = __ballot(root >= 0 && root == (int32_t)n), ins = __ballot(root >= 0);
    if (lane == 0) {
        lead_root[wave] = root;
        lead_len[wave] = len;
        n_roots[wave] = (uint32_t)__popcll(roots);
        n_inside[wave] = (uint32_t)__popcll(ins);
    }
    __syncthreads();
    if (threadIdx.x == 0) {  // the waves' leading runs: neighbours with one label are added once
        int32_t cur = -1;
        uint32_t acc = 0, nr = 0, ni = 0;
        for (int w = 0; w < kFlatWaves; ++w) {
            if (lead_root[w] != cur) {
                if (cur >= 0) atomicAdd(sizes + cur, acc);
                cur = lead_root[w];
                acc = 0;
            }
            acc += lead_len[w];
            nr += n_roots[w];
            ni += n_inside[w];
        }
        if (cur >= 0) atomicAdd(sizes + cur, acc);
        if (nr) atomicAdd(stats + 0, nr);
        if (ni) atomicAdd(stats + 1, ni);
    }
}

// (size << 32) | ~label: the greatest size wins, and among equal sizes the smallest label
__global__ __launch_bounds__(kThreads) void k_cc_largest(const uint32_t *__restrict__ sizes, uint32_t N, unsigned long long *best) {
    __shared__ unsigned long long red[kWaves];
    const uint32_t n = blockIdx.x * kThreads + threadIdx.x;
    const uint32_t s = n < N ? sizes[n] : 0u;
    const unsigned long long v = block_max(s ? ((unsigned long long)s << 32) | (unsigned long long)(~n) : 0ull, red);
    if (threadIdx.x == 0 && v) atomicMax(best, v);
}

__global__ void k_cc_unpack(uint32_t *stats) {
    const uint32_t not_label = stats[2], size = stats[3];  // the packed maximum, little-endian
    stats[2] = size;
    stats[3] = size ? ~not_label : 0u;
}

// field and out may be one array: a lane reads and writes its own element only
__global__ __launch_bounds__(kThreads) void k_cc_filter(const float *field, const int32_t *__restrict__ labels,
                                                       const uint32_t *__restrict__ sizes, const uint32_t *__restrict__ stats, uint32_t N,
                                                       float thresh, uint32_t min_points, uint32_t largest_only, float *out,
                                                       uint32_t *__restrict__ kept) {
    __shared__ uint32_t red[kWaves];
    const uint32_t n = blockIdx.x * kThreads + threadIdx.x;
    bool keep = false, is_root = false;
    if (n < N) {
        const float v = field[n];
        const int32_t lab = labels[n];
        if (lab >= 0) {
            keep = !(sizes[lab] < min_points || (largest_only && (uint32_t)lab != stats[3]));
            is_root = (uint32_t)lab == n;
        }
        out[n] = (lab >= 0 && !keep) ? thresh : v;
    }
    const uint64_t kc = __ballot(keep && is_root), kp = __ballot(keep);
    // both counts in one word: a workgroup keeps at most kThreads = 256 components (low half) and 256 points (high half)
    const uint32_t s = block_sum_of_waves((uint32_t)__popcll(kc) | ((uint32_t)__popcll(kp) << 16), red);
    if (threadIdx.x == 0) {
        const uint32_t a = s & 0xffffu, b = s >> 16;
        if (a) atomicAdd(kept + 0, a);
        if (b) atomicAdd(kept + 1, b);
    }
}

__global__ void k_cc_zero2(uint32_t *kept) {
    if (threadIdx.x < 2) kept[threadIdx.x] = 0u;
}

}  // namespace

extern "C" {

int pvd_components_label(const float *field, uint32_t R, float thresh, int32_t *labels, uint32_t *sizes, uint32_t *stats_dev,
                         pvd_stream_t stream) {
    if (!field || !labels || !sizes || !stats_dev || ((uintptr_t)stats_dev & 7u)) return PVD_ERR_INVALID;
    if (R < 2 || R > PVD_MESH_MAX_R) return PVD_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    const uint32_t N = R * R * R, NB = div_up(N, kThreads);
    int rc;
    hipLaunchKernelGGL(k_cc_init, dim3(NB), dim3(kThreads), 0, st, field, R, N, thresh, labels, sizes, stats_dev);
    if ((rc = check_launch()) != PVD_OK) return rc;
    hipLaunchKernelGGL(k_cc_merge, dim3(NB), dim3(kThreads), 0, st, field, R, N, thresh, labels);
    if ((rc = check_launch()) != PVD_OK) return rc;
    hipLaunchKernelGGL(k_cc_flatten, dim3(div_up(N, kFlatThreads)), dim3(kFlatThreads), 0, st, labels, N, sizes, stats_dev);
    if ((rc = check_launch()) != PVD_OK) return rc;
    hipLaunchKernelGGL(k_cc_largest, dim3(NB), dim3(kThreads), 0, st, (const uint32_t *)sizes, N, (unsigned long long *)(stats_dev + 2));
    if ((rc = check_launch()) != PVD_OK) return rc;
    hipLaunchKernelGGL(k_cc_unpack, dim3(1), dim3(1), 0, st, stats_dev);
    return check_launch();
}

int pvd_components_filter(const float *field, const int32_t *labels, const uint32_t *sizes, const uint32_t *stats_dev, uint32_t R,
                          float thresh, uint32_t min_points, uint32_t largest_only, float *out, uint32_t *kept_dev, pvd_stream_t stream) {
    if (!field || !labels || !sizes || !stats_dev || !out || !kept_dev) return PVD_ERR_INVALID;
    if (R < 2 || R > PVD_MESH_MAX_R) return PVD_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    const uint32_t N = R * R * R, NB = div_up(N, kThreads);
    int rc;
    hipLaunchKernelGGL(k_cc_zero2, dim3(1), dim3(kWave), 0, st, kept_dev);
    if ((rc = check_launch()) != PVD_OK) return rc;
    hipLaunchKernelGGL(k_cc_filter, dim3(NB), dim3(kThreads), 0, st, field, labels, sizes, stats_dev, N, thresh, min_points, largest_only,
                       out, kept_dev);
    return check_launch();
}

int pvd_components_neighbours(int32_t *offsets_host) {
    if (!offsets_host) return PVD_ERR_INVALID;
    for (int s = 0; s < 7; ++s)
        for (int a = 0; a < 3; ++a) {
            offsets_host[3 * s + a] = kDirs[s][a];
            offsets_host[3 * (7 + s) + a] = -kDirs[s][a];
        }
    return 14;
}

}  // extern "C"
