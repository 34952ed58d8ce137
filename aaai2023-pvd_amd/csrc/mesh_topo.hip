// mesh_topo.hip -- edge report, shells and clean-up of a triangle mesh (include/pvd_hip_mesh_topo.h): every result is a count, a
// minimum or a maximum of integers, so nothing depends on the order in which the atomics land.
//
// build
// k_tp_init         one lane per vertex: parent = itself, bucket counts, shell size and referenced mark zeroed; the list lengths.
// k_tp_count        one lane per triangle: its flags byte (bit0 when it is not valid); a valid one adds 1 under its smallest vertex.
// k_blocksum / k_scan / k_offsets (csrc/block_scan.h), 32-bit: the triangle buckets' offsets.
// k_tp_fill_tri     one lane per valid triangle: its index into its bucket, at an atomic cursor.
// k_tp_groups       one lane per valid triangle: a bucket of at most kLong entries is walked by the lane, which then settles the
//                   triangle (duplicate, cancelled or survivor; a survivor counts its edges, marks and joins its corners); a triangle
//                   with a longer bucket is appended to a list (one atomic counter).
// k_tp_groups_long  the waves take triangles from that list, grid-strided: the lanes stride the bucket by 64, lane 0 settles.
// k_blocksum / k_scan / k_offsets, 64-bit: the edge buckets' offsets (3 F entries can pass 2^32).
// k_tp_fill_edge    one lane per survivor: its three edges (other endpoint | direction, triangle) under their smaller endpoints.
// k_tp_edges        one lane per triangle: the census of a survivor's three edges when all three buckets have at most kLong
//                   entries, else the triangle goes to the list; the lowest triangle of an edge counts it; the status counts.
// k_tp_edges_long   the waves take survivors from the list: the lanes stride each of the three buckets.
// k_tp_flatten      one lane per vertex: its shell label (the root, which is the smallest vertex of the tree) or -1.
// k_tp_sizes        one lane per triangle: its shell, and 1 added to the shell's size (a wave whose lanes agree adds once).
// k_tp_largest      packed 64-bit maximum of (size, ~label) over the labels.
// k_tp_totals       one thread: the counters become totals_dev.
// clean
// k_tp_keep_*       keep flags of the triangles and of the vertices, from the shells alone; two scans; k_tp_counts: (V', T').
// k_tp_emit_*       one lane per vertex / per triangle.
// A kernel boundary is the only thing that makes one phase's plain stores visible to the next.  No workgroup waits on another one;
// the only loops whose trip count depends on other lanes are those of the union-find, which state why every trip lowers an index.
#include "block_scan.h"

#include "../../include/pvd_hip_mesh_topo.h"

namespace {

using namespace pvd;

constexpr uint32_t kMaxN = 0x7fffffffu;  // V and T
// A bucket of more than kLong entries is walked by a whole wavefront, any other one by a single lane.  One wave stride is 64 entries;
// an extracted mesh has triangle buckets of about 2 and edge buckets of about 3.  Not A/B-measured.
constexpr uint32_t kLong = 64;
constexpr uint32_t kLongBlocks = 4096;  // the most workgroups of a launch over a list

constexpr uint32_t kInvalid = 1u, kDuplicate = 2u, kCancelled = 4u, kBoundary = 8u, kInconsistent = 16u, kNonManifold = 32u;
constexpr uint32_t kDead = kInvalid | kDuplicate | kCancelled;

// the counters: 0 .. 15 are the totals of the header
enum { cValid = 0, cInvalid, cDuplicate, cCancelled, cSurvivors, cReferenced, cEdges, cBoundary, cInconsistent, cNonManifold,
       cUnbalanced, cShells, cBest = 16, cEdgeTotal = 17, kCounters = 20 };
// the 32-bit words
enum { wLongTri = 0, wLongEdge, wTriTotal, wKeptV, wKeptT, kWords = 8 };

struct Layout {  // byte offsets into the workspace
    size_t counters, ecnt, eoff, ebsum, edges;                                          // 8-byte words
    size_t toff, tcur, tbsum, tbucket, longs, parent, shell, size, vref, tshell, words;  // build, 4-byte words
    size_t fv, sv, bsv, ft, st, bst;                                                     // clean
    size_t flags, total;
};

inline Layout layout(uint32_t V, uint32_t T) {
    const size_t v = V, t = T, NV = (v + kThreads - 1) / kThreads, NT = (t + kThreads - 1) / kThreads;
    Layout l;
    l.counters = 0;
    l.ecnt = l.counters + 8 * (size_t)kCounters;
    l.eoff = l.ecnt + 8 * v;
    l.ebsum = l.eoff + 8 * (v + 1);
    l.edges = l.ebsum + 8 * NV;
    l.toff = l.edges + 24 * t;
    l.tcur = l.toff + 4 * (v + 1);
    l.tbsum = l.tcur + 4 * v;
    l.tbucket = l.tbsum + 4 * NV;
    l.longs = l.tbucket + 4 * t;
    l.parent = l.longs + 4 * t;
    l.shell = l.parent + 4 * v;
    l.size = l.shell + 4 * v;
    l.vref = l.size + 4 * v;
    l.tshell = l.vref + 4 * v;
    l.words = l.tshell + 4 * t;
    l.fv = l.words + 4 * (size_t)kWords;
    l.sv = l.fv + 4 * v;
    l.bsv = l.sv + 4 * (v + 1);
    l.ft = l.bsv + 4 * NV;
    l.st = l.ft + 4 * t;
    l.bst = l.st + 4 * (t + 1);
    l.flags = l.bst + 4 * NT;
    l.total = l.flags + t;
    return l;
}

inline bool in_limits(uint32_t V, uint32_t T) { return V <= kMaxN && T <= kMaxN; }

struct Ws {  // the arrays of a workspace
    unsigned long long *counters, *ecnt, *eoff, *ebsum;
    uint2 *edges;
    uint32_t *toff, *tcur, *tbsum, *tbucket, *longs;
    int32_t *parent, *shell;
    uint32_t *size, *vref;
    int32_t *tshell;
    uint32_t *words, *fv, *sv, *bsv, *ft, *st, *bst;
    uint8_t *flags;
};

inline Ws arrays(void *workspace, uint32_t V, uint32_t T) {
    const Layout l = layout(V, T);
    char *p = (char *)workspace;
    Ws w;
    w.counters = (unsigned long long *)(p + l.counters);
    w.ecnt = (unsigned long long *)(p + l.ecnt);
    w.eoff = (unsigned long long *)(p + l.eoff);
    w.ebsum = (unsigned long long *)(p + l.ebsum);
    w.edges = (uint2 *)(p + l.edges);
    w.toff = (uint32_t *)(p + l.toff);
    w.tcur = (uint32_t *)(p + l.tcur);
    w.tbsum = (uint32_t *)(p + l.tbsum);
    w.tbucket = (uint32_t *)(p + l.tbucket);
    w.longs = (uint32_t *)(p + l.longs);
    w.parent = (int32_t *)(p + l.parent);
    w.shell = (int32_t *)(p + l.shell);
    w.size = (uint32_t *)(p + l.size);
    w.vref = (uint32_t *)(p + l.vref);
    w.tshell = (int32_t *)(p + l.tshell);
    w.words = (uint32_t *)(p + l.words);
    w.fv = (uint32_t *)(p + l.fv);
    w.sv = (uint32_t *)(p + l.sv);
    w.bsv = (uint32_t *)(p + l.bsv);
    w.ft = (uint32_t *)(p + l.ft);
    w.st = (uint32_t *)(p + l.st);
    w.bst = (uint32_t *)(p + l.bst);
    w.flags = (uint8_t *)(p + l.flags);
    return w;
}

// ------------------------------------------------------------------------------------------------------------------ helpers
__device__ __forceinline__ bool finite_bits(uint32_t b) { return (b & 0x7f800000u) != 0x7f800000u; }

__device__ __forceinline__ bool finite_vertex(const uint32_t *__restrict__ vbits, uint32_t v) {
    return finite_bits(vbits[3 * (size_t)v]) && finite_bits(vbits[3 * (size_t)v + 1]) && finite_bits(vbits[3 * (size_t)v + 2]);
}

// a triangle as its group sees it: a the smallest vertex, b < c the other two, even iff the corner order is a rotation of (a, b, c)
struct Tri {
    uint32_t a, b, c;
    bool even;
};

// the triangle rotated so that its smallest corner comes first (a rotation keeps the parity)
__device__ __forceinline__ Tri normal_form(uint32_t i0, uint32_t i1, uint32_t i2) {
    uint32_t a = i0, x = i1, y = i2;
    if (i1 < a && i1 < i2) {
        a = i1, x = i2, y = i0;
    } else if (i2 < a && i2 < i1) {
        a = i2, x = i0, y = i1;
    }
    Tri r;
    r.a = a;
    r.even = x < y;
    r.b = r.even ? x : y;
    r.c = r.even ? y : x;
    return r;
}

__device__ __forceinline__ void load3(const int32_t *__restrict__ triangles, uint32_t t, uint32_t &i0, uint32_t &i1, uint32_t &i2) {
    i0 = (uint32_t)triangles[3 * (size_t)t];  // a negative index is a large unsigned one
    i1 = (uint32_t)triangles[3 * (size_t)t + 1];
    i2 = (uint32_t)triangles[3 * (size_t)t + 2];
}

// the sum of the wave's values added to one counter by lane 0 (all 64 lanes must call)
__device__ __forceinline__ void wave_count(unsigned long long *counter, uint32_t mine) {
    const uint32_t s = wave_sum(mine);
    if ((threadIdx.x & (kWave - 1)) == 0 && s) atomicAdd(counter, (unsigned long long)s);
}

__device__ __forceinline__ uint32_t wave_min(uint32_t v) { return ~wave_max(~v); }

// ---- the union-find of csrc/components.hip over the vertices: parent[v] <= v, parent[v] == v marks a root, parents only get smaller
__device__ __forceinline__ int32_t load_parent(int32_t *parent, int32_t x) {
    return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// Terminates: a parent is <= its vertex, so every trip either finds a root and leaves or replaces x by a strictly smaller index.
__device__ __forceinline__ int32_t find_root(int32_t *parent, int32_t x) {
    for (;;) {
        const int32_t p = load_parent(parent, x);
        if (p == x) return x;
        x = p;
    }
}
// Each trip tries to hang the larger root-as-seen under the smaller one with one atomicMin; if the larger one had got a parent
// meanwhile, what remains to be joined is that parent's tree and the smaller root's.  Terminates: in every trip that does not
// leave, max(a, b) is replaced by a strictly smaller index >= 0 and the other one is kept.  Nothing is waited for.
__device__ __forceinline__ void unite(int32_t *parent, int32_t a, int32_t b) {
    a = find_root(parent, a);
    b = find_root(parent, b);
    while (a != b) {
        const int32_t hi = a > b ? a : b, lo = a > b ? b : a;
        const int32_t old = atomicMin(parent + hi, lo);
        if (old == hi) return;
        a = find_root(parent, old);
        b = lo;
    }
}

// ------------------------------------------------------------------------------------------------------------------ build
__global__ __launch_bounds__(kThreads) void k_tp_init(uint32_t V, int32_t *__restrict__ parent, uint32_t *__restrict__ tcur,
                                                     unsigned long long *__restrict__ ecnt, uint32_t *__restrict__ size,
                                                     uint32_t *__restrict__ vref, uint32_t *__restrict__ words) {
    const uint32_t v = blockIdx.x * kThreads + threadIdx.x;
    if (v <= wTriTotal) words[v] = 0u;  // the two list lengths and build's scan total; clean's words are not build's to touch
    if (v >= V) return;
    parent[v] = (int32_t)v;
    tcur[v] = 0u;
    ecnt[v] = 0ull;
    size[v] = 0u;
    vref[v] = 0u;
}

__global__ __launch_bounds__(kThreads) void k_tp_count(const uint32_t *__restrict__ vbits, uint32_t V,
                                                      const int32_t *__restrict__ triangles, uint32_t T, uint8_t *__restrict__ flags,
                                                      uint32_t *__restrict__ tcur) {
    const uint32_t t = blockIdx.x * kThreads + threadIdx.x;
    if (t >= T) return;
    uint32_t i0, i1, i2;
    load3(triangles, t, i0, i1, i2);
    bool ok = i0 < V && i1 < V && i2 < V && i0 != i1 && i1 != i2 && i0 != i2;
    if (ok) ok = finite_vertex(vbits, i0) && finite_vertex(vbits, i1) && finite_vertex(vbits, i2);
    flags[t] = ok ? 0u : (uint8_t)kInvalid;
    if (ok) atomicAdd(tcur + normal_form(i0, i1, i2).a, 1u);
}

__global__ __launch_bounds__(kThreads) void k_tp_fill_tri(const int32_t *__restrict__ triangles, uint32_t T,
                                                         const uint8_t *__restrict__ flags, uint32_t *__restrict__ tcur,
                                                         uint32_t *__restrict__ tbucket) {
    const uint32_t t = blockIdx.x * kThreads + threadIdx.x;
    if (t >= T || flags[t]) return;
    uint32_t i0, i1, i2;
    load3(triangles, t, i0, i1, i2);
    const uint32_t at = atomicAdd(tcur + normal_form(i0, i1, i2).a, 1u);
    if (at < T) tbucket[at] = t;  // always, for the counts k_tp_count left
}

// what a walk over (a part of) a group's bucket finds
struct Group {
    uint32_t p, m, first_even, first_odd;
};

__device__ __forceinline__ void look(const int32_t *__restrict__ triangles, uint32_t T, const Tri &me, uint32_t u, Group &g) {
    if (u >= T) return;  // never, for a bucket k_tp_fill_tri left
    uint32_t j0, j1, j2;
    load3(triangles, u, j0, j1, j2);
    const Tri o = normal_form(j0, j1, j2);
    if (o.a != me.a || o.b != me.b || o.c != me.c) return;
    if (o.even) {
        ++g.p;
        g.first_even = u < g.first_even ? u : g.first_even;
    } else {
        ++g.m;
        g.first_odd = u < g.first_odd ? u : g.first_odd;
    }
}

// The status of triangle t from its whole group.  A survivor counts its three edges under their smaller endpoints, marks its
// corners as referenced (plain stores of the same value) and joins them.
__device__ __forceinline__ void settle(uint32_t t, uint32_t i0, uint32_t i1, uint32_t i2, const Group &g, uint8_t *__restrict__ flags,
                                       unsigned long long *__restrict__ ecnt, uint32_t *__restrict__ vref, int32_t *parent) {
    if (g.p == g.m) {
        flags[t] = (uint8_t)kCancelled;
        return;
    }
    if (t != (g.p > g.m ? g.first_even : g.first_odd)) {
        flags[t] = (uint8_t)kDuplicate;
        return;
    }
    atomicAdd(ecnt + (i0 < i1 ? i0 : i1), 1ull);
    atomicAdd(ecnt + (i1 < i2 ? i1 : i2), 1ull);
    atomicAdd(ecnt + (i2 < i0 ? i2 : i0), 1ull);
    vref[i0] = 1u;
    vref[i1] = 1u;
    vref[i2] = 1u;
    unite(parent, (int32_t)i0, (int32_t)i1);
    unite(parent, (int32_t)i0, (int32_t)i2);
}

__global__ __launch_bounds__(kThreads) void k_tp_groups(const int32_t *__restrict__ triangles, uint32_t T,
                                                       const uint32_t *__restrict__ toff, const uint32_t *__restrict__ tbucket,
                                                       uint8_t *__restrict__ flags, unsigned long long *__restrict__ ecnt,
                                                       uint32_t *__restrict__ vref, int32_t *parent, uint32_t *__restrict__ longs,
                                                       uint32_t *__restrict__ nlong) {
    const uint32_t t = blockIdx.x * kThreads + threadIdx.x;
    if (t >= T || flags[t]) return;  // a lane writes the byte of its own triangle only, and reads no other one
    uint32_t i0, i1, i2;
    load3(triangles, t, i0, i1, i2);
    const Tri me = normal_form(i0, i1, i2);
    const uint32_t lo = toff[me.a], hi = toff[me.a + 1];
    if (hi - lo > kLong) {
        const uint32_t at = atomicAdd(nlong, 1u);
        if (at < T) longs[at] = t;
        return;
    }
    Group g = {0u, 0u, 0xffffffffu, 0xffffffffu};
    for (uint32_t k = lo; k < hi; ++k) look(triangles, T, me, tbucket[k], g);
    settle(t, i0, i1, i2, g, flags, ecnt, vref, parent);
}

__global__ __launch_bounds__(kThreads) void k_tp_groups_long(const int32_t *__restrict__ triangles, uint32_t T,
                                                            const uint32_t *__restrict__ toff, const uint32_t *__restrict__ tbucket,
                                                            uint8_t *__restrict__ flags, unsigned long long *__restrict__ ecnt,
                                                            uint32_t *__restrict__ vref, int32_t *parent,
                                                            const uint32_t *__restrict__ longs, const uint32_t *__restrict__ nlong) {
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint32_t nl = *nlong < T ? *nlong : T;
    for (uint32_t i = blockIdx.x * kWaves + threadIdx.x / kWave; i < nl; i += gridDim.x * kWaves) {  // wave-uniform
        const uint32_t t = longs[i];
        if (t >= T) continue;  // never, for a list k_tp_groups left
        uint32_t i0, i1, i2;
        load3(triangles, t, i0, i1, i2);
        const Tri me = normal_form(i0, i1, i2);
        const uint32_t lo = toff[me.a], hi = toff[me.a + 1];
        Group g = {0u, 0u, 0xffffffffu, 0xffffffffu};
        for (uint32_t k = lo + lane; k < hi; k += kWave) look(triangles, T, me, tbucket[k], g);
        g.p = wave_sum(g.p);
        g.m = wave_sum(g.m);
        g.first_even = wave_min(g.first_even);
        g.first_odd = wave_min(g.first_odd);
        if (lane == 0) settle(t, i0, i1, i2, g, flags, ecnt, vref, parent);
    }
}

// E: 3 T, the room of the edge entries
__global__ __launch_bounds__(kThreads) void k_tp_fill_edge(const int32_t *__restrict__ triangles, uint32_t T,
                                                          const uint8_t *__restrict__ flags, unsigned long long *__restrict__ ecnt,
                                                          unsigned long long E, uint2 *__restrict__ edges) {
    const uint32_t t = blockIdx.x * kThreads + threadIdx.x;
    if (t >= T || flags[t]) return;  // the survivors: nothing else has a zero byte after the two group launches
    uint32_t c[3];
    load3(triangles, t, c[0], c[1], c[2]);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const uint32_t u = c[k], w = c[(k + 1) % 3];
        const uint32_t a = u < w ? u : w, b = u < w ? w : u;
        const unsigned long long at = atomicAdd(ecnt + a, 1ull);
        if (at < E) edges[at] = make_uint2(b | (u < w ? 0x80000000u : 0u), t);  // bit 31: traversed a -> b
    }
}

// what a walk over (a part of) an edge's bucket finds
struct Edge {
    uint32_t fwd, bwd, first;
};

__device__ __forceinline__ void look_edge(const uint2 e, uint32_t b, Edge &g) {
    if ((e.x & 0x7fffffffu) != b) return;
    if (e.x >> 31) {
        ++g.fwd;
    } else {
        ++g.bwd;
    }
    g.first = e.y < g.first ? e.y : g.first;
}

// the class bits of a whole edge, and what it adds to the counters when t is the lowest triangle at it
struct Census {
    uint32_t bits, edges, boundary, inconsistent, nonmanifold, unbalanced;
};

__device__ __forceinline__ void classify(const Edge &g, uint32_t t, Census &c) {
    const uint32_t n = g.fwd + g.bwd;
    const bool bd = n == 1u, inc = n == 2u && g.fwd != 1u, nm = n >= 3u, unb = g.fwd != g.bwd;
    c.bits |= (bd ? kBoundary : 0u) | (inc ? kInconsistent : 0u) | (nm ? kNonManifold : 0u);
    if (g.first == t) {
        c.edges += 1u;
        c.boundary += bd ? 1u : 0u;
        c.inconsistent += inc ? 1u : 0u;
        c.nonmanifold += nm ? 1u : 0u;
        c.unbalanced += unb ? 1u : 0u;
    }
}

__global__ __launch_bounds__(kThreads) void k_tp_edges(const int32_t *__restrict__ triangles, uint32_t T, uint32_t V,
                                                      const unsigned long long *__restrict__ eoff, const uint2 *__restrict__ edges,
                                                      uint8_t *__restrict__ flags, uint8_t *__restrict__ tri_flags,
                                                      unsigned long long *__restrict__ counters, uint32_t *__restrict__ longs,
                                                      uint32_t *__restrict__ nlong) {
    const uint32_t t = blockIdx.x * kThreads + threadIdx.x;
    const uint32_t f = t < T ? (uint32_t)flags[t] : 0xffu;
    Census c = {0u, 0u, 0u, 0u, 0u, 0u};
    if (f == 0u) {
        uint32_t v[3];
        load3(triangles, t, v[0], v[1], v[2]);
        unsigned long long lo[3], hi[3];
        uint32_t a[3], b[3];
        bool is_long = false;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const uint32_t u = v[k], w = v[(k + 1) % 3];
            a[k] = u < w ? u : w;
            b[k] = u < w ? w : u;
            lo[k] = eoff[a[k]];
            hi[k] = eoff[a[k] + 1];
            is_long = is_long || hi[k] - lo[k] > kLong;
        }
        if (is_long) {
            const uint32_t at = atomicAdd(nlong, 1u);
            if (at < T) longs[at] = t;
        } else {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                Edge g = {0u, 0u, 0xffffffffu};
                for (unsigned long long i = lo[k]; i < hi[k]; ++i) look_edge(edges[i], b[k], g);
                classify(g, t, c);
            }
            flags[t] = (uint8_t)c.bits;
            if (tri_flags) tri_flags[t] = (uint8_t)c.bits;
        }
    } else if (t < T && tri_flags) {
        tri_flags[t] = (uint8_t)f;
    }
    // every lane of the workgroup arrives here
    wave_count(counters + cInvalid, f == kInvalid ? 1u : 0u);
    wave_count(counters + cDuplicate, f == kDuplicate ? 1u : 0u);
    wave_count(counters + cCancelled, f == kCancelled ? 1u : 0u);
    wave_count(counters + cSurvivors, f == 0u ? 1u : 0u);
    wave_count(counters + cValid, (t < T && f != kInvalid) ? 1u : 0u);
    wave_count(counters + cEdges, c.edges);
    wave_count(counters + cBoundary, c.boundary);
    wave_count(counters + cInconsistent, c.inconsistent);
    wave_count(counters + cNonManifold, c.nonmanifold);
    wave_count(counters + cUnbalanced, c.unbalanced);
}

// The survivors of the list have flags 0 until this launch writes them, and so has no other triangle: k_tp_edges has given every
// survivor that is not on the list its class bits, which may be 0 too -- the list, not the byte, says whom this launch serves.
__global__ __launch_bounds__(kThreads) void k_tp_edges_long(const int32_t *__restrict__ triangles, uint32_t T,
                                                           const unsigned long long *__restrict__ eoff,
                                                           const uint2 *__restrict__ edges, uint8_t *__restrict__ flags,
                                                           uint8_t *__restrict__ tri_flags, unsigned long long *__restrict__ counters,
                                                           const uint32_t *__restrict__ longs, const uint32_t *__restrict__ nlong) {
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint32_t nl = *nlong < T ? *nlong : T;
    for (uint32_t i = blockIdx.x * kWaves + threadIdx.x / kWave; i < nl; i += gridDim.x * kWaves) {  // wave-uniform
        const uint32_t t = longs[i];
        if (t >= T) continue;  // never, for a list k_tp_edges left
        uint32_t v[3];
        load3(triangles, t, v[0], v[1], v[2]);
        Census c = {0u, 0u, 0u, 0u, 0u, 0u};
        for (int k = 0; k < 3; ++k) {
            const uint32_t u = v[k], w = v[(k + 1) % 3];
            const uint32_t a = u < w ? u : w, b = u < w ? w : u;
            const unsigned long long lo = eoff[a], hi = eoff[a + 1];
            Edge g = {0u, 0u, 0xffffffffu};
            for (unsigned long long j = lo + lane; j < hi; j += kWave) look_edge(edges[j], b, g);
            g.fwd = wave_sum(g.fwd);
            g.bwd = wave_sum(g.bwd);
            g.first = wave_min(g.first);
            if (lane == 0) classify(g, t, c);
        }
        if (lane == 0) {
            flags[t] = (uint8_t)c.bits;
            if (tri_flags) tri_flags[t] = (uint8_t)c.bits;
            if (c.edges) atomicAdd(counters + cEdges, (unsigned long long)c.edges);
            if (c.boundary) atomicAdd(counters + cBoundary, (unsigned long long)c.boundary);
            if (c.inconsistent) atomicAdd(counters + cInconsistent, (unsigned long long)c.inconsistent);
            if (c.nonmanifold) atomicAdd(counters + cNonManifold, (unsigned long long)c.nonmanifold);
            if (c.unbalanced) atomicAdd(counters + cUnbalanced, (unsigned long long)c.unbalanced);
        }
    }
}

// Plain loads: the forest no longer changes in this launch (nothing writes `parent`), so the walk passes through ancestors and
// ends at the root.  Terminates as find_root does.
__global__ __launch_bounds__(kThreads) void k_tp_flatten(const int32_t *__restrict__ parent, const uint32_t *__restrict__ vref, uint32_t V,
                                                        int32_t *__restrict__ shell, int32_t *__restrict__ vertex_shell,
                                                        unsigned long long *__restrict__ counters) {
    const uint32_t v = blockIdx.x * kThreads + threadIdx.x;
    bool ref = false, root = false;
    if (v < V) {
        int32_t x = (int32_t)v;
        for (;;) {
            const int32_t p = parent[x];
            if (p == x || p < 0 || p > x) break;  // the last two never, for parents the group launches left
            x = p;
        }
        ref = vref[v] != 0u;
        root = ref && x == (int32_t)v;
        const int32_t label = ref ? x : -1;
        shell[v] = label;
        if (vertex_shell) vertex_shell[v] = label;
    }
    wave_count(counters + cReferenced, ref ? 1u : 0u);
    wave_count(counters + cShells, root ? 1u : 0u);
}

__global__ __launch_bounds__(kThreads) void k_tp_sizes(const int32_t *__restrict__ triangles, uint32_t T, uint32_t V,
                                                      const uint8_t *__restrict__ flags, const int32_t *__restrict__ shell,
                                                      int32_t *__restrict__ tshell, uint32_t *__restrict__ size) {
    const uint32_t t = blockIdx.x * kThreads + threadIdx.x;
    int32_t label = -1;
    if (t < T) {
        if (!((uint32_t)flags[t] & kDead)) {
            const uint32_t i0 = (uint32_t)triangles[3 * (size_t)t];
            if (i0 < V) label = shell[i0];  // always in range, for a survivor
        }
        tshell[t] = label;
    }
    // one add for all lanes of the wave that agree with its first survivor: the giant shell of a real mesh would put every
    // triangle's increment on one address
    const uint64_t live = __ballot(label >= 0);
    if (!live) return;  // wave-uniform
    const int32_t lead = __shfl(label, __ffsll((long long)live) - 1, kWave);
    const uint64_t same = __ballot(label == lead);
    const uint32_t lane = threadIdx.x & (kWave - 1);
    if (label >= 0 && (uint32_t)label < V) {
        if (label != lead) {
            atomicAdd(size + label, 1u);
        } else if (lane == (uint32_t)__ffsll((long long)same) - 1u) {
            atomicAdd(size + label, (uint32_t)__popcll(same));
        }
    }
}

// (size << 32) | ~label: the greatest size wins, and among equal sizes the smallest label
__global__ __launch_bounds__(kThreads) void k_tp_largest(const int32_t *__restrict__ shell, const uint32_t *__restrict__ size, uint32_t V,
                                                        unsigned long long *best) {
    __shared__ unsigned long long red[kWaves];
    const uint32_t v = blockIdx.x * kThreads + threadIdx.x;
    const uint32_t s = (v < V && shell[v] == (int32_t)v) ? size[v] : 0u;
    const unsigned long long x = block_max(s ? ((unsigned long long)s << 32) | (unsigned long long)(~v) : 0ull, red);
    if (threadIdx.x == 0 && x) atomicMax(best, x);
}

__global__ void k_tp_totals(const unsigned long long *__restrict__ counters, int64_t *__restrict__ totals) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    for (int i = 0; i < 12; ++i) totals[i] = (int64_t)counters[i];
    const unsigned long long best = counters[cBest];
    totals[12] = (int64_t)(best >> 32);
    totals[13] = best ? (int64_t)(~(uint32_t)best) : -1;
    totals[14] = 0;
    totals[15] = 0;
}

// V == 0 or T == 0: no survivor
__global__ __launch_bounds__(kThreads) void k_tp_trivial(uint32_t V, uint32_t T, int64_t *__restrict__ totals,
                                                        uint8_t *__restrict__ tri_flags, int32_t *__restrict__ vertex_shell) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i < T && tri_flags) tri_flags[i] = (uint8_t)kInvalid;
    if (i < V && vertex_shell) vertex_shell[i] = -1;
    if (i == 0) {
        for (int k = 0; k < PVD_MESH_TOPO_TOTALS; ++k) totals[k] = 0;
        totals[cInvalid] = (int64_t)T;
        totals[13] = -1;
    }
}

// ------------------------------------------------------------------------------------------------------------------ clean
__device__ __forceinline__ bool shell_kept(int32_t label, uint32_t V, const uint32_t *__restrict__ size, unsigned long long best,
                                           uint32_t min_size, uint32_t largest_only) {
    if (label < 0 || (uint32_t)label >= V) return false;
    if (size[label] < min_size) return false;
    return !largest_only || (best && (uint32_t)label == ~(uint32_t)best);
}

__global__ __launch_bounds__(kThreads) void k_tp_keep_tri(const int32_t *__restrict__ tshell, uint32_t T, uint32_t V,
                                                         const uint32_t *__restrict__ size, const unsigned long long *__restrict__ counters,
                                                         uint32_t min_size, uint32_t largest_only, uint32_t *__restrict__ ft) {
    const uint32_t t = blockIdx.x * kThreads + threadIdx.x;
    if (t < T) ft[t] = shell_kept(tshell[t], V, size, counters[cBest], min_size, largest_only) ? 1u : 0u;
}

// a vertex is kept iff a kept triangle uses it: iff it is referenced and its shell is kept (every survivor at it is of that shell)
__global__ __launch_bounds__(kThreads) void k_tp_keep_vertex(const int32_t *__restrict__ shell, uint32_t V, const uint32_t *__restrict__ size,
                                                            const unsigned long long *__restrict__ counters, uint32_t min_size,
                                                            uint32_t largest_only, uint32_t *__restrict__ fv) {
    const uint32_t v = blockIdx.x * kThreads + threadIdx.x;
    if (v < V) fv[v] = shell_kept(shell[v], V, size, counters[cBest], min_size, largest_only) ? 1u : 0u;
}

__global__ void k_tp_counts(const uint32_t *__restrict__ words, int64_t *__restrict__ counts, uint32_t none) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    counts[0] = none ? 0 : (int64_t)words[wKeptV];
    counts[1] = none ? 0 : (int64_t)words[wKeptT];
}

// sv [V + 1]: the exclusive scan of the keep flags and their total; a vertex is kept iff its successor's offset is larger
__global__ __launch_bounds__(kThreads) void k_tp_emit_vertex(const uint32_t *__restrict__ vbits, uint32_t V, const uint32_t *__restrict__ sv,
                                                            uint32_t *__restrict__ out_bits, int32_t *__restrict__ vertex_map) {
    const uint32_t v = blockIdx.x * kThreads + threadIdx.x;
    if (v >= V) return;
    const uint32_t at = sv[v];
    const bool kept = sv[v + 1] > at;
    vertex_map[v] = kept ? (int32_t)at : -1;
    if (kept && out_bits) {
#pragma unroll
        for (int a = 0; a < 3; ++a) out_bits[3 * (size_t)at + a] = vbits[3 * (size_t)v + a];
    }
}

__global__ __launch_bounds__(kThreads) void k_tp_emit_tri(const int32_t *__restrict__ triangles, uint32_t T, uint32_t V,
                                                         const uint32_t *__restrict__ st, const uint32_t *__restrict__ sv,
                                                         int32_t *__restrict__ out_triangles, int32_t *__restrict__ triangle_map) {
    const uint32_t t = blockIdx.x * kThreads + threadIdx.x;
    if (t >= T) return;
    const uint32_t at = st[t];
    const bool kept = st[t + 1] > at;
    triangle_map[t] = kept ? (int32_t)at : -1;
    if (kept && out_triangles) {
        uint32_t c[3];
        load3(triangles, t, c[0], c[1], c[2]);
#pragma unroll
        for (int k = 0; k < 3; ++k) out_triangles[3 * (size_t)at + k] = c[k] < V ? (int32_t)sv[c[k]] : -1;  // in range, for a survivor
    }
}

// V == 0 or T == 0: nothing is kept
__global__ __launch_bounds__(kThreads) void k_tp_emit_none(uint32_t V, uint32_t T, int32_t *__restrict__ vertex_map,
                                                          int32_t *__restrict__ triangle_map) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i < V) vertex_map[i] = -1;
    if (i < T) triangle_map[i] = -1;
}

int check_args(uint32_t V, uint32_t T, const void *workspace, size_t workspace_bytes) {
    if (!workspace || ((uintptr_t)workspace & 15u)) return PVD_ERR_INVALID;
    if (workspace_bytes < layout(V, T).total) return PVD_ERR_INVALID;
    return PVD_OK;
}

uint32_t list_blocks(uint32_t T) {
    const uint32_t n = div_up(T, kWaves);
    return n < kLongBlocks ? n : kLongBlocks;
}

}  // namespace

#define PVD_TP_LAUNCH(kernel, blocks, threads, ...)                                     \
    do {                                                                                \
        hipLaunchKernelGGL(kernel, dim3(blocks), dim3(threads), 0, st, __VA_ARGS__);    \
        if ((rc = check_launch()) != PVD_OK) return rc;                                 \
    } while (0)

extern "C" {

size_t pvd_mesh_topo_workspace_bytes(uint32_t V, uint32_t T) { return in_limits(V, T) ? layout(V, T).total : 0; }

int pvd_mesh_topo_build(const float *vertices, uint32_t V, const int32_t *triangles, uint32_t T, void *workspace,
                        size_t workspace_bytes, int64_t *totals_dev, uint8_t *tri_flags, int32_t *vertex_shell, pvd_stream_t stream) {
    if (!in_limits(V, T)) return PVD_ERR_UNSUPPORTED;
    if (!totals_dev) return PVD_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    int rc;
    if (V == 0 || T == 0) {
        const uint32_t n = V > T ? V : T;
        PVD_TP_LAUNCH(k_tp_trivial, n ? div_up(n, kThreads) : 1u, kThreads, V, T, totals_dev, tri_flags, vertex_shell);
        return PVD_OK;
    }
    if (!vertices || !triangles) return PVD_ERR_INVALID;
    if ((rc = check_args(V, T, workspace, workspace_bytes)) != PVD_OK) return rc;
    const Ws w = arrays(workspace, V, T);
    const uint32_t *vbits = (const uint32_t *)vertices;
    const uint32_t NV = div_up(V, kThreads), NT = div_up(T, kThreads);
    if ((rc = check_memset(hipMemsetAsync(w.counters, 0, 8 * (size_t)kCounters, st))) != PVD_OK) return rc;
    PVD_TP_LAUNCH(k_tp_init, NV, kThreads, V, w.parent, w.tcur, w.ecnt, w.size, w.vref, w.words);
    PVD_TP_LAUNCH(k_tp_count, NT, kThreads, vbits, V, triangles, T, w.flags, w.tcur);
    PVD_TP_LAUNCH(k_blocksum<uint32_t>, NV, kThreads, (const uint32_t *)w.tcur, V, w.tbsum);
    PVD_TP_LAUNCH(k_scan<uint32_t>, 1, kScanThreads, w.tbsum, NV, w.toff + V, w.words + wTriTotal);
    PVD_TP_LAUNCH(k_offsets<uint32_t>, NV, kThreads, w.tcur, V, (const uint32_t *)w.tbsum, w.toff);
    PVD_TP_LAUNCH(k_tp_fill_tri, NT, kThreads, triangles, T, (const uint8_t *)w.flags, w.tcur, w.tbucket);
    PVD_TP_LAUNCH(k_tp_groups, NT, kThreads, triangles, T, (const uint32_t *)w.toff, (const uint32_t *)w.tbucket, w.flags, w.ecnt, w.vref,
                  w.parent, w.longs, w.words + wLongTri);
    PVD_TP_LAUNCH(k_tp_groups_long, list_blocks(T), kThreads, triangles, T, (const uint32_t *)w.toff, (const uint32_t *)w.tbucket, w.flags,
                  w.ecnt, w.vref, w.parent, (const uint32_t *)w.longs, (const uint32_t *)(w.words + wLongTri));
    PVD_TP_LAUNCH(k_blocksum<unsigned long long>, NV, kThreads, (const unsigned long long *)w.ecnt, V, w.ebsum);
    PVD_TP_LAUNCH(k_scan<unsigned long long>, 1, kScanThreads, w.ebsum, NV, w.eoff + V, w.counters + cEdgeTotal);
    PVD_TP_LAUNCH(k_offsets<unsigned long long>, NV, kThreads, w.ecnt, V, (const unsigned long long *)w.ebsum, w.eoff);
    PVD_TP_LAUNCH(k_tp_fill_edge, NT, kThreads, triangles, T, (const uint8_t *)w.flags, w.ecnt, 3ull * T, w.edges);
    PVD_TP_LAUNCH(k_tp_edges, NT, kThreads, triangles, T, V, (const unsigned long long *)w.eoff, (const uint2 *)w.edges, w.flags, tri_flags,
                  w.counters, w.longs, w.words + wLongEdge);
    PVD_TP_LAUNCH(k_tp_edges_long, list_blocks(T), kThreads, triangles, T, (const unsigned long long *)w.eoff, (const uint2 *)w.edges, w.flags,
                  tri_flags, w.counters, (const uint32_t *)w.longs, (const uint32_t *)(w.words + wLongEdge));
    PVD_TP_LAUNCH(k_tp_flatten, NV, kThreads, (const int32_t *)w.parent, (const uint32_t *)w.vref, V, w.shell, vertex_shell, w.counters);
    PVD_TP_LAUNCH(k_tp_sizes, NT, kThreads, triangles, T, V, (const uint8_t *)w.flags, (const int32_t *)w.shell, w.tshell, w.size);
    PVD_TP_LAUNCH(k_tp_largest, NV, kThreads, (const int32_t *)w.shell, (const uint32_t *)w.size, V, w.counters + cBest);
    PVD_TP_LAUNCH(k_tp_totals, 1, 1, (const unsigned long long *)w.counters, totals_dev);
    return PVD_OK;
}

int pvd_mesh_topo_clean_count(uint32_t V, uint32_t T, void *workspace, size_t workspace_bytes, uint32_t min_shell_triangles,
                              uint32_t largest_only, int64_t *counts_dev, pvd_stream_t stream) {
    if (!in_limits(V, T)) return PVD_ERR_UNSUPPORTED;
    if (!counts_dev) return PVD_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    int rc;
    if (V == 0 || T == 0) {
        PVD_TP_LAUNCH(k_tp_counts, 1, 1, (const uint32_t *)nullptr, counts_dev, 1u);
        return PVD_OK;
    }
    if ((rc = check_args(V, T, workspace, workspace_bytes)) != PVD_OK) return rc;
    const Ws w = arrays(workspace, V, T);
    const uint32_t NV = div_up(V, kThreads), NT = div_up(T, kThreads);
    PVD_TP_LAUNCH(k_tp_keep_tri, NT, kThreads, (const int32_t *)w.tshell, T, V, (const uint32_t *)w.size,
                  (const unsigned long long *)w.counters, min_shell_triangles, largest_only, w.ft);
    PVD_TP_LAUNCH(k_tp_keep_vertex, NV, kThreads, (const int32_t *)w.shell, V, (const uint32_t *)w.size,
                  (const unsigned long long *)w.counters, min_shell_triangles, largest_only, w.fv);
    PVD_TP_LAUNCH(k_blocksum<uint32_t>, NV, kThreads, (const uint32_t *)w.fv, V, w.bsv);
    PVD_TP_LAUNCH(k_scan<uint32_t>, 1, kScanThreads, w.bsv, NV, w.sv + V, w.words + wKeptV);
    PVD_TP_LAUNCH(k_offsets<uint32_t>, NV, kThreads, w.fv, V, (const uint32_t *)w.bsv, w.sv);
    PVD_TP_LAUNCH(k_blocksum<uint32_t>, NT, kThreads, (const uint32_t *)w.ft, T, w.bst);
    PVD_TP_LAUNCH(k_scan<uint32_t>, 1, kScanThreads, w.bst, NT, w.st + T, w.words + wKeptT);
    PVD_TP_LAUNCH(k_offsets<uint32_t>, NT, kThreads, w.ft, T, (const uint32_t *)w.bst, w.st);
    PVD_TP_LAUNCH(k_tp_counts, 1, 1, (const uint32_t *)w.words, counts_dev, 0u);
    return PVD_OK;
}

int pvd_mesh_topo_clean_emit(const float *vertices, uint32_t V, const int32_t *triangles, uint32_t T, void *workspace,
                             size_t workspace_bytes, float *out_vertices, int32_t *out_triangles, int32_t *vertex_map,
                             int32_t *triangle_map, pvd_stream_t stream) {
    if (!in_limits(V, T)) return PVD_ERR_UNSUPPORTED;
    if ((V && !vertex_map) || (T && !triangle_map)) return PVD_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    int rc;
    if (V == 0 || T == 0) {
        const uint32_t n = V > T ? V : T;
        if (n) PVD_TP_LAUNCH(k_tp_emit_none, div_up(n, kThreads), kThreads, V, T, vertex_map, triangle_map);
        return PVD_OK;
    }
    if (!vertices || !triangles) return PVD_ERR_INVALID;
    if ((rc = check_args(V, T, workspace, workspace_bytes)) != PVD_OK) return rc;
    const Ws w = arrays(workspace, V, T);
    PVD_TP_LAUNCH(k_tp_emit_vertex, div_up(V, kThreads), kThreads, (const uint32_t *)vertices, V, (const uint32_t *)w.sv,
                  (uint32_t *)out_vertices, vertex_map);
    PVD_TP_LAUNCH(k_tp_emit_tri, div_up(T, kThreads), kThreads, triangles, T, V, (const uint32_t *)w.st, (const uint32_t *)w.sv, out_triangles,
                  triangle_map);
    return PVD_OK;
}

}  // extern "C"
