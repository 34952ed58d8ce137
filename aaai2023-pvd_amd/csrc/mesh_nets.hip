// mesh_nets.hip -- naive surface nets for the level set u = thresh of a density volume (csrc/pvd_hip_mesh_nets.h): one vertex per active
// cell, at the mean of the cell's edge crossings, and one quad -- two triangles, split along the shorter diagonal -- per crossing interior
// lattice edge.  The second mesher next to the marching tetrahedra of csrc/mesh.hip, in the same count / scan / emit shape.
//
// reference: extract_fields / extract_geometry, distill_mutual/utils.py:442-488 (mcubes.marching_cubes on the host).
//
// k_nets_count      one lane per lattice point p (k fastest, so a wave reads consecutive floats): the 8 corners of p's cell -> one byte of
//                   flags (kActive: the cell is active; kQuad << a: the edge p -> p + e_a crosses and is interior; kInside: p is inside)
//                   and the sums of the two counts -- vertices (0..1) and triangles (0, 2, 4, 6) -- over the workgroup's 256 points.
// k_nets_scan       ONE workgroup: the exclusive scan of both arrays of sums in place, side by side (scan_sums, csrc/block_scan.h); the
//                   two totals to totals_dev.
// k_nets_offsets    one lane per lattice point: exclusive scan of the two counts inside the workgroup + the workgroup's base -> the index
//                   of the cell's vertex and of the point's first triangle.
// k_nets_vertices   one lane per lattice point: the vertex of an active cell, from the crossings of its 12 edges in ascending order.
// k_nets_triangles  one lane per lattice point, after k_nets_vertices: per quad flag the four cells around the edge -- a neighbour cell's
//                   vertex index is its offset --, the two diagonals from the emitted positions, two triangles.  Reads no field.
// k_nets_normals    one lane per lattice point: the normal of an active cell's vertex, from the lattice gradients at its 8 corners.
// No workgroup waits on another one of the same launch, nothing is atomic, and the output does not depend on the order in which
// workgroups run.
//
// NO LDS TILE OF THE FIELD.  A lane's 8 corner loads are 2 consecutive floats of 4 rows; across a wave each row is 65 consecutive floats,
// i.e. whole cache lines that the lanes share, and the rows j + 1 and i + 1 are the rows j and i of lanes R and R * R further on, which the
// vector L1 and L2 hold (the count pass, the only one that touches every point's corners, streams the field once from HBM; its other
// traffic is one byte per point).  A tile would need a halo in three directions for a LINEAR range of 256 points that is not a box of
// the lattice (R is any number 2 .. 512), a barrier per tile, and would save loads that already hit the caches.  The emit and normal passes
// touch the field only in active cells, a surface's worth of the volume.  profiles/mesh_nets.txt has the kernel times next to one read of
// the field.
#include "block_scan.h"
#include "mesh_gradient.h"

#include "pvd_hip_mesh_nets.h"

#pragma clang fp contract(off)

namespace {

using namespace pvd;

constexpr uint32_t kActive = 1u, kQuad = 2u, kInside = 16u;  // kQuad << a, a = 0..2

struct Layout {  // byte offsets into the workspace
    size_t voff, toff, bsum_v, bsum_t, flags, total;
};

inline Layout layout(uint32_t R) {  // the 32-bit arrays first, so that a 4-byte aligned workspace aligns them all
    const size_t N = (size_t)R * R * R, NB = (N + kThreads - 1) / kThreads;
    Layout l;
    l.voff = 0;
    l.toff = l.voff + 4 * N;
    l.bsum_v = l.toff + 4 * N;
    l.bsum_t = l.bsum_v + 4 * NB;
    l.flags = l.bsum_t + 4 * NB;
    l.total = l.flags + N;
    return l;
}

// corner code of an offset (ox, oy, oz) in {0,1}^3: ox * 4 + oy * 2 + oz; the bit of axis a in a code
__host__ __device__ constexpr uint32_t axis_bit(uint32_t a) { return 4u >> a; }
// edge e = 4a + 2 o_b + o_c of a cell: its axis and the corner codes of its ends A and B = A + e_a
__host__ __device__ constexpr uint32_t edge_axis(uint32_t e) { return e >> 2; }
__host__ __device__ constexpr uint32_t edge_a(uint32_t e) {
    return ((e >> 1) & 1u) * axis_bit((edge_axis(e) + 1) % 3) + (e & 1u) * axis_bit((edge_axis(e) + 2) % 3);
}
__host__ __device__ constexpr uint32_t edge_b(uint32_t e) { return edge_a(e) | axis_bit(edge_axis(e)); }
// mask of the crossing edges of a cell from the inside bits of its corners (bit = corner code)
__device__ __forceinline__ uint32_t crossing_edges(uint32_t in) {
    uint32_t m = 0;
#pragma unroll
    for (uint32_t e = 0; e < PVD_MESH_NETS_CELL_EDGES; ++e) m |= (((in >> edge_a(e)) ^ (in >> edge_b(e))) & 1u) << e;
    return m;
}

// Inside a workgroup the vertex count (low half) and the triangle count (high half) of a point travel as one word: a point counts at most
// 1 vertex and 6 triangles, so neither half of a sum over kThreads points reaches 2^16.
constexpr uint32_t kPairShift = 16, kPairMask = 0xffffu;
static_assert(6u * kThreads <= kPairMask, "a half of the pair overflows into the other");

__device__ __forceinline__ uint32_t counts_of(uint32_t f) { return (f & kActive) | ((2u * (uint32_t)__popc((f >> 1) & 7u)) << kPairShift); }

__global__ __launch_bounds__(kThreads) void k_nets_count(const float *__restrict__ u, uint32_t R, uint32_t N, float thresh,
                                                        uint8_t *__restrict__ flags, uint32_t *__restrict__ bsum_v,
                                                        uint32_t *__restrict__ bsum_t) {
    __shared__ uint32_t red[kWaves];
    const uint32_t n = blockIdx.x * kThreads + threadIdx.x;
    uint32_t f = 0;
    if (n < N) {
        const uint32_t i = n / (R * R), r = n - i * R * R, j = r / R, k = r - j * R;
        // the inside bits of the 8 corners, bit = corner code; a corner outside the lattice is not read
        uint32_t in = 0;
        const bool xi = i + 1 < R, xj = j + 1 < R, xk = k + 1 < R;
#pragma unroll
        for (uint32_t c = 0; c < 8; ++c) {
            const uint32_t ox = c >> 2, oy = (c >> 1) & 1u, oz = c & 1u;
            if ((!ox || xi) && (!oy || xj) && (!oz || xk)) {
                if (u[n + (ox * R + oy) * R + oz] > thresh) in |= 1u << c;
            }
        }
        if (xi && xj && xk && in != 0u && in != 0xffu) f |= kActive;
        if (in & 1u) f |= kInside;
        const uint32_t p[3] = {i, j, k};
#pragma unroll
        for (uint32_t a = 0; a < 3; ++a) {
            const uint32_t b = (a + 1) % 3, c = (a + 2) % 3;
            const bool interior = p[a] + 1 < R && p[b] >= 1 && p[b] + 1 < R && p[c] >= 1 && p[c] + 1 < R;
            if (interior && (((in >> axis_bit(a)) ^ in) & 1u)) f |= kQuad << a;  // (p + e_a exists, so its bit was read)
        }
        flags[n] = (uint8_t)f;
    }
    const uint32_t s = block_sum(counts_of(f), red);
    if (threadIdx.x == 0) {
        bsum_v[blockIdx.x] = s & kPairMask;
        bsum_t[blockIdx.x] = s >> kPairShift;
    }
}

// one workgroup; sums [NB] -> exclusive scan in place, for both arrays; totals[0], totals[1]
__global__ __launch_bounds__(kScanThreads) void k_nets_scan(uint32_t *__restrict__ bsum_v, uint32_t *__restrict__ bsum_t, uint32_t NB,
                                                           uint32_t *__restrict__ totals) {
    uint32_t *const sums[2] = {bsum_v, bsum_t};
    uint32_t total[2];
    scan_sums(sums, NB, total);
    if (threadIdx.x == 0) {
        totals[0] = total[0];
        totals[1] = total[1];
    }
}

__global__ __launch_bounds__(kThreads) void k_nets_offsets(const uint8_t *__restrict__ flags, uint32_t N, const uint32_t *__restrict__ bsum_v,
                                                          const uint32_t *__restrict__ bsum_t, uint32_t *__restrict__ voff,
                                                          uint32_t *__restrict__ toff) {
    __shared__ uint32_t wtot[kWaves];
    const uint32_t n = blockIdx.x * kThreads + threadIdx.x;
    const uint32_t e = block_exclusive(n < N ? counts_of(flags[n]) : 0u, wtot);
    if (n < N) {
        voff[n] = bsum_v[blockIdx.x] + (e & kPairMask);
        toff[n] = bsum_t[blockIdx.x] + (e >> kPairShift);
    }
}

// the 8 corner values of the ACTIVE cell at lattice point n (all of them are lattice points) and their inside bits
__device__ __forceinline__ uint32_t load_cell(const float *__restrict__ u, uint32_t R, uint32_t n, float thresh, float uc[8]) {
    uint32_t in = 0;
#pragma unroll
    for (uint32_t c = 0; c < 8; ++c) {
        uc[c] = u[n + ((c >> 2) * R + ((c >> 1) & 1u)) * R + (c & 1u)];
        if (uc[c] > thresh) in |= 1u << c;
    }
    return in;
}

__global__ __launch_bounds__(kThreads) void k_nets_vertices(const float *__restrict__ u, uint32_t R, uint32_t N, float thresh,
                                                           const float *__restrict__ bmin3, const float *__restrict__ bmax3,
                                                           const uint8_t *__restrict__ flags, const uint32_t *__restrict__ voff,
                                                           float *__restrict__ vertices, uint32_t V) {
    const uint32_t n = blockIdx.x * kThreads + threadIdx.x;
    if (n >= N || !(flags[n] & kActive)) return;
    const uint32_t at = voff[n];
    if (at >= V) return;
    const uint32_t i = n / (R * R), r = n - i * R * R, j = r / R, k = r - j * R;
    float uc[8];
    const uint32_t cross = crossing_edges(load_cell(u, R, n, thresh, uc));
    float s[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
    for (uint32_t e = 0; e < PVD_MESH_NETS_CELL_EDGES; ++e) {
        if ((cross >> e) & 1u) {
            const uint32_t a = edge_axis(e), b = (a + 1) % 3, c = (a + 2) % 3;
            const float ua = uc[edge_a(e)], ub = uc[edge_b(e)];
            const float t = (thresh - ua) / (ub - ua);
            s[a] = s[a] + t;
            s[b] = s[b] + (float)((e >> 1) & 1u);
            s[c] = s[c] + (float)(e & 1u);
        }
    }
    const float cnt = (float)__popc(cross), rm1 = (float)(R - 1);
    const float q[3] = {(float)i, (float)j, (float)k};
    float *v = vertices + 3 * (size_t)at;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float lo = bmin3[a], ext = bmax3[a] - lo;
        const float m = s[a] / cnt;
        v[a] = (q[a] + m) / rm1 * ext + lo;
    }
}

__global__ __launch_bounds__(kThreads) void k_nets_triangles(uint32_t R, uint32_t N, const uint8_t *__restrict__ flags,
                                                            const uint32_t *__restrict__ voff, const uint32_t *__restrict__ toff,
                                                            const float *__restrict__ vertices, uint32_t V, int32_t *__restrict__ triangles,
                                                            uint32_t T) {
    const uint32_t n = blockIdx.x * kThreads + threadIdx.x;
    if (n >= N) return;
    const uint32_t f = flags[n];
    if (!(f & (7u * kQuad))) return;
    const uint32_t stride[3] = {R * R, R, 1u};
    uint32_t tri = toff[n];
#pragma unroll
    for (uint32_t a = 0; a < 3; ++a) {
        if (!(f & (kQuad << a))) continue;
        if (tri < T) {
            const uint32_t sb = stride[(a + 1) % 3], sc = stride[(a + 2) % 3];  // an interior edge: p_b, p_c >= 1, so the four cells exist
            const uint32_t q0 = voff[n - sb - sc], q1 = voff[n - sc], q2 = voff[n], q3 = voff[n - sb];
            const bool in = (f & kInside) != 0;
            const uint32_t k0 = q0, k1 = in ? q1 : q3, k2 = q2, k3 = in ? q3 : q1;
            float d02 = NAN, d13 = NAN;
            if (k0 < V && k1 < V && k2 < V && k3 < V) {
                const float *p0 = vertices + 3 * (size_t)k0, *p1 = vertices + 3 * (size_t)k1, *p2 = vertices + 3 * (size_t)k2,
                            *p3 = vertices + 3 * (size_t)k3;
                const float ax = p2[0] - p0[0], ay = p2[1] - p0[1], az = p2[2] - p0[2];
                const float bx = p3[0] - p1[0], by = p3[1] - p1[1], bz = p3[2] - p1[2];
                d02 = (ax * ax + ay * ay) + az * az;
                d13 = (bx * bx + by * by) + bz * bz;
            }
            int32_t *o = triangles + 3 * (size_t)tri;
            const bool other = d13 < d02;  // false on ties and NaN
            o[0] = (int32_t)k0;
            o[1] = (int32_t)k1;
            o[2] = (int32_t)(other ? k3 : k2);
            if (tri + 1 < T) {  // (T is even when it is the total of the count pass)
                o[3] = (int32_t)(other ? k1 : k0);
                o[4] = (int32_t)k2;
                o[5] = (int32_t)k3;
            }
        }
        tri += 2;
    }
}

__global__ __launch_bounds__(kThreads) void k_nets_normals(const float *__restrict__ u, uint32_t R, uint32_t N, float thresh,
                                                          const float *__restrict__ bmin3, const float *__restrict__ bmax3,
                                                          const uint8_t *__restrict__ flags, const uint32_t *__restrict__ voff,
                                                          float *__restrict__ normals, uint32_t V) {
    const uint32_t n = blockIdx.x * kThreads + threadIdx.x;
    if (n >= N || !(flags[n] & kActive)) return;
    const uint32_t at = voff[n];
    if (at >= V) return;
    const uint32_t i = n / (R * R), r = n - i * R * R, j = r / R, k = r - j * R;
    const float rm1 = (float)(R - 1);
    const float inv_h[3] = {rm1 / (bmax3[0] - bmin3[0]), rm1 / (bmax3[1] - bmin3[1]), rm1 / (bmax3[2] - bmin3[2])};
    float uc[8], g[8][3];
    const uint32_t cross = crossing_edges(load_cell(u, R, n, thresh, uc));
#pragma unroll
    for (uint32_t c = 0; c < 8; ++c) {
        const uint32_t ox = c >> 2, oy = (c >> 1) & 1u, oz = c & 1u;
        const uint32_t cc[3] = {i + ox, j + oy, k + oz};
        world_gradient(u, R, n + (ox * R + oy) * R + oz, cc, inv_h, g[c]);
    }
    float G[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
    for (uint32_t e = 0; e < PVD_MESH_NETS_CELL_EDGES; ++e) {
        if ((cross >> e) & 1u) {
            const uint32_t A = edge_a(e), B = edge_b(e);
            const float t = (thresh - uc[A]) / (uc[B] - uc[A]);
#pragma unroll
            for (int a = 0; a < 3; ++a) G[a] = G[a] + (g[A][a] + t * (g[B][a] - g[A][a]));
        }
    }
    const float cnt = (float)__popc(cross);
    const float gx = G[0] / cnt, gy = G[1] / cnt, gz = G[2] / cnt;
    const float len = sqrtf(gx * gx + gy * gy + gz * gz);
    const bool ok = len > 0.0f && len < INFINITY;  // false for NaN
    float *o = normals + 3 * (size_t)at;
    o[0] = ok ? -gx / len : 0.0f;
    o[1] = ok ? -gy / len : 0.0f;
    o[2] = ok ? -gz / len : 0.0f;
}

int check_args(const void *field, uint32_t R, const void *workspace, size_t workspace_bytes) {
    if (!field || !workspace || ((uintptr_t)workspace & 3u)) return PVD_ERR_INVALID;
    if (R < 2 || R > PVD_MESH_MAX_R) return PVD_ERR_UNSUPPORTED;
    if (workspace_bytes < layout(R).total) return PVD_ERR_INVALID;
    return PVD_OK;
}

}  // namespace

extern "C" {

size_t pvd_mesh_nets_workspace_bytes(uint32_t R) { return (R < 2 || R > PVD_MESH_MAX_R) ? 0 : layout(R).total; }

int pvd_mesh_nets_count(const float *field, uint32_t R, float thresh, void *workspace, size_t workspace_bytes, uint32_t *totals_dev,
                        pvd_stream_t stream) {
    if (!totals_dev) return PVD_ERR_INVALID;
    int rc = check_args(field, R, workspace, workspace_bytes);
    if (rc != PVD_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    const Layout l = layout(R);
    const uint32_t N = R * R * R, NB = div_up(N, kThreads);
    char *ws = (char *)workspace;
    uint32_t *voff = (uint32_t *)(ws + l.voff), *toff = (uint32_t *)(ws + l.toff);
    uint32_t *bsum_v = (uint32_t *)(ws + l.bsum_v), *bsum_t = (uint32_t *)(ws + l.bsum_t);
    uint8_t *flags = (uint8_t *)(ws + l.flags);
    hipLaunchKernelGGL(k_nets_count, dim3(NB), dim3(kThreads), 0, st, field, R, N, thresh, flags, bsum_v, bsum_t);
    if ((rc = check_launch()) != PVD_OK) return rc;
    hipLaunchKernelGGL(k_nets_scan, dim3(1), dim3(kScanThreads), 0, st, bsum_v, bsum_t, NB, totals_dev);
    if ((rc = check_launch()) != PVD_OK) return rc;
    hipLaunchKernelGGL(k_nets_offsets, dim3(NB), dim3(kThreads), 0, st, flags, N, bsum_v, bsum_t, voff, toff);
    return check_launch();
}

int pvd_mesh_nets_emit(const float *field, uint32_t R, float thresh, const float *bmin3, const float *bmax3, const void *workspace,
                       size_t workspace_bytes, float *vertices, uint32_t V, int32_t *triangles, uint32_t T, pvd_stream_t stream) {
    if (!bmin3 || !bmax3) return PVD_ERR_INVALID;
    int rc = check_args(field, R, workspace, workspace_bytes);
    if (rc != PVD_OK) return rc;
    if (V == 0 && T == 0) return PVD_OK;
    if ((V && !vertices) || (T && !triangles)) return PVD_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const Layout l = layout(R);
    const uint32_t N = R * R * R, NB = div_up(N, kThreads);
    const char *ws = (const char *)workspace;
    const uint8_t *flags = (const uint8_t *)(ws + l.flags);
    const uint32_t *voff = (const uint32_t *)(ws + l.voff), *toff = (const uint32_t *)(ws + l.toff);
    if (V) {
        hipLaunchKernelGGL(k_nets_vertices, dim3(NB), dim3(kThreads), 0, st, field, R, N, thresh, bmin3, bmax3, flags, voff, vertices, V);
        if ((rc = check_launch()) != PVD_OK) return rc;
    }
    if (T) {
        hipLaunchKernelGGL(k_nets_triangles, dim3(NB), dim3(kThreads), 0, st, R, N, flags, voff, toff, (const float *)vertices, V, triangles, T);
        rc = check_launch();
    }
    return rc;
}

int pvd_mesh_nets_normals(const float *field, uint32_t R, float thresh, const float *bmin3, const float *bmax3, const void *workspace,
                          size_t workspace_bytes, float *normals, uint32_t V, pvd_stream_t stream) {
    if (!bmin3 || !bmax3) return PVD_ERR_INVALID;
    const int rc = check_args(field, R, workspace, workspace_bytes);
    if (rc != PVD_OK) return rc;
    if (V == 0) return PVD_OK;
    if (!normals) return PVD_ERR_INVALID;
    const Layout l = layout(R);
    const uint32_t N = R * R * R, NB = div_up(N, kThreads);
    const char *ws = (const char *)workspace;
    hipLaunchKernelGGL(k_nets_normals, dim3(NB), dim3(kThreads), 0, (hipStream_t)stream, field, R, N, thresh, bmin3, bmax3,
                       (const uint8_t *)(ws + l.flags), (const uint32_t *)(ws + l.voff), normals, V);
    return check_launch();
}

}  // extern "C"
