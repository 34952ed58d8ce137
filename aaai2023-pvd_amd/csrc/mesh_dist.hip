// mesh_dist.hip -- the distance from many points to a triangle mesh (include/pvd_hip_mesh_dist.h): a uniform grid over the
// triangles' centroids, built on the device, and an exact nearest-triangle search over its Chebyshev rings, float64 per test.
//
// k_md_count     one lane per triangle: validity, the centroid's cell (kept per triangle for the fill pass), one integer atomicAdd
//                on the cell's count, one atomicMax on rho (the bits of a non-negative float order like unsigned integers).
// k_blocksum, k_scan, k_offsets   (csrc/block_scan.h) the per-cell counts -> the cell's start and, the same value,
//                its fill cursor; the total (the number of valid triangles) to start[C] and to the header.
// k_md_fill      one lane per triangle: a slot from the cell's cursor (integer atomicAdd), the nine coordinates and the index into it.
// k_md_query     one lane per point: rings of cells around the point's cell until no unvisited triangle can win.
// The count -> one-workgroup scan -> offsets shape of csrc/block_scan.h: no workgroup waits on another one of the same launch, and
// no loop retries an atomic.  The order of the triangles inside a cell depends on the run; the query's (d, index) minimum does not.
#include "block_scan.h"
#include "mesh_grid.h"

#include "../../include/pvd_hip_mesh_dist.h"

namespace {

using namespace pvd;

constexpr uint32_t kNoCell = 0xffffffffu;
constexpr uint32_t kMaxT = 0x7fffffffu;

// header words (uint32): 0 = rho (float bits), 1..3 = bmin, 4..6 = bmax (float bits), 7 = valid triangles; 64 bytes in all
constexpr size_t kHeaderBytes = 64;

struct Layout {  // byte offsets into the workspace; the 16-byte records first, so that a 16-byte aligned workspace aligns them
    size_t packed, start, cursor, bsum, tcell, total;
};

inline Layout layout(uint32_t T, uint32_t G) {
    const size_t C = (size_t)G * G * G, NB = (C + kThreads - 1) / kThreads;
    Layout l;
    l.packed = kHeaderBytes;
    l.start = l.packed + 48 * (size_t)T;
    l.cursor = l.start + 4 * (C + 1);
    l.bsum = l.cursor + 4 * C;
    l.tcell = l.bsum + 4 * NB;
    l.total = l.tcell + 4 * (size_t)T;
    return l;
}

// the pure parts (cells, distance, ring walk) are PVD_HD, __host__ __device__: a CPU build can walk the same code
PVD_HD float next_up(float x) { return u2f(f2u(x) + 1u); }  // the float above a finite non-negative float
PVD_HD int imin(int a, int b) { return a < b ? a : b; }
PVD_HD int imax(int a, int b) { return a > b ? a : b; }

struct Box {  // per axis: the origin, cells per unit length (0 on a flat axis); h_min over the axes that are not flat (0: none)
    double lo[3], inv_h[3], h_min;
};

PVD_HD Box box_of(const float *__restrict__ bmin3, const float *__restrict__ bmax3, uint32_t G) {
    Box b;
    b.h_min = 0.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double lo = (double)bmin3[a], hi = (double)bmax3[a];
        const double ext = hi - lo;
        const bool ok = ext > 0.0 && ext < (double)INFINITY;  // false for NaN
        b.lo[a] = ok ? lo : 0.0;
        b.inv_h[a] = ok ? (double)G / ext : 0.0;
        if (ok) {
            const double h = ext / (double)G;
            b.h_min = b.h_min > 0.0 ? fmin(b.h_min, h) : h;
        }
    }
    return b;
}

// the cell of a valid triangle's centroid, and the largest distance from the centroid to a corner, rounded up twice over: the
// float64 square root scaled up by more than its rounding, then to the float above
PVD_HD uint32_t bin_triangle(const Box &box, uint32_t G, const float a[3], const float b[3], const float c[3], float *rho) {
    double ra = 0.0, rb = 0.0, rc = 0.0;
    int k[3];
    for (int q = 0; q < 3; ++q) {
        const double m = ((double)a[q] + (double)b[q] + (double)c[q]) / 3.0;
        k[q] = cell_axis(box, q, m, G);
        const double da = (double)a[q] - m, db = (double)b[q] - m, dc = (double)c[q] - m;
        ra += da * da;
        rb += db * db;
        rc += dc * dc;
    }
    const double r = sqrt(fmax(ra, fmax(rb, rc))) * (1.0 + 0x1p-50);
    const float f = (float)r;
    *rho = (double)f < r ? next_up(f) : f;  // (an infinite f stays infinite: r is then infinite too)
    return ((uint32_t)k[0] * G + (uint32_t)k[1]) * G + (uint32_t)k[2];
}

// the grid has at least one workgroup, so that the box reaches the header when T == 0 too
__global__ __launch_bounds__(kThreads) void k_md_count(const float *__restrict__ vertices, uint32_t V, const int32_t *__restrict__ triangles,
                                                      uint32_t T, const float *__restrict__ bmin3, const float *__restrict__ bmax3, uint32_t G,
                                                      uint32_t *__restrict__ header, uint32_t *__restrict__ cursor,
                                                      uint32_t *__restrict__ tcell) {
    const uint32_t t = blockIdx.x * kThreads + threadIdx.x;
    if (t < 3) {
        header[1 + t] = f2u(bmin3[t]);
        header[4 + t] = f2u(bmax3[t]);
    }
    if (t >= T) return;
    const int32_t ia = triangles[3 * (size_t)t], ib = triangles[3 * (size_t)t + 1], ic = triangles[3 * (size_t)t + 2];
    uint32_t cell = kNoCell;
    if ((uint32_t)ia < V && (uint32_t)ib < V && (uint32_t)ic < V) {  // a negative index is a large unsigned one
        const float *pa = vertices + 3 * (size_t)ia, *pb = vertices + 3 * (size_t)ib, *pc = vertices + 3 * (size_t)ic;
        const float a[3] = {pa[0], pa[1], pa[2]}, b[3] = {pb[0], pb[1], pb[2]}, c[3] = {pc[0], pc[1], pc[2]};
        if (finite3(a[0], a[1], a[2]) && finite3(b[0], b[1], b[2]) && finite3(c[0], c[1], c[2])) {
            float rho;
            cell = bin_triangle(box_of(bmin3, bmax3, G), G, a, b, c, &rho);  // the query reads the same six floats from the header
            atomicAdd(&cursor[cell], 1u);
            atomicMax(&header[0], f2u(rho));
        }
    }
    tcell[t] = cell;
}

__global__ __launch_bounds__(kThreads) void k_md_fill(const float *__restrict__ vertices, const int32_t *__restrict__ triangles, uint32_t T,
                                                     const uint32_t *__restrict__ tcell, uint32_t *__restrict__ cursor,
                                                     float4 *__restrict__ packed) {
    const uint32_t t = blockIdx.x * kThreads + threadIdx.x;
    if (t >= T) return;
    const uint32_t cell = tcell[t];
    if (cell == kNoCell) return;
    const uint32_t slot = atomicAdd(&cursor[cell], 1u);
    if (slot >= T) return;  // cannot happen (the cursors partition 0 .. valid triangles); keeps a damaged workspace inside itself
    const float *pa = vertices + 3 * (size_t)triangles[3 * (size_t)t], *pb = vertices + 3 * (size_t)triangles[3 * (size_t)t + 1],
                *pc = vertices + 3 * (size_t)triangles[3 * (size_t)t + 2];
    float4 *o = packed + 3 * (size_t)slot;
    o[0] = make_float4(pa[0], pa[1], pa[2], pb[0]);
    o[1] = make_float4(pb[1], pb[2], pc[0], pc[1]);
    o[2] = make_float4(pc[2], u2f(t), 0.0f, 0.0f);
}

// ---------------------------------------------------------------------------------------------- the distance, in float64
PVD_HD double dot3(const double u[3], const double v[3]) { return u[0] * v[0] + u[1] * v[1] + u[2] * v[2]; }

// squared distance from the origin-shifted point (ap = p - a) to the segment a -> a + e
PVD_HD double segment_d2(const double ap[3], const double e[3]) {
    const double L = dot3(e, e);
    double s = L > 0.0 ? dot3(ap, e) / L : 0.0;
    s = fmin(1.0, fmax(0.0, s));
    const double r[3] = {ap[0] - s * e[0], ap[1] - s * e[1], ap[2] - s * e[2]};
    return dot3(r, r);
}

PVD_HD double triangle_d2(const double p[3], const double a[3], const double b[3], const double c[3]) {
    const double ab[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, ac[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
    const double ap[3] = {p[0] - a[0], p[1] - a[1], p[2] - a[2]};
    const double n[3] = {ab[1] * ac[2] - ab[2] * ac[1], ab[2] * ac[0] - ab[0] * ac[2], ab[0] * ac[1] - ab[1] * ac[0]};
    const double nn = dot3(n, n);
    const double bp[3] = {p[0] - b[0], p[1] - b[1], p[2] - b[2]};
    if (nn <= 0x1p-40 * dot3(ab, ab) * dot3(ac, ac)) {  // degenerate: the three segments
        const double bc[3] = {c[0] - b[0], c[1] - b[1], c[2] - b[2]};
        return fmin(segment_d2(ap, ab), fmin(segment_d2(ap, ac), segment_d2(bp, bc)));
    }
    const double d1 = dot3(ab, ap), d2 = dot3(ac, ap);
    if (d1 <= 0.0 && d2 <= 0.0) return dot3(ap, ap);  // corner a
    const double d3 = dot3(ab, bp), d4 = dot3(ac, bp);
    if (d3 >= 0.0 && d4 <= d3) return dot3(bp, bp);  // corner b
    const double cp[3] = {p[0] - c[0], p[1] - c[1], p[2] - c[2]};
    const double d5 = dot3(ab, cp), d6 = dot3(ac, cp);
    if (d6 >= 0.0 && d5 <= d6) return dot3(cp, cp);  // corner c
    if (d1 * d4 - d3 * d2 <= 0.0 && d1 >= 0.0 && d3 <= 0.0) return segment_d2(ap, ab);  // edge ab
    if (d5 * d2 - d1 * d6 <= 0.0 && d2 >= 0.0 && d6 <= 0.0) return segment_d2(ap, ac);  // edge ac
    if (d3 * d6 - d5 * d4 <= 0.0 && d4 - d3 >= 0.0 && d5 - d6 >= 0.0) {                 // edge bc
        const double bc[3] = {c[0] - b[0], c[1] - b[1], c[2] - b[2]};
        return segment_d2(bp, bc);
    }
    const double s = dot3(n, ap);
    return s * s / nn;  // interior: the distance to the plane
}

struct Best {
    float d;      // the best rounded distance so far (starts at max_dist)
    int32_t t;    // its triangle (starts above every index)
    double thr2;  // next_up(d)^2, exact in float64: a test with d^2 >= thr2 rounds to a float above d and cannot win
};

// the triangles in the slots [s0, s1) of the packed array
PVD_HD void visit(const float4 *__restrict__ packed, uint32_t s0, uint32_t s1, const double p[3], Best &best) {
    for (uint32_t s = s0; s < s1; ++s) {
        const float4 q0 = packed[3 * (size_t)s], q1 = packed[3 * (size_t)s + 1], q2 = packed[3 * (size_t)s + 2];
        const double a[3] = {(double)q0.x, (double)q0.y, (double)q0.z}, b[3] = {(double)q0.w, (double)q1.x, (double)q1.y};
        const double c[3] = {(double)q1.z, (double)q1.w, (double)q2.x};
        const double d2 = triangle_d2(p, a, b, c);
        if (!(d2 < best.thr2)) continue;  // the common case, without the square root
        const float d = (float)sqrt(d2);
        const int32_t t = (int32_t)f2u(q2.y);
        if (d < best.d || (d == best.d && t < best.t)) {
            best.d = d;
            best.t = t;
            const double u = (double)next_up(d);
            best.thr2 = u * u;
        }
    }
}

// the search of one finite point: (best distance below max_dist or max_dist, its triangle or -1)
PVD_HD void query_point(const double p[3], uint32_t T, uint32_t G, const uint32_t *__restrict__ header, const uint32_t *__restrict__ start,
                        const float4 *__restrict__ packed, float max_dist, float *out_d, int32_t *out_t) {
    const Box box = box_of((const float *)(header + 1), (const float *)(header + 4), G);
    const double rho = (double)u2f(header[0]);
    const int g = (int)G, c0 = cell_axis(box, 0, p[0], G), c1 = cell_axis(box, 1, p[1], G), c2 = cell_axis(box, 2, p[2], G);
    const int r_last = imax(imax(imax(c0, g - 1 - c0), imax(c1, g - 1 - c1)), imax(c2, g - 1 - c2));
    Best best;
    best.d = max_dist;
    best.t = 0x7fffffff;
    {
        const double u = (double)next_up(max_dist);  // max_dist == FLT_MAX: infinity, and every finite d^2 is below it
        best.thr2 = u * u;
    }
    const uint32_t valid = umin(header[7], T);  // every slot index below is clamped to it: a damaged workspace stays inside itself
    for (int r = 0; r <= r_last; ++r) {
        const int x0 = imax(c0 - r, 0), x1 = imin(c0 + r, g - 1), y0 = imax(c1 - r, 0), y1 = imin(c1 + r, g - 1);
        const int z0 = imax(c2 - r, 0), z1 = imin(c2 + r, g - 1);
        for (int x = x0; x <= x1; ++x) {
            for (int y = y0; y <= y1; ++y) {
                const uint32_t row = ((uint32_t)x * G + (uint32_t)y) * G;
                if (x - c0 == r || c0 - x == r || y - c1 == r || c1 - y == r) {
                    // the whole z-run of the row belongs to the ring: consecutive cells, so one range of slots
                    visit(packed, umin(start[row + z0], valid), umin(start[row + z1 + 1], valid), p, best);
                } else {  // r > 0 here: only the two end cells, where they are in the grid
                    if (c2 - r >= 0) visit(packed, umin(start[row + c2 - r], valid), umin(start[row + c2 - r + 1], valid), p, best);
                    if (c2 + r < g) visit(packed, umin(start[row + c2 + r], valid), umin(start[row + c2 + r + 1], valid), p, best);
                }
            }
        }
        // best.d <= max_dist throughout; the factors: include/pvd_hip_mesh_dist.h, "Search"
        if ((double)r * box.h_min * (1.0 - 0x1p-20) - rho * (1.0 + 0x1p-20) > (double)best.d * (1.0 + 0x1p-20)) break;
    }
    const bool found = best.d < max_dist;
    *out_d = found ? best.d : max_dist;
    *out_t = found ? best.t : -1;
}

__global__ __launch_bounds__(kThreads) void k_md_query(const float *__restrict__ points, uint32_t N, uint32_t T, uint32_t G,
                                                      const uint32_t *__restrict__ header, const uint32_t *__restrict__ start,
                                                      const float4 *__restrict__ packed, float max_dist, float *__restrict__ dist,
                                                      int32_t *__restrict__ tri) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= N) return;
    const float px = points[3 * (size_t)i], py = points[3 * (size_t)i + 1], pz = points[3 * (size_t)i + 2];
    if (!finite3(px, py, pz)) {
        dist[i] = u2f(0x7fc00000u);
        tri[i] = -1;
        return;
    }
    const double p[3] = {(double)px, (double)py, (double)pz};
    float d;
    int32_t t;
    query_point(p, T, G, header, start, packed, max_dist, &d, &t);
    dist[i] = d;
    tri[i] = t;
}

int check_args(uint32_t T, uint32_t G, const void *workspace, size_t workspace_bytes) {
    if (!workspace || ((uintptr_t)workspace & 15u)) return PVD_ERR_INVALID;
    if (G < 1 || G > PVD_MESH_DIST_MAX_G || T > kMaxT) return PVD_ERR_UNSUPPORTED;
    if (workspace_bytes < layout(T, G).total) return PVD_ERR_INVALID;
    return PVD_OK;
}

}  // namespace

extern "C" {

size_t pvd_mesh_dist_workspace_bytes(uint32_t T, uint32_t G) {
    return (G < 1 || G > PVD_MESH_DIST_MAX_G || T > kMaxT) ? 0 : layout(T, G).total;
}

int pvd_mesh_dist_build(const float *vertices, uint32_t V, const int32_t *triangles, uint32_t T, const float *bmin3, const float *bmax3,
                        uint32_t G, void *workspace, size_t workspace_bytes, pvd_stream_t stream) {
    if (!bmin3 || !bmax3 || (T && !triangles) || (T && V && !vertices)) return PVD_ERR_INVALID;
    int rc = check_args(T, G, workspace, workspace_bytes);
    if (rc != PVD_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    const Layout l = layout(T, G);
    const uint32_t C = G * G * G, NB = div_up(C, kThreads), TB = T ? div_up(T, kThreads) : 1u;
    char *ws = (char *)workspace;
    uint32_t *header = (uint32_t *)ws, *start = (uint32_t *)(ws + l.start), *cursor = (uint32_t *)(ws + l.cursor);
    uint32_t *bsum = (uint32_t *)(ws + l.bsum), *tcell = (uint32_t *)(ws + l.tcell);
    float4 *packed = (float4 *)(ws + l.packed);
    if ((rc = check_memset(hipMemsetAsync(header, 0, kHeaderBytes, st))) != PVD_OK) return rc;
    if ((rc = check_memset(hipMemsetAsync(cursor, 0, 4 * (size_t)C, st))) != PVD_OK) return rc;
    hipLaunchKernelGGL(k_md_count, dim3(TB), dim3(kThreads), 0, st, vertices, V, triangles, T, bmin3, bmax3, G, header, cursor, tcell);
    if ((rc = check_launch()) != PVD_OK) return rc;
    hipLaunchKernelGGL(k_blocksum<uint32_t>, dim3(NB), dim3(kThreads), 0, st, cursor, C, bsum);
    if ((rc = check_launch()) != PVD_OK) return rc;
    hipLaunchKernelGGL(k_scan<uint32_t>, dim3(1), dim3(kScanThreads), 0, st, bsum, NB, start + C, header + 7);
    if ((rc = check_launch()) != PVD_OK) return rc;
    hipLaunchKernelGGL(k_offsets<uint32_t>, dim3(NB), dim3(kThreads), 0, st, cursor, C, bsum, start);
    if ((rc = check_launch()) != PVD_OK) return rc;
    if (T == 0) return PVD_OK;
    hipLaunchKernelGGL(k_md_fill, dim3(TB), dim3(kThreads), 0, st, vertices, triangles, T, tcell, cursor, packed);
    return check_launch();
}

int pvd_mesh_dist_query(const float *points, uint32_t N, uint32_t T, uint32_t G, const void *workspace, size_t workspace_bytes,
                        float max_dist, float *dist, int32_t *tri, pvd_stream_t stream) {
    if (!(max_dist > 0.0f && max_dist < INFINITY)) return PVD_ERR_INVALID;  // false for NaN
    const int rc = check_args(T, G, workspace, workspace_bytes);
    if (rc != PVD_OK) return rc;
    if (N == 0) return PVD_OK;
    if (!points || !dist || !tri) return PVD_ERR_INVALID;
    const Layout l = layout(T, G);
    const char *ws = (const char *)workspace;
    hipLaunchKernelGGL(k_md_query, dim3(div_up(N, kThreads)), dim3(kThreads), 0, (hipStream_t)stream, points, N, T, G, (const uint32_t *)ws,
                       (const uint32_t *)(ws + l.start), (const float4 *)(ws + l.packed), max_dist, dist, tri);
    return check_launch();
}

}  // extern "C"
