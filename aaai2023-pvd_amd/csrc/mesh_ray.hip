// mesh_ray.hip -- the first hit of many rays on a triangle mesh (include/pvd_hip_mesh_ray.h): a uniform grid over the triangles'
// dilated bounding boxes, built on the device, and a 3D-DDA walk per ray with the watertight test in unfused float64.
//
// k_mr_count     one lane per triangle: validity, inside / outside, the number of cells of its range; one integer atomicAdd per
//                wave on each of the two 64-bit totals.
// k_mr_bin       one lane per triangle: the packed record (index -1: invalid), one integer atomicAdd per cell of its range on the
//                cell's count, or a slot of the outside list.
// k_blocksum, k_scan, k_offsets   (csrc/block_scan.h) the per-cell counts -> the cell starts and fill cursors; the
//                total (the number of pairs) to start[C] and to the header.
// k_mr_fill      one lane per triangle: per cell of its range a slot from the cell's cursor (integer atomicAdd), its index into it.
// k_mr_cast      one lane per ray: clip, walk, outside list.  No LDS, no atomics.
// No workgroup waits on another one of the same launch, and no loop retries an atomic.  The order of the pairs inside a cell depends
// on the run; the cast's (t, index) minimum does not.
#include "block_scan.h"
#include "mesh_grid.h"

#include "../../include/pvd_hip_mesh_ray.h"

namespace {

using namespace pvd;

constexpr uint32_t kMaxT = 0x7fffffffu;
constexpr uint64_t kMaxPairs = 0x7fffffffull;

// header words (uint32): 0 = outside triangles (the list's cursor), 1..3 = bmin, 4..6 = bmax (float bits), 7 = pairs; 64 bytes in all
constexpr size_t kHeaderBytes = 64;

struct Layout {  // byte offsets into the workspace; the 16-byte records first, so that a 16-byte aligned workspace aligns them
    size_t packed, start, cursor, bsum, outside, pairs, total;
};

inline Layout layout(uint32_t T, uint32_t G, uint64_t pairs) {
    const size_t C = (size_t)G * G * G, NB = (C + kThreads - 1) / kThreads;
    Layout l;
    l.packed = kHeaderBytes;
    l.start = l.packed + 48 * (size_t)T;
    l.cursor = l.start + 4 * (C + 1);
    l.bsum = l.cursor + 4 * C;
    l.outside = l.bsum + 4 * NB;
    l.pairs = l.outside + 4 * (size_t)T;
    l.total = l.pairs + 4 * (size_t)pairs;
    return l;
}

// the pure parts (box, ranges, the test, the walk) are PVD_HD, __host__ __device__: a CPU build can walk the same code
PVD_HD float sel3(float x, float y, float z, int k) { return k == 0 ? x : (k == 1 ? y : z); }

struct Box {  // per axis: flat (one layer from -inf to +inf), the bounds, the cell size and its inverse, the dilation eps
    bool flat[3];
    double lo[3], hi[3], h[3], inv_h[3], eps[3];
};

PVD_HD Box box_of(const float *__restrict__ bmin3, const float *__restrict__ bmax3, uint32_t G) {
    Box b;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double lo = (double)bmin3[a], hi = (double)bmax3[a];
        const double ext = hi - lo;
        const bool ok = ext > 0.0 && ext < (double)INFINITY;  // false for NaN
        b.flat[a] = !ok;
        b.lo[a] = ok ? lo : 0.0;
        b.hi[a] = ok ? hi : 0.0;
        b.h[a] = ok ? ext / (double)G : 0.0;
        b.inv_h[a] = ok ? (double)G / ext : 0.0;
        b.eps[a] = ok ? 0x1p-20 * ext : 0.0;
    }
    return b;
}

enum : int { kInvalid = 0, kInside = 1, kOutside = 2 };

// the class of triangle t and, for an inside one, its range of cells k0 .. k1 per axis
PVD_HD int classify(const float *__restrict__ vertices, uint32_t V, const int32_t *__restrict__ triangles, uint32_t t, const Box &box,
                    uint32_t G, int k0[3], int k1[3], float corners[9]) {
    const int32_t ia = triangles[3 * (size_t)t], ib = triangles[3 * (size_t)t + 1], ic = triangles[3 * (size_t)t + 2];
    if (!((uint32_t)ia < V && (uint32_t)ib < V && (uint32_t)ic < V)) return kInvalid;  // a negative index is a large unsigned one
    const float *pa = vertices + 3 * (size_t)ia, *pb = vertices + 3 * (size_t)ib, *pc = vertices + 3 * (size_t)ic;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        corners[q] = pa[q];
        corners[3 + q] = pb[q];
        corners[6 + q] = pc[q];
    }
    if (!(finite3(corners[0], corners[1], corners[2]) && finite3(corners[3], corners[4], corners[5]) &&
          finite3(corners[6], corners[7], corners[8])))
        return kInvalid;
    bool inside = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double mn = (double)fminf(corners[a], fminf(corners[3 + a], corners[6 + a]));
        const double mx = (double)fmaxf(corners[a], fmaxf(corners[3 + a], corners[6 + a]));
        if (!box.flat[a] && !(box.lo[a] <= mn && mx <= box.hi[a])) inside = false;
        k0[a] = cell_axis(box, a, mn - box.eps[a], G);
        k1[a] = cell_axis(box, a, mx + box.eps[a], G);
    }
    return inside ? kInside : kOutside;
}

// a triangle's range holds at most 2^24 cells and a wave 64 triangles: the wave's sum fits 32 bits, the totals are 64 bits wide
__global__ __launch_bounds__(kThreads) void k_mr_count(const float *__restrict__ vertices, uint32_t V, const int32_t *__restrict__ triangles,
                                                      uint32_t T, const float *__restrict__ bmin3, const float *__restrict__ bmax3, uint32_t G,
                                                      unsigned long long *__restrict__ totals) {
    const uint32_t t = blockIdx.x * kThreads + threadIdx.x;
    uint32_t cells = 0, out = 0;
    if (t < T) {
        int k0[3], k1[3];
        float c[9];
        const int cls = classify(vertices, V, triangles, t, box_of(bmin3, bmax3, G), G, k0, k1, c);
        if (cls == kInside) cells = (uint32_t)(k1[0] - k0[0] + 1) * (uint32_t)(k1[1] - k0[1] + 1) * (uint32_t)(k1[2] - k0[2] + 1);
        out = cls == kOutside ? 1u : 0u;
    }
    cells = wave_sum(cells);
    out = wave_sum(out);
    if ((threadIdx.x & (kWave - 1)) == 0) {
        if (cells) atomicAdd(&totals[0], (unsigned long long)cells);
        if (out) atomicAdd(&totals[1], (unsigned long long)out);
    }
}

// the grid has at least one workgroup, so that the box reaches the header when T == 0 too
__global__ __launch_bounds__(kThreads) void k_mr_bin(const float *__restrict__ vertices, uint32_t V, const int32_t *__restrict__ triangles,
                                                    uint32_t T, const float *__restrict__ bmin3, const float *__restrict__ bmax3, uint32_t G,
                                                    uint32_t *__restrict__ header, uint32_t *__restrict__ cursor,
                                                    uint32_t *__restrict__ outside, float4 *__restrict__ packed) {
    const uint32_t t = blockIdx.x * kThreads + threadIdx.x;
    if (t < 3) {
        header[1 + t] = f2u(bmin3[t]);
        header[4 + t] = f2u(bmax3[t]);
    }
    if (t >= T) return;
    int k0[3], k1[3];
    float c[9] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    const int cls = classify(vertices, V, triangles, t, box_of(bmin3, bmax3, G), G, k0, k1, c);
    float4 *o = packed + 3 * (size_t)t;
    o[0] = make_float4(c[0], c[1], c[2], c[3]);
    o[1] = make_float4(c[4], c[5], c[6], c[7]);
    o[2] = make_float4(c[8], u2f(cls == kInvalid ? 0xffffffffu : t), 0.0f, 0.0f);
    if (cls == kInside) {
        for (int x = k0[0]; x <= k1[0]; ++x)
            for (int y = k0[1]; y <= k1[1]; ++y)
                for (int z = k0[2]; z <= k1[2]; ++z) atomicAdd(&cursor[((uint32_t)x * G + (uint32_t)y) * G + (uint32_t)z], 1u);
    } else if (cls == kOutside) {
        const uint32_t slot = atomicAdd(&header[0], 1u);
        if (slot < T) outside[slot] = t;  // (always: at most T triangles are outside)
    }
}

__global__ __launch_bounds__(kThreads) void k_mr_fill(const float *__restrict__ vertices, uint32_t V, const int32_t *__restrict__ triangles,
                                                     uint32_t T, const uint32_t *__restrict__ header, uint32_t G, uint32_t pairs,
                                                     uint32_t *__restrict__ cursor, uint32_t *__restrict__ list) {
    const uint32_t t = blockIdx.x * kThreads + threadIdx.x;
    if (t >= T) return;
    int k0[3], k1[3];
    float c[9];
    // the same box, bit for bit, as k_mr_bin read: the ranges agree with the counts
    if (classify(vertices, V, triangles, t, box_of((const float *)(header + 1), (const float *)(header + 4), G), G, k0, k1, c) != kInside) return;
    for (int x = k0[0]; x <= k1[0]; ++x)
        for (int y = k0[1]; y <= k1[1]; ++y)
            for (int z = k0[2]; z <= k1[2]; ++z) {
                const uint32_t slot = atomicAdd(&cursor[((uint32_t)x * G + (uint32_t)y) * G + (uint32_t)z], 1u);
                if (slot < pairs) list[slot] = t;  // a `pairs` below the true total loses pairs and stays inside the workspace
            }
}

// ------------------------------------------------------------------------------------------- the watertight test, in float64
struct Ray {  // the ray's constants, once per lane: the permuted origin, the shear, the permutation
    double ox, oy, oz, Sx, Sy, Sz;
    int kx, ky, kz;
};

PVD_HD Ray ray_of(const double o[3], const double d[3]) {
    Ray r;
    const double ax = fabs(d[0]), ay = fabs(d[1]), az = fabs(d[2]);
    r.kz = ax >= ay && ax >= az ? 0 : (ay >= az ? 1 : 2);  // argmax |d|, ties to the lowest axis
    r.kx = (r.kz + 1) % 3;
    r.ky = (r.kx + 1) % 3;
    const double dz = r.kz == 0 ? d[0] : (r.kz == 1 ? d[1] : d[2]);
    if (dz < 0.0) {
        const int s = r.kx;
        r.kx = r.ky;
        r.ky = s;
    }
    const double dx = r.kx == 0 ? d[0] : (r.kx == 1 ? d[1] : d[2]), dy = r.ky == 0 ? d[0] : (r.ky == 1 ? d[1] : d[2]);
    r.Sx = dx / dz;
    r.Sy = dy / dz;
    r.Sz = 1.0 / dz;
    r.ox = r.kx == 0 ? o[0] : (r.kx == 1 ? o[1] : o[2]);
    r.oy = r.ky == 0 ? o[0] : (r.ky == 1 ? o[1] : o[2]);
    r.oz = r.kz == 0 ? o[0] : (r.kz == 1 ? o[1] : o[2]);
    return r;
}

struct Best {
    double t;     // the best t so far (starts at t_max)
    int32_t tri;  // its triangle (-1: none yet)
    double v, w;  // V / det, W / det of the best
};

// record j of the packed array against the ray: include/pvd_hip_mesh_ray.h, steps 3 .. 8 and "Result"
PVD_HD void test(const float4 *__restrict__ packed, uint32_t j, const Ray &r, double t_min, double t_max, Best &best) {
#pragma clang fp contract(off)
    const float4 q0 = packed[3 * (size_t)j], q1 = packed[3 * (size_t)j + 1], q2 = packed[3 * (size_t)j + 2];
    const int32_t idx = (int32_t)f2u(q2.y);
    if (idx < 0) return;  // an invalid triangle
    const double Ax = (double)sel3(q0.x, q0.y, q0.z, r.kx) - r.ox, Ay = (double)sel3(q0.x, q0.y, q0.z, r.ky) - r.oy;
    const double Az = (double)sel3(q0.x, q0.y, q0.z, r.kz) - r.oz;
    const double Bx = (double)sel3(q0.w, q1.x, q1.y, r.kx) - r.ox, By = (double)sel3(q0.w, q1.x, q1.y, r.ky) - r.oy;
    const double Bz = (double)sel3(q0.w, q1.x, q1.y, r.kz) - r.oz;
    const double Cx = (double)sel3(q1.z, q1.w, q2.x, r.kx) - r.ox, Cy = (double)sel3(q1.z, q1.w, q2.x, r.ky) - r.oy;
    const double Cz = (double)sel3(q1.z, q1.w, q2.x, r.kz) - r.oz;
    const double Xa = Ax - r.Sx * Az, Ya = Ay - r.Sy * Az;
    const double Xb = Bx - r.Sx * Bz, Yb = By - r.Sy * Bz;
    const double Xc = Cx - r.Sx * Cz, Yc = Cy - r.Sy * Cz;
    const double U = Xc * Yb - Yc * Xb, V = Xa * Yc - Ya * Xc, W = Xb * Ya - Yb * Xa;
    if ((U < 0.0 || V < 0.0 || W < 0.0) && (U > 0.0 || V > 0.0 || W > 0.0)) return;
    const double det = (U + V) + W;
    if (det == 0.0) return;
    const double Za = r.Sz * Az, Zb = r.Sz * Bz, Zc = r.Sz * Cz;
    const double t = ((U * Za + V * Zb) + W * Zc) / det;
    if (!(t >= t_min && t < t_max)) return;  // false for NaN
    if (t < best.t || (t == best.t && best.tri >= 0 && idx < best.tri)) {  // best.t <= t_max throughout
        best.t = t;
        best.tri = idx;
        best.v = V / det;
        best.w = W / det;
    }
}

// the search of one valid ray
PVD_HD void cast_ray(const double o[3], const double d[3], uint32_t T, uint32_t G, const uint32_t *__restrict__ header,
                     const uint32_t *__restrict__ start, const uint32_t *__restrict__ list, const uint32_t *__restrict__ outside,
                     const float4 *__restrict__ packed, uint32_t pairs, double t_min, double t_max, Best &best) {
    const Ray r = ray_of(o, d);
    const Box box = box_of((const float *)(header + 1), (const float *)(header + 4), G);
    best.t = t_max;
    best.tri = -1;
    best.v = best.w = 0.0;
    // every index below is clamped: a damaged workspace stays inside itself
    const uint32_t n_pairs = umin(header[7], pairs), n_out = umin(header[0], T);
    // (1) clip to the dilated slabs
    double t0 = t_min, t1 = t_max, inv_d[3];
    bool touches = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        inv_d[a] = 0.0;
        if (box.flat[a]) continue;
        const double e4 = 0.25 * box.eps[a];
        if (d[a] == 0.0) {
            if (o[a] < box.lo[a] - e4 || o[a] > box.hi[a] + e4) touches = false;
            continue;
        }
        inv_d[a] = 1.0 / d[a];
        const double ta = ((box.lo[a] - e4) - o[a]) * inv_d[a], tb = ((box.hi[a] + e4) - o[a]) * inv_d[a];
        t0 = fmax(t0, fmin(ta, tb));
        t1 = fmin(t1, fmax(ta, tb));
    }
    touches = touches && t0 <= t1;
    if (touches) {  // far rays: the rounding of a position is no longer small against eps
        bool far = false;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            if (box.flat[a]) continue;
            double M = fabs(o[a]) + fabs(box.lo[a]) + fabs(box.hi[a]);
            if (d[a] != 0.0) M += fabs(d[a]) * t1;  // t1 is finite here: this axis has clipped it
            if (!(0x1p-40 * M <= box.eps[a])) far = true;
        }
        if (far) {
            for (uint32_t j = 0; j < T; ++j) test(packed, j, r, t_min, t_max, best);
            return;
        }
        // (2) the start cell
        int k[3], step[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            k[a] = box.flat[a] ? 0 : cell_axis(box, a, o[a] + t0 * d[a], G);
            step[a] = (box.flat[a] || d[a] == 0.0) ? 0 : (d[a] > 0.0 ? 1 : -1);
        }
        for (uint32_t it = 0; it < 3u * G; ++it) {  // at most 3 (G - 1) steps
            // (3) the cell's triangles
            const uint32_t c = ((uint32_t)k[0] * G + (uint32_t)k[1]) * G + (uint32_t)k[2];
            const uint32_t s1 = umin(start[c + 1], n_pairs);
            for (uint32_t s = umin(start[c], n_pairs); s < s1; ++s) {
                const uint32_t j = list[s];
                if (j < T) test(packed, j, r, t_min, t_max, best);
            }
            // (4) the exit, from the integer face
            double t_exit = (double)INFINITY;
            int axis = -1;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                if (step[a] == 0) continue;
                const double face = box.lo[a] + (double)(k[a] + (step[a] > 0 ? 1 : 0)) * box.h[a];
                const double te = (face - o[a]) * inv_d[a];
                if (te < t_exit) {
                    t_exit = te;
                    axis = a;
                }
            }
            // (5) stop or step
            if (axis < 0 || !(t_exit < t1)) break;
            if (best.tri >= 0 && best.t < t_exit * (1.0 - 0x1p-30)) break;
            k[axis] += step[axis];
            if (k[axis] < 0 || k[axis] >= (int)G) break;
        }
    }
    // (6) the outside list
    for (uint32_t s = 0; s < n_out; ++s) {
        const uint32_t j = outside[s];
        if (j < T) test(packed, j, r, t_min, t_max, best);
    }
}

__global__ __launch_bounds__(kThreads) void k_mr_cast(const float *__restrict__ origins, const float *__restrict__ dirs, uint32_t N, uint32_t T,
                                                     uint32_t G, uint32_t pairs, const uint32_t *__restrict__ header,
                                                     const uint32_t *__restrict__ start, const uint32_t *__restrict__ list,
                                                     const uint32_t *__restrict__ outside, const float4 *__restrict__ packed, float t_min,
                                                     float t_max, float *__restrict__ out_t, int32_t *__restrict__ out_tri,
                                                     float *__restrict__ out_bary) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= N) return;
    const float ox = origins[3 * (size_t)i], oy = origins[3 * (size_t)i + 1], oz = origins[3 * (size_t)i + 2];
    const float dx = dirs[3 * (size_t)i], dy = dirs[3 * (size_t)i + 1], dz = dirs[3 * (size_t)i + 2];
    if (!finite3(ox, oy, oz) || !finite3(dx, dy, dz) || (dx == 0.0f && dy == 0.0f && dz == 0.0f)) {
        out_t[i] = u2f(0x7fc00000u);
        out_tri[i] = -1;
        out_bary[2 * (size_t)i] = 0.0f;
        out_bary[2 * (size_t)i + 1] = 0.0f;
        return;
    }
    const double o[3] = {(double)ox, (double)oy, (double)oz}, d[3] = {(double)dx, (double)dy, (double)dz};
    Best best;
    cast_ray(o, d, T, G, header, start, list, outside, packed, pairs, (double)t_min, (double)t_max, best);
    const bool hit = best.tri >= 0;
    out_t[i] = hit ? (float)best.t : t_max;
    out_tri[i] = hit ? best.tri : -1;
    out_bary[2 * (size_t)i] = hit ? (float)best.v : 0.0f;
    out_bary[2 * (size_t)i + 1] = hit ? (float)best.w : 0.0f;
}

bool in_range(uint32_t T, uint32_t G, uint64_t pairs) { return G >= 1 && G <= PVD_MESH_RAY_MAX_G && T <= kMaxT && pairs <= kMaxPairs; }

int check_args(uint32_t T, uint32_t G, uint64_t pairs, const void *workspace, size_t workspace_bytes) {
    if (!workspace || ((uintptr_t)workspace & 15u)) return PVD_ERR_INVALID;
    if (!in_range(T, G, pairs)) return PVD_ERR_UNSUPPORTED;
    if (workspace_bytes < layout(T, G, pairs).total) return PVD_ERR_INVALID;
    return PVD_OK;
}

}  // namespace

extern "C" {

size_t pvd_mesh_ray_workspace_bytes(uint32_t T, uint32_t G, uint64_t pairs) { return in_range(T, G, pairs) ? layout(T, G, pairs).total : 0; }

int pvd_mesh_ray_count(const float *vertices, uint32_t V, const int32_t *triangles, uint32_t T, const float *bmin3, const float *bmax3,
                       uint32_t G, uint64_t *totals, pvd_stream_t stream) {
    if (!bmin3 || !bmax3 || !totals || (T && !triangles) || (T && V && !vertices)) return PVD_ERR_INVALID;
    if (!in_range(T, G, 0)) return PVD_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    int rc;
    if ((rc = check_memset(hipMemsetAsync(totals, 0, 16, st))) != PVD_OK) return rc;
    if (T == 0) return PVD_OK;
    hipLaunchKernelGGL(k_mr_count, dim3(div_up(T, kThreads)), dim3(kThreads), 0, st, vertices, V, triangles, T, bmin3, bmax3, G,
                       (unsigned long long *)totals);
    return check_launch();
}

int pvd_mesh_ray_build(const float *vertices, uint32_t V, const int32_t *triangles, uint32_t T, const float *bmin3, const float *bmax3,
                       uint32_t G, uint64_t pairs, void *workspace, size_t workspace_bytes, pvd_stream_t stream) {
    if (!bmin3 || !bmax3 || (T && !triangles) || (T && V && !vertices)) return PVD_ERR_INVALID;
    int rc = check_args(T, G, pairs, workspace, workspace_bytes);
    if (rc != PVD_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    const Layout l = layout(T, G, pairs);
    const uint32_t C = G * G * G, NB = div_up(C, kThreads), TB = T ? div_up(T, kThreads) : 1u;
    char *ws = (char *)workspace;
    uint32_t *header = (uint32_t *)ws, *start = (uint32_t *)(ws + l.start), *cursor = (uint32_t *)(ws + l.cursor);
    uint32_t *bsum = (uint32_t *)(ws + l.bsum), *outside = (uint32_t *)(ws + l.outside), *list = (uint32_t *)(ws + l.pairs);
    float4 *packed = (float4 *)(ws + l.packed);
    if ((rc = check_memset(hipMemsetAsync(header, 0, kHeaderBytes, st))) != PVD_OK) return rc;
    if ((rc = check_memset(hipMemsetAsync(cursor, 0, 4 * (size_t)C, st))) != PVD_OK) return rc;
    hipLaunchKernelGGL(k_mr_bin, dim3(TB), dim3(kThreads), 0, st, vertices, V, triangles, T, bmin3, bmax3, G, header, cursor, outside, packed);
    if ((rc = check_launch()) != PVD_OK) return rc;
    hipLaunchKernelGGL(k_blocksum<uint32_t>, dim3(NB), dim3(kThreads), 0, st, cursor, C, bsum);
    if ((rc = check_launch()) != PVD_OK) return rc;
    hipLaunchKernelGGL(k_scan<uint32_t>, dim3(1), dim3(kScanThreads), 0, st, bsum, NB, start + C, header + 7);
    if ((rc = check_launch()) != PVD_OK) return rc;
    hipLaunchKernelGGL(k_offsets<uint32_t>, dim3(NB), dim3(kThreads), 0, st, cursor, C, bsum, start);
    if ((rc = check_launch()) != PVD_OK) return rc;
    if (T == 0) return PVD_OK;
    hipLaunchKernelGGL(k_mr_fill, dim3(TB), dim3(kThreads), 0, st, vertices, V, triangles, T, header, G, (uint32_t)pairs, cursor, list);
    return check_launch();
}

int pvd_mesh_ray_cast(const float *origins, const float *dirs, uint32_t N, uint32_t T, uint32_t G, uint64_t pairs, const void *workspace,
                      size_t workspace_bytes, float t_min, float t_max, float *t, int32_t *tri, float *bary, pvd_stream_t stream) {
    if (!(t_min >= 0.0f && t_min < INFINITY) || !(t_max > t_min)) return PVD_ERR_INVALID;  // false for NaN
    const int rc = check_args(T, G, pairs, workspace, workspace_bytes);
    if (rc != PVD_OK) return rc;
    if (N == 0) return PVD_OK;
    if (!origins || !dirs || !t || !tri || !bary) return PVD_ERR_INVALID;
    const Layout l = layout(T, G, pairs);
    const char *ws = (const char *)workspace;
    hipLaunchKernelGGL(k_mr_cast, dim3(div_up(N, kThreads)), dim3(kThreads), 0, (hipStream_t)stream, origins, dirs, N, T, G, (uint32_t)pairs,
                       (const uint32_t *)ws, (const uint32_t *)(ws + l.start), (const uint32_t *)(ws + l.pairs),
                       (const uint32_t *)(ws + l.outside), (const float4 *)(ws + l.packed), t_min, t_max, t, tri, bary);
    return check_launch();
}

}  // extern "C"
