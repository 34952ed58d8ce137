// mesh_winding.hip -- the integer winding number of points, and of every point of an R^3 lattice, against a triangle mesh
// (include/pvd_hip_mesh_winding.h): signed crossings of the ray along +z, in unfused float64, over a two-dimensional grid of the
// triangles' dilated bounding boxes in x and y, built on the device (csrc/mesh_tri_grid.h, two binned axes: k_tg_count<2>,
// k_tg_bin<2>, the scan of csrc/block_scan.h, k_tg_fill<2>; the record carries the directions of the triangle's three edges).
//
// k_mw_points    one lane per point: the cell's list, then the outside list.  No LDS, no atomics.
// k_mw_lattice   one wave per column (i, j), kColsPerWave columns after one another: the lanes share out the column's triangles,
//                every crossing adds its sign into the column's difference array in LDS (integer LDS atomics), the wave takes the
//                suffix sum in chunks of 64 with a carry (wave_scan of block_scan.h) and stores 64 consecutive ints per chunk.
//                The four totals: registers -> one workgroup sum -> at most four integer atomics per workgroup.
// No workgroup waits on another one of the same launch, and no loop retries an atomic.  The order of the pairs inside a cell depends
// on the run; a sum of integers does not.
#include "mesh_tri_grid.h"

namespace {

using namespace pvd;
using namespace pvd::tgrid;  // the workspace's layout and its build

constexpr int kMaxR = PVD_MESH_WINDING_MAX_R;
constexpr int kColsPerWave = 4;  // columns a wave of k_mw_lattice walks: neighbours in j, so mostly one cell's list, still warm

// ------------------------------------------------------------------------------------------ one triangle against one column
// the directed edge function of u -> w at (px, py), evaluated from the lower to the higher index (`up`: u is the lower one) and
// negated for the other direction; (dx, dy) the directed edge's vector
PVD_HD double edge(double xu, double yu, double xw, double yw, bool up, double px, double py, double &dx, double &dy) {
#pragma clang fp contract(off)
    const double lx = up ? xu : xw, ly = up ? yu : yw, hx = up ? xw : xu, hy = up ? yw : yu;
    const double ex = hx - lx, ey = hy - ly;
    const double E = ex * (py - ly) - ey * (px - lx);
    dx = up ? ex : -ex;
    dy = up ? ey : -ey;
    return up ? E : -E;
}

PVD_HD bool owned(double e, double dx, double dy) { return e > 0.0 || (e == 0.0 && (dy > 0.0 || (dy == 0.0 && dx < 0.0))); }

// record j of the packed array against the column (px, py): s (0: no coverage) and z_hit -- steps 1 .. 4 of the header
PVD_HD int cover(const float4 *__restrict__ packed, uint32_t j, double px, double py, double &z_hit) {
#pragma clang fp contract(off)
    const float4 q0 = packed[3 * (size_t)j], q1 = packed[3 * (size_t)j + 1], q2 = packed[3 * (size_t)j + 2];
    if ((int32_t)f2u(q2.y) < 0) return 0;  // an invalid triangle
    const uint32_t dirs = f2u(q2.z);
    const double ax = (double)q0.x, ay = (double)q0.y, az = (double)q0.z;
    const double bx = (double)q0.w, by = (double)q1.x, bz = (double)q1.y;
    const double cx = (double)q1.z, cy = (double)q1.w, cz = (double)q2.x;
    double dx, dy;
    const double area = edge(ax, ay, bx, by, (dirs & 4u) != 0, cx, cy, dx, dy);
    if (!(area != 0.0)) return 0;
    const int s = area > 0.0 ? 1 : -1;
    const double sd = (double)s;
    const double e_bc = edge(bx, by, cx, cy, (dirs & 1u) != 0, px, py, dx, dy) * sd;
    if (!owned(e_bc, dx * sd, dy * sd)) return 0;
    const double e_ca = edge(cx, cy, ax, ay, (dirs & 2u) != 0, px, py, dx, dy) * sd;
    if (!owned(e_ca, dx * sd, dy * sd)) return 0;
    const double e_ab = edge(ax, ay, bx, by, (dirs & 4u) != 0, px, py, dx, dy) * sd;
    if (!owned(e_ab, dx * sd, dy * sd)) return 0;
    z_hit = ((e_bc * az + e_ca * bz) + e_ab * cz) / ((e_bc + e_ca) + e_ab);
    return s;
}

// what a column (px, py) tests: the list of its cell, [s0, s1) of `list` (empty outside the box), and the n_out outside triangles;
// every index is clamped, so that a damaged workspace stays inside itself
struct Column {
    uint32_t s0, n_cell, n_out;
};

PVD_HD Column column_of(double px, double py, uint32_t T, uint32_t G, uint32_t pairs, const uint32_t *__restrict__ header,
                        const uint32_t *__restrict__ start) {
    const Box<2> box = box_of<2>((const float *)(header + 1), (const float *)(header + 4), G);
    const uint32_t n_pairs = umin(header[7], pairs);
    Column c;
    c.n_out = umin(header[0], T);
    c.s0 = c.n_cell = 0;
    const bool in_x = box.flat[0] || (box.lo[0] <= px && px <= box.hi[0]), in_y = box.flat[1] || (box.lo[1] <= py && py <= box.hi[1]);
    if (in_x && in_y) {
        const uint32_t cell = (uint32_t)cell_axis(box, 0, px, G) * G + (uint32_t)cell_axis(box, 1, py, G);
        const uint32_t s0 = umin(start[cell], n_pairs), s1 = umin(start[cell + 1], n_pairs);
        c.s0 = s0;
        c.n_cell = s1 > s0 ? s1 - s0 : 0u;
    }
    return c;
}

// item q of a column: a record of the packed array, or T (none) for a damaged entry
PVD_HD uint32_t item_of(const Column &c, uint32_t q, uint32_t T, const uint32_t *__restrict__ list, const uint32_t *__restrict__ outside) {
    const uint32_t j = q < c.n_cell ? list[c.s0 + q] : outside[q - c.n_cell];
    return j < T ? j : T;
}

__global__ __launch_bounds__(kThreads) void k_mw_points(const float *__restrict__ points, uint32_t N, uint32_t T, uint32_t G, uint32_t pairs,
                                                       const uint32_t *__restrict__ header, const uint32_t *__restrict__ start,
                                                       const uint32_t *__restrict__ list, const uint32_t *__restrict__ outside,
                                                       const float4 *__restrict__ packed, int32_t *__restrict__ winding) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= N) return;
    const float x = points[3 * (size_t)i], y = points[3 * (size_t)i + 1], z = points[3 * (size_t)i + 2];
    if (!finite3(x, y, z)) {
        winding[i] = PVD_MESH_WINDING_INVALID;
        return;
    }
    const double px = (double)x, py = (double)y, pz = (double)z;
    const Column c = column_of(px, py, T, G, pairs, header, start);
    int32_t w = 0;
    for (uint32_t q = 0; q < c.n_cell + c.n_out; ++q) {
        const uint32_t j = item_of(c, q, T, list, outside);
        if (j >= T) continue;
        double z_hit;
        const int s = cover(packed, j, px, py, z_hit);
        if (s != 0 && z_hit > pz) w += s;  // false for a z_hit that is NaN
    }
    winding[i] = w;
}

// ---------------------------------------------------------------------------------------------------------- the lattice
// coordinate n of an axis of the lattice: each operation rounded to float32 (the build has -ffp-contract=off)
PVD_HD float lattice_coord(uint32_t n, float r1, float d, float lo) {
#pragma clang fp contract(off)
    const float f = (float)n / r1;
    const float g = f * d;
    return g + lo;
}

__global__ __launch_bounds__(kThreads) void k_mw_lattice(uint32_t R, const float *__restrict__ lat_lo, const float *__restrict__ lat_hi, uint32_t T,
                                                        uint32_t G, uint32_t pairs, const uint32_t *__restrict__ header,
                                                        const uint32_t *__restrict__ start, const uint32_t *__restrict__ list,
                                                        const uint32_t *__restrict__ outside, const float4 *__restrict__ packed,
                                                        int32_t *__restrict__ winding, unsigned long long *__restrict__ totals) {
    __shared__ int32_t diff[kWaves][kMaxR];  // per wave: the column's difference array, in walk order (16 KiB per workgroup)
    __shared__ uint32_t red0[kWaves], red1[kWaves], red2[kWaves], red3[kWaves];
    const uint32_t lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const float r1 = (float)(R - 1);
    const float lo_x = lat_lo[0], lo_y = lat_lo[1], lo_z = lat_lo[2];
    const float d_x = lat_hi[0] - lo_x, d_y = lat_hi[1] - lo_y, d_z = lat_hi[2] - lo_z;
    // z_k is monotone in k: every step of lattice_coord is.  The walk index m runs upwards in z: m = k, or R - 1 - k where d_z < 0.
    const bool down = d_z < 0.0f;
    int32_t *mine = diff[wave];
    for (uint32_t m = lane; m < R; m += kWave) mine[m] = 0;
    __syncthreads();
    uint32_t n_nonzero = 0, n_positive = 0, n_leaky = 0, max_abs = 0;
    const uint32_t columns = R * R;  // at most 2^20
    for (int c4 = 0; c4 < kColsPerWave; ++c4) {  // the same trip count for every thread: the barriers below are reached by all
        const uint32_t col = (blockIdx.x * kWaves + wave) * kColsPerWave + (uint32_t)c4;
        const bool active = col < columns;
        const float x = lattice_coord(active ? col / R : 0u, r1, d_x, lo_x), y = lattice_coord(active ? col % R : 0u, r1, d_y, lo_y);
        const bool col_ok = active && finite1(x) && finite1(y);
        int32_t leak = 0;
        if (col_ok) {
            const double px = (double)x, py = (double)y;
            const Column c = column_of(px, py, T, G, pairs, header, start);
            for (uint32_t q = lane; q < c.n_cell + c.n_out; q += kWave) {
                const uint32_t j = item_of(c, q, T, list, outside);
                if (j >= T) continue;
                double z_hit;
                const int s = cover(packed, j, px, py, z_hit);
                if (s == 0 || !(z_hit > -(double)INFINITY)) continue;  // false for NaN
                leak += s;
                // cnt = the number of walk indices m with z(m) < z_hit, a prefix 0 .. cnt - 1: a guess from the float64 quotient,
                // corrected against the float32 coordinates themselves (each loop ends after at most R steps, whatever the guess)
                const double at = (z_hit - (double)lo_z) / (double)d_z * (double)r1;  // the real k at which z_k == z_hit
                const double guess = ceil(down ? (double)r1 - at : at);
                int cnt = guess >= (double)R ? (int)R : (guess > 0.0 ? (int)guess : 0);  // NaN -> 0
                while (cnt > 0 && !((double)lattice_coord(down ? R - (uint32_t)cnt : (uint32_t)cnt - 1u, r1, d_z, lo_z) < z_hit)) --cnt;
                while (cnt < (int)R && (double)lattice_coord(down ? R - 1u - (uint32_t)cnt : (uint32_t)cnt, r1, d_z, lo_z) < z_hit) ++cnt;
                if (cnt > 0) atomicAdd(&mine[cnt - 1], s);
            }
        }
        __syncthreads();
        const uint32_t leak_sum = wave_sum((uint32_t)leak);  // wrap-around: the sum of the signs
        if (lane == 0 && col_ok && leak_sum != 0u) ++n_leaky;
        // w(m) = the sum of mine[m ..]: chunks of one wave from the top, lane l takes m = R - 1 - (base + l)
        uint32_t carry = 0;
        for (uint32_t base = 0; base < R; base += kWave) {  // the same trip count for every thread
            const uint32_t off = base + lane;
            const bool has = off < R;
            const uint32_t m = has ? R - 1u - off : 0u;
            const uint32_t v = has ? (uint32_t)mine[m] : 0u;
            if (has) mine[m] = 0;  // ready for the wave's next column
            const uint32_t sum = wave_scan(v) + carry;
            carry = (uint32_t)__shfl((int)sum, kWave - 1, kWave);
            if (has && active) {
                const uint32_t k = down ? R - 1u - m : m;
                const bool ok = col_ok && finite1(lattice_coord(k, r1, d_z, lo_z));
                const int32_t w = ok ? (int32_t)sum : PVD_MESH_WINDING_INVALID;
                winding[(size_t)col * R + k] = w;  // 64 consecutive ints per chunk
                if (ok && w != 0) {
                    const uint32_t a = w < 0 ? 0u - (uint32_t)w : (uint32_t)w;
                    ++n_nonzero;
                    n_positive += w > 0 ? 1u : 0u;
                    max_abs = a > max_abs ? a : max_abs;
                }
            }
        }
        __syncthreads();  // the zeros are in place before the next column's atomics
    }
    n_nonzero = block_sum(n_nonzero, red0);
    n_positive = block_sum(n_positive, red1);
    n_leaky = block_sum(n_leaky, red2);
    max_abs = block_max(max_abs, red3);
    if (threadIdx.x == 0) {
        if (n_nonzero) atomicAdd(&totals[0], (unsigned long long)n_nonzero);
        if (n_positive) atomicAdd(&totals[1], (unsigned long long)n_positive);
        if (n_leaky) atomicAdd(&totals[2], (unsigned long long)n_leaky);
        if (max_abs) atomicMax(&totals[3], (unsigned long long)max_abs);
    }
}

}  // namespace

extern "C" {

size_t pvd_mesh_winding_workspace_bytes(uint32_t T, uint32_t G, uint64_t pairs) { return in_range<2>(T, G, pairs) ? layout<2>(T, G, pairs).total : 0; }

int pvd_mesh_winding_count(const float *vertices, uint32_t V, const int32_t *triangles, uint32_t T, const float *bmin3, const float *bmax3,
                           uint32_t G, uint64_t *totals, pvd_stream_t stream) {
    if (!bmin3 || !bmax3 || !totals || (T && !triangles) || (T && V && !vertices)) return PVD_ERR_INVALID;
    if (!in_range<2>(T, G, 0)) return PVD_ERR_UNSUPPORTED;
    return count<2>(vertices, V, triangles, T, bmin3, bmax3, G, totals, (hipStream_t)stream);
}

int pvd_mesh_winding_build(const float *vertices, uint32_t V, const int32_t *triangles, uint32_t T, const float *bmin3, const float *bmax3,
                           uint32_t G, uint64_t pairs, void *workspace, size_t workspace_bytes, pvd_stream_t stream) {
    if (!bmin3 || !bmax3 || (T && !triangles) || (T && V && !vertices)) return PVD_ERR_INVALID;
    const int rc = check_args<2>(T, G, pairs, workspace, workspace_bytes);
    if (rc != PVD_OK) return rc;
    return build<2>(vertices, V, triangles, T, bmin3, bmax3, G, pairs, workspace, (hipStream_t)stream);
}

int pvd_mesh_winding_points(const float *points, uint32_t N, uint32_t T, uint32_t G, uint64_t pairs, const void *workspace,
                            size_t workspace_bytes, int32_t *winding, pvd_stream_t stream) {
    const int rc = check_args<2>(T, G, pairs, workspace, workspace_bytes);
    if (rc != PVD_OK) return rc;
    if (N == 0) return PVD_OK;
    if (!points || !winding) return PVD_ERR_INVALID;
    const Layout l = layout<2>(T, G, pairs);
    const char *ws = (const char *)workspace;
    hipLaunchKernelGGL(k_mw_points, dim3(div_up(N, kThreads)), dim3(kThreads), 0, (hipStream_t)stream, points, N, T, G, (uint32_t)pairs,
                       (const uint32_t *)ws, (const uint32_t *)(ws + l.start), (const uint32_t *)(ws + l.pairs),
                       (const uint32_t *)(ws + l.outside), (const float4 *)(ws + l.packed), winding);
    return check_launch();
}

int pvd_mesh_winding_lattice(uint32_t R, const float *lat_bmin3, const float *lat_bmax3, uint32_t T, uint32_t G, uint64_t pairs,
                             const void *workspace, size_t workspace_bytes, int32_t *winding, int64_t *totals, pvd_stream_t stream) {
    if (!lat_bmin3 || !lat_bmax3 || !winding || !totals) return PVD_ERR_INVALID;
    int rc = check_args<2>(T, G, pairs, workspace, workspace_bytes);
    if (rc != PVD_OK) return rc;
    if (R < 2 || R > PVD_MESH_WINDING_MAX_R) return PVD_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    if ((rc = check_memset(hipMemsetAsync(totals, 0, 32, st))) != PVD_OK) return rc;
    const Layout l = layout<2>(T, G, pairs);
    const char *ws = (const char *)workspace;
    hipLaunchKernelGGL(k_mw_lattice, dim3(div_up(R * R, kWaves * kColsPerWave)), dim3(kThreads), 0, st, R, lat_bmin3, lat_bmax3, T, G,
                       (uint32_t)pairs, (const uint32_t *)ws, (const uint32_t *)(ws + l.start), (const uint32_t *)(ws + l.pairs),
                       (const uint32_t *)(ws + l.outside), (const float4 *)(ws + l.packed), winding, (unsigned long long *)totals);
    return check_launch();
}

}  // extern "C"
