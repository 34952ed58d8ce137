// mesh.hip -- triangle mesh of the level set u = thresh of a density volume (include/pvd_hip_mesh.h): marching tetrahedra on the
// Kuhn split of every cell, shared vertices on lattice edges, deterministic order.
//
// reference: extract_fields / extract_geometry, distill_mutual/utils.py:442-488 (mcubes.marching_cubes on the host).
//
// k_mesh_count    one lane per lattice point (k fastest, so a wave reads consecutive floats): the 8 corners of the point's cell ->
//                 the 7-bit mask of owned edges that carry a vertex and the number of triangles of the owned cell (0..12), one byte
//                 each, and the sums of both over the workgroup's 256 points.
// k_mesh_scan     ONE workgroup: the exclusive scan of both arrays of sums in place, side by side (scan_sums, csrc/block_scan.h);
//                 the two totals to totals_dev.
// k_mesh_offsets  one lane per lattice point: exclusive scan of the two byte counts inside the workgroup + the workgroup's base
//                 -> the point's first vertex index and first triangle index.
// Inside a workgroup the two counts travel as one word (kPairShift): 256 points own at most 1792 vertices and 3072 triangles.
// k_mesh_emit     one lane per lattice point: the owned vertices (world positions) and the owned cell's triangles; a triangle
//                 finds a vertex another point owns from that point's mask and first vertex index.
// k_mesh_normals  (include/pvd_hip_mesh_attr.h) one lane per lattice point: the normal of every owned vertex, from the gradient of
//                 the field at the two ends of its edge; reads the mask and the first vertex index the passes above left.
// The count -> one-workgroup scan -> offsets shape of csrc/block_scan.h: no workgroup waits on another one of the same launch,
// nothing is atomic, and the output does not depend on the order in which workgroups run.
#include "block_scan.h"
#include "mesh_gradient.h"

#include "../../include/pvd_hip_mesh.h"
#include "../../include/pvd_hip_mesh_attr.h"

namespace {

using namespace pvd;

// corner / direction code of an offset (ox, oy, oz) in {0,1}^3: ox * 4 + oy * 2 + oz, so codes order like linear indices
// edge slot of a direction code: (1,0,0) (0,1,0) (0,0,1) (1,1,0) (1,0,1) (0,1,1) (1,1,1) = slots 0..6
__device__ __forceinline__ uint32_t slot_of(uint32_t dcode) { return (0x63405120u >> (4 * dcode)) & 7u; }  // code 1..7 -> 2 1 5 0 4 3 6
// direction code of an edge slot
__device__ __forceinline__ uint32_t dcode_of(uint32_t slot) { return (0x7356124u >> (4 * slot)) & 7u; }  // slot 0..6 -> 4 2 1 6 5 3 7

// corner codes 1 and 2 of tetrahedron 0..5 = xyz xzy yxz yzx zxy zyx (corner 0 is code 0, corner 3 is code 7)
__device__ __forceinline__ uint32_t tet_corner(uint32_t tet, uint32_t c) {
    // first axis bit: x x y y z z = 4 4 2 2 1 1; first two axes: xy xz yx yz zx zy = 6 5 6 3 5 3
    const uint32_t c1 = (0x112244u >> (4 * tet)) & 7u, c2 = (0x353656u >> (4 * tet)) & 7u;
    return c == 0 ? 0u : c == 1 ? c1 : c == 2 ? c2 : 7u;
}
// odd permutations of the axes: xzy (1), yxz (2), zyx (5)
__device__ __forceinline__ uint32_t tet_odd(uint32_t tet) { return (0x26u >> tet) & 1u; }

struct Layout {  // byte offsets into the workspace
    size_t voff, toff, bsum_v, bsum_t, vmask, tcnt, total;
};

inline Layout layout(uint32_t R) {  // the 32-bit arrays first, so that a 4-byte aligned workspace aligns them all
    const size_t N = (size_t)R * R * R, NB = (N + kThreads - 1) / kThreads;
    Layout l;
    l.voff = 0;
    l.toff = l.voff + 4 * N;
    l.bsum_v = l.toff + 4 * N;
    l.bsum_t = l.bsum_v + 4 * NB;
    l.vmask = l.bsum_t + 4 * NB;
    l.tcnt = l.vmask + N;
    l.total = l.tcnt + N;
    return l;
}

// the inside bits of the 8 corners of the cell at (i, j, k), bit = corner code; corners outside the lattice read as outside and
// are reported in `exists`
__device__ __forceinline__ uint32_t corner_bits(const float *__restrict__ u, uint32_t R, uint32_t i, uint32_t j, uint32_t k, uint32_t n,
                                                float thresh, uint32_t *exists) {
    uint32_t in = 0, ex = 0;
#pragma unroll
    for (uint32_t c = 0; c < 8; ++c) {
        const uint32_t ox = c >> 2, oy = (c >> 1) & 1u, oz = c & 1u;
        if (i + ox < R && j + oy < R && k + oz < R) {
            ex |= 1u << c;
            if (u[n + (ox * R + oy) * R + oz] > thresh) in |= 1u << c;
        }
    }
    *exists = ex;
    return in;
}

// mask of the owned edges (slots 0..6) whose endpoints differ
__device__ __forceinline__ uint32_t owned_edges(uint32_t in, uint32_t ex) {
    const uint32_t differ = ((in & 1u) ? ~in : in) & ex;  // bit c: corner c exists and is on the other side of corner 0
    uint32_t m = 0;
#pragma unroll
    for (uint32_t s = 0; s < 7; ++s) m |= ((differ >> dcode_of(s)) & 1u) << s;
    return m;
}

// 4-bit inside mask of the corners 0..3 of a tetrahedron
__device__ __forceinline__ uint32_t tet_bits(uint32_t in, uint32_t tet) {
    return (in & 1u) | (((in >> tet_corner(tet, 1)) & 1u) << 1) | (((in >> tet_corner(tet, 2)) & 1u) << 2) | (((in >> 7) & 1u) << 3);
}

// Inside a workgroup the vertex count (low half) and the triangle count (high half) of a point are summed and scanned as one word:
// a byte count is at most 255, so neither half of a sum over kThreads points reaches 2^16, whatever the bytes hold.
constexpr uint32_t kPairShift = 16, kPairMask = 0xffffu;
static_assert(255u * kThreads <= kPairMask, "a half of the pair overflows into the other");

__global__ __launch_bounds__(kThreads) void k_mesh_count(const float *__restrict__ u, uint32_t R, uint32_t N, float thresh,
                                                        uint8_t *__restrict__ vmask, uint8_t *__restrict__ tcnt,
                                                        uint32_t *__restrict__ bsum_v, uint32_t *__restrict__ bsum_t) {
    __shared__ uint32_t red[kWaves];
    const uint32_t n = blockIdx.x * kThreads + threadIdx.x;
    uint32_t nv = 0, nt = 0;
    if (n < N) {
        const uint32_t i = n / (R * R), r = n - i * R * R, j = r / R, k = r - j * R;
        uint32_t ex;
        const uint32_t in = corner_bits(u, R, i, j, k, n, thresh, &ex);
        const uint32_t m = owned_edges(in, ex);
        nv = __popc(m);
        if (ex == 0xffu && in != 0u && in != 0xffu) {
#pragma unroll
            for (uint32_t tet = 0; tet < 6; ++tet) {
                const uint32_t c = __popc(tet_bits(in, tet));
                nt += c == 2 ? 2u : (c == 1 || c == 3) ? 1u : 0u;
            }
        }
        vmask[n] = (uint8_t)m;
        tcnt[n] = (uint8_t)nt;
    }
    const uint32_t s = block_sum(nv | (nt << kPairShift), red);
    if (threadIdx.x == 0) {
        bsum_v[blockIdx.x] = s & kPairMask;
        bsum_t[blockIdx.x] = s >> kPairShift;
    }
}

// one workgroup; sums [NB] -> exclusive scan in place, for both arrays; totals[0], totals[1]
__global__ __launch_bounds__(kScanThreads) void k_mesh_scan(uint32_t *__restrict__ bsum_v, uint32_t *__restrict__ bsum_t, uint32_t NB,
                                                           uint32_t *__restrict__ totals) {
    uint32_t *const sums[2] = {bsum_v, bsum_t};
    uint32_t total[2];
    scan_sums(sums, NB, total);
    if (threadIdx.x == 0) {
        totals[0] = total[0];
        totals[1] = total[1];
    }
}

__global__ __launch_bounds__(kThreads) void k_mesh_offsets(const uint8_t *__restrict__ vmask, const uint8_t *__restrict__ tcnt, uint32_t N,
                                                          const uint32_t *__restrict__ bsum_v, const uint32_t *__restrict__ bsum_t,
                                                          uint32_t *__restrict__ voff, uint32_t *__restrict__ toff) {
    __shared__ uint32_t wtot[kWaves];
    const uint32_t n = blockIdx.x * kThreads + threadIdx.x;
    const uint32_t nv = n < N ? (uint32_t)__popc((uint32_t)vmask[n]) : 0u, nt = n < N ? (uint32_t)tcnt[n] : 0u;
    const uint32_t e = block_exclusive(nv | (nt << kPairShift), wtot);
    if (n < N) {
        voff[n] = bsum_v[blockIdx.x] + (e & kPairMask);
        toff[n] = bsum_t[blockIdx.x] + (e >> kPairShift);
    }
}

__global__ __launch_bounds__(kThreads) void k_mesh_emit(const float *__restrict__ u, uint32_t R, uint32_t N, float thresh,
                                                       const float *__restrict__ bmin3, const float *__restrict__ bmax3,
                                                       const uint8_t *__restrict__ vmask, const uint32_t *__restrict__ voff,
                                                       const uint32_t *__restrict__ toff, float *__restrict__ vertices, uint32_t V,
                                                       int32_t *__restrict__ triangles, uint32_t T) {
    const uint32_t n = blockIdx.x * kThreads + threadIdx.x;
    if (n >= N) return;
    const uint32_t mask = vmask[n];
    const uint32_t i = n / (R * R), r = n - i * R * R, j = r / R, k = r - j * R;

    // ---- the vertices this point owns, in slot order
    if (mask) {
        const float ua = u[n], fi = (float)i, fj = (float)j, fk = (float)k, rm1 = (float)(R - 1);
        const float lo[3] = {bmin3[0], bmin3[1], bmin3[2]};
        const float ext[3] = {bmax3[0] - lo[0], bmax3[1] - lo[1], bmax3[2] - lo[2]};
        uint32_t at = voff[n];
#pragma unroll
        for (uint32_t s = 0; s < 7; ++s) {
            if ((mask >> s) & 1u) {
                const uint32_t d = dcode_of(s), ox = d >> 2, oy = (d >> 1) & 1u, oz = d & 1u;
                const float ub = u[n + (ox * R + oy) * R + oz];
                const float t = (thresh - ua) / (ub - ua);
                const float px = ox ? fi + t : fi, py = oy ? fj + t : fj, pz = oz ? fk + t : fk;
                if (at < V) {
                    float *v = vertices + 3 * (size_t)at;
                    v[0] = px / rm1 * ext[0] + lo[0];
                    v[1] = py / rm1 * ext[1] + lo[1];
                    v[2] = pz / rm1 * ext[2] + lo[2];
                }
                ++at;
            }
        }
    }

    // ---- the triangles of the cell this point owns
    if (i + 1 >= R || j + 1 >= R || k + 1 >= R) return;
    uint32_t ex;
    const uint32_t in = corner_bits(u, R, i, j, k, n, thresh, &ex);
    if (in == 0u || in == 0xffu) return;
    uint32_t tri = toff[n];
    // index of the vertex on the edge between the corners with codes ca, cb (ca a subset of cb) of this cell
    auto vertex = [&](uint32_t ca, uint32_t cb) -> int32_t {
        const uint32_t owner = n + (((ca >> 2) & 1u) * R + ((ca >> 1) & 1u)) * R + (ca & 1u);
        const uint32_t slot = slot_of(ca ^ cb);
        return (int32_t)(voff[owner] + (uint32_t)__popc((uint32_t)vmask[owner] & ((1u << slot) - 1u)));
    };
    auto put = [&](int32_t a, int32_t b, int32_t c, bool flip) {
        if (tri < T) {
            int32_t *o = triangles + 3 * (size_t)tri;
            o[0] = a;
            o[1] = flip ? c : b;
            o[2] = flip ? b : c;
        }
        ++tri;
    };
    for (uint32_t tet = 0; tet < 6; ++tet) {
        const uint32_t m4 = tet_bits(in, tet), cnt = __popc(m4);
        if (cnt == 0 || cnt == 4) continue;
        const uint32_t odd = tet_odd(tet);
        // corners of the tetrahedron by number -> corner codes; an edge runs from the lower-numbered corner (a subset) to the higher
        auto edge = [&](uint32_t x, uint32_t y) -> int32_t {
            const uint32_t lo = x < y ? x : y, hi = x < y ? y : x;
            return vertex(tet_corner(tet, lo), tet_corner(tet, hi));
        };
        if (cnt == 2) {
            const uint32_t A = __ffs(m4) - 1, B = 31 - __clz(m4), out = ~m4 & 15u, C = __ffs(out) - 1, D = 31 - __clz(out);
            const uint32_t inv = (A > C) + (A > D) + (B > C) + (B > D);
            const bool flip = (odd ^ (inv & 1u)) != 0;
            const int32_t ac = edge(A, C), ad = edge(A, D), bd = edge(B, D), bc = edge(B, C);
            put(ac, ad, bd, flip);
            put(ac, bd, bc, flip);
        } else {
            const uint32_t lone = cnt == 1 ? m4 : (~m4 & 15u);
            const uint32_t A = __ffs(lone) - 1;
            const uint32_t B = A == 0 ? 1u : 0u, C = A <= 1 ? 2u : 1u, D = A == 3 ? 2u : 3u;
            const bool flip = (odd ^ (A & 1u) ^ (cnt == 3 ? 1u : 0u)) != 0;
            put(edge(A, B), edge(A, C), edge(A, D), flip);
        }
    }
}

// one lane per lattice point, as k_mesh_emit: the normals of the vertices this point owns, in slot order, to the rows voff[n] ...
// A wave's points are consecutive along k, so its stencil loads are consecutive floats of 5 rows for the owner and of the rows
// one step further for the other endpoints; they overlap between neighbouring lanes and slots and are served by L1 / L2.
__global__ __launch_bounds__(kThreads) void k_mesh_normals(const float *__restrict__ u, uint32_t R, uint32_t N, float thresh,
                                                          const float *__restrict__ bmin3, const float *__restrict__ bmax3,
                                                          const uint8_t *__restrict__ vmask, const uint32_t *__restrict__ voff,
                                                          float *__restrict__ normals, uint32_t V) {
    const uint32_t n = blockIdx.x * kThreads + threadIdx.x;
    if (n >= N) return;
    const uint32_t mask = vmask[n];
    if (!mask) return;
    const uint32_t i = n / (R * R), r = n - i * R * R, j = r / R, k = r - j * R;
    const float rm1 = (float)(R - 1);
    const float inv_h[3] = {rm1 / (bmax3[0] - bmin3[0]), rm1 / (bmax3[1] - bmin3[1]), rm1 / (bmax3[2] - bmin3[2])};
    const uint32_t ca[3] = {i, j, k};
    const float ua = u[n];
    float ga[3];
    world_gradient(u, R, n, ca, inv_h, ga);
    uint32_t at = voff[n];
#pragma unroll
    for (uint32_t s = 0; s < 7; ++s) {
        if ((mask >> s) & 1u) {
            if (at < V) {
                const uint32_t d = dcode_of(s), ox = d >> 2, oy = (d >> 1) & 1u, oz = d & 1u;
                const uint32_t b = n + (ox * R + oy) * R + oz;  // a lattice point: the count pass sets a slot only where it is one
                const uint32_t cb[3] = {i + ox, j + oy, k + oz};
                float gb[3];
                world_gradient(u, R, b, cb, inv_h, gb);
                const float ub = u[b];
                const float t = (thresh - ua) / (ub - ua);
                const float gx = ga[0] + t * (gb[0] - ga[0]), gy = ga[1] + t * (gb[1] - ga[1]), gz = ga[2] + t * (gb[2] - ga[2]);
                const float len = sqrtf(gx * gx + gy * gy + gz * gz);
                const bool ok = len > 0.0f && len < INFINITY;  // false for NaN
                float *o = normals + 3 * (size_t)at;
                o[0] = ok ? -gx / len : 0.0f;
                o[1] = ok ? -gy / len : 0.0f;
                o[2] = ok ? -gz / len : 0.0f;
            }
            ++at;
        }
    }
}

int check_args(const void *field, uint32_t R, const void *workspace, size_t workspace_bytes) {
    if (!field || !workspace || ((uintptr_t)workspace & 3u)) return PVD_ERR_INVALID;
    if (R < 2 || R > PVD_MESH_MAX_R) return PVD_ERR_UNSUPPORTED;
    if (workspace_bytes < layout(R).total) return PVD_ERR_INVALID;
    return PVD_OK;
}

}  // namespace

extern "C" {

size_t pvd_mesh_workspace_bytes(uint32_t R) { return (R < 2 || R > PVD_MESH_MAX_R) ? 0 : layout(R).total; }

int pvd_mesh_count(const float *field, uint32_t R, float thresh, void *workspace, size_t workspace_bytes, uint32_t *totals_dev,
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
    uint8_t *vmask = (uint8_t *)(ws + l.vmask), *tcnt = (uint8_t *)(ws + l.tcnt);
    hipLaunchKernelGGL(k_mesh_count, dim3(NB), dim3(kThreads), 0, st, field, R, N, thresh, vmask, tcnt, bsum_v, bsum_t);
    if ((rc = check_launch()) != PVD_OK) return rc;
    hipLaunchKernelGGL(k_mesh_scan, dim3(1), dim3(kScanThreads), 0, st, bsum_v, bsum_t, NB, totals_dev);
    if ((rc = check_launch()) != PVD_OK) return rc;
    hipLaunchKernelGGL(k_mesh_offsets, dim3(NB), dim3(kThreads), 0, st, vmask, tcnt, N, bsum_v, bsum_t, voff, toff);
    return check_launch();
}

int pvd_mesh_emit(const float *field, uint32_t R, float thresh, const float *bmin3, const float *bmax3, const void *workspace,
                  size_t workspace_bytes, float *vertices, uint32_t V, int32_t *triangles, uint32_t T, pvd_stream_t stream) {
    if (!bmin3 || !bmax3) return PVD_ERR_INVALID;
    const int rc = check_args(field, R, workspace, workspace_bytes);
    if (rc != PVD_OK) return rc;
    if (V == 0 && T == 0) return PVD_OK;
    if ((V && !vertices) || (T && !triangles)) return PVD_ERR_INVALID;
    const Layout l = layout(R);
    const uint32_t N = R * R * R, NB = div_up(N, kThreads);
    const char *ws = (const char *)workspace;
    hipLaunchKernelGGL(k_mesh_emit, dim3(NB), dim3(kThreads), 0, (hipStream_t)stream, field, R, N, thresh, bmin3, bmax3,
                       (const uint8_t *)(ws + l.vmask), (const uint32_t *)(ws + l.voff), (const uint32_t *)(ws + l.toff), vertices, V,
                       triangles, T);
    return check_launch();
}

int pvd_mesh_normals(const float *field, uint32_t R, float thresh, const float *bmin3, const float *bmax3, const void *workspace,
                     size_t workspace_bytes, float *normals, uint32_t V, pvd_stream_t stream) {
    if (!bmin3 || !bmax3) return PVD_ERR_INVALID;
    const int rc = check_args(field, R, workspace, workspace_bytes);
    if (rc != PVD_OK) return rc;
    if (V == 0) return PVD_OK;
    if (!normals) return PVD_ERR_INVALID;
    const Layout l = layout(R);
    const uint32_t N = R * R * R, NB = div_up(N, kThreads);
    const char *ws = (const char *)workspace;
    hipLaunchKernelGGL(k_mesh_normals, dim3(NB), dim3(kThreads), 0, (hipStream_t)stream, field, R, N, thresh, bmin3, bmax3,
                       (const uint8_t *)(ws + l.vmask), (const uint32_t *)(ws + l.voff), normals, V);
    return check_launch();
}

}  // extern "C"
