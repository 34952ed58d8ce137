/*
 * pvd_hip_mesh_simplify.h -- a triangle mesh made smaller by uniform-grid vertex clustering (Rossignac & Borrel 1993), in
 * libpvd_hip.so next to the mesh extraction of pvd_hip_mesh.h and the distance of pvd_hip_mesh_dist.h (pvd/mesh.py: simplify_mesh,
 * extract_surface(simplify=G)).  Same conventions as pvd_hip.h (device pointers, caller-allocated buffers, the stream as void*,
 * PVD_OK or a negative pvd_status).  pvd_abi_version() is not changed by this addition.
 *
 * Every sum below is a sum of integers, so every output is an exact function of the inputs that does not depend on the order in
 * which the atomics land: the results are bit-identical from run to run, and tests/mesh_simplify_restatement.py restates them in
 * numpy bit for bit.  The library is built with -ffp-contract=off, so the float64 expressions mean on the device what they mean
 * there.
 *
 * Inputs   vertices [V,3] f32, triangles [T,3] i32, attrs [V,K] f32 with K in 0 .. PVD_MESH_SIMPLIFY_MAX_K (unit normals and / or
 *          colours: values are clamped to [-1, 1]), a box bmin3 .. bmax3 (device f32 [3] each), G cells per axis in
 *          1 .. PVD_MESH_SIMPLIFY_MAX_G; V and T at most 2^31 - 1.  Everything below is float64 from the f32 inputs unless it says
 *          integer.
 *
 * Vertex   VALID iff its three coordinates are finite.
 *
 * q_a      the quantised position of a valid vertex along axis a.  e_a = bmax_a - bmin_a; the axis is FLAT iff e_a is not a positive
 *          finite number.  Flat: q_a = 0.  Otherwise
 *              f_a = clamp((x_a - bmin_a) / e_a, 0, 1),      q_a = llrint(f_a * 2^30)   (ties to even; an integer in 0 .. 2^30).
 *          A vertex outside the box is thereby PROJECTED ONTO THE BOX: it takes part, in the cell sums too, with the position of
 *          the nearest point of the box.
 *
 * Cell     k_a = min(G - 1, (q_a * G) >> 30), an integer computed from q_a alone; the cell's linear index is (k_x G + k_y) G + k_z.
 *          The cell and the mean come from the same integers: k_a = k iff k 2^30 / G <= q_a < (k + 1) 2^30 / G (the last cell also
 *          holds q_a = 2^30), an interval of integers, and the mean of integers of one interval lies in it -- the mean of a cell's
 *          members can never leave the cell.
 *
 * Triangle VALID iff its three indices are in [0, V) and the three vertices are valid.  It SURVIVES iff it is valid and its three
 *          corners lie in three different cells.
 *
 * Kept     a cell is KEPT iff a corner of at least one surviving triangle lies in it.  The new vertices are the kept cells in
 *          ascending linear index; V' is their number.  MEMBERS of a new vertex: every valid vertex whose cell is that kept cell,
 *          whether or not a triangle refers to it.  vertex_map[v] = the new index of v's cell; -1 for a vertex that is not valid or
 *          whose cell is not kept.  Per kept cell, in integers:
 *              n = the number of members,   S_a = sum of q_a  (int64; at most 2^31 * 2^30 = 2^61),
 *              A_j = sum of llrint(clamp(attr_j, -1, 1) * 2^30)   (signed int64; an attribute that is not finite contributes 0).
 *
 * Outputs  x'_a    = (float)(bmin_a + ((double)S_a / (double)n) * (e_a * 2^-30))      on an axis that is not flat, bmin_a on a flat one;
 *          attr'_j = (float)(((double)A_j / (double)n) * 2^-30);
 *          triangles' = the surviving triangles in input order, corners replaced through vertex_map, corner order kept (so the
 *          orientation stays); T' is their number.
 *
 * Not done Two input triangles that map to the same three cells give two output triangles: DUPLICATES ARE NOT MERGED.  The result
 *          is NOT GUARANTEED MANIFOLD (an edge of the output may belong to more than two triangles, sheets closer than a cell are
 *          welded).  Error quadrics (placing the new vertex where it costs the least) are out of scope: the new vertex is the mean.
 *
 * Bound    For a vertex v with vertex_map[v] >= 0 whose coordinate x_a lies inside the box (bmin_a <= x_a <= bmax_a, axis not flat):
 *              |x_a - x'_a|  <=  e_a / G  +  2^-30 e_a  +  2^-23 max(|bmin_a|, |bmax_a|).
 *          Derivation.  In real numbers x_a = bmin_a + f e_a with f = (x_a - bmin_a) / e_a in [0, 1] (no clamp acts).  The computed
 *          f_a carries at most two float64 roundings (the difference, the quotient): |f_a - f| <= 2^-52.  q_a / 2^30 differs from
 *          f_a by at most 2^-31 (one quantisation).  v and the mean m = S_a / n lie in the same interval of width 2^30 / G (Cell), so
 *          |q_a - m| <= 2^30 / G.  The computed (double)S_a / (double)n carries three roundings of 2^-53 relative to m <= 2^30, and
 *          the product with e_a 2^-30 (exact unless it underflows) one more: together below 2^-50 e_a.  Hence, before the last sum,
 *              |x_a - (bmin_a + m 2^-30 e_a)|  <=  e_a (1 / G + 2^-31 + 2^-52 + 2^-50)  <  e_a / G + 2^-30 e_a
 *          (the second term has room for two quantisations of 2^-31 e_a; only one is spent).  The float64 sum and its rounding to
 *          float32 give x'_a with |x'_a - exact| <= (2^-24 + 2^-53) |exact|, and |exact| <= max(|bmin_a|, |bmax_a|) (1 + 2^-50) because
 *          m 2^-30 is in [0, 1]: below 2^-23 max(|bmin_a|, |bmax_a|).  The three terms are the cell width, the quantisations and
 *          the f32 rounding of the result.  PVD_MESH_SIMPLIFY_BOUND(e, G, lo, hi) below is this bound; the tests use it.
 *          A point of a triangle moves no further than the farthest of its corners, so the simplified surface stays within
 *          sqrt(sum of the squares of the three per-axis bounds) -- the cell diagonal plus slack -- of every surviving triangle.
 */
#ifndef PVD_HIP_MESH_SIMPLIFY_H
#define PVD_HIP_MESH_SIMPLIFY_H

#include "pvd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Cells per axis: 1 .. PVD_MESH_SIMPLIFY_MAX_G.  Attributes per vertex: 0 .. PVD_MESH_SIMPLIFY_MAX_K.  V, T: at most 2^31 - 1. */
#define PVD_MESH_SIMPLIFY_MAX_G 512
#define PVD_MESH_SIMPLIFY_MAX_K 8

/* The displacement bound derived above, per axis (float64): extent e, cells per axis G, the box lo .. hi on that axis. */
#define PVD_MESH_SIMPLIFY_ABS_(x) ((x) < 0 ? -(x) : (x))
#define PVD_MESH_SIMPLIFY_BOUND(e, G, lo, hi) \
    ((e) / (double)(G) + 0x1p-30 * (e) +      \
     0x1p-23 * (PVD_MESH_SIMPLIFY_ABS_(lo) > PVD_MESH_SIMPLIFY_ABS_(hi) ? PVD_MESH_SIMPLIFY_ABS_(lo) : PVD_MESH_SIMPLIFY_ABS_(hi)))

/* Bytes of workspace for V vertices, T triangles, G^3 cells and K attributes (0 for a G, K, V or T outside the limits), with
 * C = G^3 and M = min(V, C), the largest possible number of new vertices:
 *     8 (4 + K) M (per new vertex n, S_x, S_y, S_z, A_0 .. A_{K-1}, 64-bit each)
 *     + 4 V (the cell of every vertex)  +  4 C (per cell the flag, then its new index)  +  4 ceil(C / 256) (partial sums)
 *     + 4 T (per triangle the flag, then its output row)  +  4 ceil(T / 256) (partial sums). */
size_t pvd_mesh_simplify_workspace_bytes(uint32_t V, uint32_t T, uint32_t G, uint32_t K);

/* The count phase: per vertex its cell; per triangle whether it survives, and a 1 stored into the flag word of each of its three
 * cells; exclusive scans over the G^3 cell flags and the T triangle flags (per-256 sums, a one-workgroup scan, offsets).  Leaves the
 * workspace as pvd_mesh_simplify_emit needs it and totals_dev int32 [2] <- (V', T') on the device.  One memset and eight launches on
 * the stream; no workgroup waits on another one, no retry loops, no float atomics (no atomics at all in this phase).  V == 0 or
 * T == 0 is allowed (vertices / triangles may then be NULL).  The workspace must be 16-byte aligned.  NULL pointer, unaligned or
 * short workspace (pvd_mesh_simplify_workspace_bytes(V, T, G, K)): PVD_ERR_INVALID; G, K, V or T outside the limits:
 * PVD_ERR_UNSUPPORTED; both before any device call. */
int pvd_mesh_simplify_count(const float *vertices, uint32_t V, const int32_t *triangles, uint32_t T, const float *bmin3,
                            const float *bmax3, uint32_t G, uint32_t K, void *workspace, size_t workspace_bytes, int32_t *totals_dev,
                            pvd_stream_t stream);

/* The emit phase, for the SAME vertices, triangles, box, G, K and the workspace pvd_mesh_simplify_count left; Vn and Tn are the
 * totals it wrote.  vertex_map [V] i32 is always written when V > 0 (all -1 when Vn == 0).  Per vertex: vertex_map and 64-bit
 * integer atomicAdd into the kept cell's n, S, A; per new vertex: out_vertices [Vn,3] f32 and out_attrs [Vn,K] f32; per surviving
 * triangle: its remapped row of out_triangles [Tn,3] i32 at its scanned offset.  One memset and up to three launches.  Rows past Vn /
 * Tn are never written, whatever the workspace holds.  attrs and out_attrs may be NULL when K == 0, out_vertices / out_attrs when
 * Vn == 0, out_triangles when Tn == 0, vertex_map when V == 0.  Argument checks as for pvd_mesh_simplify_count; Vn > min(V, G^3) or
 * Tn > T: PVD_ERR_INVALID. */
int pvd_mesh_simplify_emit(const float *vertices, uint32_t V, const int32_t *triangles, uint32_t T, const float *attrs, uint32_t K,
                           const float *bmin3, const float *bmax3, uint32_t G, void *workspace, size_t workspace_bytes,
                           float *out_vertices, uint32_t Vn, float *out_attrs, int32_t *out_triangles, uint32_t Tn, int32_t *vertex_map,
                           pvd_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* PVD_HIP_MESH_SIMPLIFY_H */
