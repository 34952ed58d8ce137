/*
 * pvd_hip_mesh_winding.h -- is this point inside the mesh?  The integer winding number of many points, and of every point of an
 * R^3 lattice, against a triangle mesh, in libpvd_hip.so next to the ray casting of pvd_hip_mesh_ray.h: the primitive under
 * pvd/mesh.py: mesh_winding, mesh_contains, voxelize_mesh, mesh_signed_distance, mesh_to_sdf and compare_meshes(volume=R).  Same
 * conventions as pvd_hip.h (device pointers, caller-allocated buffers, the stream as void*, PVD_OK or a negative pvd_status).
 * pvd_abi_version() is not changed by this addition.
 *
 * Mesh     vertices [V,3] f32, triangles [T,3] i32.  A triangle is VALID under the rule of pvd_hip_mesh_dist.h: its three indices
 *          are in [0, V) and its nine coordinates are finite.  Invalid triangles take no part.
 *
 * w(p)     the number of signed crossings of the ray from p along +z:   w(p) = sum of s(t) over the valid triangles t that cross,
 *          s = +1 where the triangle's normal has a positive z component, -1 where it is negative.  A point inside a closed mesh
 *          oriented as pvd_mesh_emit orients it (normals outwards) gets +1, a point outside gets 0.  Rays go along +z because z is
 *          the fastest axis of a volume: a column of lattice points that share a ray is contiguous in memory.
 *
 * Arithmetic   everything is evaluated in float64 from the float32 inputs.  Every operation below is ONE IEEE float64 add,
 *          subtract, multiply or divide, in the order written, and NO PRODUCT IS FUSED INTO A SUM (no fused multiply-add).
 *
 * Edge function   of the UNDIRECTED edge between the vertex indices iu < iw, at p:
 *              E(p) = (xw - xu) * (py - yu) - (yw - yu) * (px - xu).
 *          The directed edge from the lower to the higher index has the edge function E and the vector (xw - xu, yw - yu); the
 *          directed edge from the higher to the lower index has -E and the negated vector.  (iu == iw: either; both are 0.)
 *          Why: two triangles that share an edge evaluate ONE expression on the same float64 numbers, whatever their corner order,
 *          and use it with opposite signs -- bitwise negations of one number.  With every product rounded on its own that number
 *          has one sign, so the two triangles cannot both see the point on their inner side of the edge, nor both on their outer
 *          side: a ray that enters a closed mesh cannot slip between two triangles, and cannot be counted by both.  A fused
 *          a * b - c * d rounds c * d but not a * b; evaluating the edge in each triangle's own corner order rounds differently
 *          in the two.  Either breaks that symmetry.
 *
 * Triangle (a, b, c) against p:
 *            1. s = the sign of the directed edge function of (a, b) at c.  s == 0 (the projected area is zero): skipped.
 *            2. e_bc, e_ca, e_ab = the directed edge functions of (b, c), (c, a), (a, b) at p, each multiplied by s;
 *               (dx, dy) of an edge = the directed edge's vector, multiplied by s.
 *            3. COVERAGE: p is covered iff for each of the three edges   e > 0,   or   e == 0 and (dy > 0, or dy == 0 and dx < 0).
 *               Two triangles on the two sides of an edge have opposite (dx, dy) there, so a ray through a shared edge or a shared
 *               vertex is counted by exactly one side.
 *            4. z_hit = ((e_bc * za + e_ca * zb) + e_ab * zc) / ((e_bc + e_ca) + e_ab).
 *            5. CROSSING: the triangle crosses iff it covers p and z_hit > pz, strictly (false for a z_hit that is NaN).
 *
 * Points that are not finite get PVD_MESH_WINDING_INVALID.
 *
 * Independence   w is a sum of integers.  It depends on the set of valid triangles and on p only: not on the order of the
 *          triangles or of a triangle's corners (a rotation; a reversal negates w), not on G, the box or the run.  The grid only
 *          decides WHICH triangles a point tests, and it never leaves out one that covers it: a computed edge value has the sign
 *          of the exact one or is 0 (differences of float32 numbers keep their sign in float64, products of them neither
 *          overflow nor underflow, and rounding is monotone), so a covered p lies in the closed bounding box of the triangle's x
 *          and y, hence in a cell of its range.
 *
 * Limits   A point EXACTLY ON THE SURFACE is decided by the rule above, not by geometry: z_hit carries the rounding of step 4, and
 *          a point within that rounding of a triangle may land on either side.  An OPEN or INCONSISTENTLY ORIENTED mesh has no
 *          inside: its values depend on the direction of the ray, and are what the ray along +z gives.  (pvd_hip_mesh_topo.h
 *          reports boundary and inconsistent edges; the third total of pvd_mesh_winding_lattice counts the columns that saw it.)
 *
 * Grid     G^2 cells over the x and y extent of the box bmin .. bmax (the z entries are not read), y fastest: the cell function,
 *          the flat axes and eps_a = 2^-20 e_a of pvd_hip_mesh_ray.h, on two axes.  A valid triangle whose bounding box in x and y
 *          lies in the box is INSIDE and is entered into every cell of k_a(min_a - eps_a) .. k_a(max_a + eps_a); every other valid
 *          triangle is OUTSIDE and goes onto a list that every point tests.  A point tests the list of the cell (k_x(px), k_y(py))
 *          when lo_a <= p_a <= hi_a on both axes that are not flat, and the outside list always.
 *          Work per triangle in the build: ONE LANE walks the whole range of a triangle, one integer atomicAdd per cell in the
 *          bin pass and one in the fill pass; a triangle that spans the box costs G^2 of them.
 *
 * Lattice  the point (i, j, k) of an R^3 lattice over lat_bmin .. lat_bmax is the float32 triple
 *              c_a(n) = (float)n / (float)(R - 1) * (hi_a - lo_a) + lo_a,        every operation rounded to float32,
 *          of (i, j, k) on the axes (x, y, z).  The volume is x-major, z fastest: winding[(i * R + j) * R + k].
 */
#ifndef PVD_HIP_MESH_WINDING_H
#define PVD_HIP_MESH_WINDING_H

#include "pvd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The value of a point that is not finite: INT32_MIN. */
#define PVD_MESH_WINDING_INVALID (-2147483647 - 1)

/* Cells per axis: 1 .. PVD_MESH_WINDING_MAX_G.  1024, not the 256 of the three-dimensional grids: the grid has G^2 cells, not G^3
 * (8 bytes each: 8 MiB at 1024), and a column of the lattice tests its cell's whole list whatever its z, so finer cells cut that
 * work directly; a lattice of up to 1024^2 columns can have a cell per column.  Points per lattice axis: 2 .. PVD_MESH_WINDING_MAX_R
 * (a column's difference array lives in LDS, 4 bytes per point).  Triangles and (cell, triangle) pairs: at most 2^31 - 1 each. */
#define PVD_MESH_WINDING_MAX_G 1024
#define PVD_MESH_WINDING_MAX_R 1024

/* Bytes of workspace for T triangles, G^2 cells and `pairs` (cell, triangle) pairs (0 for a G outside 1 .. PVD_MESH_WINDING_MAX_G, a
 * T or a pairs above 2^31 - 1): a header of 64 bytes (the box, the two totals), 48 bytes per triangle (the nine coordinates, the
 * index and the directions of the three edges, packed in input order: a test reads three aligned 16-byte words), per cell a start and
 * a cursor (4 bytes each, one more start) plus one partial sum per 256 cells, 4 bytes per triangle for the outside list and 4 bytes
 * per pair:
 *     64 + 48 T + 4 (G^2 + 1) + 4 G^2 + 4 ceil(G^2 / 256) + 4 T + 4 pairs. */
size_t pvd_mesh_winding_workspace_bytes(uint32_t T, uint32_t G, uint64_t pairs);

/* totals [2] u64 on the device <- (the number of (cell, triangle) pairs, the number of outside triangles) of the mesh over G^2 cells of
 * the box bmin3 .. bmax3 (device f32 [3] each).  One memset and one launch, one lane per triangle, one integer atomicAdd per wave and
 * total.  The caller reads the first total back and sizes the workspace with it.  T == 0 is allowed (triangles may be NULL; V == 0:
 * vertices may be NULL).  NULL bmin3, bmax3 or totals: PVD_ERR_INVALID; G outside 1 .. PVD_MESH_WINDING_MAX_G or T above 2^31 - 1:
 * PVD_ERR_UNSUPPORTED; both before any device call. */
int pvd_mesh_winding_count(const float *vertices, uint32_t V, const int32_t *triangles, uint32_t T, const float *bmin3, const float *bmax3,
                           uint32_t G, uint64_t *totals, pvd_stream_t stream);

/* Fills the workspace with what the two queries need, for the SAME mesh, box and G as pvd_mesh_winding_count and the `pairs` it left.
 * Bin -> per-256-cell sums -> one-workgroup scan -> offsets -> fill: five launches and two memsets on the stream, integer atomics
 * only, no workgroup waits on another one, no retry loops.  The order of the pairs inside a cell and of the outside list depends on
 * the run; no output of the queries does.  A `pairs` smaller than the true total loses pairs but never writes outside the workspace.
 * The workspace must be 16-byte aligned.  NULL pointer, unaligned or short workspace (pvd_mesh_winding_workspace_bytes(T, G, pairs)):
 * PVD_ERR_INVALID; G, T or pairs out of range: PVD_ERR_UNSUPPORTED; both before any device call. */
int pvd_mesh_winding_build(const float *vertices, uint32_t V, const int32_t *triangles, uint32_t T, const float *bmin3, const float *bmax3,
                           uint32_t G, uint64_t pairs, void *workspace, size_t workspace_bytes, pvd_stream_t stream);

/* winding [N] i32 <- w of the points [N,3] f32 against the mesh pvd_mesh_winding_build left in the workspace for the SAME T, G and
 * pairs.  One launch, one lane per point, no LDS, no atomics; rows past N are never written.  The workspace checks of
 * pvd_mesh_winding_build; then N == 0: PVD_OK with no launch (points and winding may be NULL); then NULL points or winding:
 * PVD_ERR_INVALID.  All before any device call. */
int pvd_mesh_winding_points(const float *points, uint32_t N, uint32_t T, uint32_t G, uint64_t pairs, const void *workspace,
                            size_t workspace_bytes, int32_t *winding, pvd_stream_t stream);

/* winding [R,R,R] i32 <- w of every point of the lattice over lat_bmin3 .. lat_bmax3 (device f32 [3] each; see "Lattice"), equal bit
 * for bit to what pvd_mesh_winding_points returns for those points; totals [4] i64 on the device <- (points with w != 0, points with
 * w > 0, leaky columns, the largest |w|), points that are not finite left out.  A LEAKY COLUMN is an (i, j) whose crossings (the
 * covering triangles with z_hit > -inf) do not sum to 0: the winding number seen from below everything, 0 for a closed mesh.
 * One memset and one launch: one wave per column tests the column's triangles ONCE, finds per crossing the number of k with
 * z_k < z_hit (z_k is monotone in k: a guess from the float64 quotient, corrected against the exact float32 z_k), adds s into a
 * difference array in LDS with integer LDS atomics, takes the suffix sum over the column in chunks of a wave with a carry, and writes
 * the column with coalesced stores.  R outside 2 .. PVD_MESH_WINDING_MAX_R: PVD_ERR_UNSUPPORTED; NULL pointers: PVD_ERR_INVALID; the
 * workspace checks of pvd_mesh_winding_build.  All before any device call. */
int pvd_mesh_winding_lattice(uint32_t R, const float *lat_bmin3, const float *lat_bmax3, uint32_t T, uint32_t G, uint64_t pairs,
                             const void *workspace, size_t workspace_bytes, int32_t *winding, int64_t *totals, pvd_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* PVD_HIP_MESH_WINDING_H */
