/*
 * pvd_hip_mesh_ray.h -- the first hit of many rays on a triangle mesh, in libpvd_hip.so next to the point-to-mesh distance of
 * pvd_hip_mesh_dist.h: the primitive under rendering an extracted mesh from a camera pose (pvd/mesh.py: mesh_raycast, render_mesh,
 * evaluate_mesh_views).  Same conventions as pvd_hip.h (device pointers, caller-allocated buffers, the stream as void*, PVD_OK or a
 * negative pvd_status).  pvd_abi_version() is not changed by this addition.
 *
 * Mesh     vertices [V,3] f32, triangles [T,3] i32.  A triangle is VALID under the rule of pvd_hip_mesh_dist.h: its three indices
 *          are in [0, V) and its nine coordinates are finite.  Invalid triangles take no part.
 *
 * Ray      (o, d), six f32.  d need not be unit length; t is in units of |d|.  A ray is VALID iff its six numbers are finite and
 *          d != 0.  An invalid ray returns t = NaN, tri = -1, bary = (0, 0), and the search is not entered.
 *
 * hit(ray, triangle (a, b, c))    the watertight test of Woop, Benthin and Wald (JCGT 2013), evaluated entirely in float64 from the
 *          float32 inputs.  Every operation below is ONE IEEE float64 add, subtract, multiply or divide, in the order written, and
 *          NO PRODUCT IS FUSED INTO A SUM (no fused multiply-add):
 *            1. kz = argmax |d|, ties to the lowest axis; kx = (kz + 1) % 3, ky = (kx + 1) % 3; kx and ky swapped when d[kz] < 0.
 *            2. Sx = d[kx] / d[kz],  Sy = d[ky] / d[kz],  Sz = 1 / d[kz].
 *            3. per corner, P = corner - o:   X = P[kx] - Sx * P[kz],   Y = P[ky] - Sy * P[kz],   Z = Sz * P[kz].
 *            4. U = Xc * Yb - Yc * Xb,   V = Xa * Yc - Ya * Xc,   W = Xb * Ya - Yb * Xa.
 *            5. miss iff some of U, V, W is < 0 and some is > 0.
 *            6. det = (U + V) + W; miss iff det == 0.
 *            7. t = ((U * Za + V * Zb) + W * Zc) / det.
 *            8. hit iff t_min <= t < t_max, compared on the float64 t.  Both faces count.
 *          Why no fusion: the edge function of the edge (b, c) is Xc * Yb - Yc * Xb in one triangle and Xb * Yc - Yb * Xc in its
 *          neighbour across that edge (the corners' X and Y are the same float64 numbers in both, they depend on the corner and the
 *          ray only).  With every product rounded on its own, the second is the bitwise negation of the first, so the two triangles
 *          cannot both see the ray on their outer side of the edge: a ray that enters a closed mesh cannot slip between two
 *          triangles.  A fused a * b - c * d rounds c * d but not a * b and breaks that symmetry.
 *
 * Result   the winner is the smallest (t, triangle index) over the valid triangles that are hit, compared lexicographically on the
 *          float64 t.  Hit: t = that t rounded once to float32, tri = the index, bary = ((float)(V / det), (float)(W / det)) -- the
 *          weights of the corners b and c; a's is 1 - the two.  No hit: t = (float)t_max, tri = -1, bary = (0, 0).
 *          t_min must be finite and >= 0; t_max > t_min, and may be +inf.
 *
 * Independence   t, tri and bary depend on neither G, the box, the order of the triangles inside a cell, nor the run: hit() is a
 *          function of the ray and the triangle alone and the minimum is exact, so the only thing the grid can change is WHICH
 *          triangles are tested.  "Walk" below shows that the winner is always among them -- WITH ONE EXCEPTION, named under "THE
 *          POINT OF THE TRIANGLE": a triangle that the ray sees edge-on, within rounding of its plane, may report a hit whose point
 *          lies outside its own range of cells; a grid that stops on another hit before reaching that range then differs from G = 1,
 *          which tests everything.  For every other (ray, triangle) pair the promise holds without condition.
 *
 * Grid     G^3 cells over the box bmin .. bmax, z fastest.  Along an axis whose extent e_a = bmax_a - bmin_a is a positive finite
 *          number, h_a = e_a / G and the cell coordinate of x is
 *              k_a(x) = clamp(floor((x - bmin_a) * (G / e_a)), 0, G - 1)                     (float64, one monotone function of x).
 *          An axis whose extent is not a positive finite number is FLAT: it has one layer of cells (k_a = 0) that reaches from
 *          -inf to +inf, and takes no part in clipping or stepping.
 *          eps_a = 2^-20 e_a.  A valid triangle whose bounding box lies in the box (bmin_a <= min and max <= bmax_a on every axis
 *          that is not flat) is INSIDE and is entered into every cell of k_a(min_a - eps_a) .. k_a(max_a + eps_a), all axes.  Every
 *          other valid triangle is OUTSIDE and goes onto a list that every ray tests one by one.  With the box the bounding box of
 *          the vertices that list is empty.
 *
 * Walk     one lane per ray.  (1) Clip: [t0, t1] = [t_min, t_max] cut by the slabs bmin_a - eps_a / 4 .. bmax_a + eps_a / 4 of the
 *          axes that are not flat; empty: the grid is skipped.  (2) Start in the cell k(o + t0 d).  (3) Test the cell's triangles.
 *          (4) t_exit = the smallest, over the axes the ray moves along, of ((bmin_a + j h_a) - o_a) * (1 / d_a), j the cell's face
 *          in the direction of travel -- computed afresh from the integer j in every cell, never accumulated.  (5) Stop when
 *          t_exit >= t1, when a hit is held with best_t < t_exit (1 - 2^-30), or when the step leaves the grid; otherwise step
 *          along the axis of t_exit and go to (3).  (6) Test the outside list.
 *          FAR RAYS.  With M_a = |o_a| + |d_a| t1 + |bmin_a| + |bmax_a|: if 2^-40 M_a > eps_a on some axis that is not flat, the
 *          grid is not used and the ray tests every triangle.  For all other rays every float64 rounding of a position on the ray
 *          or of a face (a handful of roundings of 2^-53 M_a each) is below sigma_a = 2^-50 M_a <= 2^-10 eps_a.
 *          WHY NO WINNER IS MISSED.  Along an axis the ray's coordinate is monotone in t.  At the t_exit of a cell it is within
 *          sigma_a of the face the walk steps through, and along the other axes it has not passed their faces by more than sigma_a
 *          (t_exit is the smallest); the start lies within eps_a / 4 + sigma_a of its cell (the clip's dilation, then the clamp of
 *          k_a, whose own rounding moves a cell boundary by less than 2^-41 h_a).  By induction every point o + t d, t0 <= t <=
 *          t_exit, lies within eps_a / 2 of a cell that has been visited.  Take an INSIDE triangle that is hit at t* <= best_t with
 *          a point of the triangle within eps_a / 4 of o + t* d on every axis (see below).  Its bounding box lies in the box, so
 *          that point survives the clip, t0 <= t* <= t1; and if the walk stopped on best_t then t* < t_exit.  So o + t* d is
 *          within eps_a / 2 of a visited cell, the triangle's bounding box is within 3 eps_a / 4 of it, and its range
 *          k_a(min_a - eps_a) .. k_a(max_a + eps_a) contains that cell: the triangle was tested.  The margin 2^-30 only makes the
 *          walk stop later.  OUTSIDE triangles and far rays are tested against everything.
 *          THE POINT OF THE TRIANGLE.  Step 7 is a mean of Za, Zb, Zc with the weights U / det, V / det, W / det, which are >= 0
 *          for a hit, so o + t* d lies within the triangle's extent along kz up to rounding -- always.  Along kx and ky the same
 *          weights place it within a few 2^-53 M_a of the triangle as long as det is not itself rounding noise, i.e. unless the
 *          ray lies in the plane of the triangle to within about 2^-30 (relative) AND the triangle's image under step 3 is a
 *          segment on a line through the origin.  hit() of such a pair is decided by the last bits of U, V, W and may report a t
 *          anywhere in the triangle's Z range; it is still a fixed function of the ray and the triangle, but for that pair alone
 *          the walk's argument does not hold.  (A ray that lies EXACTLY in the plane gives U = V = W = 0, det == 0: a miss.)
 *          Work per ray: at most 3 (G - 1) + 1 cells, each triangle once per cell it shares with the ray.
 *          Work per triangle in the build: ONE LANE walks the whole range of a triangle, one integer atomicAdd per cell in the bin
 *          pass and one in the fill pass.  A mesh of lattice-sized triangles has a handful of cells each (1.1 .. 5.1 at G = 16 .. 256
 *          for a 256^3 extraction); a single triangle that spans the box costs G^3 atomics on its lane, 16.7 million at G = 256,
 *          and that many pairs: a mesh with large triangles wants a small G, or a box that leaves them outside.  Not measured
 *          beyond one box-spanning triangle at G = 32.
 */
#ifndef PVD_HIP_MESH_RAY_H
#define PVD_HIP_MESH_RAY_H

#include "pvd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Cells per axis: 1 .. PVD_MESH_RAY_MAX_G.  Triangles: at most 2^31 - 1 (indices are int32).  (cell, triangle) pairs: at most 2^31 - 1. */
#define PVD_MESH_RAY_MAX_G 256

/* Bytes of workspace for T triangles, G^3 cells and `pairs` (cell, triangle) pairs (0 for a G outside 1 .. PVD_MESH_RAY_MAX_G, a T or a
 * pairs above 2^31 - 1): a header of 64 bytes (the box, the two totals), 48 bytes per triangle (the nine coordinates and the index,
 * packed in input order: a test reads three aligned 16-byte words), per cell a start and a cursor (4 bytes each, one more start) plus
 * one partial sum per 256 cells, 4 bytes per triangle for the outside list and 4 bytes per pair (an index into the packed array):
 *     64 + 48 T + 4 (G^3 + 1) + 4 G^3 + 4 ceil(G^3 / 256) + 4 T + 4 pairs. */
size_t pvd_mesh_ray_workspace_bytes(uint32_t T, uint32_t G, uint64_t pairs);

/* totals [2] u64 on the device <- (the number of (cell, triangle) pairs, the number of outside triangles) of the mesh (vertices [V,3]
 * f32, triangles [T,3] i32) over G^3 cells of the box bmin3 .. bmax3 (device f32 [3] each).  One memset and one launch, one lane per
 * triangle, one integer atomicAdd per wave and total.  The caller reads the first total back and sizes the workspace with it.  T == 0
 * is allowed (triangles may be NULL; V == 0: vertices may be NULL).  NULL bmin3, bmax3 or totals: PVD_ERR_INVALID; G outside
 * 1 .. PVD_MESH_RAY_MAX_G or T above 2^31 - 1: PVD_ERR_UNSUPPORTED; both before any device call. */
int pvd_mesh_ray_count(const float *vertices, uint32_t V, const int32_t *triangles, uint32_t T, const float *bmin3, const float *bmax3,
                       uint32_t G, uint64_t *totals, pvd_stream_t stream);

/* Fills the workspace with what pvd_mesh_ray_cast needs, for the SAME mesh, box and G as pvd_mesh_ray_count and the `pairs` it left:
 * the box, the packed triangles, the cell starts (a CSR over the cells), the pair list and the outside list.  Bin (integer atomicAdd per
 * pair on the cell's count, one per outside triangle) -> per-256-cell sums -> one-workgroup scan -> offsets -> fill (integer atomicAdd
 * on the cell's cursor): five launches and two memsets on the stream, no workgroup waits on another one, no retry loops.  The order of
 * the pairs inside a cell and of the outside list depends on the run; no output of the cast does.  A `pairs` smaller than the true
 * total loses pairs but never writes outside the workspace.  The workspace must be 16-byte aligned.  NULL pointer, unaligned or short
 * workspace (pvd_mesh_ray_workspace_bytes(T, G, pairs)): PVD_ERR_INVALID; G, T or pairs out of range: PVD_ERR_UNSUPPORTED; both
 * before any device call. */
int pvd_mesh_ray_build(const float *vertices, uint32_t V, const int32_t *triangles, uint32_t T, const float *bmin3, const float *bmax3,
                       uint32_t G, uint64_t pairs, void *workspace, size_t workspace_bytes, pvd_stream_t stream);

/* t [N] f32, tri [N] i32, bary [N,2] f32 <- the result defined above for the rays origins [N,3] f32, dirs [N,3] f32, against the mesh
 * pvd_mesh_ray_build left in the workspace for the SAME T, G and pairs (the cast reads the mesh and the box from the workspace only).
 * One launch, one lane per ray, no LDS, no atomics; rows past N are never written.  t_min finite and >= 0, t_max > t_min (+inf
 * allowed), else PVD_ERR_INVALID; then the workspace checks of pvd_mesh_ray_build; then N == 0: PVD_OK with no launch (the ray and
 * result pointers may be NULL); then NULL ray or result pointers: PVD_ERR_INVALID.  All before any device call. */
int pvd_mesh_ray_cast(const float *origins, const float *dirs, uint32_t N, uint32_t T, uint32_t G, uint64_t pairs, const void *workspace,
                      size_t workspace_bytes, float t_min, float t_max, float *t, int32_t *tri, float *bary, pvd_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* PVD_HIP_MESH_RAY_H */
