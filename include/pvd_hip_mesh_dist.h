/*
 * pvd_hip_mesh_dist.h -- the distance from many points to a triangle mesh, in libpvd_hip.so next to the mesh extraction of
 * pvd_hip_mesh.h: the primitive under the one-sided mean surface distance, Chamfer and Hausdorff distance and precision / recall /
 * F-score at a tolerance (pvd/mesh.py: mesh_distance, compare_meshes).  Same conventions as pvd_hip.h (device pointers,
 * caller-allocated buffers, the stream as void*, PVD_OK or a negative pvd_status).  pvd_abi_version() is not changed by this addition.
 *
 * Mesh     vertices [V,3] f32, triangles [T,3] i32.  A triangle is VALID iff its three indices are in [0, V) and its nine
 *          coordinates are finite.  Invalid triangles are skipped by the build and never reach the query.
 *
 * d(p, t)  the Euclidean distance from the point p to the closest point of the (closed) triangle t = (a, b, c), evaluated in
 *          float64 from the float32 inputs and rounded to float32 at the very end:
 *              ab = b - a, ac = c - a, n = ab x ac.
 *              t is DEGENERATE iff |n|^2 <= 2^-40 * |ab|^2 * |ac|^2 (sin^2 of the angle at a; repeated corners and collinear corners
 *              included): d^2 is then the smallest squared distance from p to the three segments ab, ac, bc (a segment of length 0
 *              is its end point).
 *              Otherwise the closest point lies in one of seven regions -- a corner, an edge, the interior --; for a corner
 *              d^2 = |p - corner|^2, for an edge |p - q|^2 with q the foot of p on the edge, for the interior (n . (p - a))^2 / |n|^2.
 *              d = (float)sqrt(d^2).
 *          Float64 because marching tetrahedra emits slivers (a crossing edge with t near 0 or 1): in float32 the normal of a
 *          sliver has a relative error of about eps / sin(angle), and a wrong normal gives a plane distance that is too small.
 *
 * Result   best = min over valid t of d(p, t); ties go to the smallest triangle index ((d, t) compared lexicographically, d as the
 *          rounded float32).  best < max_dist: dist = best, tri = t.  Otherwise, and when no triangle is valid: dist = max_dist,
 *          tri = -1.  A point with a coordinate that is not finite: dist = NaN, tri = -1, and the search is not entered.
 *          d depends on neither the grid nor the order of visits, and min is exact: dist and tri are bit-identical for every G, for
 *          every box and from run to run.
 *
 * Grid     G^3 cells over the box bmin .. bmax; h_a = (bmax_a - bmin_a) / G.  The cell coordinate of x along axis a is
 *              k_a(x) = clamp(floor((x - bmin_a) * (G / (bmax_a - bmin_a))), 0, G - 1)        (float64; one monotone function of x,
 *          the same for triangles and points), and 0 for every x on an axis whose extent is not a positive finite number (a "flat"
 *          axis).  A triangle is binned by the cell of its centroid m = (a + b + c) / 3 (float64); centroids outside the box land in
 *          border cells.  rho = the largest |corner - m| over the valid triangles, rounded up.
 *
 * Search   one lane per point p, cell k(p).  Ring r = the cells at Chebyshev distance exactly r from k(p) that lie in the grid;
 *          rings are visited in the order r = 0, 1, ...  After ring r a triangle that was not visited has its centroid m in a cell
 *          with |k_a(m) - k_a(p)| >= r + 1 on some axis a, which is not flat (on a flat axis every coordinate is 0).  Say
 *          k_a(m) >= k_a(p) + r + 1.  Then k_a(m) >= 1: m was not clamped from below, floor(..) >= k_a(m), so
 *          m_a >= bmin_a + k_a(m) h_a.  And k_a(p) <= G - 2: p was not clamped from above (it may have been clamped from below,
 *          which only moves it further away), floor(..) <= k_a(p), so p_a < bmin_a + (k_a(p) + 1) h_a.  Together
 *              |m - p| >= m_a - p_a > (k_a(m) - k_a(p) - 1) h_a >= r h_a >= r h_min,      h_min = the smallest h_a of a non-flat axis,
 *          for points outside the box and for centroids clamped into border cells alike; the other direction is symmetric.  Every
 *          point of the triangle is within rho of m, hence
 *              d(p, t) >= |p - m| - rho > r h_min - rho            for every t not visited after ring r.
 *          The search stops after ring r when   r h_min (1 - 2^-20) - rho (1 + 2^-20) > min(best, max_dist) (1 + 2^-20)   in float64.
 *          The three factors make rounding stop the search later, never earlier: the float64 cell coordinate moves a cell boundary by
 *          less than 2^-41 h_a (|k| <= 256, four roundings of 2^-53), h_min and rho carry one rounding each (rho upwards), d of a
 *          non-degenerate triangle is within 2^-53 * 2^20 of the exact one relative to |p - a| <= d + 2 rho, and the float32 rounding
 *          of d moves it by 2^-24 d -- so a triangle that was not visited has a rounded d strictly above best and cannot win a tie.
 *          It also stops when the ring has left the grid on all sides (r > the largest of k_a(p), G - 1 - k_a(p)); with no non-flat
 *          axis ring 0 is the whole mesh.  Work per point is bounded by (2 ceil((max_dist + rho) / h_min) + 1)^3 cells.
 */
#ifndef PVD_HIP_MESH_DIST_H
#define PVD_HIP_MESH_DIST_H

#include "pvd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Cells per axis: 1 .. PVD_MESH_DIST_MAX_G.  Triangles: at most 2^31 - 1 (indices are int32). */
#define PVD_MESH_DIST_MAX_G 256

/* Bytes of workspace for T triangles and G^3 cells (0 for a G outside 1 .. PVD_MESH_DIST_MAX_G or a T above 2^31 - 1): a header of 64
 * bytes (rho, the box, the number of valid triangles), 48 bytes per triangle (the nine coordinates and the index, packed in cell
 * order: a visit reads three aligned 16-byte words per triangle instead of gathering three indices and nine floats), 4 bytes per
 * triangle (its cell), and per cell a start and a cursor plus one partial sum per 256 cells. */
size_t pvd_mesh_dist_workspace_bytes(uint32_t T, uint32_t G);

/* Bins the valid triangles into the grid and leaves in the workspace what pvd_mesh_dist_query needs: the cell starts (a CSR over
 * the cells, z fastest), the triangles packed in that order, rho and the box.  vertices [V,3] f32, triangles [T,3] i32, bmin3 / bmax3:
 * device f32 [3].  Count (integer atomicAdd per cell, atomicMax for rho) -> per-256-cell sums -> one-workgroup scan -> offsets ->
 * fill (integer atomicAdd on the cell's cursor): five launches and two memsets on the stream, no workgroup waits on another one, no
 * retry loops.  The order of the triangles inside a cell depends on the run; no output of the query does.  T == 0 is allowed
 * (triangles may be NULL; V == 0: vertices may be NULL).  The workspace must be 16-byte aligned.  NULL pointer, unaligned or short
 * workspace (pvd_mesh_dist_workspace_bytes(T, G)): PVD_ERR_INVALID; G outside 1 .. PVD_MESH_DIST_MAX_G or T above 2^31 - 1:
 * PVD_ERR_UNSUPPORTED; both before any device call. */
int pvd_mesh_dist_build(const float *vertices, uint32_t V, const int32_t *triangles, uint32_t T, const float *bmin3, const float *bmax3,
                        uint32_t G, void *workspace, size_t workspace_bytes, pvd_stream_t stream);

/* dist [N] f32, tri [N] i32 <- the result defined above for points [N,3] f32, against the mesh pvd_mesh_dist_build left in the
 * workspace for the SAME T and G (the query reads the mesh and the box from the workspace only, so they cannot disagree with the
 * build).  One launch, one lane per point; rows past N are never written.  N == 0: PVD_OK with no launch (points, dist, tri may be
 * NULL).  max_dist must be finite and > 0, else PVD_ERR_INVALID; the other argument checks are those of pvd_mesh_dist_build, all
 * before any device call. */
int pvd_mesh_dist_query(const float *points, uint32_t N, uint32_t T, uint32_t G, const void *workspace, size_t workspace_bytes,
                        float max_dist, float *dist, int32_t *tri, pvd_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* PVD_HIP_MESH_DIST_H */
