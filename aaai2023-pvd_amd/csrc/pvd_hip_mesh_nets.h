/*
 * pvd_hip_mesh_nets.h -- a second mesher for the level set u = thresh of a density volume: NAIVE SURFACE NETS, one vertex per active
 * cell and one quad (two triangles) per sign-changing lattice edge, in libpvd_hip.so next to the marching tetrahedra of
 * include/pvd_hip_mesh.h (pvd/mesh.py: extract_mesh(..., method="nets")).  Marching tetrahedra stay the default and are untouched.  Same
 * conventions as pvd_hip.h (device pointers, caller-allocated buffers, the stream as void*, PVD_OK or a negative pvd_status).
 * pvd_abi_version() is not changed by this addition.
 * (This header lives next to csrc/mesh_nets.hip and not in include/: tests/test_abi_mesh_tex.py pins the list of files there.)
 *
 * reference: extract_fields / extract_geometry, distill_mutual/utils.py:442-488 (mcubes.marching_cubes on the host).  Surface nets need
 * no case table: everything below is counting, integer scans and per-item float arithmetic.
 *
 * EVERY FLOAT OPERATION BELOW IS ONE IEEE float32 OPERATION, IN THE ORDER WRITTEN, AND NOTHING IS FUSED.
 *
 * Field, lattice, inside rule and box mapping are those of pvd_hip_mesh.h: u [R,R,R] f32, x-major, u[(i * R + j) * R + k]; a lattice
 *          point is INSIDE iff u > thresh (NaN and u == thresh: outside); a lattice position v maps to the world position
 *          ((v / (float)(R-1)) * (bmax - bmin)) + bmin per axis; R is 2 .. PVD_MESH_MAX_R.
 *
 * Cells    cell q = (i,j,k), 0 <= i,j,k <= R-2, has the 8 corners q + o, o in {0,1}^3.  A cell is ACTIVE iff at least one corner is
 *          inside and at least one is not.  Cell q is indexed by the linear index of its lowest corner as a lattice point,
 *          (i * R + j) * R + k; a lattice point with a coordinate R-1 owns no cell.
 *
 * Edges of a cell   edge e = 4a + 2*o_b + o_c, with a = 0,1,2, b = (a+1)%3, c = (a+2)%3 and o_b, o_c in {0,1}, runs from
 *          A = q + o_b e_b + o_c e_c to B = A + e_a.  It CROSSES iff exactly one of A, B is inside.  On a crossing edge
 *              t = (thresh - u_A) / (u_B - u_A)          (two rounded differences, one division: the very expression of pvd_hip_mesh.h,
 *                                                         so the four cells around a lattice edge see the same bits)
 *
 * Vertex of an active cell   the local coordinate of a crossing is l_a = t, l_b = (float)o_b, l_c = (float)o_c.
 *              s = the sum of l over the crossing edges in ascending e, sequential, per axis (s starts at 0.0f)
 *              n = the number of crossing edges (3 .. 12 in an active cell),   m = s / (float)n
 *              lattice position (float)q + m (one rounded sum per axis), then the box mapping above.
 *          0 <= m <= 1 EXACTLY for finite u: 0 <= t <= 1 (pvd_hip_mesh.h), so every term lies in [0,1]; a partial sum of k terms is the
 *          rounding of a real number in [0,k], and k is representable, so by the monotonicity of rounding it lies in [0,k]; s lies in
 *          [0,n] and s / n, rounded, in [0,1].  (float)q + m then lies in [q, q+1]: THE VERTEX NEVER LEAVES ITS CELL.
 *          An edge whose outside endpoint is NaN has t = NaN and gives the vertex NaN coordinates, as in pvd_hip_mesh.h.
 *          Vertex order: ascending cell index.  V = the number of active cells.
 *
 * Quads    take a lattice point p and an axis a with p_a <= R-2.  The lattice edge p -> p + e_a is INTERIOR iff 1 <= p_b <= R-2 and
 *          1 <= p_c <= R-2.  Every crossing interior edge emits one quad over the vertices of the four cells
 *              q0 = p - e_b - e_c,   q1 = p - e_c,   q2 = p,   q3 = p - e_b          (all four are active: each contains the edge)
 *          in the sequence (k0,k1,k2,k3) = (q0,q1,q2,q3) if p is inside, else (q0,q3,q2,q1).  Seen from +a the first sequence runs
 *          counter-clockwise, so normals point from inside to outside and a closed component has positive signed volume.
 *          Crossing edges on the box faces emit nothing: THE SURFACE IS OPEN WHERE IT LEAVES THE BOX.
 *
 * Split of a quad   from the emitted float32 world positions P0..P3 of k0..k3:
 *              d02 = (dx*dx + dy*dy) + dz*dz with d = P2 - P0,    d13 the same with d = P3 - P1
 *              if d13 < d02:  triangles (k0,k1,k3) and (k1,k2,k3);   otherwise, and on ties or NaN:  (k0,k1,k2) and (k0,k2,k3).
 *          Triangle order: ascending (p's linear index, a), two triangles per quad in the order above.
 *          T = 2 * (the number of crossing interior lattice edges).
 *
 * Normals  the gradient of the field at the vertex.  With the lattice gradient g(.) (central differences, one-sided on the faces, times
 *          inv_h_a = (float)(R - 1) / (bmax_a - bmin_a)) and the per-edge expression G_e = g(A) + t * (g(B) - g(A)) EXACTLY as
 *          include/pvd_hip_mesh_attr.h defines them:
 *              G = (the sum of G_e over the same crossing edges, same order, sequential from 0.0f, per axis) / (float)n
 *              len = sqrtf(G_x * G_x + G_y * G_y + G_z * G_z)  (summed left to right),    n_a = (-G_a) / len
 *          and n = (0, 0, 0) when len is 0 or not finite, the rule of that header.
 *
 * Properties and limits
 *          - All of it is integer scans (csrc/block_scan.h) plus per-item float arithmetic, with NO ATOMICS: the bits are the same every
 *            run, and do not depend on the order in which workgroups run.
 *          - Away from the box faces every triangle edge is shared an even number of times: a quad side joins two cells that share a
 *            lattice face, the quads through it are those of the face's crossing edges, and a face has 0, 2 or 4 of them; a diagonal is
 *            used by the two triangles of its quad only.
 *          - Where a lattice face has exactly its two diagonal corners inside (an AMBIGUOUS face) all four of its edges cross, four quads
 *            meet in one triangle edge and the mesh is NOT MANIFOLD there.
 *          - A cell whose inside corners (or whose outside corners) fall apart under the cube's edges joins two sheets in one vertex.
 *          - Sharp features are not recovered: the vertex is a mean of edge crossings.  QEF placement, i.e. dual contouring, is not
 *            attempted.
 *          - Connected components (include/pvd_hip_components.h) follow the Kuhn split's connectivity; at ambiguous faces the shells of
 *            this mesh can differ from them.
 */
#ifndef PVD_HIP_MESH_NETS_H
#define PVD_HIP_MESH_NETS_H

#include "../../include/pvd_hip_mesh.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PVD_MESH_NETS_CELL_EDGES 12 /* edges of a cell: e = 4a + 2*o_b + o_c */
#define PVD_MESH_NETS_TOTALS 2      /* V, T */

/* Bytes of workspace for a field of R^3 samples (0 for an R outside 2 .. PVD_MESH_MAX_R): per lattice point two 32-bit offsets and one
 * byte of flags (bit 0: the point's cell is active; bits 1..3: the edge p -> p + e_a, a = 0..2, emits a quad), plus two partial sums per
 * 256 points.  Host only. */
size_t pvd_mesh_nets_workspace_bytes(uint32_t R);

/* Count pass and the two exclusive scans (three launches, no workgroup waits on another): leaves in the workspace what the passes below
 * need and writes totals_dev[0] = V, totals_dev[1] = T (device uint32 [2]).  The workspace must be 4-byte aligned.  NULL pointer,
 * unaligned or short workspace: PVD_ERR_INVALID; R outside 2 .. PVD_MESH_MAX_R: PVD_ERR_UNSUPPORTED; both before any device call. */
int pvd_mesh_nets_count(const float *field, uint32_t R, float thresh, void *workspace, size_t workspace_bytes, uint32_t *totals_dev,
                        pvd_stream_t stream);

/* Emit pass: vertices [V,3] f32 (world positions), triangles [T,3] i32, for the SAME field, R, thresh and the workspace as
 * pvd_mesh_nets_count left it; V and T are the totals it wrote (rows past V or T are never written, and no vertex row past V is read: a
 * quad with such a corner takes the NaN branch of the split).  Two launches, the vertices and then the triangles, which read them.
 * bmin3 / bmax3: device f32 [3].  V == 0 and T == 0: PVD_OK with no launch (vertices / triangles may be NULL).
 * Otherwise the argument checks of pvd_mesh_nets_count, before any device call. */
int pvd_mesh_nets_emit(const float *field, uint32_t R, float thresh, const float *bmin3, const float *bmax3, const void *workspace,
                       size_t workspace_bytes, float *vertices, uint32_t V, int32_t *triangles, uint32_t T, pvd_stream_t stream);

/* normals [V,3] f32: row v is the normal of vertex v of pvd_mesh_nets_emit ("Normals" above), same field, R, thresh, box and workspace.
 * One launch.  V == 0: PVD_OK with no launch (normals may be NULL).  Otherwise the argument checks of pvd_mesh_nets_count, all of them
 * before any device call. */
int pvd_mesh_nets_normals(const float *field, uint32_t R, float thresh, const float *bmin3, const float *bmax3, const void *workspace,
                          size_t workspace_bytes, float *normals, uint32_t V, pvd_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* PVD_HIP_MESH_NETS_H */
