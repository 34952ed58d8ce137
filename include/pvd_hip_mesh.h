/*
 * pvd_hip_mesh.h -- a triangle mesh of the level set u = thresh of a density volume, in libpvd_hip.so next to the entry points
 * pvd_hip.h declares.  Same conventions as pvd_hip.h (device pointers, caller-allocated buffers, the stream as void*, PVD_OK or a
 * negative pvd_status).  pvd_abi_version() is not changed by these additions.
 *
 * reference: extract_fields / extract_geometry, distill_mutual/utils.py:442-488 (a density volume of resolution^3 samples,
 * mcubes.marching_cubes on the host, vertices mapped back into the box at utils.py:484-487).  Here the surface is extracted on
 * the device by marching tetrahedra on the Kuhn split of every cell, which has no ambiguous case and is watertight by construction.
 *
 * Field    u [R,R,R] f32, x-major: u[(i * R + j) * R + k].  A lattice point is INSIDE iff u > thresh (NaN and u == thresh: outside).
 * Split    each of the (R-1)^3 cells is cut into the 6 tetrahedra around its diagonal (0,0,0) -> (1,1,1), one per order in which
 *          the axes are walked: tetrahedron (a,b,c) has the corners 0, e_a, e_a + e_b, (1,1,1), numbered 0..3 in that order; the
 *          tetrahedra are numbered 0..5 = xyz, xzy, yxz, yzx, zxy, zyx.  The split is the same in every cell.
 * Vertices live on lattice edges.  Point p owns the 7 edges p -> p + d, d = (1,0,0), (0,1,0), (0,0,1), (1,1,0), (1,0,1), (0,1,1),
 *          (1,1,1) (edge slots 0..6), where p + d is a lattice point.  An edge carries a vertex iff exactly one endpoint is inside.
 *          With a = p, b = p + d:  t = (thresh - u_a) / (u_b - u_a)  (f32: two rounded differences, one division),  lattice position
 *          p + d * t (one rounded sum per moving axis),  world position ((v / (R-1)) * (bmax - bmin)) + bmin per axis.  0 <= t <= 1
 *          for finite u; an edge whose outside endpoint is NaN carries a vertex with NaN coordinates.
 *          Order: ascending (owner's linear index, edge slot).
 * Triangles index those vertices (no duplicates).  Order: ascending (cell linear index, tetrahedron, triangle 0..1).  In a tetrahedron
 *          with one corner A on one side and B < C < D on the other: (AB, AC, AD), where XY is the vertex on the edge between corners X
 *          and Y; with A < B on the inside and C < D outside: (AC, AD, BD) and (AC, BD, BC).  The second and third vertex of every
 *          triangle are exchanged where needed so that normals point from inside to outside: for one / three inside corners iff
 *          (tetrahedron is xzy, yxz or zyx) xor (A is odd) xor (three are inside); for two iff (tetrahedron is xzy, yxz or zyx) xor
 *          (the number of pairs (inside corner > outside corner) is odd).  A closed component has positive signed volume.
 */
#ifndef PVD_HIP_MESH_H
#define PVD_HIP_MESH_H

#include "pvd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Lattice points per edge: 2 .. PVD_MESH_MAX_R.  Offsets are 32-bit: the worst case, 7 * 512^3 vertices, fits an int32 index. */
#define PVD_MESH_MAX_R 512

/* Bytes of workspace for a field of R^3 samples (0 for an R outside 2 .. PVD_MESH_MAX_R): per lattice point two 32-bit offsets and
 * two bytes of counts, plus two partial sums per 256 points. */
size_t pvd_mesh_workspace_bytes(uint32_t R);

/* Count pass and the two exclusive scans (three launches, no workgroup waits on another): leaves in the workspace what
 * pvd_mesh_emit needs and writes totals_dev[0] = number of vertices V, totals_dev[1] = number of triangles T (device uint32 [2]).
 * The workspace must be 4-byte aligned.  NULL pointer, unaligned or short workspace: PVD_ERR_INVALID; R outside
 * 2 .. PVD_MESH_MAX_R: PVD_ERR_UNSUPPORTED; both before any device call. */
int pvd_mesh_count(const float *field, uint32_t R, float thresh, void *workspace, size_t workspace_bytes, uint32_t *totals_dev,
                   pvd_stream_t stream);

/* Emit pass: vertices [V,3] f32 (world positions), triangles [T,3] i32, for the SAME field, R, thresh and the workspace as
 * pvd_mesh_count left it; V and T are the totals it wrote (rows past V or T are never written).  bmin3 / bmax3: device f32 [3].
 * V == 0 and T == 0: PVD_OK with no launch (vertices / triangles may be NULL).  Otherwise the argument checks of pvd_mesh_count. */
int pvd_mesh_emit(const float *field, uint32_t R, float thresh, const float *bmin3, const float *bmax3, const void *workspace,
                  size_t workspace_bytes, float *vertices, uint32_t V, int32_t *triangles, uint32_t T, pvd_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* PVD_HIP_MESH_H */
