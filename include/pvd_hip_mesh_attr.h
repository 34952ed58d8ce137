/*
 * pvd_hip_mesh_attr.h -- per-vertex attributes of the mesh include/pvd_hip_mesh.h extracts, in libpvd_hip.so next to its entry
 * points.  Same conventions as pvd_hip.h (device pointers, caller-allocated buffers, the stream as void*, PVD_OK or a negative
 * pvd_status).  pvd_abi_version() is not changed by this addition.
 *
 * reference: extract_fields / extract_geometry, distill_mutual/utils.py:442-488 -- the reference's mesh is geometry only; its users
 * recompute normals on the host.  Here the normal of a vertex is the normalised gradient of the density volume the vertex was cut
 * from, interpolated along the vertex's lattice edge.
 *
 * Field, lattice, edges, vertex order and t are those of pvd_hip_mesh.h: u [R,R,R] f32, x-major; vertex v sits on the edge A -> B,
 * A = the owner p, B = p + d (d = the edge slot's direction), at t = (thresh - u_A) / (u_B - u_A).
 *
 * All arithmetic is f32 and every operation below is rounded on its own (no fused multiply-add).
 * Lattice gradient at a lattice point q, per axis a, with c = q's index along a and e_a the unit step along a:
 *          0 < c < R-1:   d_a(q) = (u[q + e_a] - u[q - e_a]) * 0.5f
 *          c == 0:        d_a(q) = u[q + e_a] - u[q]
 *          c == R-1:      d_a(q) = u[q] - u[q - e_a]              (R == 2: only the two one-sided forms exist)
 * World gradient  g_a(q) = d_a(q) * inv_h_a,  inv_h_a = (float)(R - 1) / (bmax_a - bmin_a)  (one rounded difference, one division):
 *          a non-cubic box tilts the normal.
 * At the vertex   G_a = g_a(A) + t * (g_a(B) - g_a(A))               (difference, product, sum)
 *                 len = sqrtf(G_x * G_x + G_y * G_y + G_z * G_z)     (three products, summed left to right, one square root)
 *                 n_a = (-G_a) / len                                 (outwards: inside is u > thresh, so u falls along n)
 *          n = (0, 0, 0) when len is 0 or not finite; a NaN anywhere in the two stencils or in t lands there too.
 */
#ifndef PVD_HIP_MESH_ATTR_H
#define PVD_HIP_MESH_ATTR_H

#include "pvd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* normals [V,3] f32: row v is the normal of vertex v of pvd_mesh_emit, for the SAME field, R, thresh and the workspace as
 * pvd_mesh_count left it (same order: ascending (owner's linear index, edge slot)); V is the total it wrote (rows past V are never
 * written).  bmin3 / bmax3: device f32 [3].  One launch, one lane per lattice point, nothing atomic: two runs give the same bits.
 * V == 0: PVD_OK with no launch (normals may be NULL).  NULL pointer, unaligned or short workspace (pvd_mesh_workspace_bytes(R)):
 * PVD_ERR_INVALID; R outside 2 .. PVD_MESH_MAX_R (pvd_hip_mesh.h): PVD_ERR_UNSUPPORTED; both before any device call. */
int pvd_mesh_normals(const float *field, uint32_t R, float thresh, const float *bmin3, const float *bmax3, const void *workspace,
                     size_t workspace_bytes, float *normals, uint32_t V, pvd_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* PVD_HIP_MESH_ATTR_H */
