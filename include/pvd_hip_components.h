/*
 * pvd_hip_components.h -- the connected components of the inside set of a density volume, in libpvd_hip.so next to the entry points
 * pvd_hip.h and pvd_hip_mesh.h declare: label them, measure them, and push the small ones ("floaters") out of the level set before
 * pvd_mesh_count / pvd_mesh_emit mesh it.  Same conventions as pvd_hip_mesh.h (device pointers, caller-allocated buffers, the stream
 * as void* and last, PVD_OK or a negative pvd_status, no allocation, no synchronisation).  pvd_abi_version() is not changed by these
 * additions.
 *
 * reference: distill_mutual/network.py:601 ("lots of noisy outliers in hashnerf") and extract_fields / extract_geometry,
 * distill_mutual/utils.py:442-488, whose mesh carries every such outlier as a small closed shell.
 *
 * Field    u [R,R,R] f32, x-major: u[(i * R + j) * R + k], 2 <= R <= PVD_MESH_MAX_R.  A lattice point is INSIDE iff u > thresh (NaN
 *          and u == thresh: outside) -- the mesher's rule.
 * Connectivity.  The mesher cuts every cell into the six Kuhn tetrahedra, so two inside points belong to one solid exactly when a
 *          chain of Kuhn edges over inside points joins them: the neighbours of p are the 14 points p + d and p - d, d one of the
 *          seven owned-edge directions of pvd_hip_mesh.h, (1,0,0), (0,1,0), (0,0,1), (1,1,0), (1,0,1), (0,1,1), (1,1,1).  Neither 6-
 *          nor 26-connectivity: (0,0,0) and (1,1,1) are neighbours, (0,1,0) and (1,0,0) are not.
 * Labels   the label of a component is the smallest linear index of its points, so labels, sizes and statistics are functions of
 *          the field alone (no run-to-run freedom), all in integers.
 * Filter   a dropped component's points are set to thresh, i.e. moved outside.  Such a component touches, through Kuhn edges, only
 *          outside points and its own, so the mesh of the filtered field is the mesh of the field without the shells of the dropped
 *          components; every surviving vertex keeps its bits.
 */
#ifndef PVD_HIP_COMPONENTS_H
#define PVD_HIP_COMPONENTS_H

#include "pvd_hip_mesh.h"

#ifdef __cplusplus
extern "C" {
#endif

/* labels[p] = smallest linear index of any point of p's component (14-neighbour Kuhn connectivity), -1 for an outside point.
 * sizes[q]  = number of points of the component whose label is q, at q itself; 0 everywhere else.   Both [R^3]; every element of
 * both is written.
 * stats_dev uint32[4], 8-byte aligned, written by the call: {components, inside points, size of the largest component, its label}
 * (largest: greatest size, ties to the smaller label; {0,0,0,0} for an empty inside set).
 * Five launches (init, merge, flatten + count, largest, its unpacking); no workgroup waits on another.  NULL pointer or a stats_dev
 * that is not 8-byte aligned: PVD_ERR_INVALID; R outside 2 .. PVD_MESH_MAX_R: PVD_ERR_UNSUPPORTED; both before any device call. */
int pvd_components_label(const float *field, uint32_t R, float thresh, int32_t *labels, uint32_t *sizes, uint32_t *stats_dev,
                         pvd_stream_t stream);

/* out[p] = field[p], except thresh where p is inside and its component is dropped.  Dropped: size < min_points, or
 * (largest_only != 0 and label != stats_dev[3]).  out may be the same pointer as field (in place).
 * labels, sizes, stats_dev: as pvd_components_label left them for the SAME field, R and thresh.
 * kept_dev uint32[2], written by the call: {components kept, points kept}.
 * NULL pointer: PVD_ERR_INVALID; R outside 2 .. PVD_MESH_MAX_R: PVD_ERR_UNSUPPORTED; both before any device call. */
int pvd_components_filter(const float *field, const int32_t *labels, const uint32_t *sizes, const uint32_t *stats_dev, uint32_t R,
                          float thresh, uint32_t min_points, uint32_t largest_only, float *out, uint32_t *kept_dev, pvd_stream_t stream);

/* the 14 offsets, for callers and tests: writes 14 * 3 int32 (the seven directions above in that order, then their negatives in
 * the same order), returns 14; NULL: PVD_ERR_INVALID.  A host call. */
int pvd_components_neighbours(int32_t *offsets_host);

#ifdef __cplusplus
}
#endif

#endif /* PVD_HIP_COMPONENTS_H */
