/*
 * pvd_hip_mesh_tsdf.h -- depth-map fusion: many depth (and colour) images with their cameras are integrated into a truncated signed
 * distance volume on an R^3 lattice (Curless and Levoy), whose zero level is the surface the images saw, in libpvd_hip.so next to the
 * mesher of include/pvd_hip_mesh.h: the primitive under pvd/mesh.py: tsdf_volume, tsdf_integrate, tsdf_field, tsdf_vertex_colors and
 * extract_surface_tsdf.  Same conventions as pvd_hip.h (device pointers, caller-allocated buffers, the stream as void*, PVD_OK or a
 * negative pvd_status).  pvd_abi_version() is not changed by this addition.
 * (This header lives next to csrc/mesh_tsdf.hip and not in include/: tests/test_abi_mesh_tex.py pins the list of files there.)
 *
 * EVERY FLOAT OPERATION BELOW IS ONE IEEE float32 OPERATION, IN THE ORDER WRITTEN, AND NOTHING IS FUSED.  Divisions and square roots
 * are the correctly rounded ones.
 *
 * Lattice  the voxel n = (i * R + j) * R + k (x-major, z fastest) sits at the float32 triple p = (c_x(i), c_y(j), c_z(k)) of
 *          include/pvd_hip_mesh_winding.h ("Lattice") over the box bmin .. bmax:
 *              c_a(n) = (float)n / (float)(R - 1) * (hi_a - lo_a) + lo_a
 *          -- the lattice of pvd/mesh.py: density_field and of pvd_mesh_emit, so a field made here is meshed where it was sampled.
 *
 * Camera   poses [V,4,4] f32, row-major cam2world M in the convention of pvd/scene.py: get_rays: the camera looks along its +z, a
 *          pixel's ray is M[:3,:3] applied to ((i + 0.5 - cx) / fx, (j + 0.5 - cy) / fy, 1), and o = (M[0][3], M[1][3], M[2][3]).
 *          intrinsics [V,4] f32 = (fx, fy, cx, cy).  The fourth row of M is not read.
 *
 * Images   depth [V,H,W] f32: the DISTANCE ALONG THE UNIT RAY, in world units, of pixel (i, j) at depth[v][j][i] (i along W).
 *          +inf: the ray left the scene -- free space all the way.  NaN or <= 0: no observation.
 *          color [V,H,W,3] f32 (optional) and weight [V,H,W] f32 (optional; without it w = 1).
 *
 * Integrate   per voxel p, for v = 0 .. V - 1 in ascending order:
 *              d   = p - o                                                          (per component)
 *              q_a = (M[0][a] * d_x + M[1][a] * d_y) + M[2][a] * d_z                (a = x, y, z: the columns 0, 1, 2 of M)
 *              q_z > 0, or the view is skipped                                      (a NaN skips)
 *              x = (fx * q_x) / q_z + cx,      y = (fy * q_y) / q_z + cy
 *              0 <= x < W and 0 <= y < H, or the view is skipped                    (W, H as float32; a NaN or an infinity skips)
 *              i = (int)floorf(x),  j = (int)floorf(y)                              (the NEAREST pixel: centres are at + 0.5)
 *              D = depth[v][j][i];  D > 0, or the view is skipped                   (a NaN skips; +inf stays)
 *              r = sqrtf((d_x * d_x + d_y * d_y) + d_z * d_z)
 *              s = D - r
 *              s >= -tau, or the view is skipped                                    (s == -tau is kept; a NaN skips)
 *              t = fminf(s / tau, 1)
 *              w = weight[v][j][i], or 1;  0 < w < +inf, or the view is skipped     (a NaN skips)
 *              acc_d = acc_d + w * t
 *              acc_w = acc_w + w
 *              acc_c[c] = acc_c[c] + w * color[v][j][i][c]                          (c = 0, 1, 2; only with color and acc_c)
 *          (the product, then the sum).  The three accumulators are read once before the first view and written once after the last:
 *          a call of V views leaves the bits that V calls of one view leave, in that order -- views can arrive in batches.
 *          Depth is not interpolated, so no depth is invented across a silhouette.  What a view says about a voxel: t = 1 in front
 *          of the surface it saw by tau or more, a ramp through 0 at the surface, nothing from tau behind it.
 *
 * Finalize    per voxel:   acc_w >= min_weight:  field = fmaxf(fminf(acc_d / acc_w, 1), -1)       (OBSERVED)
 *                          otherwise:            field = unknown                                  (UNKNOWN; a NaN acc_w is unknown)
 *          The field is in [-1, 1] and POSITIVE OUTSIDE.  unknown = -1 treats unseen space as solid: the interior behind the
 *          truncation band is never observed, so a watertight result needs it, and it also fills whatever no camera covers.
 *          unknown = +1 treats unseen space as empty: nothing is invented where no camera looked, and every surface gets an inner
 *          shell tau behind it, where the band ends.  pvd_mesh_count / pvd_mesh_emit mesh field > thresh as inside, so the caller hands
 *          them -field at the level 0 (pvd/mesh.py: extract_surface_tsdf keeps that sign convention in one place).  The second total
 *          counts field <= 0; the mesher's inside is -field > 0, so a voxel whose field is exactly 0 is counted here and lies ON the
 *          meshed surface, on its outer side.
 *
 * Sample colour   at a point P: not finite, or outside the box: 0.  Per axis, with r1 = (float)(R - 1):
 *              u_a = (P_a - lo_a) / (hi_a - lo_a) * r1;     0 <= u_a <= r1, or the point is outside          (a NaN is outside)
 *              i_a = min((int)floorf(u_a), R - 2);          f_a = u_a - (float)i_a;      g_a = 1 - f_a
 *          The corner (a, b, c) in {0, 1}^3 is the voxel (i_x + a, i_y + b, i_z + c) with the weight
 *              m_abc = (h_x * h_y) * h_z,       h = g for the offset 0, f for the offset 1.
 *          Over the OBSERVED corners (acc_w >= min_weight), in the order of the code 4 a + 2 b + c, from +0:
 *              M = M + m_abc;        C_c = C_c + m_abc * (acc_c[c] / acc_w)
 *              M > 0:  colors[c] = fminf(fmaxf(C_c / M, 0), 1);        otherwise (no observed corner carries weight): 0.
 */
#ifndef PVD_HIP_MESH_TSDF_H
#define PVD_HIP_MESH_TSDF_H

#include "../../include/pvd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Points per lattice axis: 2 .. PVD_MESH_TSDF_MAX_R (R^3 <= 2^30 voxels: a voxel index fits 32 bits).  Image sides: 1 ..
 * PVD_MESH_TSDF_MAX_SIDE (a side is exact as a float32). */
#define PVD_MESH_TSDF_MAX_R 1024
#define PVD_MESH_TSDF_MAX_SIDE 16384

/* acc_d [R,R,R] f32 (sum of w t), acc_w [R,R,R] f32 (sum of w) and acc_c [R,R,R,3] f32 (sum of w rgb; NULL: no colour) += the V
 * views depth [V,H,W] f32, color [V,H,W,3] f32 (NULL: no colour), weight [V,H,W] f32 (NULL: w = 1), poses [V,4,4] f32, intrinsics
 * [V,4] f32 over the lattice of the box bmin3 .. bmax3 (device f32 [3] each), as "Integrate" defines.  The caller zeroes the
 * accumulators before the first call.  acc_c is only touched when color and acc_c are both given.
 * One launch: ONE LANE PER VOXEL, z fastest, so the accumulators move as coalesced loads and stores and neighbouring lanes gather
 * neighbouring pixels; the lane walks the V views; the twelve numbers of a camera that are read and its four intrinsics -- sixteen per view -- are wave-uniform loads (the
 * views are not staged in LDS and not chunked); no LDS, no atomics.  R outside 2 .. PVD_MESH_TSDF_MAX_R, H or W outside 1 ..
 * PVD_MESH_TSDF_MAX_SIDE: PVD_ERR_UNSUPPORTED; then tau <= 0 or not finite: PVD_ERR_INVALID; then V == 0: PVD_OK with no launch
 * (every pointer may be NULL); then NULL depth, poses, intrinsics, bmin3, bmax3, acc_d or acc_w: PVD_ERR_INVALID.  All before any
 * device call. */
int pvd_mesh_tsdf_integrate(const float *depth, const float *color, const float *weight, const float *poses, const float *intrinsics,
                            uint32_t V, uint32_t H, uint32_t W, uint32_t R, const float *bmin3, const float *bmax3, float tau,
                            float *acc_d, float *acc_w, float *acc_c, pvd_stream_t stream);

/* field [R,R,R] f32 <- "Finalize" of acc_d, acc_w; totals [3] i64 on the device <- (observed voxels, observed voxels with field <= 0,
 * unknown voxels).  One memset and one launch, a grid-stride walk with one lane per voxel; the totals by one integer atomic per wave
 * and total.  R outside 2 .. PVD_MESH_TSDF_MAX_R: PVD_ERR_UNSUPPORTED; then min_weight <= 0 or not finite, or unknown not finite:
 * PVD_ERR_INVALID; then NULL acc_d, acc_w, field or totals: PVD_ERR_INVALID.  All before any device call. */
int pvd_mesh_tsdf_finalize(const float *acc_d, const float *acc_w, uint32_t R, float min_weight, float unknown, float *field,
                           int64_t *totals, pvd_stream_t stream);

/* colors [N,3] f32 <- "Sample colour" of acc_c, acc_w at points [N,3] f32.  One launch, one lane per point, eight gathers of 4 + 12
 * bytes; no LDS, no atomics; rows past N are never written.  R outside 2 .. PVD_MESH_TSDF_MAX_R: PVD_ERR_UNSUPPORTED; then min_weight
 * <= 0 or not finite: PVD_ERR_INVALID; then N == 0: PVD_OK with no launch (every pointer may be NULL); then NULL acc_c, acc_w, bmin3,
 * bmax3, points or colors: PVD_ERR_INVALID.  All before any device call. */
int pvd_mesh_tsdf_sample_color(const float *acc_c, const float *acc_w, uint32_t R, const float *bmin3, const float *bmax3,
                               float min_weight, const float *points, uint32_t N, float *colors, pvd_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* PVD_HIP_MESH_TSDF_H */
