/*
 * pvd_hip_mesh_project.h -- colour for surface points from posed images: every view is projected onto the points, views that look at
 * a point from behind, at a grazing angle, from outside their frame or through other geometry are discarded, and the rest are
 * blended (or the best one is taken), in libpvd_hip.so next to the first-hit cast of include/pvd_hip_mesh_ray.h, whose workspace, grid
 * and hit() it uses (pvd/mesh.py: project_views, view_source, view_vertex_colors).  Same conventions as pvd_hip.h (device pointers,
 * caller-allocated buffers, the stream as void*, PVD_OK or a negative pvd_status).  pvd_abi_version() is not changed by this addition.
 * (This header lives next to csrc/mesh_project.hip and not in include/: tests/test_abi_mesh_tex.py pins the list of files there.)
 *
 * EVERY FLOAT OPERATION BELOW IS ONE IEEE float32 OPERATION, IN THE ORDER WRITTEN, AND NOTHING IS FUSED.  Divisions and square roots
 * are the correctly rounded ones.  The occlusion test alone is in float64, and it is hit() of include/pvd_hip_mesh_ray.h.
 *
 * Inputs   points [N,3] f32 and normals [N,3] f32 (normals need not be unit length); color [V,H,W,3] f32; weight [V,H,W] f32 or NULL;
 *          poses [V,4,4] f32 and intrinsics [V,4] f32 exactly as under "Camera" in pvd_hip_mesh_tsdf.h (row-major cam2world M, the
 *          camera looks along its +z, o = (M[0][3], M[1][3], M[2][3]), intrinsics = (fx, fy, cx, cy); pixel (i, j) is at
 *          color[v][j][i], i along W, and its centre projects to x = i + 0.5, y = j + 0.5).  The mesh is whatever pvd_mesh_ray_build
 *          left in the workspace for the same T, G and pairs.  acc_c [N,3] f32 and acc_w [N] f32: the caller zeroes them.
 *
 * Point    L = sqrtf((n_x * n_x + n_y * n_y) + n_z * n_z)
 *          A point takes no part if any of its six numbers is not finite, or if L is not both > 0 and finite: its accumulators stay
 *          untouched.  Otherwise u = n / L (per component).
 *
 * Per view, v = 0 .. V - 1 in ascending order; a view is skipped as soon as one of these steps fails, and EVERY NaN SKIPS:
 *     1. Distance      e = o - p                                                   (per component)
 *                      r = sqrtf((e_x * e_x + e_y * e_y) + e_z * e_z);    r > 0, or the view is skipped
 *     2. Facing        c = ((u_x * e_x + u_y * e_y) + u_z * e_z) / r
 *                      sides = both:   s = -1 if c < 0 and s = 1 otherwise, then c = |c|;      sides = front:   s = 1
 *                      c > cos_min, or the view is skipped
 *     3. Projection    d = p - o, then q, x, y exactly as "Integrate" of pvd_hip_mesh_tsdf.h:
 *                      q_a = (M[0][a] * d_x + M[1][a] * d_y) + M[2][a] * d_z
 *                      q_z > 0, or the view is skipped
 *                      x = (fx * q_x) / q_z + cx,      y = (fy * q_y) / q_z + cy
 *     4. In frame      0.5 <= x <= W - 0.5 and 0.5 <= y <= H - 0.5, or the view is skipped      (W, H as float32; between the centres
 *                      of the outermost pixels: nothing is extrapolated)
 *     5. Texel         a = x - 0.5;   i = min((int)floorf(a), W - 2);   f = a - (float)i
 *                      b = y - 0.5;   j = min((int)floorf(b), H - 2);   g = b - (float)j
 *     6. Bilinear colour
 *                      m00 = (1 - f) * (1 - g),   m10 = f * (1 - g),   m01 = (1 - f) * g,   m11 = f * g
 *                      C_ch = ((m00 * I00 + m10 * I10) + m01 * I01) + m11 * I11,      I_ab = color[v][j + b][i + a][ch]
 *                      all twelve values I must be finite, or the view is skipped
 *                      with weight:  wp = ((m00 * w00 + m10 * w10) + m01 * w01) + m11 * w11,   w_ab = weight[v][j + b][i + a];
 *                      0 < wp < +inf, or the view is skipped
 *     7. View weight   w = 1;   w = w * c, `power` times (power 0 .. 8);   with weight: w = w * wp
 *     8. Occlusion     last, because it is the expensive step.  The ray starts at
 *                          o'_a = p_a + (s * bias) * u_a                           (float32: the product s * bias, the product, the sum)
 *                      and has, in float64, the origin o' and the direction D_a = (double)o_a - (double)o'_a: t = 1 is the camera.
 *                      The view is BLOCKED, and skipped, iff some valid triangle has hit(ray, triangle) with 0 <= t < 1 on the float64
 *                      t; hit is exactly steps 1 .. 8 of include/pvd_hip_mesh_ray.h (unfused float64, both faces count).  A triangle
 *                      beyond the camera (t >= 1) does not block; one nearer to p than bias along the offset lies behind o' and does
 *                      not block either.  A ray whose six numbers are not all finite, or whose D is (0, 0, 0), is blocked by nothing.
 *     9. Accumulate    mode = blend:   acc_w = acc_w + w;   acc_c[ch] = acc_c[ch] + w * C_ch          (the product, then the sum)
 *                      mode = best:    if w > acc_w:  acc_w = w and acc_c = C        (ties keep the earlier view)
 *          The accumulators are read once before view 0 and written once after view V - 1: V views in one call leave the same bits as
 *          V calls of one view, in that order -- views can arrive in batches.  A point no view of the call reached is not written.
 *
 * Independence   Blocked is an OR over triangles of a fixed function of (ray, triangle), so the accumulators depend on neither G, the
 *          box, the order of the triangles inside a cell nor the run -- WITH THE ONE EXCEPTION include/pvd_hip_mesh_ray.h names under
 *          "THE POINT OF THE TRIANGLE", as under "Independence" in pvd_hip_mesh_expose.h: a triangle that the ray sees edge-on, within
 *          rounding of its plane, may report a hit whose point lies outside its own range of cells; the walk then need not test it,
 *          and G = 1, which tests everything, may call a view blocked that a finer grid lets through.  For every other (ray, triangle)
 *          pair the promise holds without condition.
 *
 * Finalize    per point:   acc_w >= min_weight (SEEN):   seen = 1 and
 *                              mode = blend:   colors[ch] = fminf(fmaxf(acc_c[ch] / acc_w, 0), 1)
 *                              mode = best:    colors[ch] = fminf(fmaxf(acc_c[ch], 0), 1)
 *                          otherwise (a NaN acc_w too):  seen = 0, and colors is LEFT AS THE CALLER FILLED IT -- the fallback.
 *          totals [2] i64 = (seen points, unseen points).
 *
 * Kernel   integrate: ONE LANE PER POINT, consecutive lanes take consecutive points -- the texels of an atlas row are neighbours on
 *          the surface, so a wave sends near-parallel rays through the same cells and gathers neighbouring pixels.  The lane keeps its
 *          point, unit normal and four accumulators in registers through the views of the call; v is uniform, so the sixteen numbers
 *          of a view's camera are wave-uniform loads.  The occlusion walk is mray::walk of csrc/mesh_ray_walk.h with an any-hit
 *          visitor, as in csrc/mesh_expose.hip; lanes whose view was skipped idle while their neighbours walk.  No LDS, no atomics.
 *          finalize: one memset and one launch, a grid-stride walk with one lane per point; the two totals by one integer atomic per
 *          wave and total.
 */
#ifndef PVD_HIP_MESH_PROJECT_H
#define PVD_HIP_MESH_PROJECT_H

#include "../../include/pvd_hip_mesh_ray.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Image sides: 2 .. PVD_MESH_PROJECT_MAX_SIDE (a side is exact as a float32; two pixels make one bilinear cell).  The exponent of the
 * facing cosine: 0 .. PVD_MESH_PROJECT_MAX_POWER. */
#define PVD_MESH_PROJECT_MAX_SIDE 16384
#define PVD_MESH_PROJECT_MAX_POWER 8
#define PVD_MESH_PROJECT_SIDES_FRONT 0
#define PVD_MESH_PROJECT_SIDES_BOTH 1
#define PVD_MESH_PROJECT_MODE_BLEND 0
#define PVD_MESH_PROJECT_MODE_BEST 1

/* acc_c [N,3] f32 and acc_w [N] f32 <- steps 1 .. 9 above for the points, the V views and the mesh pvd_mesh_ray_build left in the
 * workspace for the SAME T, G and pairs (the mesh and the box are read from the workspace only).  One launch, no memset.
 * W or H outside 2 .. PVD_MESH_PROJECT_MAX_SIDE, power above PVD_MESH_PROJECT_MAX_POWER, or an unknown sides or mode:
 * PVD_ERR_UNSUPPORTED; then cos_min outside [0, 1) or NaN: PVD_ERR_INVALID; then bias negative or not finite: PVD_ERR_INVALID; then the
 * workspace checks of pvd_mesh_ray_build (NULL, unaligned or short: PVD_ERR_INVALID; G, T or pairs out of range: PVD_ERR_UNSUPPORTED);
 * then N == 0 or V == 0: PVD_OK with no launch (every other pointer may be NULL); then NULL points, normals, color, poses, intrinsics,
 * acc_c or acc_w: PVD_ERR_INVALID (weight may be NULL: no weight image).  All before any device call. */
int pvd_mesh_project_integrate(const float *points, const float *normals, uint32_t N, const float *color, const float *weight,
                               const float *poses, const float *intrinsics, uint32_t V, uint32_t H, uint32_t W, uint32_t T, uint32_t G,
                               uint64_t pairs, const void *workspace, size_t workspace_bytes, float cos_min, uint32_t power, float bias,
                               uint32_t sides, uint32_t mode, float *acc_c, float *acc_w, pvd_stream_t stream);

/* colors [N,3] f32, seen [N] u8 and totals [2] i64 on the device <- "Finalize" of acc_c [N,3], acc_w [N].  An unknown mode:
 * PVD_ERR_UNSUPPORTED; then min_weight not positive or not finite: PVD_ERR_INVALID; then N == 0: PVD_OK with no device call (every
 * pointer may be NULL; totals is not written); then NULL acc_c, acc_w, colors, seen or totals: PVD_ERR_INVALID.  All before any device
 * call. */
int pvd_mesh_project_finalize(const float *acc_c, const float *acc_w, uint32_t N, float min_weight, uint32_t mode, float *colors,
                              uint8_t *seen, int64_t *totals, pvd_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* PVD_HIP_MESH_PROJECT_H */
