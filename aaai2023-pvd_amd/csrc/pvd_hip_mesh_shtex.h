/*
 * pvd_hip_mesh_shtex.h -- a VIEW-DEPENDENT texture atlas: a small spherical-harmonics expansion of the outgoing colour per texel in
 * place of one colour, in libpvd_hip.so next to the atlas of include/pvd_hip_mesh_tex.h, whose layout, ownership rule, addressing and
 * no-gutter argument it uses unchanged -- only the payload of a texel grows, from 3 floats to K x 3 (pvd/mesh.py: sh_basis,
 * sh_fit_matrix, bake_sh_texture, sample_sh_texture, render_mesh with a 4-D texture).  Same conventions as pvd_hip.h (device pointers,
 * caller-allocated buffers, the stream as void*, PVD_OK or a negative pvd_status).  pvd_abi_version() is not changed by this addition.
 * (This header lives next to csrc/mesh_shtex.hip and not in include/: tests/test_abi_mesh_tex.py pins the list of files there.)
 *
 * EVERY FLOAT OPERATION BELOW IS ONE IEEE float32 OPERATION, IN THE ORDER WRITTEN, AND NOTHING IS FUSED.  Every constant is the float32
 * its literal names.
 *
 * Bands    L in 1 .. PVD_MESH_SHTEX_MAX_L and K = L * L (1, 4, 9, 16) coefficients per channel; the index is l * l + l + m, as in
 *          csrc/sh_basis.inc, with its signs.
 *
 * Basis    Y_0 .. Y_{K-1} of a direction (x, y, z), USED AS GIVEN AND NOT NORMALISED (the caller's rays are unit).  With
 *              xx = x * x,  yy = y * y,  zz = z * z,  xy = x * y,  yz = y * z,  xz = x * z:
 *              Y_0  =  0.282094806f
 *              Y_1  = -0.488602519f * y
 *              Y_2  =  0.488602519f * z
 *              Y_3  = -0.488602519f * x
 *              Y_4  =  1.09254849f * xy
 *              Y_5  = -1.09254849f * yz
 *              Y_6  =  0.946174681f * zz - 0.31539157f
 *              Y_7  = -1.09254849f * xz
 *              Y_8  =  0.546274245f * (xx - yy)
 *              Y_9  = -0.590043604f * (y * (3.0f * xx - yy))
 *              Y_10 =  2.89061141f * (xy * z)
 *              Y_11 =  (0.457045794f - 2.28522897f * zz) * y
 *              Y_12 =  (1.86588168f * zz - 1.11952901f) * z
 *              Y_13 =  (0.457045794f - 2.28522897f * zz) * x
 *              Y_14 =  1.44530571f * (z * (xx - yy))
 *              Y_15 = -0.590043604f * (x * (xx - 3.0f * yy))
 *          Each is the real polynomial of csrc/sh_basis.inc written as at most two monomials; where there are two they have one sign
 *          before the subtraction (squares), so the difference is no larger than the larger of them.  Counting one half ulp for every
 *          product, difference and literal on the way of a monomial, the worst (Y_9, Y_15) stays within 7 * 2^-24 of the larger
 *          monomial: tests/test_mesh_shtex_restatement.py pins 8 ulps against float64.  (pvd_sh_basis of sh_basis.inc fuses its products
 *          and is not this basis bit for bit.)
 *
 * Atlas    texture [Ht, Wt, K, 3] f32 with (Ht, Wt) of pvd_mesh_tex_layout(T, S): the K x 3 floats of a texel are contiguous, coef[k][c]
 *          at 3 k + c.
 *
 * Sample   at (tri, bary, dir).  tri < 0 or tri >= T: the background colour; nothing is read and nothing is clamped.  Otherwise i0, j0,
 *          tx, ty and the four texel addresses are EXACTLY those of include/pvd_hip_mesh_tex.h ("Sample"), and with Y = the basis of dir,
 *          for each of the four texels PQ and each channel
 *              c_PQ = (...((coef[0] * Y_0) + coef[1] * Y_1) + ...) + coef[K-1] * Y_{K-1}                (k ascending)
 *              c    = (c00 * (1 - tx) + c10 * tx) * (1 - ty) + (c01 * (1 - tx) + c11 * tx) * ty         (that header's expression)
 *              out  = fminf(fmaxf(c, 0), 1)                                                             (a NaN becomes 0)
 *          The reads stay inside the hit triangle's own cell, as there, whatever bary and dir hold.  At L = 1 this is that header's
 *          sample of the texture coef[0] * Y_0, clamped.
 *
 * Query directions for the bake   given a texel's normal n as pvd_mesh_tex_points returns it (unnormalised, possibly NaN) and a fitting
 *          direction u -- a direction of travel, as the model's d argument: a ray that SEES the surface has d . n < 0:
 *              s = (ux * nx + uy * ny) + uz * nz,      q = (nx * nx + ny * ny) + nz * nz
 *              s > 0 and q finite and q > 0:   r = (2 * s) / q   and   d = u - r * n  per component (the product, then the difference)
 *              otherwise (s NaN included):     d = u.
 *          A direction that would look at the surface from behind is mirrored in the tangent plane, so no colour is ever taken from
 *          behind the surface, the fitted function is even across the tangent plane, and ONE fixed full-sphere set u_0 .. u_{D-1}
 *          serves every texel.
 *
 * Projection   coef[t][k][c] is built from acc = +0; for j = 0 .. D - 1 in order: acc = acc + P[k][j] * rgb[j][t][c] (the product,
 *          then the sum).  P [K,D] is the fit matrix of the set (pvd/mesh.py: sh_fit_matrix, the pseudo-inverse of the basis at the
 *          u_j).  The D directions may run in several batches: the accumulators are stored to coef and reloaded, which changes no bit.
 */
#ifndef PVD_HIP_MESH_SHTEX_H
#define PVD_HIP_MESH_SHTEX_H

#include "../../include/pvd_hip_mesh_tex.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The largest number of bands: K = L * L <= 16 coefficients per channel. */
#define PVD_MESH_SHTEX_MAX_L 4

/* out [N,K] f32 <- the basis defined above of dirs [N,3] f32.  One launch, one lane per direction; no LDS, no atomics; rows past N are
 * never written.  L outside 1 .. PVD_MESH_SHTEX_MAX_L: PVD_ERR_UNSUPPORTED; then N == 0: PVD_OK with no launch (every pointer may be
 * NULL); then NULL dirs or out: PVD_ERR_INVALID.  All before any device call. */
int pvd_mesh_shtex_basis(const float *dirs, uint32_t N, uint32_t L, float *out, pvd_stream_t stream);

/* d [J,M,3] f32 <- the query directions defined above of the normals n [M,3] f32 and the fitting directions U [J,3] f32.  One launch,
 * one lane per normal (consecutive lanes along M), which runs through the J directions; no LDS, no atomics.  M == 0 or J == 0: PVD_OK
 * with no launch (every pointer may be NULL); then NULL n, U or d: PVD_ERR_INVALID.  All before any device call. */
int pvd_mesh_shtex_dirs(const float *n, uint32_t M, const float *U, uint32_t J, float *d, pvd_stream_t stream);

/* coef [M,K,3] f32 <- the projection defined above over the J directions of a batch: rgb [J,M,3] f32 and Pcols [K,J] f32, the batch's
 * columns of P.  first != 0 starts from +0 (coef is not read); first == 0 starts from coef.  One launch, one lane per texel, the K x 3
 * accumulators in registers through the J directions, rgb read along M; no LDS, no atomics; nothing outside coef's M rows is written.
 * L outside 1 .. PVD_MESH_SHTEX_MAX_L: PVD_ERR_UNSUPPORTED; then M == 0 or J == 0: PVD_OK with no launch (every pointer may be NULL, and
 * coef is left as it is, also where first != 0); then NULL rgb, Pcols or coef: PVD_ERR_INVALID.  All before any device call. */
int pvd_mesh_shtex_project(const float *rgb, const float *Pcols, uint32_t L, uint32_t J, uint32_t M, float *coef, uint32_t first,
                           pvd_stream_t stream);

/* color [N,3] f32 <- the sample defined above of texture [Ht, Wt, K, 3] f32 (the atlas of T triangles at the cell edge S, K = L * L) at
 * tri [N] i32, bary [N,2] f32, dirs [N,3] f32; bg3: device f32 [3].  One launch, one lane per ray, four gathers of K * 12 contiguous
 * bytes per hit; no LDS, no atomics; rows past N are never written.  The layout's errors (pvd_mesh_tex_layout) and L outside
 * 1 .. PVD_MESH_SHTEX_MAX_L: PVD_ERR_UNSUPPORTED; then N == 0: PVD_OK with no launch (every pointer may be NULL); then NULL texture, tri,
 * bary, dirs, bg3 or color: PVD_ERR_INVALID.  All before any device call. */
int pvd_mesh_shtex_sample(const float *texture, uint32_t T, uint32_t S, uint32_t L, const int32_t *tri, const float *bary,
                          const float *dirs, uint32_t N, const float *bg3, float *color, pvd_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* PVD_HIP_MESH_SHTEX_H */
