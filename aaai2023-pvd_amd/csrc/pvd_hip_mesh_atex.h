/*
 * pvd_hip_mesh_atex.h -- an AREA-ADAPTIVE texture atlas for a triangle mesh: the per-triangle atlas of include/pvd_hip_mesh_tex.h with a
 * cell edge chosen PER TRIANGLE from the texel density the caller asks for, in libpvd_hip.so next to it (pvd/mesh.py: adaptive_atlas, and
 * texture_layout, texture_uv, texture_points, bake_texture, sample_texture, render_mesh with that atlas in place of the integer S).  The
 * uniform atlas is untouched and stays the default.  Same conventions as pvd_hip.h (device pointers, caller-allocated buffers, the stream
 * as void*, PVD_OK or a negative pvd_status).  pvd_abi_version() is not changed by this addition.
 * (This header lives next to csrc/mesh_atex.hip and not in include/: tests/test_abi_mesh_tex.py pins the list of files there.)
 *
 * EVERY FLOAT OPERATION BELOW IS ONE IEEE float32 OPERATION, IN THE ORDER WRITTEN, AND NOTHING IS FUSED.
 *
 * Classes  five cell edges S_c = 4, 8, 16, 32, 64 for c = 0 .. 4 (S_c = 4 << c); the step count is m_c = S_c - 3 = 1, 5, 13, 29, 61.
 *
 * Class of a triangle   from its float32 corners A, B, Cc, the caller's density > 0 (texels per unit length) and max_class in 0 .. 4:
 *              dAB = ((ux*ux + uy*uy) + uz*uz) with u = B - A;   dAC the same with u = Cc - A;   dBC the same with u = Cc - B;
 *              L2 = fmaxf(fmaxf(dAB, dAC), dBC)                                         (the longest edge, squared)
 *              q = L2 * rho2,   rho2 = density * density (float32, computed on the host and passed to the kernel)
 *          A density that is not > 0, or a rho2 that is not finite or not > 0 (it overflowed or underflowed): PVD_ERR_INVALID.
 *              c0 = the number of i in 0 .. 3 with q > (float)(m_i * m_i)               (the thresholds 1, 25, 169, 841)
 *              c = min(c0, max_class)
 *          A triangle is CAPPED when c0 > max_class or q > 3721 (= 61 * 61): it got fewer texels than the density asks for.
 *          An INVALID triangle -- the rule of pvd_hip_mesh_tex.h: an index outside [0, V) or a corner that is not finite -- has class 0
 *          and is not capped.  (Finite corners give no NaN here: a difference or a square that overflows is +inf, and is capped.)
 *          CONSEQUENCE: every valid, uncapped triangle has m_c >= density * (its longest edge); its texel spacing along AB and along AC
 *          is at most 1 / density.  (q <= m_c^2 in float32; the roundings of q are a few ulp, see tests/test_mesh_atex_restatement.py.)
 *
 * Rank     rank(f) = the number of triangles f' < f of the same class: a stable counting sort by class.  It comes from the integer
 *          reduce-then-scan of csrc/block_scan.h (per-workgroup sums, one scanning workgroup, per-item offsets), NOT FROM ATOMICS: the
 *          layout is the same bits from run to run.  With count_c the triangles of class c and base_c = sum of count_c' over c' < c:
 *              slot[f]  u32 = c << 28 | rank                    (T < 2^28)
 *              order[base_c + rank] u32 = f                     (a permutation of 0 .. T - 1 that inverts slot)
 *              totals[6] u32 = count_0 .. count_4, the number of capped triangles
 *
 * Layout   from the five counts, on the host (the caller reads the six totals back, as the count / emit pairs elsewhere do):
 *              cells_c = ceil(count_c / 2);   A = sum of cells_c * S_c * S_c;
 *              Wt = the smallest multiple of 64 with Wt * Wt >= A, and at least 64;
 *              class c is a horizontal band: C_c = Wt / S_c cells per row, rows_c = ceil(cells_c / C_c) (0 for an empty class), height
 *              rows_c * S_c; the bands are stacked in the order of c from y0_0 = 0:   y0_(c+1) = y0_c + rows_c * S_c;
 *              Ht = sum of rows_c * S_c.   T = 0 gives Wt = 64, Ht = 4, with nothing owned.
 *          Wt or Ht above PVD_MESH_ATEX_MAX_SIDE: PVD_ERR_UNSUPPORTED.  Every S_c divides 64, so C_c * S_c = Wt exactly.
 *
 * Inside a band   everything is the text of pvd_hip_mesh_tex.h with S = S_c, C = C_c, y - y0_c in place of y, and the RANK in place of
 *          f: texel (x, y) of band c lies in the cell k = ((y - y0_c) / S_c) * C_c + (x / S_c) at i = x % S_c, j = (y - y0_c) % S_c; the
 *          lower half (i + j <= S_c - 1) belongs to rank 2k with p = i, q = j, the upper half to rank 2k + 1 with p = S_c - 1 - i,
 *          q = S_c - 1 - j; ranks 2k and 2k + 1 share cell k.  A texel is OWNED iff its rank < count_c, by f = order[base_c + rank].
 *          A triangle owns S_c (S_c + 1) / 2 texels in a lower half and S_c (S_c - 1) / 2 in an upper half.  The weights
 *              beta = (float)p / (float)m_c,   gamma = (float)q / (float)m_c,   alpha = (1 - beta) - gamma,
 *          the point X = (alpha * A + beta * B) + gamma * Cc, the normal, and the six NaNs (0x7fc00000) for invalid and unowned texels
 *          are unchanged (with vertex normals a triangle whose three normals are not all finite is invalid for its texels, as there).
 *          Corner coordinates, with (cx, cy) = (k % C_c, k / C_c), k = rank / 2, S = S_c, m = m_c:
 *              lower: a = (cx S + 0.5,     y0_c + cy S + 0.5),       b = a + (m, 0),   c = a + (0, m);
 *              upper: a = (cx S + S - 0.5, y0_c + cy S + S - 0.5),   b = a - (m, 0),   c = a - (0, m);     uv = (X / Wt, 1 - Y / Ht).
 *          WHY NO GUTTER IS NEEDED holds per cell, unchanged: a bilinear lookup inside a triangle reads texels of its own half of its
 *          own cell.  THE ONE EXCEPTION, WITH WEIGHT ZERO, restated for ranks: at a point of the hypotenuse where fu and fv are both
 *          whole numbers the fourth texel lies on the cell's diagonal, which belongs to the even rank: a triangle of odd rank reads one
 *          texel of the triangle of rank - 1 of ITS CLASS (order[base_c + rank - 1], which exists), times tx = 0 and ty = 0.
 *
 * Sample   (tri, bary).  tri < 0 or tri >= T: the background colour, and nothing is read.  Otherwise ONE 4-byte gather s = slot[tri],
 *          c = s >> 28, rank = s & 0x0fffffff; a slot with c > 4 or rank >= count_c (no pvd_mesh_atex_build writes one) gives the
 *          background and reads nothing more.  Then the sample of pvd_hip_mesh_tex.h with S = S_c, C = C_c, m = m_c and the rank for tri:
 *              fu = fminf(fmaxf(beta * m, 0), m)  (a NaN becomes 0);   i0 = min((int)floorf(fu), m);   tx = fu - i0;   the same for fv, j0, ty;
 *              the four texels (i0 | i0 + 1, j0 | j0 + 1), mirrored for an odd rank, with y0_c added to the two rows;
 *              c = (c00 * (1 - tx) + c10 * tx) * (1 - ty) + (c01 * (1 - tx) + c11 * tx) * ty.
 *          Every read stays inside the triangle's own cell, whatever bary holds.
 *
 * Cost     one more DEPENDENT gather per hit than k_mt_sample (slot[tri] before the four texels); the points kernel reads order[] once
 *          per texel (lanes of a cell half share the word).  profiles/mesh_atex.txt has the kernel times next to the uniform kernels.
 */
#ifndef PVD_HIP_MESH_ATEX_H
#define PVD_HIP_MESH_ATEX_H

#include "../../include/pvd_hip_mesh_tex.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PVD_MESH_ATEX_CLASSES 5
#define PVD_MESH_ATEX_MAX_T 268435455 /* 2^28 - 1: the rank shares a word with the class */
#define PVD_MESH_ATEX_MAX_SIDE 16384
#define PVD_MESH_ATEX_TOTALS 6        /* count_0 .. count_4, capped */
#define PVD_MESH_ATEX_LAYOUT_WORDS 17 /* Wt, Ht, y0[5], rows[5], C[5] */

/* Bytes of workspace pvd_mesh_atex_build needs for T triangles (at least 16); 0 for T above PVD_MESH_ATEX_MAX_T.  Host only. */
size_t pvd_mesh_atex_workspace_bytes(uint32_t T);

/* slot [T] u32, order [T] u32 and totals_dev [6] u32 on the device <- "Class" and "Rank" above for the mesh (vertices [V,3] f32, triangles
 * [T,3] i32).  Three launches -- classify + six sums per workgroup (the five classes and the capped), the one-workgroup scan, the slots --
 * and no float or integer atomics.  T above PVD_MESH_ATEX_MAX_T or max_class above 4: PVD_ERR_UNSUPPORTED; then density not > 0, or
 * rho2 = density * density (float32) not finite or not > 0: PVD_ERR_INVALID; then NULL totals_dev: PVD_ERR_INVALID; then T == 0: totals_dev <- six zeros by one
 * memset, PVD_OK with no launch (every other pointer may be NULL); then NULL vertices (V not 0), triangles, slot or order, or a workspace
 * that is NULL, not 16-byte aligned or shorter than pvd_mesh_atex_workspace_bytes(T): PVD_ERR_INVALID.  All before any device call. */
int pvd_mesh_atex_build(const float *vertices, uint32_t V, const int32_t *triangles, uint32_t T, float density, uint32_t max_class,
                        void *workspace, size_t workspace_bytes, uint32_t *slot, uint32_t *order, uint32_t *totals_dev, pvd_stream_t stream);

/* out[PVD_MESH_ATEX_LAYOUT_WORDS] <- (Wt, Ht, y0_0 .. y0_4, rows_0 .. rows_4, C_0 .. C_4) of "Layout" above for the five counts.  Host
 * only: no device call.  NULL counts or out: PVD_ERR_INVALID; a sum of the counts above PVD_MESH_ATEX_MAX_T, or a side above
 * PVD_MESH_ATEX_MAX_SIDE: PVD_ERR_UNSUPPORTED (out is not written). */
int pvd_mesh_atex_layout(const uint32_t counts[5], uint32_t out[]);

/* x, n [(row1 - row0) * Wt, 3] f32 <- the point and the normal of every texel of the image rows row0 .. row1 - 1 of the adaptive atlas
 * (counts: HOST u32 [5], the first five totals; order [T] u32 on the device; normals [V,3] f32 or NULL: face normals).  One launch, one
 * lane per texel, consecutive lanes along x; the class of a row from y against at most five y0; no LDS, no atomics; nothing outside the
 * band is written; an order entry outside [0, T) makes its texels unowned.  NULL counts: PVD_ERR_INVALID; then the layout's errors; then
 * a sum of the counts that is not T: PVD_ERR_INVALID; then row0 > row1 or row1 > Ht: PVD_ERR_INVALID; then row0 == row1: PVD_OK with no
 * launch (every pointer may be NULL); then NULL vertices (T and V not 0), triangles or order (T not 0), x or n: PVD_ERR_INVALID.  All
 * before any device call. */
int pvd_mesh_atex_points(const float *vertices, uint32_t V, const int32_t *triangles, uint32_t T, const float *normals,
                         const uint32_t counts[5], const uint32_t *order, uint32_t row0, uint32_t row1, float *x, float *n,
                         pvd_stream_t stream);

/* color [N,3] f32 <- "Sample" above of texture [Ht, Wt, 3] f32 at tri [N] i32, bary [N,2] f32 (counts: HOST u32 [5]; slot [T] u32 on the
 * device; bg3: device f32 [3]).  One launch, one lane per hit: the gather of slot[tri], then four 12-byte gathers; no LDS, no atomics;
 * rows past N are never written.  NULL counts: PVD_ERR_INVALID; then the layout's errors; then a sum of the counts that is not T:
 * PVD_ERR_INVALID; then N == 0: PVD_OK with no launch (every pointer may be NULL); then NULL texture, slot (T not 0), tri, bary, bg3 or
 * color: PVD_ERR_INVALID.  All before any device call. */
int pvd_mesh_atex_sample(const float *texture, uint32_t T, const uint32_t counts[5], const uint32_t *slot, const int32_t *tri,
                         const float *bary, uint32_t N, const float *bg3, float *color, pvd_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* PVD_HIP_MESH_ATEX_H */
