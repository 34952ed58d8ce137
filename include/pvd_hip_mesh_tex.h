/*
 * pvd_hip_mesh_tex.h -- a texture atlas for a triangle mesh, in libpvd_hip.so next to the ray cast of pvd_hip_mesh_ray.h: the surface
 * point of every texel (what a colour field is baked at) and the bilinear lookup of a baked texture at the hits of a cast (pvd/mesh.py:
 * texture_layout, texture_uv, texture_points, bake_texture, sample_texture, render_mesh(texture=...)).  Same conventions as pvd_hip.h
 * (device pointers, caller-allocated buffers, the stream as void*, PVD_OK or a negative pvd_status).  pvd_abi_version() is not changed by
 * this addition.
 *
 * Layout   a per-triangle atlas in closed form: nothing is packed, sorted or read back.  S is the cell edge in texels,
 *          PVD_MESH_TEX_MIN_S <= S <= PVD_MESH_TEX_MAX_S, and m = S - 3.  Two triangles share a square cell of S x S texels:
 *              cells = ceil(T / 2);   C = the smallest integer >= 1 with C * C >= cells (integer arithmetic);
 *              rows = max(1, ceil(cells / C));   Wt = C * S;   Ht = rows * S.
 *          Wt or Ht above PVD_MESH_TEX_MAX_SIDE: PVD_ERR_UNSUPPORTED.  T = 0 gives one cell that nothing owns.
 *
 * Ownership   texel (x, y) of the image texture[y, x] lies in the cell k = (y / S) * C + (x / S), at i = x % S, j = y % S.
 *          The LOWER half of the cell is i + j <= S - 1 (the diagonal included): it belongs to the triangle f = 2k, with p = i, q = j.
 *          The UPPER half belongs to f = 2k + 1, with p = S - 1 - i, q = S - 1 - j.  A texel is OWNED iff f < T.  A triangle owns
 *          S (S + 1) / 2 texels in a lower half and S (S - 1) / 2 in an upper half.
 *
 * Weights  each operation below is ONE IEEE float32 operation, in the order written, and NOTHING IS FUSED:
 *              beta = (float)p / (float)m,   gamma = (float)q / (float)m,   alpha = (1 - beta) - gamma.
 *          Texels off the triangle proper (p + q > m) get weights slightly outside [0, 1]: the linear extrapolation in the triangle's
 *          plane, not a clamp.  The texel at (p, q) = (0, 0), (m, 0), (0, m) has the weights (1, 0, 0), (0, 1, 0), (0, 0, 1) exactly.
 *
 * Point    X = (alpha * A + beta * B) + gamma * Cc per component, from the float32 corners A, B, Cc of the triangle; at a corner's
 *          texel that is the corner, bit for bit (the other two products are +-0).
 *
 * Normal   with vertex normals: the same expression on the three vertex normals, left unnormalised.  Without: the face normal
 *          cross(B - A, Cc - A) = (uy vz - uz vy, uz vx - ux vz, ux vy - uy vx) with u = B - A, v = Cc - A, every product rounded on
 *          its own; every texel of the triangle gets the same value.
 *
 * Invalid and unowned   a triangle is VALID under the rule of pvd_hip_mesh_dist.h (its three indices are in [0, V) and its nine
 *          coordinates are finite); when normals are given its three normals (nine numbers) must be finite as well.  The texels of an
 *          invalid triangle, and unowned texels, get six NaNs (the quiet NaN 0x7fc00000).
 *
 * Corner coordinates   in continuous texel units (texel centres at integer + 0.5), with (cx, cy) = (k % C, k / C):
 *              lower: a = (cx S + 0.5,     cy S + 0.5),       b = a + (m, 0),   c = a + (0, m);
 *              upper: a = (cx S + S - 0.5, cy S + S - 0.5),   b = a - (m, 0),   c = a - (0, m).
 *          OBJ convention: uv = (X / Wt, 1 - Y / Ht).  The corners are texel centres, so a bilinear filter returns the baked value of
 *          the corner there.
 *
 * WHY THE LAYOUT WORKS.  For weights inside the triangle, fu + fv <= m with fu = beta m and fv = gamma m.  The four texels bilinear
 *          filtering touches are (i0 | i0 + 1, j0 | j0 + 1) with i0 = floor fu, j0 = floor fv.  Three of them have p + q <= i0 + j0 + 1
 *          <= m + 1 = S - 2.  The fourth, (i0 + 1, j0 + 1), has p + q = i0 + j0 + 2; where fu or fv has a fraction, i0 + j0 <= m - 1 and
 *          it is <= S - 2 as well.  All of these have p, q <= S - 2 and p + q <= S - 2: they lie in the same cell, strictly on the
 *          triangle's side of the cell's diagonal, and are owned by it, in a lower and in an upper half alike.  Their values are the
 *          linear function of (p, q) above, extrapolated past the hypotenuse p + q = m.  So a bilinear lookup inside a triangle mixes
 *          values of that triangle's plane only: NO GUTTER PASS IS NEEDED AND NO NEIGHBOUR CONTRIBUTES.
 *          THE ONE EXCEPTION, WITH WEIGHT ZERO: at a point of the hypotenuse where fu and fv are both whole numbers (the corners b and
 *          c among them), i0 + j0 = m, tx = ty = 0, and the fourth texel lies ON the diagonal, p + q = S - 1.  The diagonal belongs to
 *          the lower half: an even triangle reads its own texel, an odd triangle reads one of triangle tri - 1 (which exists), and the
 *          sample multiplies it by tx = 0 and by ty = 0.  With a finite texture (bake_texture writes no other) the result does not depend
 *          on it; a NaN there would come through, as 0 * NaN.  A lookup whose bary lies outside the triangle (a cast never returns one)
 *          may read more of the cell's other triangle, never another cell.
 *
 * Cost     the fill is m^2 / S^2 of the image (the two triangles proper, m^2 / 2 each): 39 % at S = 8, 66 % at S = 16, 91 % at S = 64.
 *          ONE TEXEL DENSITY SERVES ALL TRIANGLES: a triangle has m texels along its two short edges whatever its size, so a large
 *          triangle is undersampled next to a small one.  Extracted meshes have triangles of one lattice cell; simplified ones do not.
 *          An area-adaptive cell size is not attempted.
 *
 * Sample   (tri, bary = (beta, gamma) as pvd_mesh_ray_cast returns them).  tri < 0 or tri >= T: the background colour, and nothing is
 *          read.  Otherwise, in float32, unfused, in this order:
 *              fu = fminf(fmaxf(beta * m, 0), m)  (a NaN becomes 0);   i0 = min((int)floorf(fu), m);   tx = fu - i0;
 *              the same for fv, j0, ty from gamma;
 *              the four texels (i0 | i0 + 1, j0 | j0 + 1) in (p, q) coordinates, mirrored (i = S - 1 - p, j = S - 1 - q) for an odd tri;
 *              c = (c00 * (1 - tx) + c10 * tx) * (1 - ty) + (c01 * (1 - tx) + c11 * tx) * ty      (cPQ: the texel (i0 + P, j0 + Q)).
 *          0 <= i0, j0 <= m, so every read has 0 <= p, q <= m + 1 = S - 2 and stays inside the triangle's own cell, whatever bary holds.
 */
#ifndef PVD_HIP_MESH_TEX_H
#define PVD_HIP_MESH_TEX_H

#include "pvd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The cell edge in texels, and the largest side of an atlas. */
#define PVD_MESH_TEX_MIN_S 4
#define PVD_MESH_TEX_MAX_S 64
#define PVD_MESH_TEX_MAX_SIDE 16384

/* out[4] <- (C, rows, Wt, Ht) of the layout above for T triangles and a cell edge S.  Host only: no device call.  NULL out:
 * PVD_ERR_INVALID; S outside PVD_MESH_TEX_MIN_S .. PVD_MESH_TEX_MAX_S, or a side above PVD_MESH_TEX_MAX_SIDE: PVD_ERR_UNSUPPORTED (out is
 * not written). */
int pvd_mesh_tex_layout(uint32_t T, uint32_t S, uint32_t out[4]);

/* x, n [(row1 - row0) * Wt, 3] f32 <- the point and the normal defined above of every texel of the image rows row0 .. row1 - 1 of the
 * atlas of the mesh (vertices [V,3] f32, triangles [T,3] i32; normals [V,3] f32 or NULL: face normals), so that a large atlas can be baked
 * in bands.  One launch, one lane per texel, consecutive lanes along x; no LDS, no atomics; nothing outside the band is written.  T == 0
 * is allowed (triangles may be NULL; V == 0: vertices and normals may be NULL).  The layout's errors first; then row0 > row1 or
 * row1 > Ht: PVD_ERR_INVALID; then row0 == row1: PVD_OK with no launch (every pointer may be NULL); then NULL vertices (T and V not 0),
 * triangles (T not 0), x or n: PVD_ERR_INVALID.  All before any device call. */
int pvd_mesh_tex_points(const float *vertices, uint32_t V, const int32_t *triangles, uint32_t T, const float *normals, uint32_t S,
                        uint32_t row0, uint32_t row1, float *x, float *n, pvd_stream_t stream);

/* color [N,3] f32 <- the sample defined above of texture [Ht, Wt, 3] f32 (the atlas of T triangles at the cell edge S) at tri [N] i32,
 * bary [N,2] f32; bg3: device f32 [3].  One launch, one lane per ray, four 12-byte gathers per hit; no LDS, no atomics; rows past N are
 * never written.  The layout's errors first; then N == 0: PVD_OK with no launch (every pointer may be NULL); then NULL texture, tri, bary,
 * bg3 or color: PVD_ERR_INVALID.  All before any device call. */
int pvd_mesh_tex_sample(const float *texture, uint32_t T, uint32_t S, const int32_t *tri, const float *bary, uint32_t N, const float *bg3,
                        float *color, pvd_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* PVD_HIP_MESH_TEX_H */
