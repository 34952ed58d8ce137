/*
 * pvd_hip_mesh_smooth.h -- a triangle mesh smoothed by Taubin's lambda|mu filter (Taubin 1995: a Laplacian step with weight
 * lambda > 0, then one with weight mu < -lambda; it takes out the high frequencies without the shrinkage of plain Laplacian
 * smoothing), in libpvd_hip.so next to the clustering of pvd_hip_mesh_simplify.h (pvd/mesh.py: smooth_mesh,
 * extract_surface(smooth=N)).  Same conventions as pvd_hip.h (device pointers, caller-allocated buffers, the stream as void*,
 * PVD_OK or a negative pvd_status).  pvd_abi_version() is not changed by this addition.
 *
 * Every sum below is a sum of integers, so every output is an exact function of the inputs that does not depend on the order in
 * which anything lands: the results are bit-identical from run to run, and tests/mesh_smooth_restatement.py restates them in numpy
 * bit for bit.  The library is built with -ffp-contract=off, so the float64 expressions mean on the device what they mean there.
 *
 * Inputs   vertices [V,3] f32, triangles [T,3] i32, a box bmin3 .. bmax3 (device f32 [3] each), an optional pinned [V] u8 (a
 *          vertex is PINNED iff its byte is not 0; NULL: nothing is pinned); V and T at most 2^31 - 1.  Everything below is float64
 *          from the f32 inputs unless it says integer.
 *
 * Vertex   VALID iff its three coordinates are finite.
 *
 * q_a      the quantised position of a valid vertex along axis a, exactly the q_a of pvd_hip_mesh_simplify.h.  e_a = bmax_a -
 *          bmin_a; the axis is FLAT iff e_a is not a positive finite number.  Flat: q_a = 0.  Otherwise
 *              f_a = clamp((x_a - bmin_a) / e_a, 0, 1),      q_a = llrint(f_a * 2^30)   (ties to even; an integer in 0 .. 2^30).
 *          A vertex outside the box is thereby PROJECTED ONTO THE BOX: it takes part, as a neighbour too, with the position of the
 *          nearest point of the box.
 *
 * Triangle VALID iff its three indices are in [0, V), its three vertices are valid, and its three indices are pairwise different.
 *
 * Row      the row of vertex v is a MULTISET: every valid triangle that has v as a corner contributes its other two corners.  n_v is
 *          the row's size, 2 x the number of valid triangles at v.  A NEIGHBOUR ACROSS AN EDGE SHARED BY k VALID TRIANGLES APPEARS
 *          k TIMES: on a closed manifold mesh every neighbour appears twice, which is the uniform umbrella; across a boundary edge
 *          the weight is 1, half that of an interior edge of the same vertex.  A vertex that is not valid never appears in a row.
 *
 * Movable  a vertex is MOVABLE iff it is valid, not pinned, and n_v > 0.
 *
 * Pass     with weight w, applied to all movable vertices at once from the positions the previous pass left (two buffers, never in
 *          place).  Per axis, in integers, S_a = the sum of q_a over the row (int64; at most 2^32 * 2^30 = 2^62); then in float64,
 *          each operation rounded on its own,
 *              q'_a = clamp(q_a + llrint(w * ((double)S_a / (double)n_v - (double)q_a)), 0, 2^30).
 *          A vertex that is not movable keeps its q; it still acts as a neighbour when it is valid.
 *
 * Iteration  a pass with lambda, then a pass with mu.  lambda and mu are finite doubles with |w| <= 1; iterations is
 *          0 .. PVD_MESH_SMOOTH_MAX_ITERATIONS.
 *
 * Output   out_vertices [V,3] f32.  A movable vertex: x'_a = (float)(bmin_a + (double)q_a * (e_a * 2^-30)) on an axis that is not
 *          flat, bmin_a on a flat one.  A vertex that is not movable: its input bits (a NaN's payload is copied, not recomputed).
 *          iterations == 0: every vertex gets its input bits.  The triangles are not touched: topology and order stay.
 *
 * Not done No cotangent weights, no feature preservation, no volume correction beyond what lambda|mu gives.  A vertex outside
 *          the box does not come back to where it was: it is projected (q_a) before the first pass.
 *
 * Bound    With lambda = mu = 0 and iterations >= 1, for a movable vertex whose coordinate x_a lies inside the box (bmin_a <= x_a
 *          <= bmax_a, axis not flat):
 *              |x_a - x'_a|  <=  2^-30 e_a  +  2^-23 max(|bmin_a|, |bmax_a|).
 *          Derivation, the one of pvd_hip_mesh_simplify.h without its cell term.  A pass with w = 0 adds llrint(+-0) = 0: q_a
 *          stays the quantised input.  In real numbers x_a = bmin_a + f e_a with f = (x_a - bmin_a) / e_a in [0, 1] (no clamp acts).
 *          The computed f_a carries at most two float64 roundings (the difference, the quotient): |f_a - f| <= 2^-52.  q_a / 2^30
 *          differs from f_a by at most 2^-31 (one quantisation).  (double)q_a is exact, e_a * 2^-30 is exact unless it underflows,
 *          and their product carries one rounding of 2^-53 relative to at most e_a.  Hence, before the last sum,
 *              |x_a - (bmin_a + q_a 2^-30 e_a)|  <=  e_a (2^-31 + 2^-52 + 2^-53)  <  2^-30 e_a.
 *          The float64 sum and its rounding to float32 give x'_a with |x'_a - exact| <= (2^-24 + 2^-53) |exact|, and |exact| <=
 *          max(|bmin_a|, |bmax_a|) (1 + 2^-50) because q_a 2^-30 is in [0, 1]: below 2^-23 max(|bmin_a|, |bmax_a|).  The two terms are
 *          the quantisation and the f32 rounding of the result.  PVD_MESH_SMOOTH_BOUND(e, lo, hi) below is this bound; the tests
 *          use it.
 */
#ifndef PVD_HIP_MESH_SMOOTH_H
#define PVD_HIP_MESH_SMOOTH_H

#include "pvd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* iterations: 0 .. PVD_MESH_SMOOTH_MAX_ITERATIONS.  V, T: at most 2^31 - 1. */
#define PVD_MESH_SMOOTH_MAX_ITERATIONS 1024

/* The round-trip bound derived above, per axis (float64): extent e, the box lo .. hi on that axis. */
#define PVD_MESH_SMOOTH_ABS_(x) ((x) < 0 ? -(x) : (x))
#define PVD_MESH_SMOOTH_BOUND(e, lo, hi) \
    (0x1p-30 * (e) + 0x1p-23 * (PVD_MESH_SMOOTH_ABS_(lo) > PVD_MESH_SMOOTH_ABS_(hi) ? PVD_MESH_SMOOTH_ABS_(lo) : PVD_MESH_SMOOTH_ABS_(hi)))

/* Bytes of workspace for V vertices and T triangles (0 for a V or T outside the limits):
 *     64 V + 12 ceil(V / 256) + 24 T + 24
 * that is 3 x 16 V (per vertex q_x, q_y, q_z and the flags, 32-bit each: what build quantised, and the two buffers of the passes)
 * + 8 (V + 1) (row offsets, 64-bit: the entries can pass 2^32) + 8 ceil(V / 256) + 4 ceil(V / 256) (per 256 rows their sum and their
 * largest) + 4 V (row sizes, then the fill cursors) + 4 V (the list of long rows) + 24 T (the rows: at most 6 T entries of 32 bits)
 * + 16 (the number of long rows). */
size_t pvd_mesh_smooth_workspace_bytes(uint32_t V, uint32_t T);

/* Builds the rows: per vertex q and its flags; per valid triangle a 32-bit integer atomicAdd of 2 into the row size of each corner;
 * the sizes scanned into 64-bit row offsets (per-256 sums, a one-workgroup scan in chunks, offsets); the movable rows longer than the
 * wavefront threshold of csrc/mesh_smooth.hip compacted into a list (in any order); per valid triangle its six entries written at an
 * atomic cursor per row (the order inside a row is arbitrary: a row is a multiset).  totals_dev int64 [2] <- (the row entries of
 * all vertices together, the largest n_v) on the device.  Two memsets and six launches on the stream; no workgroup waits on another
 * one, no retry loops, no float atomics.  V == 0: PVD_OK without a launch (every array may then be NULL, totals_dev is not written).
 * T == 0 is allowed (triangles may be NULL): all rows are empty.  The workspace must be 16-byte aligned.  NULL pointer (pinned
 * excepted), unaligned or short workspace (pvd_mesh_smooth_workspace_bytes(V, T)): PVD_ERR_INVALID; V or T outside the limits:
 * PVD_ERR_UNSUPPORTED; both before any device call.  No index of `triangles` is used before it is checked against [0, V). */
int pvd_mesh_smooth_build(const float *vertices, uint32_t V, const int32_t *triangles, uint32_t T, const float *bmin3,
                          const float *bmax3, const uint8_t *pinned, void *workspace, size_t workspace_bytes, int64_t *totals_dev,
                          pvd_stream_t stream);

/* `iterations` iterations (a pass with lambda, a pass with mu) for the SAME vertices, V, T, box and the workspace
 * pvd_mesh_smooth_build left, then out_vertices [V,3] f32 as defined above: 2 x iterations pass launches and one output launch.  A
 * pass is a gather: no atomics and no float accumulation.  What build left is only read, so a second run on the same build gives the
 * same bits.  out_vertices must not overlap vertices.  V == 0: PVD_OK without a launch.  Argument checks as for
 * pvd_mesh_smooth_build; lambda or mu not finite or above 1 in magnitude, iterations above PVD_MESH_SMOOTH_MAX_ITERATIONS:
 * PVD_ERR_INVALID. */
int pvd_mesh_smooth_run(const float *vertices, uint32_t V, uint32_t T, const float *bmin3, const float *bmax3, void *workspace,
                        size_t workspace_bytes, double lambda, double mu, uint32_t iterations, float *out_vertices,
                        pvd_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* PVD_HIP_MESH_SMOOTH_H */
