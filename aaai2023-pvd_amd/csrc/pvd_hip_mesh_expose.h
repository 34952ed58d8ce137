/*
 * pvd_hip_mesh_expose.h -- which triangles of a mesh an outside view can see: an occlusion (any-hit) query from the surface outwards,
 * in libpvd_hip.so next to the first-hit cast of include/pvd_hip_mesh_ray.h, whose workspace, grid and hit() it uses (pvd/mesh.py:
 * mesh_exposure, cull_hidden).  Same conventions as pvd_hip.h (device pointers, caller-allocated buffers, the stream as void*, PVD_OK or
 * a negative pvd_status).  pvd_abi_version() is not changed by this addition.
 * (This header lives next to csrc/mesh_expose.hip and not in include/: tests/test_abi_mesh_tex.py pins the list of files there.)
 *
 * Mesh     vertices [V,3] f32, triangles [T,3] i32.  A triangle is VALID under the rule of pvd_hip_mesh_dist.h: its three indices
 *          are in [0, V) and its nine coordinates are finite.  Invalid triangles take no part: they block nothing, cast nothing.
 *
 * Directions   dirs [D,3] f32, 1 <= D <= PVD_MESH_EXPOSE_MAX_D.  A direction that is not finite or is (0, 0, 0) takes no part.  ONE set
 *          serves every triangle and both of its sides (see "Side"): no hemisphere frame is built.
 *
 * Sample points   every valid triangle f = (a, b, c) has S sample points, S = 1 or S = 4, with the weights (wa, wb, wc)
 *              p = 0: (1/3, 1/3, 1/3)     the centroid -- the only one for S = 1
 *              p = 1: (2/3, 1/6, 1/6)     p = 2: (1/6, 2/3, 1/6)     p = 3: (1/6, 1/6, 2/3)
 *          the weights being the float64 quotients 1.0 / 3.0, 2.0 / 3.0 and 1.0 / 6.0.  Per coordinate
 *              o = (float)((wa * a + wb * b) + wc * c)
 *          in float64 from the float32 corners: three products, two sums in the order written, NOTHING IS FUSED, one rounding to
 *          float32.  The rays start from that float32 point.  A point that is not finite (corners near the largest float32) casts
 *          nothing.
 *
 * Side     n = (b - a) x (c - a) and s = (n_x * d_x + n_y * d_y) + n_z * d_z in float64 from the float32 corners and direction:
 *              e = b - a,  g = c - a,  n_x = e_y * g_z - e_z * g_y,  n_y = e_z * g_x - e_x * g_z,  n_z = e_x * g_y - e_y * g_x,
 *          every product and every sum ONE float64 operation, in the order written, nothing fused.
 *              s > 0   the ray (o, d) is a FRONT ray of f: front is the outward side in the orientation pvd_mesh_emit gives
 *              s < 0   it is a BACK ray of f
 *              else    (s == 0, or s is NaN after an overflow) it is not cast.
 *
 * Blocked  a ray of f is BLOCKED iff some valid triangle g != f has hit(ray, g) with 0 <= t < +inf on the float64 t; hit is exactly
 *          steps 1 .. 8 of include/pvd_hip_mesh_ray.h (unfused float64, both faces count).  g != f compares INDICES: a geometric
 *          duplicate of f does block f (and f blocks it).  A ray that is not blocked ESCAPES.
 *
 * Result   counts [T,4] i32, per triangle: front rays cast, front rays that escaped, back rays cast, back rays that escaped, summed
 *          over its S points and the D directions (at most S * D = 4096 each).  An invalid triangle has four zeros.
 *          totals [5] u64: rays cast, rays that escaped, valid triangles with a front escape, valid triangles with a back escape,
 *          valid triangles with no escape at all.  Integers only: bit-identical from run to run.
 *
 * Independence   Blocked is an OR over triangles of a fixed function of (ray, triangle), so counts and totals depend on neither G,
 *          the box, the order of the triangles inside a cell, the banding nor the run -- WITH THE ONE EXCEPTION include/
 *          pvd_hip_mesh_ray.h names under "THE POINT OF THE TRIANGLE": a triangle that the ray sees edge-on, within rounding of its
 *          plane, may report a hit whose point lies outside its own range of cells; the walk then need not test it, and G = 1, which
 *          tests everything, may call a ray blocked that a finer grid lets escape.  For every other (ray, triangle) pair the promise
 *          holds without condition: the walk of pvd_hip_mesh_ray.h visits every cell along [0, +inf) until a hit is held, and the
 *          argument "WHY NO WINNER IS MISSED" there shows that every triangle that is hit is among those tested.  Far rays test every
 *          triangle, as there.
 *
 * Kernel   one wave of 64 lanes per triangle, four triangles per workgroup.  Lanes are directions, 64 at a time; an outer loop runs
 *          over the S points and the ceil(D / 64) chunks.  A lane stops at its first hit.  The four counts are ballots and population
 *          counts in the wave: no LDS, no atomics but one integer atomicAdd per wave and nonzero total.  Rays are never written to
 *          memory.  Work per ray: the walk's, but it ends at the first hit -- for a ray that escapes, every cell to the edge of the box.
 */
#ifndef PVD_HIP_MESH_EXPOSE_H
#define PVD_HIP_MESH_EXPOSE_H

#include "../../include/pvd_hip_mesh_ray.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Directions per call: 1 .. PVD_MESH_EXPOSE_MAX_D.  Sample points per triangle: 1 or 4. */
#define PVD_MESH_EXPOSE_MAX_D 1024

/* counts [(tri1 - tri0), 4] i32 <- the result defined above for the triangles tri0 .. tri1 - 1 (row 0 is triangle tri0) of the mesh
 * pvd_mesh_ray_build left in the workspace for the SAME T, G and pairs (the mesh and the box are read from the workspace only);
 * totals [5] u64 += the band's totals: the caller zeroes totals before the first band, and the bands of a mesh add up to the totals of
 * the whole.  dirs [D,3] f32 on the device.  One launch, no memset.  D outside 1 .. PVD_MESH_EXPOSE_MAX_D or S other than 1 or 4:
 * PVD_ERR_UNSUPPORTED; then the workspace checks of pvd_mesh_ray_build (NULL, unaligned or short: PVD_ERR_INVALID; G, T or pairs out of
 * range: PVD_ERR_UNSUPPORTED); then tri0 <= tri1 <= T, else PVD_ERR_INVALID; then tri0 == tri1: PVD_OK with no launch (dirs, counts and
 * totals may be NULL); then NULL dirs, counts or totals: PVD_ERR_INVALID.  All before any device call. */
int pvd_mesh_expose(const float *dirs, uint32_t D, uint32_t S, uint32_t tri0, uint32_t tri1, uint32_t T, uint32_t G, uint64_t pairs,
                    const void *workspace, size_t workspace_bytes, int32_t *counts, uint64_t *totals, pvd_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* PVD_HIP_MESH_EXPOSE_H */
