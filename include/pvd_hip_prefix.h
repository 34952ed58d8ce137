/*
 * pvd_hip_prefix.h -- the student-independent prefix of a training step (batch, march, teacher compositing) for a GROUP of G
 * consecutive steps in one launch per stage, in libpvd_hip.so next to the entry points pvd_hip.h declares.  Same conventions as
 * pvd_hip.h (device pointers, caller-allocated buffers, the stream as void*, PVD_OK or a negative pvd_status).
 * pvd_abi_version() is not changed by these additions: the single-step entry points keep their signatures and their kernels.
 *
 * Layout: every per-ray array of a group is [G][N ...], every per-sample array [G][M ...]: SEGMENT j is slice j, and what a
 * segment holds is bit for bit what the j-th of G sequential single-step calls writes into its own buffers -- offsets in a
 * segment's `rays` table are relative to its slice.  The frozen teacher's forward needs no entry point of its own: it runs
 * over the G * M rows of the group (pvd_hash_head_forward_fused takes a row count; rows are independent of each other and M is
 * a whole number of its 128-row tiles wherever the trainers allocate it).
 */
#ifndef PVD_HIP_PREFIX_H
#define PVD_HIP_PREFIX_H

#include "pvd_hip_march.h"

#ifdef __cplusplus
extern "C" {
#endif

/* G batches of pvd_make_ray_batch in one launch: batch j uses pose (state[0] + j) % P and the PCG32 stream of batch counter
 * state[1] + j, the same draws per ray in the same order; outputs [G][N ...] (inds and bg may be NULL).  The state afterwards is
 * the state after G single calls: {(state[0] + G) % P, state[1] + G, 0}.  Needs state[0] < P and G <= 65535. */
int pvd_make_ray_batch_group(const float *poses, uint32_t P, int64_t *state, uint64_t seed, float fx, float fy, float cx,
                             float cy, uint32_t H, uint32_t W, uint32_t N, uint32_t G, const float *aabb, float min_near,
                             int64_t *inds, float *rays_o, float *rays_d, float *bg, float *nears, float *fars,
                             pvd_stream_t stream);

/* Scratch of pvd_march_rays_train_group: G * (N + 1) records of 256 bytes. */
size_t pvd_march_group_workspace_bytes(uint32_t N, uint32_t G);

/* pvd_march_rays_train_mask over G segments of N rays each in two launches (count, write from the chunk records with the scan
 * folded in per segment).  rays_o, rays_d [G][N,3]; nears, fars [G][N]; xyzs, dirs [G][M,3]; deltas [G][M,2]; rays [G][N,3];
 * counter [G][2].  Every segment has its own exclusive scan from 0, its own counter, its own overflow rule (its trailing rays
 * are dropped against min(M, budget_dev[j * budget_stride]); budget_dev NULL: M; budget_stride 0: one budget for all) and, with
 * PVD_MARCH_FRESH, its own cleared tail.  Without PVD_MARCH_FRESH counter[j][0] is segment j's running offset, as in the single
 * call.  N <= 16384 (the per-workgroup prefix of a segment), G <= 65535; the workspace is required (PVD_ERR_INVALID without). */
int pvd_march_rays_train_group(const float *rays_o, const float *rays_d, const uint8_t *grid, float bound, float dt_gamma,
                               uint32_t max_steps, uint32_t N, uint32_t G, uint32_t C, uint32_t H, uint32_t M, const float *nears,
                               const float *fars, float *xyzs, float *dirs, float *deltas, int32_t *rays, int32_t *counter,
                               uint32_t perturb, void *workspace, size_t workspace_bytes, uint32_t flags,
                               const int32_t *budget_dev, uint32_t budget_stride, const uint8_t *coarse_mask, pvd_stream_t stream);

/* pvd_composite_rays_train_bg_forward over G segments in one launch: sigmas [G][M], rgbs [G][M,3], deltas [G][M,2], rays
 * [G][N,3] (slice-relative offsets), bg [G][N,3] or NULL, nears, fars [G][N]; weights_sum, depth [G][N], image [G][N,3].
 * budget_dev / budget_stride as above. */
int pvd_composite_rays_train_bg_forward_group(const float *sigmas, const float *rgbs, const float *deltas, const int32_t *rays,
                                              uint32_t M, uint32_t N, uint32_t G, const float *bg, float bg_scalar,
                                              const float *nears, const float *fars, float depth_eps, float *weights_sum,
                                              float *depth, float *image, const int32_t *budget_dev, uint32_t budget_stride,
                                              pvd_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* PVD_HIP_PREFIX_H */
