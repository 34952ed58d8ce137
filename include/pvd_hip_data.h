/*
 * pvd_hip_data.h -- training batches drawn on the device from a resident uint8 image stack, in libpvd_hip.so next to the entry
 * points pvd_hip.h declares.  Same conventions as pvd_hip.h (device pointers unless the name says host, caller-allocated
 * buffers, the stream as void*, PVD_OK or a negative pvd_status, no state kept between calls beyond the `state` words the
 * caller owns).  The data side of a teacher step: NeRFDataset.collate (distill_mutual/provider.py:278-308) -> get_rays incl.
 * its error_map branch (distill_mutual/utils.py:324-404, :357-381), the random background and alpha blend of train_step
 * (utils.py:987-995), near_far_from_aabb, and the error-map feedback at the end of train_step (utils.py:1120-1129).
 * pvd_abi_version() is not changed by these additions: the entry points of pvd_hip.h keep their signatures.
 */
#ifndef PVD_HIP_DATA_H
#define PVD_HIP_DATA_H

#include "pvd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Largest side g of the coarse error-map grid (the reference's is fixed at 128): the draw is one workgroup of 1024 lanes
 * holding 16 keys each. */
#define PVD_DATA_MAX_GRID 128

/* One training batch of N rays from ONE view of images [V,H,W,C] uint8 (C = 3 or 4), cameras poses [V,4,4] f32.
 *
 * state  int64 [3] = {position in `order`, batch counter, scratch (0 between calls)}; the call reads it on the device and
 *        advances it exactly once: position <- (position + 1) % V, counter <- counter + 1 (as pvd_make_ray_batch does).
 * view   = order[position % V] (order int32 [V], values in [0, V); NULL: the identity), written to view_out [1] int32.
 * Random numbers: PCG32 (XSH-RR 64/32) seeded with initstate = seed + 0x9E3779B97F4A7C15 * (counter + 1).
 *        Ray n: initseq 1, advance(8 n); draw 0 the uniform pixel id, draws 1 and 2 the jitter along rows and along columns,
 *        draws 3..5 the background colour.  Cell c (error-map mode): initseq 2, advance(c), one draw.
 * Pixel: error_map == NULL: k = (draw0 * H * W) >> 32.
 *        error_map [V, g*g] f32 (g <= PVD_DATA_MAX_GRID): N DISTINCT cells of the view's row w, drawn without replacement by the
 *        exponential race torch.multinomial(replacement=False) uses: key_c = w_c / e_c with e_c = 0 - logf(1 - u_c)
 *        (key_c = 0 where w_c is not > 0); the N largest keys win, equal keys go to the lower cell; the winners are written to
 *        inds_coarse [N] int64 in ascending cell order.  A cell becomes a pixel as get_rays does, in float32, each operation
 *        rounded: row = min((long)(cx sx + u1 sx), H - 1), col = min((long)(cy sy + u2 sy), W - 1) with cx = c / g, cy = c % g,
 *        sx = (float)(H / (double)g), sy = (float)(W / (double)g); k = row W + col.
 * Out:   inds [N] int64 = k; rays_o, rays_d [N,3] and nears, fars [N] as pvd_make_ray_batch computes them (get_rays at the
 *        pixel centre, near_far_from_aabb against aabb [6] with min_near);
 *        C == 4: bg [N,3] = draws 3..5, gt [N,3] = rgb a + bg (1 - a) with rgb = (float)u8 / 255.0f, a = (float)u8_a / 255.0f,
 *        products rounded before the sum; C == 3: gt = rgb, bg is not touched (and may be NULL).
 *        keys_out [g*g] f32 or NULL: the keys of the draw (for tests).
 * Launches: error-map mode the draw (one workgroup: radix select on the key bits, prefix-scan compaction), then in both modes
 * one grid of N lanes.  No host synchronisation; capturable into a hipGraph.
 *
 * N == 0: PVD_OK, nothing launched.  A NULL required pointer, V, H or W == 0, H W >= 2^32, C outside {3, 4}, C == 4 without bg,
 * error-map mode without inds_coarse or with N > g*g: PVD_ERR_INVALID.  error-map mode with g == 0 or g > PVD_DATA_MAX_GRID:
 * PVD_ERR_UNSUPPORTED.  All checked before any launch. */
int pvd_image_batch(const uint8_t *images, const float *poses, const int32_t *order, uint32_t V, uint32_t H, uint32_t W, uint32_t C,
                    int64_t *state, uint64_t seed, float fx, float fy, float cx, float cy, uint32_t N, const float *aabb,
                    float min_near, const float *error_map, uint32_t g, int32_t *view_out, int64_t *inds, int64_t *inds_coarse,
                    float *rays_o, float *rays_d, float *gt, float *bg, float *nears, float *fars, float *keys_out,
                    pvd_stream_t stream);

/* The feedback of a step into the sampling weights (utils.py:1120-1129): for ray n of the batch drawn from view[0]
 * (int32 [1] on the device: pvd_image_batch's view_out), err = ((d0^2 + d1^2) + d2^2) / 3 with d = pred[n] - gt[n] and
 * error_map[view][inds_coarse[n]] = 0.1f old + 0.9f err.  The cells of a batch are distinct, so every lane owns its cell
 * (plain stores).  pred, gt [N,3] f32, error_map [.., g*g] f32; a cell outside [0, g*g) is skipped.
 * N == 0: PVD_OK.  NULL pointers or g == 0: PVD_ERR_INVALID. */
int pvd_error_map_update(float *error_map, uint32_t g, const int32_t *view, const int64_t *inds_coarse, const float *pred,
                         const float *gt, uint32_t N, pvd_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* PVD_HIP_DATA_H */
