/*
 * pvd_hip_metrics.h -- image metrics of a held-out evaluation in libpvd_hip.so, next to the entry points pvd_hip.h declares.
 * Same conventions as pvd_hip.h (device pointers unless the name says host, caller-allocated buffers, the stream as void*,
 * PVD_OK or a negative pvd_status, no state kept between calls).  The metrics: compute_ssim, distill_mutual/utils.py:219-300,
 * as Trainer.evaluate calls it (utils.py:1275-1279), and the squared error PSNRMeter.update takes (utils.py:491-529).
 * pvd_abi_version() is not changed by these additions: the entry points of pvd_hip.h keep their signatures.
 */
#ifndef PVD_HIP_METRICS_H
#define PVD_HIP_METRICS_H

#include "pvd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Edge of the square output tile one workgroup of the SSIM kernel computes (the binding repeats it as METRICS_TILE so that the
 * tests can put image edges on tile seams). */
#define PVD_METRICS_TILE 32
/* Largest (odd) window the kernel implements. */
#define PVD_METRICS_MAX_FILTER 15

/* Floats of workspace the call below needs for B images of H x W x C (returned as the int: always > 0 for valid sizes;
 * PVD_ERR_UNSUPPORTED if the count does not fit an int).  Layout: [0] the max_val the SSIM kernel used, [4 .. 4 + 256) partial
 * maxima of the device-side maximum, then per (image, tile) two partial sums {SSIM map, squared difference}. */
int pvd_image_metrics_workspace_floats(uint32_t B, uint32_t H, uint32_t W, uint32_t C);

/* SSIM and mean squared error of B image pairs, img0 / img1 [B,H,W,C] float32 (channels last), C in 1..4.
 * Per image and channel: the five moments E[x], E[y], E[x^2], E[y^2], E[xy] under the separable window taps_host (filter_size
 * HOST floats, odd filter_size <= PVD_METRICS_MAX_FILTER; the blur runs along W first, then along H, with ZEROS outside the image
 * and no renormalisation, as conv2d(padding = filter_size / 2) does), then
 *     s00 = max(E[x^2] - mu0^2, 0), s11 = max(E[y^2] - mu1^2, 0), s01 = sign(s01) min(sqrt(s00 s11), |s01|),
 *     c1 = (k1 max_val)^2, c2 = (k2 max_val)^2,
 *     map = (2 mu0 mu1 + c1)(2 s01 + c2) / ((mu0^2 + mu1^2 + c1)(s00 + s11 + c2)).
 * ssim[b] = the mean of the map over H W C; mse[b] = the mean of (img0 - img1)^2 over H W C (PSNR = -10 log10(mse[b]));
 * ssim_map [B,H,W,C] (or NULL) receives the map itself.
 * max_val > 0 is used as given; max_val <= 0 stands for max(img0.max(), img1.max()) over BOTH WHOLE BATCHES, taken by a small
 * reduction launch ahead of the SSIM launch and handed over in the workspace (no host read-back; workspace[0] holds it after
 * the call).  One workgroup per (image, tile) writes its two partial sums into the workspace; a last launch adds them in a
 * fixed order (in double): no float atomics, so two calls on the same inputs give the same bits.
 * The tap sums use fmaf (as the convolution libraries behind conv2d do); everything after them is rounded operation by
 * operation in the order of utils.py:279-298.
 * An even filter_size, filter_size > PVD_METRICS_MAX_FILTER, C > 4 (or 0), or more than 2^31 - 1 tiles: PVD_ERR_UNSUPPORTED.
 * B == 0 is PVD_OK and launches nothing. */
int pvd_image_metrics(const float *img0, const float *img1, uint32_t B, uint32_t H, uint32_t W, uint32_t C,
                      const float *taps_host, uint32_t filter_size, float k1, float k2, float max_val, float *workspace,
                      float *ssim, float *mse, float *ssim_map, pvd_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* PVD_HIP_METRICS_H */
