/*
 * pvd_hip_mlp.h -- inference entry points of the frozen `mlp` (NeRF trunk) model in libpvd_hip.so, next to the ones pvd_hip.h
 * declares.  Same conventions as pvd_hip.h (device pointers unless the name says host, caller-allocated buffers, the stream as
 * void*, PVD_OK or a negative pvd_status, no state kept between calls).  The model: NeRFNetwork.forward with model_type "mlp",
 * distill_mutual/network.py:154-182 and :413-437; the loop: the eval branch of run_cuda, distill_mutual/renderer.py:450-543.
 * pvd_abi_version() is not changed by these additions: the entry points of pvd_hip.h keep their signatures.
 */
#ifndef PVD_HIP_MLP_H
#define PVD_HIP_MLP_H

#include "pvd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* pvd_mlp_head_forward_fused with a device-side row count, as pvd_head_forward / pvd_hash_head_forward_fused take one:
 * rows_dev (DEVICE int32, or NULL = all M rows): only the first min(M, *rows_dev) rows are computed and written, M sizes the
 * launch (inference rounds whose extent the host does not know); rows of pts_f16 / dirs past the count are never read.
 * Every other argument as for pvd_mlp_head_forward_fused, which forwards here with rows_dev = NULL. */
int pvd_mlp_head_forward_fused_rows(const void *pts_f16, uint32_t M, const void *wstream_f16, uint32_t n_before,
                                    uint32_t n_after, const float *dirs, const float *Wa1, const float *Wa2, const float *Wc1,
                                    const float *Wc2, const float *Wc3, const void *image, float clip_sigma_min, float clip_max,
                                    float *sigma, float *rgb, float *feat16, const int32_t *rows_dev, pvd_stream_t stream);

/* A whole inference render of a frozen `mlp` model in ONE persistent launch (+ the first-hit pass that builds the ray queue):
 * run_cuda's eval branch (renderer.py:450-543, raymarching.cu:704-948) over the positional encoding (tools/encoding.py:6-49),
 * the NeRF trunk and the sigma / colour head (network.py:154-182, :413-437).  rays_o / rays_d [N,3], nears / fars [N]
 * (pvd_near_far_from_aabb); bitfield / bound / dt_gamma / max_steps / C / H as for pvd_march_rays (perturb = 0); sigma_scale =
 * density_scale (renderer.py:528).  freq_bands_host: n_freqs HOST floats, the encoder's frequencies; only n_freqs = 10 with the
 * inputs included (63 columns, padded to 64) is implemented, anything else is PVD_ERR_UNSUPPORTED.  wstream_f16 / n_before /
 * n_after / Wa1 .. Wc3 / image / clips as for pvd_mlp_head_forward_fused.  workspace: 2 N + 12 int32, laid out as for
 * pvd_infer_image_hash ([0] rays queued, [2 N + 2 .. 2 N + 6): local rounds, rows shaded, walk-only rounds, workgroups used).
 * weights_sum [N], depth [N], image_out [N,3]: ZERO-FILLED by the caller, written for every ray that enters the box -- the
 * values the round loop leaves there (background compositing and depth normalisation stay with the caller,
 * renderer.py:545-548).  Per sample the arithmetic of pvd_freq_encode(PVD_F16, 64) + pvd_mlp_head_forward_fused, per ray
 * pvd_composite_rays' sums in its order: a ray's result does not depend on how rays are grouped into rounds, so the image is the
 * round loop's, bit for bit; the reference stops ALL rays once the rounds' steps add up to max_steps, here a ray stops after ITS
 * OWN max_steps samples.  N == 0 is PVD_OK and launches nothing. */
int pvd_infer_image_mlp(const float *rays_o, const float *rays_d, const float *nears, const float *fars, uint32_t N,
                        const uint8_t *bitfield, float bound, float dt_gamma, uint32_t max_steps, uint32_t C, uint32_t H,
                        float sigma_scale, const float *freq_bands_host, uint32_t n_freqs, const void *wstream_f16,
                        uint32_t n_before, uint32_t n_after, const float *Wa1, const float *Wa2, const float *Wc1,
                        const float *Wc2, const float *Wc3, const void *image, float clip_sigma_min, float clip_max,
                        int32_t *workspace, float *weights_sum, float *depth, float *image_out, pvd_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* PVD_HIP_MLP_H */
