/*
 * pvd_hip_march.h -- a coarse "may be occupied" mask of the density bitfield and the training marcher that uses it, in
 * libpvd_hip.so next to the entry points pvd_hip.h declares.  Same conventions as pvd_hip.h (device pointers, caller-allocated
 * buffers, the stream as void*, PVD_OK or a negative pvd_status).  pvd_abi_version() is not changed by these additions: the
 * entry points of pvd_hip.h keep their signatures and pass no mask.
 */
#ifndef PVD_HIP_MARCH_H
#define PVD_HIP_MARCH_H

#include "pvd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Fine cells per edge of a coarse block.  The mask holds, per cascade, (H / 8)^3 bytes in plain linear order
 * ((bx * G + by) * G + bz, G = H / 8): 4 KB per cascade at H = 128. */
#define PVD_COARSE_BLOCK 8

/* mask [C * (H/8)^3] u8 from the Morton-ordered bitfield [C * H^3 / 8] u8 (pvd_packbits): byte = 1 iff any bit is set in the
 * block itself or in one of its (up to) 26 neighbours of the same cascade, else 0.  One launch, every byte written.
 * H must be a power of two >= 8 (PVD_ERR_UNSUPPORTED otherwise: the 8^3 cells of a block are 64 consecutive bytes of a Morton order
 * that stays inside the cascade only then) and the bitfield 16-byte aligned (PVD_ERR_INVALID). */
int pvd_occ_coarse_mask(const uint8_t *bitfield, uint32_t C, uint32_t H, uint8_t *mask, pvd_stream_t stream);

/* pvd_march_rays_train_ws with the mask of `grid` (pvd_occ_coarse_mask of the SAME bitfield, C and H; the caller keeps it
 * up to date).  The count pass tests 64 evenly spaced points of [t0, far] of a ray against the mask before it walks the
 * ray: a ray none of whose points can lie in an occupied cell is not walked, and the walk of the others ends behind the
 * last point that can.  Every output -- xyzs, dirs, deltas, rays, counter, the chunk records -- is bit-identical to
 * pvd_march_rays_train_ws.  coarse_mask == NULL: exactly pvd_march_rays_train_ws.  The mask is ignored (full walk) for
 * dt_gamma != 0, for an H that is no power of two >= 8, and per ray wherever the spacing of the 64 points is not safely below a
 * coarse block's edge. */
int pvd_march_rays_train_mask(const float *rays_o, const float *rays_d, const uint8_t *grid, float bound, float dt_gamma,
                              uint32_t max_steps, uint32_t N, uint32_t C, uint32_t H, uint32_t M, const float *nears,
                              const float *fars, float *xyzs, float *dirs, float *deltas, int32_t *rays, int32_t *counter,
                              uint32_t perturb, void *workspace, size_t workspace_bytes, uint32_t flags,
                              const int32_t *budget_dev, const uint8_t *coarse_mask, pvd_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* PVD_HIP_MARCH_H */
