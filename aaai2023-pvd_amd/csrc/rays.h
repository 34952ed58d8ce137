// rays.h -- one pixel's ray and its near/far against the scene box, shared by the kernels that make rays
// (raymarching.hip: k_near_far, k_get_rays, k_make_ray_batch; databatch.hip: k_image_batch).
#pragma once

#include <float.h>

#include "pvd_device.h"

namespace pvd {

// reference: kernel_near_far_from_aabb, raymarching.cu:93-147
__device__ __forceinline__ void near_far_of(const float o[3], const float d[3], const float *__restrict__ aabb, float min_near, float &near,
                                            float &far) {
    float tn = 0.f, tf = 0.f;
    bool miss = false;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const float rd = 1.0f / d[a];
        float lo = (aabb[a] - o[a]) * rd;
        float hi = (aabb[a + 3] - o[a]) * rd;
        if (lo > hi) { const float s = lo; lo = hi; hi = s; }
        if (a == 0) {
            tn = lo; tf = hi;
        } else if (!miss) {
            if (tn > hi || lo > tf) miss = true;
            else {
                if (lo > tn) tn = lo;
                if (hi < tf) tf = hi;
            }
        }
    }
    if (miss) {
        near = FLT_MAX; far = FLT_MAX;
    } else {
        near = tn < min_near ? min_near : tn;
        far = tf;
    }
}

// reference: get_rays, distill_mutual/utils.py:324-404 (pixel-centre directions through K^-1, normalise,
// rotate by the camera-to-world pose).  One thread per ray instead of ~20 elementwise launches.
__device__ __forceinline__ void ray_of_pixel(const float *__restrict__ pose, float fx, float fy, float cx, float cy, int64_t k, uint32_t W,
                                             float o[3], float d[3]) {
    const float i = (float)(k % W) + 0.5f, j = (float)(k / W) + 0.5f;
    const float x = (i - cx) / fx, y = (j - cy) / fy, z = 1.0f;
    const float inv = 1.0f / sqrtf(x * x + y * y + z * z);
    const float dx = x * inv, dy = y * inv, dz = z * inv;
#pragma unroll
    for (int r = 0; r < 3; r++) {
        d[r] = dx * pose[4 * r] + dy * pose[4 * r + 1] + dz * pose[4 * r + 2];
        o[r] = pose[4 * r + 3];
    }
}

}  // namespace pvd
