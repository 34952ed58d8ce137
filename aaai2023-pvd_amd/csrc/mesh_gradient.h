// mesh_gradient.h -- the lattice gradient of include/pvd_hip_mesh_attr.h, shared by the normals of both meshers (csrc/mesh.hip,
// csrc/mesh_nets.hip).
#pragma once

#include "pvd_device.h"

namespace pvd {

// world gradient of u at the lattice point q = (c[0], c[1], c[2]) (include/pvd_hip_mesh_attr.h): central differences inside the
// lattice, one-sided ones on its faces, each scaled by the axis' lattice points per world unit
__device__ __forceinline__ void world_gradient(const float *__restrict__ u, uint32_t R, uint32_t q, const uint32_t c[3], const float inv_h[3],
                                               float g[3]) {
    const uint32_t stride[3] = {R * R, R, 1u};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        float d;
        if (c[a] == 0)
            d = u[q + stride[a]] - u[q];
        else if (c[a] == R - 1)
            d = u[q] - u[q - stride[a]];
        else
            d = (u[q + stride[a]] - u[q - stride[a]]) * 0.5f;
        g[a] = d * inv_h[a];
    }
}

}  // namespace pvd
