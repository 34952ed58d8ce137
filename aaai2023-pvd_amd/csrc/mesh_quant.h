// mesh_quant.h -- the fixed-point position format of include/pvd_hip_mesh_simplify.h (q_a, an integer in 0 .. 2^30 per axis of a
// box), shared by csrc/mesh_simplify.hip and csrc/mesh_smooth.hip so that both quantise with the same instructions.
#pragma once

#include "mesh_grid.h"

namespace pvd {

struct Box {  // per axis: the origin, the extent, whether the axis is flat
    double lo[3], ext[3];
    bool flat[3];
};

PVD_HD Box box_of(const float *__restrict__ bmin3, const float *__restrict__ bmax3) {
    Box b;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        b.lo[a] = (double)bmin3[a];
        b.ext[a] = (double)bmax3[a] - b.lo[a];
        b.flat[a] = !(b.ext[a] > 0.0 && b.ext[a] < (double)INFINITY);  // NaN: flat
    }
    return b;
}

// q_a of a finite coordinate: 0 .. 2^30
PVD_HD int64_t quantise(const Box &b, int a, float x) {
    if (b.flat[a]) return 0;
    const double f = fmin(1.0, fmax(0.0, ((double)x - b.lo[a]) / b.ext[a]));
    return (int64_t)llrint(f * 0x1p30);
}

}  // namespace pvd
