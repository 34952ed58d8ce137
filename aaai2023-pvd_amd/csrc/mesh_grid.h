// mesh_grid.h -- the small pure helpers the mesh kernels share: bit casts, finiteness, the cell of a coordinate in a uniform grid
// over a box.  Each file keeps its own Box (they hold different things); cell_axis reads lo and inv_h of whichever it is given.
#pragma once

#include "pvd_device.h"

namespace pvd {

// the pure parts are __host__ __device__: a CPU build can walk the same code
#define PVD_HD __host__ __device__ __forceinline__

PVD_HD float u2f(uint32_t u) { return __builtin_bit_cast(float, u); }
PVD_HD uint32_t f2u(float f) { return __builtin_bit_cast(uint32_t, f); }
PVD_HD uint32_t umin(uint32_t a, uint32_t b) { return a < b ? a : b; }

PVD_HD bool finite1(float x) { return fabsf(x) < INFINITY; }  // false for NaN
PVD_HD bool finite3(float x, float y, float z) {
    return fabsf(x) < INFINITY && fabsf(y) < INFINITY && fabsf(z) < INFINITY;  // false for NaN
}

// the cell coordinate of x along axis a of a grid of G cells per axis: one monotone function of x, so that whatever is binned and
// whatever is looked up agree on it
template <typename B>
PVD_HD int cell_axis(const B &b, int a, double x, uint32_t G) {
    const double v = (x - b.lo[a]) * b.inv_h[a];
    return v >= 1.0 ? (int)fmin(v, (double)(G - 1)) : 0;  // NaN and everything below 1 -> 0; a flat axis (inv_h 0) -> 0
}

}  // namespace pvd
