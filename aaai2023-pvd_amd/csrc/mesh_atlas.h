// mesh_atlas.h -- the addressing of the per-triangle texture atlas of include/pvd_hip_mesh_tex.h, once: the four texels around the
// (tri, bary) of a ray cast, their two weights and the bilinear blend, which the flat lookup (k_mt_sample, csrc/mesh_tex.hip) and the
// view-dependent one (k_st_sample<L>, csrc/mesh_shtex.hip) share.  Every float operation is a single float32 one in the order of the
// header; nothing is fused (the build's -ffp-contract=off, and the pragmas below for a build without it).
#pragma once

#include "mesh_grid.h"

namespace pvd {
namespace atlas {

struct __attribute__((packed, aligned(4))) F3 {  // three floats moved as one 12-byte access
    float x, y, z;
};

PVD_HD float mix3(float wa, float wb, float wc, float a, float b, float c) {
#pragma clang fp contract(off)
    return (wa * a + wb * b) + wc * c;
}

// The point X and the normal N of the texel (p, q) of triangle f at the cell edge S ("Weights", "Point", "Normal", "Invalid" of the
// header): six NaNs for an invalid triangle.  f < T is the caller's; k_mt_points and k_ax_points (csrc/mesh_atex.hip) share this.
__device__ __forceinline__ void texel_point(const float *__restrict__ vertices, uint32_t V, const int32_t *__restrict__ triangles,
                                            const float *__restrict__ normals, uint32_t f, uint32_t p, uint32_t q, uint32_t S, F3 &X,
                                            F3 &N) {
#pragma clang fp contract(off)
    const float nan = u2f(0x7fc00000u);
    X = {nan, nan, nan};
    N = {nan, nan, nan};
    const int32_t ia = triangles[3 * (size_t)f], ib = triangles[3 * (size_t)f + 1], ic = triangles[3 * (size_t)f + 2];
    if (!((uint32_t)ia < V && (uint32_t)ib < V && (uint32_t)ic < V)) return;  // a negative index is a large unsigned one
    const float *pa = vertices + 3 * (size_t)ia, *pb = vertices + 3 * (size_t)ib, *pc = vertices + 3 * (size_t)ic;
    const float ax = pa[0], ay = pa[1], az = pa[2], bx = pb[0], by = pb[1], bz = pb[2], gx = pc[0], gy = pc[1], gz = pc[2];
    bool ok = finite3(ax, ay, az) && finite3(bx, by, bz) && finite3(gx, gy, gz);
    const float m = (float)(S - 3);
    const float beta = (float)p / m, gamma = (float)q / m;
    const float alpha = (1.0f - beta) - gamma;
    float nx, ny, nz;
    if (normals) {
        const float *na = normals + 3 * (size_t)ia, *nb = normals + 3 * (size_t)ib, *nc = normals + 3 * (size_t)ic;
        const float a0 = na[0], a1 = na[1], a2 = na[2], b0 = nb[0], b1 = nb[1], b2 = nb[2], c0 = nc[0], c1 = nc[1], c2 = nc[2];
        ok = ok && finite3(a0, a1, a2) && finite3(b0, b1, b2) && finite3(c0, c1, c2);
        nx = mix3(alpha, beta, gamma, a0, b0, c0);
        ny = mix3(alpha, beta, gamma, a1, b1, c1);
        nz = mix3(alpha, beta, gamma, a2, b2, c2);
    } else {
        const float ux = bx - ax, uy = by - ay, uz = bz - az, vx = gx - ax, vy = gy - ay, vz = gz - az;
        nx = uy * vz - uz * vy;
        ny = uz * vx - ux * vz;
        nz = ux * vy - uy * vx;
    }
    if (ok) {
        X = {mix3(alpha, beta, gamma, ax, bx, gx), mix3(alpha, beta, gamma, ay, by, gy), mix3(alpha, beta, gamma, az, bz, gz)};
        N = {nx, ny, nz};
    }
}

// fu, i0, tx of the header from one weight
__device__ __forceinline__ void texel_of(float w, uint32_t mi, uint32_t &i0, float &t) {
#pragma clang fp contract(off)
    const float m = (float)mi;
    const float fu = fminf(fmaxf(w * m, 0.0f), m);  // fmaxf(NaN, 0) = 0
    const int fl = (int)floorf(fu);                 // 0 .. m
    i0 = (uint32_t)(fl < (int)mi ? fl : (int)mi);
    t = fu - (float)i0;
}

struct Footprint {  // the texels (xa, ya), (xb, ya), (xa, yb), (xb, yb) of the atlas and the weights of the b side
    uint32_t xa, xb, ya, yb;
    float tx, ty;
};

// triangle f at (beta, gamma) on an atlas of C cells of S texels per row
__device__ __forceinline__ Footprint footprint_of(uint32_t f, float beta, float gamma, uint32_t S, uint32_t C) {
    Footprint p;
    uint32_t i0, j0;
    texel_of(beta, S - 3, i0, p.tx);
    texel_of(gamma, S - 3, j0, p.ty);
    const uint32_t k = f >> 1, cy = k / C, cx = k - cy * C;
    const bool odd = (f & 1u) != 0;
    // 0 <= i0, j0 <= S - 3: the four texels have 0 <= p, q <= S - 2 and stay inside the cell (cx, cy), so inside [Ht, Wt]
    p.xa = cx * S + (odd ? S - 1 - i0 : i0);
    p.xb = cx * S + (odd ? S - 2 - i0 : i0 + 1);
    p.ya = cy * S + (odd ? S - 1 - j0 : j0);
    p.yb = cy * S + (odd ? S - 2 - j0 : j0 + 1);
    return p;
}

__device__ __forceinline__ F3 blend(const F3 &c00, const F3 &c10, const F3 &c01, const F3 &c11, const Footprint &p) {
#pragma clang fp contract(off)
    const float tx = p.tx, ty = p.ty, sx = 1.0f - tx, sy = 1.0f - ty;
    return {(c00.x * sx + c10.x * tx) * sy + (c01.x * sx + c11.x * tx) * ty,
            (c00.y * sx + c10.y * tx) * sy + (c01.y * sx + c11.y * tx) * ty,
            (c00.z * sx + c10.z * tx) * sy + (c01.z * sx + c11.z * tx) * ty};
}

}  // namespace atlas
}  // namespace pvd
