// mesh_ray_walk.h -- what the first-hit cast (csrc/mesh_ray.hip) and the any-hit exposure query (csrc/mesh_expose.hip) share: the
// ray's constants, steps 3 .. 7 of the watertight test in unfused float64 and the walk over the grid (include/pvd_hip_mesh_ray.h:
// "Walk").  The layout of the workspace pvd_mesh_ray_build leaves and the box are those of csrc/mesh_tri_grid.h, three axes.
// The two differ in what they do with a triangle that is not missed and in when they stop; the walk takes that as a visitor:
//     void test(const float4 *packed, uint32_t j)   record j against the ray
//     bool found() const                            nothing more needs testing (the any-hit query: a hit is held; the cast: never)
//     bool settled(double t_exit) const             the walk may stop before the cell behind t_exit
// Everything is defined here (the library is built without relocatable device code): each translation unit gets its own copy.
#pragma once

#include "mesh_tri_grid.h"

namespace pvd {
namespace mray {

using Box = tgrid::Box<3>;  // the grid of pvd_mesh_ray_build: csrc/mesh_tri_grid.h with three binned axes

// the pure parts (the test, the walk) are PVD_HD, __host__ __device__: a CPU build can walk the same code
PVD_HD float sel3(float x, float y, float z, int k) { return k == 0 ? x : (k == 1 ? y : z); }

// ------------------------------------------------------------------------------------------- the watertight test, in float64
struct Ray {  // the ray's constants, once per lane: the permuted origin, the shear, the permutation
    double ox, oy, oz, Sx, Sy, Sz;
    int kx, ky, kz;
};

PVD_HD Ray ray_of(const double o[3], const double d[3]) {
    Ray r;
    const double ax = fabs(d[0]), ay = fabs(d[1]), az = fabs(d[2]);
    r.kz = ax >= ay && ax >= az ? 0 : (ay >= az ? 1 : 2);  // argmax |d|, ties to the lowest axis
    r.kx = (r.kz + 1) % 3;
    r.ky = (r.kx + 1) % 3;
    const double dz = r.kz == 0 ? d[0] : (r.kz == 1 ? d[1] : d[2]);
    if (dz < 0.0) {
        const int s = r.kx;
        r.kx = r.ky;
        r.ky = s;
    }
    const double dx = r.kx == 0 ? d[0] : (r.kx == 1 ? d[1] : d[2]), dy = r.ky == 0 ? d[0] : (r.ky == 1 ? d[1] : d[2]);
    r.Sx = dx / dz;
    r.Sy = dy / dz;
    r.Sz = 1.0 / dz;
    r.ox = r.kx == 0 ? o[0] : (r.kx == 1 ? o[1] : o[2]);
    r.oy = r.ky == 0 ? o[0] : (r.ky == 1 ? o[1] : o[2]);
    r.oz = r.kz == 0 ? o[0] : (r.kz == 1 ? o[1] : o[2]);
    return r;
}

struct Crossing {  // a triangle that steps 5 and 6 do not miss: step 7's t, and V, W, det for the weights
    double t, V, W, det;
};

// the corners q0, q1, q2 of a packed record against the ray: include/pvd_hip_mesh_ray.h, steps 3 .. 7; false: a miss
PVD_HD bool crossing(const float4 q0, const float4 q1, const float4 q2, const Ray &r, Crossing &x) {
#pragma clang fp contract(off)
    const double Ax = (double)sel3(q0.x, q0.y, q0.z, r.kx) - r.ox, Ay = (double)sel3(q0.x, q0.y, q0.z, r.ky) - r.oy;
    const double Az = (double)sel3(q0.x, q0.y, q0.z, r.kz) - r.oz;
    const double Bx = (double)sel3(q0.w, q1.x, q1.y, r.kx) - r.ox, By = (double)sel3(q0.w, q1.x, q1.y, r.ky) - r.oy;
    const double Bz = (double)sel3(q0.w, q1.x, q1.y, r.kz) - r.oz;
    const double Cx = (double)sel3(q1.z, q1.w, q2.x, r.kx) - r.ox, Cy = (double)sel3(q1.z, q1.w, q2.x, r.ky) - r.oy;
    const double Cz = (double)sel3(q1.z, q1.w, q2.x, r.kz) - r.oz;
    const double Xa = Ax - r.Sx * Az, Ya = Ay - r.Sy * Az;
    const double Xb = Bx - r.Sx * Bz, Yb = By - r.Sy * Bz;
    const double Xc = Cx - r.Sx * Cz, Yc = Cy - r.Sy * Cz;
    const double U = Xc * Yb - Yc * Xb, V = Xa * Yc - Ya * Xc, W = Xb * Ya - Yb * Xa;
    if ((U < 0.0 || V < 0.0 || W < 0.0) && (U > 0.0 || V > 0.0 || W > 0.0)) return false;
    const double det = (U + V) + W;
    if (det == 0.0) return false;
    const double Za = r.Sz * Az, Zb = r.Sz * Bz, Zc = r.Sz * Cz;
    x.t = ((U * Za + V * Zb) + W * Zc) / det;
    x.V = V;
    x.W = W;
    x.det = det;
    return true;
}

// the search of one valid ray over [t_min, t_max): clip, walk, outside list; far rays test everything
template <typename Visitor>
PVD_HD void walk(const double o[3], const double d[3], uint32_t T, uint32_t G, const uint32_t *__restrict__ header,
                 const uint32_t *__restrict__ start, const uint32_t *__restrict__ list, const uint32_t *__restrict__ outside,
                 const float4 *__restrict__ packed, uint32_t pairs, double t_min, double t_max, Visitor &vis) {
    const Box box = tgrid::box_of<3>((const float *)(header + 1), (const float *)(header + 4), G);
    // every index below is clamped: a damaged workspace stays inside itself
    const uint32_t n_pairs = umin(header[7], pairs), n_out = umin(header[0], T);
    // (1) clip to the dilated slabs
    double t0 = t_min, t1 = t_max, inv_d[3];
    bool touches = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        inv_d[a] = 0.0;
        if (box.flat[a]) continue;
        const double e4 = 0.25 * box.eps[a];
        if (d[a] == 0.0) {
            if (o[a] < box.lo[a] - e4 || o[a] > box.hi[a] + e4) touches = false;
            continue;
        }
        inv_d[a] = 1.0 / d[a];
        const double ta = ((box.lo[a] - e4) - o[a]) * inv_d[a], tb = ((box.hi[a] + e4) - o[a]) * inv_d[a];
        t0 = fmax(t0, fmin(ta, tb));
        t1 = fmin(t1, fmax(ta, tb));
    }
    touches = touches && t0 <= t1;
    if (touches) {  // far rays: the rounding of a position is no longer small against eps
        bool far = false;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            if (box.flat[a]) continue;
            double M = fabs(o[a]) + fabs(box.lo[a]) + fabs(box.hi[a]);
            if (d[a] != 0.0) M += fabs(d[a]) * t1;  // t1 is finite here: this axis has clipped it
            if (!(0x1p-40 * M <= box.eps[a])) far = true;
        }
        if (far) {
            for (uint32_t j = 0; j < T && !vis.found(); ++j) vis.test(packed, j);
            return;
        }
        // (2) the start cell
        int k[3], step[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            k[a] = box.flat[a] ? 0 : cell_axis(box, a, o[a] + t0 * d[a], G);
            step[a] = (box.flat[a] || d[a] == 0.0) ? 0 : (d[a] > 0.0 ? 1 : -1);
        }
        for (uint32_t it = 0; it < 3u * G; ++it) {  // at most 3 (G - 1) steps
            // (3) the cell's triangles
            const uint32_t c = ((uint32_t)k[0] * G + (uint32_t)k[1]) * G + (uint32_t)k[2];
            const uint32_t s1 = umin(start[c + 1], n_pairs);
            for (uint32_t s = umin(start[c], n_pairs); s < s1 && !vis.found(); ++s) {
                const uint32_t j = list[s];
                if (j < T) vis.test(packed, j);
            }
            // (4) the exit, from the integer face
            double t_exit = (double)INFINITY;
            int axis = -1;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                if (step[a] == 0) continue;
                const double face = box.lo[a] + (double)(k[a] + (step[a] > 0 ? 1 : 0)) * box.h[a];
                const double te = (face - o[a]) * inv_d[a];
                if (te < t_exit) {
                    t_exit = te;
                    axis = a;
                }
            }
            // (5) stop or step
            if (axis < 0 || !(t_exit < t1)) break;
            if (vis.settled(t_exit)) break;
            k[axis] += step[axis];
            if (k[axis] < 0 || k[axis] >= (int)G) break;
        }
    }
    // (6) the outside list
    for (uint32_t s = 0; s < n_out && !vis.found(); ++s) {
        const uint32_t j = outside[s];
        if (j < T) vis.test(packed, j);
    }
}

}  // namespace mray
}  // namespace pvd
