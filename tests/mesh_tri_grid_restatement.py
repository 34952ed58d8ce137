"""The triangle grid of csrc/mesh_tri_grid.h restated in numpy, float64: the "Grid" paragraph of include/pvd_hip_mesh_ray.h (axes = 3)
and of include/pvd_hip_mesh_winding.h (axes = 2: x and y).  Every operation is in the kernel's order -- inv_h = G / e_a, then
(x - bmin_a) * inv_h -- so what the device leaves in its workspace is compared exactly, without a tolerance, up to the order of the
pairs inside a cell and of the outside list.

    valid     all three indices in [0, V) and all nine coordinates finite
    FLAT      an axis whose extent e_a = bmax_a - bmin_a (float64 of the float32 bounds) is not a positive finite number: k_a = 0
    k_a(x)    clamp(floor((x - bmin_a) * (G / e_a)), 0, G - 1)
    INSIDE    bmin_a <= min_a and max_a <= bmax_a on every axis that is not flat; every other valid triangle is OUTSIDE
    range     k_a(min_a - eps_a) .. k_a(max_a + eps_a) with eps_a = 2^-20 e_a, min_a / max_a over the float32 corners
    cell      x-major, the last binned axis fastest
    record    twelve 32-bit words per triangle: the nine coordinates in input order (zeros where an index is out of range: there is
              nothing to read), the triangle's index or 0xffffffff for an invalid one, the edge directions for two axes -- bit 0: b < c,
              bit 1: c < a, bit 2: a < b, of a triangle whose indices are in range -- or 0 for three, and 0.
"""
import numpy as np

INVALID, INSIDE, OUTSIDE = 0, 1, 2


def box_of(bmin, bmax, G, axes):
    """Per binned axis: (flat, lo, hi, inv_h, eps), float64."""
    lo, hi = np.asarray(bmin, np.float32).astype(np.float64)[:axes], np.asarray(bmax, np.float32).astype(np.float64)[:axes]
    with np.errstate(all="ignore"):
        ext = hi - lo
        ok = (ext > 0.0) & (ext < np.inf)  # false for NaN
        safe = np.where(ok, ext, 1.0)
        return ~ok, np.where(ok, lo, 0.0), np.where(ok, hi, 0.0), np.where(ok, float(G) / safe, 0.0), np.where(ok, 2.0 ** -20 * safe, 0.0)


def cell_axis(x, lo, inv_h, G):
    """k_a(x) for float64 x (any shape): NaN and everything below 1 -> 0."""
    with np.errstate(all="ignore"):
        v = (np.asarray(x, np.float64) - lo) * inv_h
        return np.where(v >= 1.0, np.minimum(v, float(G - 1)), 0.0).astype(np.int64)


def classify(vertices, triangles, bmin, bmax, G, axes):
    """(cls [T], k0 [T,axes], k1 [T,axes], in_range [T]): the class of every triangle and, where it is INSIDE, its range of cells;
    in_range: the three indices lie in [0, V)."""
    v, t = np.asarray(vertices, np.float32).reshape(-1, 3), np.asarray(triangles, np.int64).reshape(-1, 3)
    T, V = len(t), len(v)
    in_range = ((t >= 0) & (t < V)).all(axis=1)
    c = np.zeros((T, 3, 3), np.float32)
    c[in_range] = v[t[in_range]]
    valid = in_range & np.isfinite(c).all(axis=(1, 2))
    flat, lo, hi, inv_h, eps = box_of(bmin, bmax, G, axes)
    with np.errstate(all="ignore"):
        mn, mx = c.min(axis=1).astype(np.float64)[:, :axes], c.max(axis=1).astype(np.float64)[:, :axes]
        inside = (flat | ((lo <= mn) & (mx <= hi))).all(axis=1)
        k0, k1 = cell_axis(mn - eps, lo, inv_h, G), cell_axis(mx + eps, lo, inv_h, G)
    cls = np.where(valid, np.where(inside, INSIDE, OUTSIDE), INVALID)
    return cls, k0, k1, in_range


def records(vertices, triangles, cls, in_range, axes):
    """uint32 [T,12]: the packed records."""
    v, t = np.asarray(vertices, np.float32).reshape(-1, 3), np.asarray(triangles, np.int64).reshape(-1, 3)
    T = len(t)
    c = np.zeros((T, 9), np.float32)
    c[in_range] = v[t[in_range]].reshape(-1, 9)
    out = np.zeros((T, 12), np.uint32)
    out[:, :9] = c.view(np.uint32)
    out[:, 9] = np.where(cls == INVALID, 0xFFFFFFFF, np.arange(T)).astype(np.uint32)
    if axes == 2:
        a, b, cc = t[:, 0], t[:, 1], t[:, 2]
        out[:, 10] = np.where(in_range, (b < cc) * 1 + (cc < a) * 2 + (a < b) * 4, 0).astype(np.uint32)
    return out


def grid(vertices, triangles, bmin, bmax, G, axes):
    """dict: cells -- G^axes sorted lists of triangle indices; outside -- the sorted outside list; pairs, n_outside -- the two totals of
    the count pass; records -- uint32 [T,12]."""
    assert axes in (2, 3) and G >= 1
    cls, k0, k1, in_range = classify(vertices, triangles, bmin, bmax, G, axes)
    cells = [[] for _ in range(G ** axes)]
    for t in np.nonzero(cls == INSIDE)[0]:  # ascending: every list comes out sorted
        ranges = [range(int(k0[t, a]), int(k1[t, a]) + 1) for a in range(axes)]
        for x in ranges[0]:
            for y in ranges[1]:
                for z in (ranges[2] if axes == 3 else (None,)):
                    cells[x * G + y if z is None else (x * G + y) * G + z].append(int(t))
    outside = np.nonzero(cls == OUTSIDE)[0].astype(np.uint32)
    return {"cells": cells, "outside": outside, "pairs": sum(len(c) for c in cells), "n_outside": len(outside),
            "records": records(vertices, triangles, cls, in_range, axes)}
