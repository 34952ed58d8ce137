"""The distance from points to a triangle mesh, restated in plain numpy from the definition in include/pvd_hip_mesh_dist.h (not from
the kernel): what csrc/mesh_dist.hip is compared with in tests/test_hip_mesh_dist.py, and what tests/test_mesh_dist_restatement.py
pins first.  Everything is np.longdouble arithmetic on the float32 inputs, as an [N, T] matrix, a block of points at a time.

The closest point of a triangle to p is the foot of p on the triangle's plane where that foot lies inside the triangle, and the
closest point of the three edges otherwise -- so d^2 = min over the three segments, replaced by the plane distance where the foot
is inside (Cramer's rule on the Gram matrix of ab, ac).  That is another route than the kernel's seven regions; the two meet only
in the definition.  A triangle with |n|^2 <= 2^-40 |ab|^2 |ac|^2 is degenerate and is its three segments; a triangle with an index
outside [0, V) or a corner that is not finite is invalid and takes no part.
"""
import functools

import numpy as np

import mesh_normals_restatement as nr
import mesh_restatement as mr

LD = np.longdouble
DEGENERATE = LD(2.0) ** -40
THRESH = 0.125
BMIN, BMAX = (-1.0, -0.5, 0.25), (1.0, 1.5, 2.0)  # the non-cubic box of tests/test_hip_mesh.py


def valid_triangles(vertices, triangles):
    """bool [T]: the three indices are in [0, V) and the nine coordinates are finite."""
    v, t = np.asarray(vertices, np.float32).reshape(-1, 3), np.asarray(triangles, np.int64).reshape(-1, 3)
    ok = np.all((t >= 0) & (t < len(v)), axis=1)
    safe = np.where(ok[:, None], t, 0)
    if len(v):
        ok &= np.all(np.isfinite(v[safe]), axis=(1, 2))
    return ok


def corners(vertices, triangles):
    """(a, b, c) [T',3] longdouble of the valid triangles and their indices [T'] in the original array."""
    v, t = np.asarray(vertices, np.float32).reshape(-1, 3), np.asarray(triangles, np.int64).reshape(-1, 3)
    idx = np.nonzero(valid_triangles(v, t))[0]
    tv = v[t[idx]].astype(LD) if len(idx) else np.zeros((0, 3, 3), LD)
    return tv[:, 0], tv[:, 1], tv[:, 2], idx


def sin2(a, b, c):
    """[T] longdouble: |n|^2 / (|ab|^2 |ac|^2), 0 where a side at a has length 0."""
    ab, ac = b - a, c - a
    n = np.cross(ab, ac)
    den = (ab * ab).sum(-1) * (ac * ac).sum(-1)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(den > 0, (n * n).sum(-1) / den, LD(0))


def _segment_d2(p, a, e):
    """[N,T]: squared distance from p [N,1,3] to the segments a + s e, 0 <= s <= 1 (a, e [1,T,3])."""
    L = (e * e).sum(-1)
    ap = p - a
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.where(L > 0, (ap * e).sum(-1) / np.where(L > 0, L, LD(1)), LD(0))
    s = np.clip(s, LD(0), LD(1))
    r = ap - s[..., None] * e
    return (r * r).sum(-1)


def distance_matrix(points, vertices, triangles, block=32):
    """D [N,T] longdouble: d(p_i, t_j), +inf for an invalid triangle; rows of points that are not finite are NaN."""
    pts = np.asarray(points, np.float32).reshape(-1, 3)
    T = np.asarray(triangles).reshape(-1, 3).shape[0]
    a, b, c, idx = corners(vertices, triangles)
    D = np.full((len(pts), T), np.inf, LD)
    if len(idx):
        ab, ac, bc = (b - a)[None], (c - a)[None], (c - b)[None]
        n = np.cross(ab, ac)
        nn = (n * n).sum(-1)
        g11, g12, g22 = (ab * ab).sum(-1), (ab * ac).sum(-1), (ac * ac).sum(-1)
        flat = nn <= DEGENERATE * g11 * g22
        nn_safe = np.where(flat, LD(1), nn)
        with np.errstate(invalid="ignore", over="ignore"):  # (rows of points that are not finite)
            for s in range(0, len(pts), block):
                p = pts[s:s + block].astype(LD)[:, None, :]
                d2 = np.minimum(np.minimum(_segment_d2(p, a[None], ab), _segment_d2(p, a[None], ac)), _segment_d2(p, b[None], bc))
                ap = p - a[None]
                r1, r2 = (ap * ab).sum(-1), (ap * ac).sum(-1)
                v, w = (g22 * r1 - g12 * r2) / nn_safe, (g11 * r2 - g12 * r1) / nn_safe
                inside = ~flat & (v >= 0) & (w >= 0) & (v + w <= 1)
                h = (ap * n).sum(-1)
                d2 = np.where(inside, h * h / nn_safe, d2)
                D[s:s + block, idx] = np.sqrt(d2)
    D[~np.all(np.isfinite(pts), axis=1)] = np.nan
    return D


def nearest(points, vertices, triangles, max_dist, D=None):
    """(dist [N] longdouble, tri [N] int64) by the result contract: the smallest d over the valid triangles, ties to the smallest
    index; dist = max_dist and tri = -1 where that is not below max_dist (and where no triangle is valid); NaN and -1 for a point
    that is not finite."""
    if D is None:
        D = distance_matrix(points, vertices, triangles)
    N, T = D.shape
    md = LD(np.float32(max_dist))
    dist, tri = np.full(N, md, LD), np.full(N, -1, np.int64)
    bad = np.isnan(D).any(axis=1) if T else ~np.all(np.isfinite(np.asarray(points, np.float32).reshape(-1, 3)), axis=1)
    if T:
        j = np.argmin(np.where(np.isnan(D), np.inf, D), axis=1)  # the first of equal minima: the smallest index
        best = D[np.arange(N), j]
        hit = ~bad & (best < md)
        dist[hit], tri[hit] = best[hit], j[hit]
    dist[bad] = np.nan
    return dist, tri


def spread(points, vertices, triangles, tri):
    """S [N] float64: the largest coordinate difference between the point and the corners of triangle tri (0 for tri == -1)."""
    pts = np.asarray(points, np.float32).reshape(-1, 3).astype(np.float64)
    v, t = np.asarray(vertices, np.float32).reshape(-1, 3).astype(np.float64), np.asarray(triangles, np.int64).reshape(-1, 3)
    tri = np.asarray(tri, np.int64)
    S = np.zeros(len(pts))
    ok = tri >= 0
    if ok.any():
        S[ok] = np.abs(v[t[tri[ok]]] - pts[ok][:, None, :]).max(axis=(1, 2))
    return S


def bound(ref, S):
    """2^-24 ref + 2^-30 S: one float32 rounding of the float64 result, plus the float64 rounding of the differences and the normal
    (relative 2^-53 each, a handful of them) amplified by the worst admitted 1 / sin = 2^18 (test_mesh_dist_restatement.py asserts
    that no fixture has a triangle with 0 < sin^2 < 2^-36): 2^-53 * 2^18 * 2^3 = 2^-32 of the coordinate differences, with margin."""
    return 2.0 ** -24 * np.asarray(ref, np.float64) + 2.0 ** -30 * np.asarray(S, np.float64)


# ------------------------------------------------------------------ the meshes the GPU test queries
FIXTURES = (("sphere", 9), ("sphere", 17), ("torus", 17), ("torus", 33), ("two_spheres", 17), ("smooth", 9), ("smooth", 17))


@functools.lru_cache(maxsize=None)
def fixture(kind, R):
    """(vertices [V,3] f32, triangles [T,3] i32) of the float32 restatement of the mesher on the field `kind` at R^3, read-only."""
    v, t = mr.extract(nr.field(kind, R, THRESH), THRESH, BMIN, BMAX, np.float32)
    v, t = np.ascontiguousarray(v, np.float32), np.ascontiguousarray(t, np.int32)
    v.setflags(write=False), t.setflags(write=False)
    return v, t


def precondition(vertices, triangles):
    """(triangles near the degenerate switch, share of degenerate triangles): the first must be 0 and the second at most 0.01 for
    bound() to hold."""
    a, b, c, idx = corners(vertices, triangles)
    s2 = sin2(a, b, c)
    near = int(((s2 > 0) & (s2 < LD(2.0) ** -36)).sum())
    return near, float((s2 <= DEGENERATE).sum()) / max(len(idx), 1)
