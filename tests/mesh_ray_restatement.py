"""The first hit of rays on a triangle mesh, restated in plain numpy from the definition in include/pvd_hip_mesh_ray.h (not from the
kernel): what csrc/mesh_ray.hip is compared with, bit for bit, in tests/test_hip_mesh_ray.py, and what
tests/test_mesh_ray_restatement.py pins first.  A dense [N, T] evaluation in float64, a block of rays at a time, every operation in
the header's order.  numpy rounds every product before it adds (it never fuses), so this is the bit-level reference; there is no
grid here, which is what "independent of G and the box" is measured against.
"""
import numpy as np

import mesh_dist_restatement as md

F64 = np.float64


def valid_rays(origins, dirs):
    """bool [N]: six finite numbers and d != 0."""
    o, d = np.asarray(origins, np.float32).reshape(-1, 3), np.asarray(dirs, np.float32).reshape(-1, 3)
    return np.all(np.isfinite(o), axis=1) & np.all(np.isfinite(d), axis=1) & np.any(d != 0, axis=1)


def _ray_constants(o, d):
    """Steps 1 and 2 for valid rays o, d [n,3] float64: (kx, ky, kz [n] int, Sx, Sy, Sz [n])."""
    n = len(o)
    kz = np.argmax(np.abs(d), axis=1)  # the first of equal maxima: the lowest axis
    kx = (kz + 1) % 3
    ky = (kx + 1) % 3
    rows = np.arange(n)
    swap = d[rows, kz] < 0
    kx, ky = np.where(swap, ky, kx), np.where(swap, kx, ky)
    dz = d[rows, kz]
    return kx, ky, kz, d[rows, kx] / dz, d[rows, ky] / dz, 1.0 / dz


def hit_matrix(origins, dirs, vertices, triangles, block=64):
    """(t, v, w) [N,T] float64: step 7's t where steps 5 and 6 do not miss, NaN elsewhere (misses, invalid triangles, invalid rays);
    v = V / det, w = W / det."""
    o32, d32 = np.asarray(origins, np.float32).reshape(-1, 3), np.asarray(dirs, np.float32).reshape(-1, 3)
    N, T = len(o32), np.asarray(triangles).reshape(-1, 3).shape[0]
    tv = np.asarray(vertices, np.float32).reshape(-1, 3)
    tt = np.asarray(triangles, np.int64).reshape(-1, 3)
    idx = np.nonzero(md.valid_triangles(tv, tt))[0]
    out_t, out_v, out_w = (np.full((N, T), np.nan, F64) for _ in range(3))
    ok = valid_rays(o32, d32)
    if not len(idx) or not ok.any():
        return out_t, out_v, out_w
    corners = tv[tt[idx]].astype(F64)  # [T',3 corners,3 axes]
    rays = np.nonzero(ok)[0]
    with np.errstate(all="ignore"):
        for s in range(0, len(rays), block):
            r = rays[s:s + block]
            o, d = o32[r].astype(F64), d32[r].astype(F64)
            kx, ky, kz, Sx, Sy, Sz = _ray_constants(o, d)
            P = corners[None, :, :, :] - o[:, None, None, :]  # [n,T',3,3]
            n = len(r)

            def axis(k):
                return np.take_along_axis(P, np.broadcast_to(k[:, None, None, None], (n, P.shape[1], 3, 1)), axis=3)[..., 0]  # [n,T',3]
            Px, Py, Pz = axis(kx), axis(ky), axis(kz)
            X = Px - Sx[:, None, None] * Pz
            Y = Py - Sy[:, None, None] * Pz
            Z = Sz[:, None, None] * Pz
            Xa, Xb, Xc = X[..., 0], X[..., 1], X[..., 2]
            Ya, Yb, Yc = Y[..., 0], Y[..., 1], Y[..., 2]
            U = Xc * Yb - Yc * Xb
            V = Xa * Yc - Ya * Xc
            W = Xb * Ya - Yb * Xa
            miss = ((U < 0) | (V < 0) | (W < 0)) & ((U > 0) | (V > 0) | (W > 0))
            det = (U + V) + W
            miss |= det == 0
            t = ((U * Z[..., 0] + V * Z[..., 1]) + W * Z[..., 2]) / det
            out_t[np.ix_(r, idx)] = np.where(miss, np.nan, t)
            out_v[np.ix_(r, idx)] = np.where(miss, np.nan, V / det)
            out_w[np.ix_(r, idx)] = np.where(miss, np.nan, W / det)
    return out_t, out_v, out_w


def first_hit(origins, dirs, vertices, triangles, t_min=0.0, t_max=np.inf, M=None):
    """(t [N] f32, tri [N] int32, bary [N,2] f32) by the result contract; M: hit_matrix's output, to share it between calls."""
    o32, d32 = np.asarray(origins, np.float32).reshape(-1, 3), np.asarray(dirs, np.float32).reshape(-1, 3)
    if M is None:
        M = hit_matrix(o32, d32, vertices, triangles)
    tm, vm, wm = M
    N, T = tm.shape
    lo, hi = F64(np.float32(t_min)), F64(np.float32(t_max))
    t = np.full(N, np.float32(t_max), np.float32)
    tri = np.full(N, -1, np.int32)
    bary = np.zeros((N, 2), np.float32)
    if T:
        with np.errstate(invalid="ignore"):
            cand = np.where((tm >= lo) & (tm < hi), tm, np.inf)  # NaN compares false
        j = np.argmin(cand, axis=1)  # the first of equal minima: the smallest index
        rows = np.arange(N)
        hit = cand[rows, j] < np.inf
        with np.errstate(over="ignore"):
            t[hit] = tm[rows, j][hit].astype(np.float32)
            bary[hit, 0] = vm[rows, j][hit].astype(np.float32)
            bary[hit, 1] = wm[rows, j][hit].astype(np.float32)
        tri[hit] = j[hit]
    bad = ~valid_rays(o32, d32)
    t[bad], tri[bad], bary[bad] = np.nan, -1, 0.0
    return t, tri, bary


# ------------------------------------------------------------------ the hand-made cube: coordinates 0 and 1 only
CUBE_V = np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0), (0, 0, 1), (1, 0, 1), (0, 1, 1), (1, 1, 1)], np.float32)
# two triangles per face, outward; the diagonals: z faces 0-3 / 4-7, y faces 0-5 / 2-7, x faces 0-6 / 1-7
CUBE_T = np.array([(0, 2, 3), (0, 3, 1), (4, 5, 7), (4, 7, 6), (0, 1, 5), (0, 5, 4), (2, 6, 7), (2, 7, 3), (0, 4, 6), (0, 6, 2),
                   (1, 3, 7), (1, 7, 5)], np.int32)
# (origin, direction, t, triangle): through the diagonal of the z = 0 face (a shared edge: U, V or W is exactly 0 in both triangles,
# the lower index wins), through the corner (0,0,0) from below (shared by triangles 0 and 1 of that face, and nearer than every other
# face), and along the edge from (0,0,0) to (1,0,0) from x = -1 (the ray lies in the planes y = 0 and z = 0: their triangles have
# det == 0; the face x = 0 is entered at its corner (0,0,0): triangles 8 and 9, t = 1)
CUBE_RAYS = [((0.25, 0.25, -2.0), (0.0, 0.0, 1.0), 2.0, 0),
             ((0.5, 0.5, -1.0), (0.0, 0.0, 2.0), 0.5, 0),
             ((0.75, 0.75, 3.0), (0.0, 0.0, -1.0), 2.0, 2),
             ((0.0, 0.0, -4.0), (0.0, 0.0, 1.0), 4.0, 0),
             ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), 1.0, 0),
             ((-1.0, 0.0, 0.0), (1.0, 0.0, 0.0), 1.0, 8),
             ((0.5, 0.0, -1.0), (0.0, 0.0, 1.0), 1.0, 1)]
