"""The winding number of include/pvd_hip_mesh_winding.h, restated in numpy from the header's text (not from the kernels): float64 from
the float32 inputs, every operation one IEEE operation in the header's order (numpy never fuses), the edge function evaluated from
the lower to the higher vertex index and negated for the other direction, the tie rule, the strict z_hit > pz.  Brute force: every
point against every valid triangle.  What csrc/mesh_winding.hip is compared with, as integers, in tests/test_hip_mesh_winding.py;
pinned by tests/test_mesh_winding_restatement.py."""
import numpy as np

import mesh_dist_restatement as md

INVALID = np.int32(-2 ** 31)  # PVD_MESH_WINDING_INVALID
TOTALS = ("inside", "positive", "leaky_columns", "max_abs")


def _edge(u, w, iu, iw, px, py):
    """The directed edge function of the edge u -> w at (px, py) and the edge's vector (dx, dy): evaluated on the undirected edge
    from the lower to the higher index, negated when the direction is the other one.  u, w [T,3] float64, iu, iw [T]; px, py [N,1]."""
    canon = (iu < iw)[None, :]
    lx, ly = np.where(canon, u[:, 0], w[:, 0]), np.where(canon, u[:, 1], w[:, 1])
    hx, hy = np.where(canon, w[:, 0], u[:, 0]), np.where(canon, w[:, 1], u[:, 1])
    sign = np.where(canon, 1.0, -1.0)
    E = (hx - lx) * (py - ly) - (hy - ly) * (px - lx)
    return sign * E, sign * (hx - lx), sign * (hy - ly)


def _owned(e, dx, dy):
    return (e > 0) | ((e == 0) & ((dy > 0) | ((dy == 0) & (dx < 0))))


def crossings(px, py, vertices, triangles, budget=1 << 21):
    """The (column, triangle) pairs whose triangle covers the column (px, py): (row [P], s [P] in {-1, +1}, z_hit [P] float64).
    px, py [N] float64, all finite."""
    v, t = np.asarray(vertices, np.float32).reshape(-1, 3), np.asarray(triangles, np.int64).reshape(-1, 3)
    idx = np.nonzero(md.valid_triangles(v, t))[0]
    rows, signs, zs = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)], [np.zeros(0, np.float64)]
    if len(idx) and len(px):
        ti = t[idx]
        a, b, c = (v[ti[:, q]].astype(np.float64) for q in range(3))
        ia, ib, ic = ti[:, 0], ti[:, 1], ti[:, 2]
        s = np.sign(_edge(a, b, ia, ib, c[None, :, 0], c[None, :, 1])[0]).reshape(-1)  # [T]: (a, b) at c, per triangle
        block = max(1, budget // len(idx))
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            for n0 in range(0, len(px), block):
                x, y = px[n0:n0 + block, None], py[n0:n0 + block, None]
                cover = np.broadcast_to(s[None, :] != 0, (len(x), len(idx))).copy()
                e = []
                for (u, w, iu, iw) in ((b, c, ib, ic), (c, a, ic, ia), (a, b, ia, ib)):
                    E, dx, dy = _edge(u, w, iu, iw, x, y)
                    E, dx, dy = E * s[None, :], dx * s[None, :], dy * s[None, :]
                    cover &= _owned(E, dx, dy)
                    e.append(E)
                r, k = np.nonzero(cover)
                e_bc, e_ca, e_ab = e[0][r, k], e[1][r, k], e[2][r, k]
                z = ((e_bc * a[k, 2] + e_ca * b[k, 2]) + e_ab * c[k, 2]) / ((e_bc + e_ca) + e_ab)
                rows.append(r + n0), signs.append(s[k].astype(np.int64)), zs.append(z)
    return np.concatenate(rows), np.concatenate(signs), np.concatenate(zs)


def triangle_signs(vertices, triangles):
    """s [T'] of the valid triangles (for the tests): +1 where the normal looks along +z, -1 along -z, 0 edge-on."""
    v, t = np.asarray(vertices, np.float32).reshape(-1, 3), np.asarray(triangles, np.int64).reshape(-1, 3)
    ti = t[md.valid_triangles(v, t)]
    a, b, c = (v[ti[:, q]].astype(np.float64) for q in range(3))
    return np.sign(_edge(a, b, ti[:, 0], ti[:, 1], c[None, :, 0], c[None, :, 1])[0]).reshape(-1)


def winding(points, vertices, triangles):
    """w [N] int32: the winding number of every row of points [N,3] f32; INVALID for a row that is not finite."""
    p = np.asarray(points, np.float32).reshape(-1, 3)
    ok = np.all(np.isfinite(p), axis=1)
    q = p[ok].astype(np.float64)
    rows, s, z = crossings(q[:, 0], q[:, 1], vertices, triangles)
    with np.errstate(invalid="ignore"):
        hit = z > q[rows, 2]
    w = np.full(len(p), INVALID, np.int32)
    w[ok] = np.bincount(rows[hit], weights=s[hit], minlength=len(q)).astype(np.int32)
    return w


def lattice_axes(R, lo, hi):
    """[R,3] f32: (float)i / (float)(R - 1) * (hi_a - lo_a) + lo_a, every operation rounded to float32."""
    lo, hi = np.asarray(lo, np.float32).reshape(3), np.asarray(hi, np.float32).reshape(3)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.arange(R, dtype=np.float32)[:, None] / np.float32(R - 1) * (hi - lo)[None, :] + lo[None, :]


def lattice_points(R, lo, hi):
    """[R^3,3] f32, x-major, z fastest."""
    ax = lattice_axes(R, lo, hi)
    i, j, k = np.meshgrid(np.arange(R), np.arange(R), np.arange(R), indexing="ij")
    return np.stack([ax[i.ravel(), 0], ax[j.ravel(), 1], ax[k.ravel(), 2]], axis=1)


def lattice(vertices, triangles, R, lo, hi):
    """(w [R,R,R] int32, totals dict): the winding number at every point of the lattice, column by column -- the crossings of a
    column once, each compared with the column's R float32 z -- and the four totals of pvd_mesh_winding_lattice: points with
    w != 0, points with w > 0, columns whose crossings do not sum to 0, the largest |w|; points that are not finite are INVALID
    and take no part in the totals."""
    ax = lattice_axes(R, lo, hi)
    i, j = (g.ravel() for g in np.meshgrid(np.arange(R), np.arange(R), indexing="ij"))
    px, py = ax[i, 0], ax[j, 1]
    col_ok = np.isfinite(px) & np.isfinite(py)
    cols = np.nonzero(col_ok)[0]
    rows, s, z = crossings(px[cols].astype(np.float64), py[cols].astype(np.float64), vertices, triangles)
    zk = ax[:, 2].astype(np.float64)
    w = np.zeros((R * R, R), np.int64)
    with np.errstate(invalid="ignore"):
        np.add.at(w, cols[rows], s[:, None] * (zk[None, :] < z[:, None]))
        below = z > -np.inf
    leak = np.bincount(cols[rows[below]], weights=s[below], minlength=R * R)
    ok = col_ok[:, None] & np.isfinite(ax[:, 2])[None, :]
    totals = dict(inside=int((ok & (w != 0)).sum()), positive=int((ok & (w > 0)).sum()), leaky_columns=int((col_ok & (leak != 0)).sum()),
                  max_abs=int(np.abs(np.where(ok, w, 0)).max()))
    return np.where(ok, w, int(INVALID)).astype(np.int32).reshape(R, R, R), totals
