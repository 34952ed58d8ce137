"""tests/mesh_winding_restatement.py -- the winding number of include/pvd_hip_mesh_winding.h in numpy -- pinned: against the fields the
meshes were extracted from (a closed extracted mesh has w == 1 exactly where the field is above the threshold, although EVERY crossing
of a lattice column is a tie, marching-tetrahedra vertices sitting on lattice edges), against itself along another axis, and by the
properties the header promises (order, orientation, invalid triangles, a ray through an edge or a vertex counted once).  No GPU."""
import functools

import numpy as np
import pytest

import mesh_dist_restatement as md
import mesh_normals_restatement as nr
import mesh_restatement as mr
import mesh_winding_restatement as wr

BMIN, BMAX, THRESH = md.BMIN, md.BMAX, md.THRESH
CLOSED = (("sphere", 9), ("sphere", 17), ("torus", 17), ("torus", 33), ("two_spheres", 17), ("far_spheres", 17))


def bordered(u, thresh=THRESH, layers=1):
    """The field with its six border layers set outside (0): the mesh of it is closed inside the box."""
    u = np.array(u, np.float32)
    for a in range(3):
        idx = [slice(None)] * 3
        for side in (slice(0, layers), slice(u.shape[a] - layers, None)):
            idx[a] = side
            u[tuple(idx)] = 0.0
    return u


@functools.lru_cache(maxsize=None)
def _mesh(kind, R):
    """(field, vertices, triangles), read-only; kind "smooth_bordered": the smooth field with its border set outside."""
    u = bordered(nr.field("smooth", R, THRESH)) if kind == "smooth_bordered" else nr.field(kind, R, THRESH)
    v, t = mr.extract(u, THRESH, BMIN, BMAX, np.float32)
    v, t = np.ascontiguousarray(v, np.float32), np.ascontiguousarray(t, np.int32)
    for a in (u, v, t):
        a.setflags(write=False)
    return u, v, t


@pytest.mark.parametrize("kind,R", CLOSED + (("smooth_bordered", 9), ("smooth_bordered", 17)))
def test_a_closed_extracted_mesh_winds_once_exactly_where_the_field_is_inside(kind, R):
    u, v, t = _mesh(kind, R)
    margin = float(np.abs(u.astype(np.float64) - np.float32(THRESH)).min())
    assert margin > 1e-5, margin  # the precondition: no lattice value at the threshold, where the mesher and the rule may differ
    w, totals = wr.lattice(v, t, R, BMIN, BMAX)
    inside = u > np.float32(THRESH)
    ax = wr.lattice_axes(R, BMIN, BMAX).astype(np.float64)
    rows, s, z = wr.crossings(np.repeat(ax[:, 0], R), np.tile(ax[:, 1], R), v, t)
    print("winding restatement %s R=%d: T=%d, %d inside, margin %.3g, %d crossings, totals %r" % (kind, R, len(t), inside.sum(), margin, len(rows), totals))
    assert np.array_equal(w == 1, inside) and np.array_equal(w != 0, inside)  # 0 mismatches
    assert totals == dict(inside=int(inside.sum()), positive=int(inside.sum()), leaky_columns=0, max_abs=1)
    assert len(rows) >= 2 * np.unique(rows).size > 0  # a covered column is entered and left


def test_every_crossing_of_a_lattice_column_is_a_tie():
    """The inputs above exercise the tie rule, they do not avoid it: the lattice points lie on the projected edges of the mesh."""
    u, v, t = _mesh("sphere", 9)
    ax = wr.lattice_axes(9, BMIN, BMAX).astype(np.float64)
    px, py = np.repeat(ax[:, 0], 9), np.tile(ax[:, 1], 9)
    rows, s, z = wr.crossings(px, py, v, t)
    a, b, c = (v[t[:, q]].astype(np.float64) for q in range(3))
    ties = 0
    # count the (column, triangle) pairs with an edge function that is exactly 0, over all pairs
    for (p, q, ip, iq) in ((b, c, t[:, 1], t[:, 2]), (c, a, t[:, 2], t[:, 0]), (a, b, t[:, 0], t[:, 1])):
        E = wr._edge(p, q, ip.astype(np.int64), iq.astype(np.int64), px[:, None], py[:, None])[0]
        ties += int((E == 0).sum())
    assert ties > 1000 and len(rows) > 0, ties


@pytest.mark.parametrize("R", (9, 17))
def test_an_open_mesh_leaks(R):
    u, v, t = _mesh("smooth", R)
    w, totals = wr.lattice(v, t, R, BMIN, BMAX)
    print("winding restatement smooth R=%d, open at the box: %d points differ from the field, w in %d .. %d, totals %r"
          % (R, ((w != 0) != (u > np.float32(THRESH))).sum(), w.min(), w.max(), totals))
    assert totals["leaky_columns"] > 0 and ((w != 0) != (u > np.float32(THRESH))).any()


def _seeded_points(v, n, seed):
    rng = np.random.RandomState(seed)
    lo, hi = np.array(BMIN), np.array(BMAX)
    return rng.uniform(lo - 0.05 * (hi - lo), hi + 0.05 * (hi - lo), (n, 3)).astype(np.float32)


@pytest.mark.parametrize("kind,R", (("sphere", 9), ("torus", 17), ("two_spheres", 17), ("smooth_bordered", 9)))
def test_the_ray_along_z_agrees_with_the_ray_along_x_away_from_the_surface(kind, R):
    """The same code on cyclically permuted coordinates is the winding number along +x."""
    _, v, t = _mesh(kind, R)
    p = _seeded_points(v, 300, R + len(kind))
    far = np.asarray(md.nearest(p, v, t, 10.0)[0], np.float64) > 1e-6
    wz, wx = wr.winding(p, v, t), wr.winding(p[:, [1, 2, 0]], v[:, [1, 2, 0]], t)
    print("winding restatement %s R=%d: %d of %d points further than 1e-6 from the surface, %d inside" % (kind, R, far.sum(), len(p), (wz[far] != 0).sum()))
    assert far.sum() > 250 and (wz[far] != 0).any() and (wz[far] == 0).any()
    assert np.array_equal(wz[far], wx[far])


def test_order_orientation_and_invalid_triangles():
    _, v, t = _mesh("torus", 17)
    p = np.concatenate([_seeded_points(v, 200, 5), v[::40], ((v[t[::60, 0]].astype(np.float64) + v[t[::60, 1]]) / 2).astype(np.float32)])
    w = wr.winding(p, v, t)
    assert (w == 1).sum() > 10 and (w == 0).sum() > 10
    rng = np.random.RandomState(3)
    assert np.array_equal(wr.winding(p, v, t[rng.permutation(len(t))]), w)  # the order of the triangles
    assert np.array_equal(wr.winding(p, v, t[:, [1, 2, 0]]), w) and np.array_equal(wr.winding(p, v, t[:, [2, 0, 1]]), w)  # a rotation
    mixed = np.where((np.arange(len(t)) % 3)[:, None] == 0, t, np.where((np.arange(len(t)) % 3)[:, None] == 1, t[:, [1, 2, 0]], t[:, [2, 0, 1]]))
    assert np.array_equal(wr.winding(p, v, mixed), w)
    assert np.array_equal(wr.winding(p, v, t[:, ::-1]), -w)  # every triangle reversed
    assert np.array_equal(wr.winding(p, v, np.concatenate([t, t])), 2 * w)  # the mesh twice over
    v2 = np.concatenate([v, np.array([[np.nan, 0.0, 0.0], [0.0, np.inf, 0.0]], np.float32)])
    bad = np.array([[0, 1, len(v2)], [-1, 0, 1], [0, 1, len(v)], [len(v) + 1, 2, 3], [0, 0, 1]], np.int32)  # (the last: no area)
    assert np.array_equal(wr.winding(p, v2, np.concatenate([bad[:2], t, bad[2:]])), w)
    q = np.array(p[:4])
    q[0, 0], q[1, 1], q[2, 2] = np.nan, np.inf, -np.inf
    assert np.array_equal(wr.winding(q, v, t), [wr.INVALID, wr.INVALID, wr.INVALID, w[3]])
    assert np.array_equal(wr.winding(p, v, t[:0]), np.zeros(len(p), np.int32))


@pytest.mark.parametrize("kind,R", (("sphere", 9), ("torus", 17), ("two_spheres", 17)))
def test_a_ray_through_a_vertex_or_an_edge_is_counted_once(kind, R):
    """Below the whole mesh the crossings of a closed mesh sum to 0, and above a point the sum is that of a ray moved off the edge by
    (+1e-7, +1e-9): every vertex and edge midpoint is counted once, not zero or two times."""
    _, v, t = _mesh(kind, R)
    mid = ((v[t[:, 0]].astype(np.float64) + v[t[:, 1]].astype(np.float64)) / 2).astype(np.float32)
    p = np.concatenate([v, mid[::3]])
    p[:, 2] = BMIN[2] - 1.0  # from below everything: all crossings of the column
    moved = p.astype(np.float64) + np.array([1e-7, 1e-9, 0.0])
    rows, s, z = wr.crossings(p[:, 0].astype(np.float64), p[:, 1].astype(np.float64), v, t)
    rows_m, s_m, z_m = wr.crossings(moved[:, 0], moved[:, 1], v, t)
    total, total_m = np.bincount(rows, weights=s, minlength=len(p)), np.bincount(rows_m, weights=s_m, minlength=len(p))
    assert np.array_equal(total, total_m) and not total.any()
    # and level by level: the crossings above any height, at heights between the lattice layers
    for zq in np.linspace(BMIN[2], BMAX[2], 7)[1:-1] + 0.0123:
        up = np.bincount(rows[z > zq], weights=s[z > zq], minlength=len(p))
        up_m = np.bincount(rows_m[z_m > zq], weights=s_m[z_m > zq], minlength=len(p))
        away = np.ones(len(p), bool)
        for r_, z_ in ((rows, z), (rows_m, z_m)):  # leave out the columns with a crossing within 1e-5 of this height
            away[r_[np.abs(z_ - zq) < 1e-5]] = False
        assert away.sum() > len(p) // 2 and np.array_equal(up[away], up_m[away])
        assert set(np.unique(up[away])) <= {0.0, 1.0}


def test_the_lattice_is_the_points_query_on_the_lattices_points():
    for kind, R, Rl, lo, hi in (("sphere", 9, 20, (-1.1, -0.6, 0.16), (1.1, 1.6, 2.09)), ("smooth", 9, 9, BMIN, BMAX), ("torus", 17, 12, BMAX, BMIN)):
        _, v, t = _mesh(kind, R)
        w, totals = wr.lattice(v, t, Rl, lo, hi)
        ref = wr.winding(wr.lattice_points(Rl, lo, hi), v, t).reshape(Rl, Rl, Rl)
        assert np.array_equal(w, ref) and (w != 0).any(), (kind, Rl)
        assert totals["inside"] == (ref != 0).sum() and totals["positive"] == (ref > 0).sum() and totals["max_abs"] == np.abs(ref).max()
    w, totals = wr.lattice(v, t, 5, (0.0, 0.0, 0.0), (np.inf, 1.0, 1.0))  # a lattice that is not finite: INVALID, no totals
    assert (w == wr.INVALID).all() and totals == dict(inside=0, positive=0, leaky_columns=0, max_abs=0)
