"""tests/mesh_ray_restatement.py -- the numpy restatement of include/pvd_hip_mesh_ray.h that the device is compared with bit for bit --
pinned without a GPU: against an independent long-double Moller-Trumbore, on a hand-made cube where U, V or W is exactly 0, and by
the property the unfused edge functions buy: a ray into a closed mesh cannot slip between two triangles."""
import numpy as np
import pytest

import mesh_dist_restatement as md
import mesh_ray_restatement as rr

LD = np.longdouble


def _moller_trumbore(o, d, vertices, triangles):
    """(t [N,T] longdouble, NaN where missed): the textbook test, another route than the watertight one."""
    v, t = np.asarray(vertices, np.float32).astype(LD), np.asarray(triangles, np.int64)
    a, e1, e2 = v[t[:, 0]][None], (v[t[:, 1]] - v[t[:, 0]])[None], (v[t[:, 2]] - v[t[:, 0]])[None]
    o, d = np.asarray(o, np.float32).astype(LD)[:, None, :], np.asarray(d, np.float32).astype(LD)[:, None, :]
    p = np.cross(d, e2)
    det = (e1 * p).sum(-1)
    with np.errstate(all="ignore"):
        s = o - a
        u = (s * p).sum(-1) / det
        q = np.cross(s, e1)
        w = (d * q).sum(-1) / det
        tt = (e2 * q).sum(-1) / det
        hit = (det != 0) & (u >= 0) & (w >= 0) & (u + w <= 1) & (tt >= 0)
    return np.where(hit, tt, np.nan)


@pytest.mark.parametrize("kind,R", md.FIXTURES)
def test_the_restatement_agrees_with_a_long_double_moller_trumbore(kind, R):
    verts, tris = md.fixture(kind, R)
    rng = np.random.RandomState(7 * R + len(kind))
    pick = rng.permutation(len(tris))[:48]
    centroid = verts[tris[pick]].astype(np.float64).mean(axis=1)
    lo, hi = np.array(md.BMIN), np.array(md.BMAX)
    u = rng.normal(size=(len(pick), 3))
    o = ((lo + hi) / 2 + 3.0 * np.linalg.norm(hi - lo) * u / np.linalg.norm(u, axis=1, keepdims=True)).astype(np.float32)
    d = (centroid - o).astype(np.float32)
    t, tri, bary = rr.first_hit(o, d, verts, tris)
    mt = _moller_trumbore(o, d, verts, tris)
    ref_tri = np.nanargmin(mt, axis=1)
    ref_t = mt[np.arange(len(pick)), ref_tri]
    assert np.all(tri >= 0) and np.array_equal(tri, ref_tri)
    tm = rr.hit_matrix(o, d, verts, tris)[0][np.arange(len(pick)), tri]  # the float64 t before the one rounding
    assert np.all(np.abs(tm.astype(LD) - ref_t) <= LD(2.0) ** -40 * np.abs(ref_t))
    assert np.array_equal(t, tm.astype(np.float32))
    # aimed at the centroid (d = centroid - o, rounded to float32): where that triangle is the first one hit, t is near 1
    own = tri == pick
    assert own.sum() >= len(pick) // 4
    assert np.all(np.abs(t[own] - 1.0) <= 1e-5) and np.all(bary[own] > 0) and np.all(bary[own].sum(axis=1) < 1)


def test_the_hand_made_cube_with_exact_zeros():
    for case, (o, d, t_ref, tri_ref) in enumerate(rr.CUBE_RAYS):
        t, tri, bary = rr.first_hit([o], [d], rr.CUBE_V, rr.CUBE_T)
        assert tri[0] == tri_ref and t[0] == np.float32(t_ref), (o, d, t[0], tri[0])
        tm, vm, wm = rr.hit_matrix([o], [d], rr.CUBE_V, rr.CUBE_T)
        tied = np.nonzero(tm[0] == t_ref)[0]
        # a shared edge or corner: the smallest index wins (the last case lies in the plane of the edge's other face: det == 0 there)
        assert len(tied) >= (2 if case < 6 else 1) and tied.min() == tri_ref, (o, d, tied)
    # the first four cases land on an edge or a corner of triangle 0 or 2: one weight, at least, is exactly 0
    t, tri, bary = rr.first_hit([c[0] for c in rr.CUBE_RAYS], [c[1] for c in rr.CUBE_RAYS], rr.CUBE_V, rr.CUBE_T)
    w = np.concatenate([1.0 - bary.sum(axis=1, keepdims=True), bary], axis=1)
    assert np.all((w == 0).any(axis=1)) and np.all(w >= 0)
    assert bary[0].tolist() == [0.0, 0.25] and bary[3].tolist() == [0.0, 0.0]
    # t_min / t_max: the interval is closed below and open above
    o, d = rr.CUBE_RAYS[0][:2]
    assert rr.first_hit([o], [d], rr.CUBE_V, rr.CUBE_T, t_min=2.0)[1][0] == 0
    t, tri, _ = rr.first_hit([o], [d], rr.CUBE_V, rr.CUBE_T, t_max=2.0)
    assert tri[0] == -1 and t[0] == 2.0
    t, tri, _ = rr.first_hit([o], [d], rr.CUBE_V, rr.CUBE_T, t_min=2.5)
    assert tri[0] == 2 and t[0] == 3.0  # the far face
    # invalid rays
    t, tri, bary = rr.first_hit([o, o, (np.nan, 0, 0), o], [(0, 0, 0), (np.inf, 0, 1), d, d], rr.CUBE_V, rr.CUBE_T)
    assert np.all(np.isnan(t[:3])) and np.all(tri[:3] == -1) and np.all(bary[:3] == 0) and tri[3] == 0


@pytest.mark.parametrize("R", [9, 17])
def test_a_ray_into_a_closed_mesh_does_not_slip_between_triangles(R):
    verts, tris = md.fixture("sphere", R)
    edges = np.sort(np.concatenate([tris[:, [0, 1]], tris[:, [1, 2]], tris[:, [2, 0]]]), axis=1)
    uniq, counts = np.unique(edges, axis=0, return_counts=True)
    assert np.all(counts == 2)  # closed: every edge is used exactly twice
    rng = np.random.RandomState(R)
    n = 648 if R == 9 else 300
    v64 = verts.astype(np.float64)
    targets = np.concatenate([v64[rng.permutation(len(verts))[:n]], v64[uniq[rng.permutation(len(uniq))[:n]]].mean(axis=1),
                              v64[tris[rng.permutation(len(tris))[:n]]].mean(axis=1)])
    lo, hi = np.array(md.BMIN), np.array(md.BMAX)
    centre, L = (lo + hi) / 2, np.linalg.norm(hi - lo)
    u = rng.normal(size=targets.shape)
    o = (centre + 4.0 * L * u / np.linalg.norm(u, axis=1, keepdims=True)).astype(np.float32)
    d = targets - o
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    radial = targets - centre
    cos = (d * radial).sum(axis=1) / (np.linalg.norm(d, axis=1) * np.linalg.norm(radial, axis=1))
    keep = np.abs(cos) >= 0.5
    assert keep.sum() >= len(targets) // 2
    t, tri, _ = rr.first_hit(o[keep], d[keep], verts, tris)
    dist = np.linalg.norm(targets[keep] - o[keep].astype(np.float64), axis=1)
    print("closed sphere R=%d: %d of %d rays kept, %d hit, misses among the others: %d" % (
        R, keep.sum(), len(targets), (tri >= 0).sum(), (rr.first_hit(o[~keep], d[~keep], verts, tris)[1] < 0).sum()))
    assert np.all(tri >= 0)
    assert np.all(t <= dist + 1e-5)
