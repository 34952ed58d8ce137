"""pvd_mesh_dist_build / pvd_mesh_dist_query (csrc/mesh_dist.hip, include/pvd_hip_mesh_dist.h) and what pvd/mesh.py builds on them --
mesh_distance, sample_surface, compare_meshes, read_ply -- against the numpy restatement (tests/mesh_dist_restatement.py, pinned by
tests/test_mesh_dist_restatement.py).

Tolerance.  The device evaluates d in float64 and rounds once to float32, so |dist - ref| <= 2^-24 ref + 2^-30 S, S the largest
coordinate difference between the point and the corners of the winning triangle (mesh_dist_restatement.bound: derived, not
measured; its precondition -- no triangle near the degenerate switch -- is asserted on the restated fixtures without a GPU and here
again on the very meshes extract_mesh returns).  The triangle is checked by ref_d(p, tri) <= ref_min + the same bound, not by
equality: adjacent triangles tie on shared edges.  Largest error / bound per case on an MI355X: profiles/mesh_dist_pin.txt.

Sizes.  Meshes: the fixtures of mesh_dist_restatement.FIXTURES through extract_mesh (R = 9, 17, 33; 648 to about 11 000 triangles:
one to 44 workgroups in the per-triangle passes).  N = 1 (one lane), 257 (a second workgroup with one lane) and 1000.  G = 1 (one
cell: brute force, one workgroup in the per-cell passes), 2, 7 (343 cells: a second, partial workgroup) and 32 (128 workgroups of
cells).  The reference matrix is N x T long doubles, so N = 1000 goes with the small meshes."""
import functools
import os

import numpy as np
import pytest
import torch

import mesh_dist_restatement as md
import mesh_normals_restatement as nr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BMIN, BMAX, THRESH = md.BMIN, md.BMAX, md.THRESH
FAR = 100.0  # a max_dist no query of these tests reaches


@functools.lru_cache(maxsize=None)
def _mesh(kind, R):
    """(vertices, triangles) as extract_mesh returns them, as read-only host arrays; the tolerance's precondition holds for them."""
    from pvd.mesh import extract_mesh
    v, t = extract_mesh(torch.from_numpy(np.array(nr.field(kind, R, THRESH))).to(DEV), THRESH, BMIN, BMAX)
    v, t = v.cpu().numpy(), t.cpu().numpy()
    assert np.array_equal(t, md.fixture(kind, R)[1])
    near, degenerate = md.precondition(v, t)
    assert near == 0 and degenerate <= 0.01, (kind, R, near, degenerate)
    v.setflags(write=False), t.setflags(write=False)
    return v, t


def _points(kind, R, which, N):
    """Seeded query points: the mesh's own vertices, those of another fixture, uniform in the box, uniform up to a box length outside."""
    v, _ = _mesh(kind, R)
    rng = np.random.RandomState(1000 * R + N + len(which))
    lo, hi = np.array(BMIN), np.array(BMAX)
    if which == "own":
        p = v[rng.permutation(len(v))[:N]]
    elif which == "other":
        o = _mesh("smooth" if kind != "smooth" else "torus", 17)[0]
        p = o[rng.permutation(len(o))[:N]]
    elif which == "inside":
        p = rng.uniform(lo, hi, (N, 3))
    else:
        p = rng.uniform(lo - (hi - lo), hi + (hi - lo), (N, 3))
    p = np.ascontiguousarray(p, np.float32)
    assert len(p) == N
    return p


@functools.lru_cache(maxsize=None)
def _reference(kind, R, which, N):
    """(points, D [N,T], ref dist, ref tri) -- computed once, read-only."""
    v, t = _mesh(kind, R)
    p = _points(kind, R, which, N)
    D = md.distance_matrix(p, v, t)
    dist, tri = md.nearest(p, v, t, FAR, D)
    for a in (p, D, dist, tri):
        a.setflags(write=False)
    return p, D, dist, tri


def _query(points, verts, tris, max_dist=FAR, G=None, bmin=BMIN, bmax=BMAX):
    from pvd.mesh import mesh_distance
    d, t = mesh_distance(torch.from_numpy(np.array(points, np.float32)).reshape(-1, 3).to(DEV), torch.from_numpy(np.array(verts)).to(DEV),
                         torch.from_numpy(np.array(tris)).to(DEV), max_dist, bmin, bmax, G)
    assert d.dtype == torch.float32 and t.dtype == torch.int32 and d.is_cuda and t.is_cuda and d.shape == t.shape == (len(points),)
    return d.cpu().numpy(), t.cpu().numpy()


def _compare(label, points, verts, tris, dist, tri, D, ref):
    """dist within the bound of ref; the triangle returned is, by the reference, within the bound of the nearest."""
    assert np.all(np.isfinite(dist)) and np.all(tri >= 0) and np.all(tri < len(tris)), label
    ref = ref.astype(np.float64)
    S = md.spread(points, verts, tris, tri)
    bound = md.bound(ref, S)
    err = np.abs(dist.astype(np.float64) - ref)
    own = D[np.arange(len(points)), tri].astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    print("mesh dist pin %s: T=%d N=%d, largest error %.3g, largest error / bound %.4f, largest ref %.4g"
          % (label, len(tris), len(points), err.max(), ratio.max(), ref.max()))
    assert np.all(err <= bound), (label, float(ratio.max()))
    assert np.all(own <= ref + bound), label


# ------------------------------------------------------------------------------------------------------------------ one triangle
def test_one_triangle_in_all_seven_regions():
    verts = np.array([(0.0, 0.0, 0.0), (2.0, 0.0, 0.0), (0.0, 1.0, 0.0)], np.float32)
    tris = np.array([[0, 1, 2]], np.int32)
    pts = np.array([(0.5, 0.25, 0.75), (0.5, 0.25, -0.75), (0.5, 0.25, 0.0),  # above, below, on the plane inside
                    (1.0, -0.5, 0.0), (1.0, -0.3, 0.4), (-0.25, 0.5, 0.0), (-0.3, 0.5, -0.4), (2.0, 1.0, 0.0), (1.5, 1.5, 2.0),  # edges
                    (-3.0, -4.0, 0.0), (-1.0, -2.0, 2.0), (5.0, -4.0, 0.0), (3.0, -0.5, -1.0), (-1.0, 3.0, 2.0), (0.5, 3.0, 0.0),  # corners
                    (0.0, 0.0, 0.0), (2.0, 0.0, 0.0), (0.0, 1.0, 0.0), (1.0, 0.0, 0.0), (1.0, 0.5, 0.0)], np.float32)
    D = md.distance_matrix(pts, verts, tris)
    ref, _ = md.nearest(pts, verts, tris, FAR, D)
    dist, tri = _query(pts, verts, tris, G=1, bmin=(0.0, 0.0, 0.0), bmax=(2.0, 1.0, 1.0))
    assert np.all(tri == 0)
    _compare("one triangle", pts, verts, tris, dist, tri, D, ref)
    assert np.all(dist[[2, 15, 16, 17, 18, 19]] == 0)  # on the plane, a corner passed as a point, on an edge: exactly 0
    assert dist[0] == 0.75 and dist[1] == 0.75 and dist[3] == 0.5 and dist[9] == 5.0 and dist[11] == 5.0 and dist[13] == 3.0
    for G, lo, hi in ((3, (0.0, 0.0, 0.0), (2.0, 1.0, 1.0)), (8, (-1.0, -1.0, -1.0), (3.0, 3.0, 3.0)), (4, (0.0, 0.0, 0.0), (2.0, 1.0, 0.0))):
        d2, t2 = _query(pts, verts, tris, G=G, bmin=lo, bmax=hi)  # (the last box is flat along z)
        assert d2.tobytes() == dist.tobytes() and t2.tobytes() == tri.tobytes(), G
    # a repeated corner and three collinear corners are their segments
    flat = np.array([(0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (2.0, 0.0, 0.0)], np.float32)
    for tr in ([[0, 2, 2]], [[0, 1, 2]], [[1, 0, 2]]):
        d3, _ = _query(pts, flat, np.array(tr, np.int32), G=1)
        r3, _ = md.nearest(pts, flat, np.array(tr, np.int32), FAR)
        assert np.all(np.abs(d3 - r3.astype(np.float64)) <= md.bound(r3, 5.0)), tr


# ------------------------------------------------------------------------------------------------------------------------ meshes
CASES = [("sphere", 9, "own", 257), ("sphere", 9, "inside", 1000), ("sphere", 9, "outside", 1000), ("sphere", 17, "other", 257),
         ("sphere", 17, "inside", 1), ("torus", 17, "own", 257), ("torus", 17, "outside", 257), ("torus", 33, "inside", 257),
         ("torus", 33, "own", 257), ("two_spheres", 17, "other", 257), ("two_spheres", 17, "outside", 1), ("smooth", 9, "other", 1000),
         ("smooth", 17, "own", 257), ("smooth", 17, "inside", 257)]


@pytest.mark.parametrize("kind,R,which,N", CASES)
def test_the_distance_is_the_restatements(kind, R, which, N):
    verts, tris = _mesh(kind, R)
    p, D, ref, _ = _reference(kind, R, which, N)
    dist, tri = _query(p, verts, tris, G=None if which != "outside" else 7)  # (None: the default rule of the mesh's T)
    _compare("%s R=%d %s" % (kind, R, which), p, verts, tris, dist, tri, D, ref)
    if which == "own":
        assert np.all(dist == 0)  # a corner of a triangle is at distance exactly 0 from it
    # the box defaults to the bounding box of the vertices: another box, the same bits
    from pvd.mesh import mesh_distance
    d2, t2 = mesh_distance(torch.from_numpy(np.array(p)).to(DEV), torch.from_numpy(np.array(verts)).to(DEV),
                           torch.from_numpy(np.array(tris)).to(DEV), FAR)
    assert d2.cpu().numpy().tobytes() == dist.tobytes() and t2.cpu().numpy().tobytes() == tri.tobytes()


def _centroid_cells(verts, tris, G, bmin=BMIN, bmax=BMAX):
    """The x-major cell index of every triangle's centroid in the G^3 grid over the box, as include/pvd_hip_mesh_dist.h bins it."""
    lo, hi = np.array(bmin, np.float64), np.array(bmax, np.float64)
    m = verts.astype(np.float64)[tris].sum(axis=1) / 3.0
    k = np.clip(np.floor((m - lo) * (G / (hi - lo))), 0, G - 1).astype(np.int64)
    return (k[:, 0] * G + k[:, 1]) * G + k[:, 2]


def test_the_scan_of_the_cell_counts_carries_into_a_second_chunk():
    """G = 129: 2 146 689 cells are 8386 per-workgroup sums, one chunk of 8192 and a second one that starts from the first one's
    carry; every cell from index 8192 * 256 on has its start from that carry.  The cell index is x-major, so that cell lies in the
    x-layer 126 of 129: in the box of the other tests the sphere (x = -0.6 .. 0.6 of -1 .. 1) stays below it, so this box is the same one
    stretched to x = -30, which puts x = 0 into that layer.  The reference does not depend on the box."""
    G, lo, hi = 129, (-30.0,) + BMIN[1:], (0.7,) + BMAX[1:]
    assert 8192 < -(-G ** 3 // 256) <= 2 * 8192
    verts, tris = _mesh("sphere", 9)
    cells = _centroid_cells(verts, tris, G, lo, hi)
    assert (cells < 8192 * 256).sum() > 100 and (cells >= 8192 * 256).sum() > 100  # triangles on both sides of the chunk boundary
    p, D, ref, _ = _reference("sphere", 9, "own", 257)
    dist, tri = _query(p, verts, tris, G=G, bmin=lo, bmax=hi)
    _compare("sphere R=9 own, G=129", p, verts, tris, dist, tri, D, ref)
    d7, t7 = _query(p, verts, tris, G=7, bmin=lo, bmax=hi)
    assert dist.tobytes() == d7.tobytes() and tri.tobytes() == t7.tobytes()


# ------------------------------------------------------------------------------------------------------------- grid independence
def _grid_independent(label, points, verts, tris, boxes, reference=None):
    base = None
    for lo, hi in boxes:
        for G in (1, 2, 7, 32):
            for run in range(2 if G == 7 else 1):
                d, t = _query(points, verts, tris, G=G, bmin=lo, bmax=hi)
                base = base or (d, t)
                assert d.tobytes() == base[0].tobytes() and t.tobytes() == base[1].tobytes(), (label, G, lo, hi, run)
    if reference is not None:
        _compare(label, points, verts, tris, base[0], base[1], *reference)
    return base


def test_the_result_does_not_depend_on_the_grid_or_the_box():
    verts, tris = _mesh("torus", 17)
    p, D, ref, _ = _reference("torus", 17, "outside", 257)
    squashed = (tuple(a * s for a, s in zip(BMIN, (1, 1, 0.01))), tuple(a * s for a, s in zip(BMAX, (1, 1, 0.01))))
    boxes = [(BMIN, BMAX),
             ((0.1, 0.6, 1.0), (0.2, 0.7, 1.1)),  # much smaller than the mesh: most centroids are clamped into border cells
             squashed,                             # very unequal extents: h_min is a hundredth of the other two
             ((5.0, 5.0, 5.0), (6.0, 6.0, 6.0)),   # away from the mesh altogether: every centroid in one corner cell
             ((-1.0, -0.5, 0.25), (1.0, -0.5, 0.0))]  # one flat axis and one of negative extent
    _grid_independent("torus R=17, five boxes", p, verts, tris, boxes, (D, ref))


def test_one_triangle_spanning_the_box_next_to_thousands_of_small_ones():
    """rho is as large as the box: the bound r h_min - rho stays negative for most rings, and the big triangle -- binned by its
    centroid, far from most of the points it is nearest to -- must still be found."""
    v0, t0 = _mesh("sphere", 17)
    big = np.array([(-1.0, -0.5, 0.3), (1.0, 1.5, 0.3), (1.0, -0.5, 1.9)], np.float32)
    verts = np.concatenate([v0, big])
    tris = np.concatenate([t0, np.array([[len(v0), len(v0) + 1, len(v0) + 2]], np.int32)])
    p = _points("sphere", 17, "inside", 257)
    D = md.distance_matrix(p, verts, tris)
    ref, rt = md.nearest(p, verts, tris, FAR, D)
    assert 20 < (rt == len(t0)).sum() < 237  # the big one wins for a good share of the points, not for all
    d, t = _grid_independent("sphere R=17 + one big triangle", p, verts, tris, [(BMIN, BMAX)], (D, ref))
    assert ((t == len(t0)) == (rt == len(t0))).mean() > 0.98


# -------------------------------------------------------------------------------------------------------------------- saturation
def test_max_dist_saturates_and_changes_nothing_below_it():
    verts, tris = _mesh("smooth", 17)
    p = _points("smooth", 17, "outside", 257)
    full_d, full_t = _query(p, verts, tris)
    m = float(np.median(full_d))
    below = full_d < np.float32(m)
    assert 100 < below.sum() < 157
    for G in (1, 7, 32):
        d, t = _query(p, verts, tris, max_dist=m, G=G)
        assert d[below].tobytes() == full_d[below].tobytes() and t[below].tobytes() == full_t[below].tobytes(), G
        assert np.all(d[~below] == np.float32(m)) and np.all(t[~below] == -1), G  # at max_dist exactly: saturated too
    d, t = _query(p, verts, tris[:0], max_dist=0.25)
    assert np.all(d == np.float32(0.25)) and np.all(t == -1)  # no triangles
    d, t = _query(p, verts[:0], tris, max_dist=0.25, bmin=BMIN, bmax=BMAX)
    assert np.all(d == np.float32(0.25)) and np.all(t == -1)  # no vertices: every triangle is invalid


# ----------------------------------------------------------------------------------------------------------------- invalid input
def test_invalid_triangles_and_points_and_rows_past_n():
    import pvd_hip
    v0, t0 = _mesh("sphere", 9)
    p = _points("sphere", 9, "inside", 257).copy()
    clean_d, clean_t = _query(p, v0, t0)
    verts = np.concatenate([v0, np.array([(np.nan, 0.0, 1.0), (0.0, np.inf, 1.0)], np.float32)])
    V = len(verts)
    planted = np.array([[0, 1, len(v0)], [len(v0) + 1, 2, 3], [0, 1, V], [0, -1, 2], [-2 ** 31, 1, 2], [2 ** 31 - 1, 1, 2]], np.int32)
    where = [0, 100, 100, 300, len(t0), len(t0)]
    tris = np.insert(t0, where, planted, axis=0)
    keep = np.ones(len(tris), bool)
    keep[np.array(where) + np.arange(len(where))] = False
    assert np.array_equal(tris[keep], t0) and md.valid_triangles(verts, tris).tolist() == keep.tolist()
    original = np.nonzero(keep)[0]  # index in the new array of every original triangle
    for G in (1, 7):
        d, t = _query(p, verts, tris, G=G)
        assert d.tobytes() == clean_d.tobytes() and np.array_equal(t, original[clean_t]), G
    # points that are not finite: (NaN, -1), and their neighbours are untouched
    p[3, 1], p[200, 0], p[256, 2] = np.nan, np.inf, -np.inf
    d, t = _query(p, v0, t0)
    bad = np.zeros(257, bool)
    bad[[3, 200, 256]] = True
    assert np.all(np.isnan(d[bad])) and np.all(t[bad] == -1)
    assert d[~bad].tobytes() == clean_d[~bad].tobytes() and t[~bad].tobytes() == clean_t[~bad].tobytes()
    # rows past N are never written
    vt, tt = torch.from_numpy(np.array(v0)).to(DEV), torch.from_numpy(np.array(t0)).to(DEV)
    T, G = len(t0), 7
    ws = torch.empty(pvd_hip.mesh_dist_workspace_bytes(T, G), dtype=torch.uint8, device=DEV)
    lo, hi = torch.tensor(BMIN, device=DEV), torch.tensor(BMAX, device=DEV)
    pvd_hip.mesh_dist_build(vt, tt, lo, hi, G, ws)
    pts = torch.from_numpy(_points("sphere", 9, "inside", 257)).to(DEV)
    dist, tri = torch.full((257,), 7.0, device=DEV), torch.full((257,), -7, dtype=torch.int32, device=DEV)
    pvd_hip.mesh_dist_query(pts[:100], T, G, ws, FAR, dist[:100], tri[:100])
    assert bool((dist[100:] == 7.0).all()) and bool((tri[100:] == -7).all())
    assert dist[:100].cpu().numpy().tobytes() == clean_d[:100].tobytes() and tri[:100].cpu().numpy().tobytes() == clean_t[:100].tobytes()
    pvd_hip.mesh_dist_query(pts[:0], T, G, ws, FAR, dist[:0], tri[:0])  # N == 0: PVD_OK, no launch
    for args in ((pts, T, G, ws[:-1], FAR, dist, tri), (pts, T, G, ws, 0.0, dist, tri), (pts, T, G, ws, float("nan"), dist, tri),
                 (pts, T, G, ws, FAR, dist[:100], tri), (pts.double(), T, G, ws, FAR, dist, tri), (pts, T, G, ws[1:], FAR, dist, tri)):
        with pytest.raises(pvd_hip.PvdHipError):
            pvd_hip.mesh_dist_query(*args)
    with pytest.raises(pvd_hip.PvdHipError):
        pvd_hip.mesh_dist_build(vt, tt.long(), lo, hi, G, ws)
    with pytest.raises(pvd_hip.PvdHipError):
        pvd_hip.mesh_dist_build(vt.reshape(-1), tt, lo, hi, G, ws)


# --------------------------------------------------------------------------------------------------------------- compare_meshes
def _analytic_sphere(radius, R=33):
    """The analytic density of tests/test_hip_mesh.py (sigma = 2 on the sphere around (0.1, -0.05, 0)), meshed at R^3."""
    from pvd.mesh import density_field, extract_mesh
    centre = torch.tensor([0.1, -0.05, 0.0], device=DEV)
    u = density_field(lambda x: 2.0 + 5.0 * (radius - torch.linalg.norm(x - centre, dim=1)), R, (-1.0,) * 3, (1.0,) * 3,
                      device=torch.device(DEV))
    return extract_mesh(u, 2.0, (-1.0,) * 3, (1.0,) * 3)


def test_compare_meshes():
    from pvd.mesh import compare_meshes, mesh_distance
    h = 2.0 / 32
    va, ta = _analytic_sphere(0.4)
    vb, tb = _analytic_sphere(0.45)
    keys = ["a_to_b", "b_to_a", "chamfer", "fscore", "hausdorff", "n_a", "n_b", "precision", "recall", "saturated_a", "saturated_b"]
    same = compare_meshes(va, ta, va, ta, tau=1e-6)
    assert sorted(same) == keys
    assert same["a_to_b"] == 0 and same["b_to_a"] == 0 and same["chamfer"] == 0 and same["hausdorff"] == 0
    assert same["precision"] == 1 and same["recall"] == 1 and same["fscore"] == 1 and same["saturated_a"] == 0
    assert same["n_a"] == same["n_b"] == va.shape[0]
    r = compare_meshes(va, ta, vb, tb, tau=0.05)
    print("compare_meshes spheres 0.4 / 0.45 at R=33: %s" % r)
    assert abs(r["a_to_b"] - 0.05) <= h and abs(r["b_to_a"] - 0.05) <= h
    assert r["chamfer"] == r["a_to_b"] + r["b_to_a"] and r["hausdorff"] >= max(r["a_to_b"], r["b_to_a"])
    assert r["n_a"] == va.shape[0] and r["n_b"] == vb.shape[0] and r["saturated_a"] == 0 and r["saturated_b"] == 0
    lo, hi = compare_meshes(va, ta, vb, tb, tau=0.05 - h), compare_meshes(va, ta, vb, tb, tau=0.05 + h)
    assert lo["precision"] == 0 and lo["recall"] == 0 and lo["fscore"] == 0
    assert hi["precision"] == 1 and hi["recall"] == 1 and hi["fscore"] == 1
    s = compare_meshes(vb, tb, va, ta, tau=0.05)
    assert (s["a_to_b"], s["b_to_a"], s["precision"], s["recall"], s["n_a"]) == (r["b_to_a"], r["a_to_b"], r["recall"], r["precision"], r["n_b"])
    assert s["chamfer"] == r["chamfer"] and s["hausdorff"] == r["hausdorff"]
    # the same reductions in numpy float64 on mesh_distance's own output
    md_ = float(np.linalg.norm(np.maximum(va.max(0).values.cpu().numpy(), vb.max(0).values.cpu().numpy()).astype(np.float64)
                               - np.minimum(va.min(0).values.cpu().numpy(), vb.min(0).values.cpu().numpy()).astype(np.float64)))
    dab = mesh_distance(va, vb, tb, md_)[0].cpu().numpy().astype(np.float64)
    dba = mesh_distance(vb, va, ta, md_)[0].cpu().numpy().astype(np.float64)
    assert np.isclose(r["a_to_b"], dab.mean(), rtol=1e-12) and np.isclose(r["b_to_a"], dba.mean(), rtol=1e-12)
    assert r["hausdorff"] == max(dab.max(), dba.max())
    assert r["precision"] == (dab <= 0.05).mean() and r["recall"] == (dba <= 0.05).mean()
    # a max_dist below the gap saturates every row; a point that is not finite is left out of the means and counted
    sat = compare_meshes(va, ta, vb, tb, tau=0.05, max_dist=0.01)
    assert sat["saturated_a"] == sat["n_a"] and sat["saturated_b"] == sat["n_b"] and np.isclose(sat["a_to_b"], 0.01) and sat["precision"] == 0
    va2 = va.clone()
    va2[5, 0] = float("nan")
    nan = compare_meshes(va2, ta, vb, tb, tau=0.05)
    keep = np.ones(len(dab), bool)
    keep[5] = False
    assert nan["saturated_a"] == 1 and np.isclose(nan["a_to_b"], dab[keep].mean(), rtol=1e-12) and np.isfinite(nan["b_to_a"])
    # with surface samples
    sm = compare_meshes(va, ta, vb, tb, tau=0.05 + h, samples=2000, seed=3)
    assert sm["n_a"] == 2000 and sm["n_b"] == 2000 and abs(sm["a_to_b"] - 0.05) <= h and sm["fscore"] == 1
    assert sm == compare_meshes(va, ta, vb, tb, tau=0.05 + h, samples=2000, seed=3)


# --------------------------------------------------------------------------------------------------------------- sample_surface
def test_sample_surface():
    from pvd.mesh import sample_surface
    verts, tris = _mesh("torus", 17)
    vt, tt = torch.from_numpy(np.array(verts)).to(DEV), torch.from_numpy(np.array(tris)).to(DEV)
    s = sample_surface(vt, tt, 1000, seed=11)
    assert s.shape == (1000, 3) and s.dtype == torch.float32 and s.is_cuda
    assert s.cpu().numpy().tobytes() == sample_surface(vt, tt, 1000, seed=11).cpu().numpy().tobytes()
    assert s.cpu().numpy().tobytes() != sample_surface(vt, tt, 1000, seed=12).cpu().numpy().tobytes()
    # every sample lies on its mesh: a float64 combination of three corners rounded to float32 is within 2^-24 of its coordinates
    # (at most 2 here) of the triangle, next to the distance's own bound at ref = 0
    d, t = _query(s.cpu().numpy(), verts, tris)
    S = md.spread(s.cpu().numpy(), verts, tris, t)
    assert np.all(d <= 2.0 ** -24 * 2.0 * np.sqrt(3.0) + md.bound(0.0, S)), float(d.max())
    # two triangles of areas 1 : 3, next to one of area 0, an invalid one and one with a NaN corner
    v = torch.tensor([(0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, 2.0, 0.0), (5.0, 0.0, 0.0), (8.0, 0.0, 0.0), (5.0, 2.0, 0.0),
                      (float("nan"), 0.0, 0.0)], device=DEV)
    t = torch.tensor([[0, 1, 1], [0, 1, 2], [0, 1, 7], [3, 4, 5], [0, 1, 6], [3, 3, 3]], dtype=torch.int32, device=DEV)
    n = 4096
    s = sample_surface(v, t, n, seed=0).cpu().numpy()
    first, second = (s[:, 0] <= 1.0).sum(), (s[:, 0] >= 5.0).sum()
    assert first + second == n and np.all(s[:, 2] == 0) and np.all(s[:, 1] >= 0)
    sd = np.sqrt(n * 0.25 * 0.75)
    print("sample_surface 1:3: %d of %d in the smaller triangle, expected %.0f +- %.1f" % (first, n, n * 0.25, sd))
    assert abs(first - n * 0.25) <= 5 * sd
    assert np.all(s[s[:, 0] <= 1.0][:, 1] <= 2.0 * (1.0 - s[s[:, 0] <= 1.0][:, 0]) + 1e-6)  # inside the first triangle
    assert sample_surface(v, t[:1], 10, seed=0).shape == (0, 3) and sample_surface(v, t[:0], 10, seed=0).shape == (0, 3)


# --------------------------------------------------------------------------------------------------------------------- read_ply
def test_read_ply_round_trips_all_four_layouts(tmp_path):
    from pvd.mesh import extract_mesh, read_ply, write_ply
    v, t, n = extract_mesh(torch.from_numpy(np.array(nr.field("two_spheres", 17, THRESH))).to(DEV), THRESH, BMIN, BMAX, with_normals=True)
    c = (0.5 + 0.3 * n + 0.1 * torch.sin(v)).clamp(0.0, 1.0)
    for name, kw in (("plain", {}), ("n", {"normals": n}), ("c", {"colors": c}), ("full", {"normals": n, "colors": c})):
        path = write_ply(os.path.join(str(tmp_path), name + ".ply"), v, t, **kw)
        v2, t2, n2, c2 = read_ply(path)
        assert v2.dtype == torch.float32 and t2.dtype == torch.int32 and not v2.is_cuda
        assert v2.numpy().tobytes() == v.cpu().numpy().tobytes() and torch.equal(t2, t.cpu())
        assert (n2 is None) == ("normals" not in kw) and (c2 is None) == ("colors" not in kw)
        if n2 is not None:
            assert n2.numpy().tobytes() == n.cpu().numpy().tobytes()
        if c2 is not None:
            assert torch.equal(torch.round(c2 * 255), torch.round(c.cpu() * 255)) and float(c2.min()) >= 0 and float(c2.max()) <= 1
        again = write_ply(os.path.join(str(tmp_path), name + "_again.ply"), v2, t2, normals=n2, colors=c2)
        assert open(again, "rb").read() == open(path, "rb").read()  # bit for bit
    with pytest.raises(ValueError):
        read_ply(__file__)
