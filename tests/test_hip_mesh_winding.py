"""pvd_mesh_winding_count / _build / _points / _lattice (csrc/mesh_winding.hip, include/pvd_hip_mesh_winding.h) and what pvd/mesh.py builds
on them -- mesh_winding, mesh_contains, voxelize_mesh, mesh_signed_distance, mesh_to_sdf, compare_meshes(volume=R) -- against the numpy
restatement (tests/mesh_winding_restatement.py, pinned by tests/test_mesh_winding_restatement.py).

Tolerance.  None: a winding number is a sum of +-1 decided by comparisons of float64 numbers that the device and numpy compute by the
same unfused operations in the same order, so the int32 results are compared for equality.  A difference means a fused or reordered
operation in the kernel, a triangle the grid did not offer to a point, or a column's scan gone wrong.

Sizes.  Meshes: the fixtures of mesh_dist_restatement.FIXTURES through extract_mesh (R = 9, 17, 33; 648 to about 12 000 triangles: one
to 47 workgroups in the per-triangle passes).  N = 1 (one lane), 257 (a second workgroup with one lane) and 1000.  G = 1 (one cell:
brute force), 2, 7 (49 cells) and 32 (1024 cells: four workgroups in the per-cell passes).  Lattices: R' = 2 (the smallest), the
extraction lattice itself (every column through vertices and edges: ties only), R' = 20 over a larger box (no power of two: the
float32 lattice coordinates round; 400 columns: 25 workgroups of 16 columns), R' = 65 and 130 (columns longer than one and two
waves, each with a partial chunk)."""
import functools

import numpy as np
import pytest
import torch

import mesh_dist_restatement as md
import mesh_normals_restatement as nr
import mesh_winding_restatement as wr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BMIN, BMAX, THRESH = md.BMIN, md.BMAX, md.THRESH
BIGGER = (tuple(a - 0.05 * (b - a) for a, b in zip(BMIN, BMAX)), tuple(b + 0.05 * (b - a) for a, b in zip(BMIN, BMAX)))  # 10 % larger
CLOSED = tuple(f for f in md.FIXTURES if f[0] != "smooth")


def _dev(a, dt):
    return torch.from_numpy(np.array(a, dt)).to(DEV)


def _bordered(u):
    """The field with its six border layers set outside: its mesh is closed."""
    u = np.array(u, np.float32)
    u[0], u[-1], u[:, 0], u[:, -1], u[:, :, 0], u[:, :, -1] = 0, 0, 0, 0, 0, 0
    return u


@functools.lru_cache(maxsize=None)
def _mesh(kind, R):
    """(field, vertices, triangles) as extract_mesh returns them, as read-only host arrays; "smooth_bordered": closed."""
    from pvd.mesh import extract_mesh
    u = _bordered(nr.field("smooth", R, THRESH)) if kind == "smooth_bordered" else np.array(nr.field(kind, R, THRESH))
    v, t = extract_mesh(torch.from_numpy(u).to(DEV), THRESH, BMIN, BMAX)
    v, t = v.cpu().numpy(), t.cpu().numpy()
    if kind != "smooth_bordered":
        assert np.array_equal(t, md.fixture(kind, R)[1])
    for a in (u, v, t):
        a.setflags(write=False)
    return u, v, t


def points_of(verts, tris, N, seed):
    """[N,3] f32, a seeded mix: points in and around the box, exact copies of vertices, edge midpoints, points outside the box, rows
    that are not finite.  N = 1: one point of the box."""
    rng = np.random.RandomState(seed)
    lo, hi = np.array(BMIN), np.array(BMAX)
    if N < 100:
        return rng.uniform(lo + 0.3 * (hi - lo), hi - 0.3 * (hi - lo), (N, 3)).astype(np.float32)
    n_v, n_m, n_out, n_bad = N // 8, N // 8, N // 16, 6
    around = rng.uniform(lo - 0.05 * (hi - lo), hi + 0.05 * (hi - lo), (N - n_v - n_m - n_out - n_bad, 3))
    copies = verts[rng.randint(0, len(verts), n_v)].astype(np.float64)
    copies[::2, 2] -= rng.uniform(0.0, 0.5, len(copies[::2]))  # half of them below their vertex: the ray passes through it
    e = tris[rng.randint(0, len(tris), n_m)]
    mids = (verts[e[:, 0]].astype(np.float64) + verts[e[:, 1]].astype(np.float64)) / 2
    mids[::2, 2] -= rng.uniform(0.0, 0.5, len(mids[::2]))
    out = rng.uniform(lo, hi, (n_out, 3)) + np.where(rng.rand(n_out, 3) < 0.4, 1.0, 0.0) * (hi - lo) * rng.choice([-1.5, 1.5], (n_out, 3))
    bad = rng.uniform(lo, hi, (n_bad, 3))
    bad[0, 0], bad[1, 1], bad[2, 2], bad[3, 0], bad[4, 1], bad[5] = np.nan, np.nan, np.nan, np.inf, -np.inf, np.nan
    p = np.concatenate([around, copies, mids, out, bad]).astype(np.float32)
    return np.ascontiguousarray(p[rng.permutation(len(p))])


@functools.lru_cache(maxsize=None)
def _reference(kind, R, N):
    """(points, w) -- computed once, read-only."""
    _, v, t = _mesh(kind, R)
    p = points_of(v, t, N, 1000 * R + N + len(kind))
    w = wr.winding(p, v, t)
    p.setflags(write=False), w.setflags(write=False)
    return p, w


@functools.lru_cache(maxsize=None)
def _reference_lattice(kind, R, Rl, box):
    _, v, t = _mesh(kind, R)
    w, totals = wr.lattice(v, t, Rl, *box)
    w.setflags(write=False)
    return w, totals


def _winding(p, verts, tris, G=None, bmin=None, bmax=None):
    from pvd.mesh import mesh_winding
    w = mesh_winding(_dev(p, np.float32).reshape(-1, 3), _dev(verts, np.float32), _dev(tris, np.int32), bmin, bmax, G)
    assert w.dtype == torch.int32 and w.is_cuda and w.shape == (len(np.asarray(p).reshape(-1, 3)),)
    return w.cpu().numpy()


def _same(got, ref, label):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.dtype == np.int32 and got.shape == ref.shape, label
    if not np.array_equal(got, ref):
        bad = np.nonzero((got != ref).reshape(-1))[0]
        raise AssertionError("%s: differs at %d of %d, first %d: %d against %d" % (label, len(bad), got.size, bad[0], got.reshape(-1)[bad[0]],
                                                                                    ref.reshape(-1)[bad[0]]))


# ---------------------------------------------------------------------------------------------------------------------- points
@pytest.mark.parametrize("N", (1, 257, 1000))
@pytest.mark.parametrize("kind,R", md.FIXTURES)
def test_the_winding_number_of_points_is_the_restatements(kind, R, N):
    _, verts, tris = _mesh(kind, R)
    p, ref = _reference(kind, R, N)
    print("mesh winding %s R=%d: T=%d N=%d, %d inside, %d invalid, values %r" % (kind, R, len(tris), N, ((ref != 0) & (ref != wr.INVALID)).sum(),
                                                                                   (ref == wr.INVALID).sum(), np.unique(ref).tolist()))
    if N > 1:
        assert (ref == wr.INVALID).sum() == 6 and (ref == 0).sum() > N // 8 and ((ref != 0) & (ref != wr.INVALID)).sum() > N // 50
    for G in (None, 1, 2, 7, 32):  # the default box: the bounding box of the vertices
        _same(_winding(p, verts, tris, G), ref, "%s R=%d N=%d G=%r" % (kind, R, N, G))
    lo, hi = verts.min(axis=0), verts.max(axis=0)
    small = (lo + 0.3 * (hi - lo), hi - 0.25 * (hi - lo))  # smaller than the mesh: most triangles are on the outside list
    flat = (BMIN, (BMAX[0], BMIN[1], BMAX[2]))  # flat along y: one layer of cells there
    for G in (2, 7):
        _same(_winding(p, verts, tris, G, *small), ref, "%s R=%d N=%d G=%d, a box smaller than the mesh" % (kind, R, N, G))
        _same(_winding(p, verts, tris, G, *flat), ref, "%s R=%d N=%d G=%d, a flat box" % (kind, R, N, G))
    _same(_winding(p, verts, tris, 7, BMIN, BMAX), ref, "%s R=%d N=%d, the extraction box" % (kind, R, N))


def test_mesh_contains_and_the_outside_list_is_used():
    import pvd_hip
    from pvd.mesh import mesh_contains
    _, verts, tris = _mesh("torus", 17)
    p, ref = _reference("torus", 17, 1000)
    got = mesh_contains(_dev(p, np.float32), _dev(verts, np.float32), _dev(tris, np.int32))
    assert got.dtype == torch.bool and np.array_equal(got.cpu().numpy(), (ref != 0) & (ref != wr.INVALID))
    lo, hi = verts.min(axis=0), verts.max(axis=0)
    totals = torch.zeros(2, dtype=torch.int64, device=DEV)
    pvd_hip.mesh_winding_count(_dev(verts, np.float32), _dev(tris, np.int32), _dev(lo + 0.3 * (hi - lo), np.float32), _dev(hi - 0.25 * (hi - lo), np.float32),
                               7, totals)
    pairs, outside = totals.tolist()
    assert 0 < outside < len(tris) and pairs > 0, (pairs, outside)


# --------------------------------------------------------------------------------------------------------------------- lattice
LATTICES = ([(k, R, R, (BMIN, BMAX)) for k, R in md.FIXTURES] + [(k, R, 2, (BMIN, BMAX)) for k, R in md.FIXTURES]
            + [(k, R, 20, BIGGER) for k, R in md.FIXTURES] + [("sphere", 9, 65, (BMIN, BMAX)), ("sphere", 9, 130, (BMIN, BMAX)),
                                                              ("sphere", 9, 130, ((BMIN[0], BMIN[1], BMAX[2]), (BMAX[0], BMAX[1], BMIN[2])))])


@pytest.mark.parametrize("kind,R,Rl,box", LATTICES)
def test_the_lattice_is_the_restatements_and_the_points_querys(kind, R, Rl, box):
    from pvd.mesh import voxelize_mesh
    _, verts, tris = _mesh(kind, R)
    ref, ref_totals = _reference_lattice(kind, R, Rl, box)
    w, totals = voxelize_mesh(_dev(verts, np.float32), _dev(tris, np.int32), Rl, box[0], box[1], return_totals=True)
    assert w.dtype == torch.int32 and w.is_cuda and w.shape == (Rl, Rl, Rl)
    print("mesh winding lattice %s R=%d -> %d^3: T=%d totals %r" % (kind, R, Rl, len(tris), totals))
    _same(w.cpu().numpy(), ref, "%s R=%d lattice %d" % (kind, R, Rl))
    assert totals == ref_totals
    assert totals == dict(inside=int((ref != 0).sum()), positive=int((ref > 0).sum()), leaky_columns=ref_totals["leaky_columns"],
                          max_abs=int(np.abs(ref).max()))  # counted in numpy
    if Rl > 2:
        assert totals["inside"] > 0
    pts = wr.lattice_points(Rl, *box)
    for G in (None, 3):
        _same(_winding(pts, verts, tris, G).reshape(Rl, Rl, Rl), ref, "%s R=%d lattice %d against mesh_winding G=%r" % (kind, R, Rl, G))
    w2 = voxelize_mesh(_dev(verts, np.float32), _dev(tris, np.int32), Rl, box[0], box[1], grid=5)
    assert torch.equal(w2, w)  # another grid, the same bits


@pytest.mark.parametrize("kind,R", CLOSED + (("smooth_bordered", 9), ("smooth_bordered", 17)))
def test_voxelising_an_extracted_mesh_gives_back_the_inside_of_its_field(kind, R):
    from pvd.mesh import voxelize_mesh
    u, verts, tris = _mesh(kind, R)
    assert np.abs(u.astype(np.float64) - np.float32(THRESH)).min() > 1e-5  # (the precondition of tests/test_mesh_winding_restatement.py)
    w, totals = voxelize_mesh(_dev(verts, np.float32), _dev(tris, np.int32), R, BMIN, BMAX, return_totals=True)
    inside = u > np.float32(THRESH)
    assert np.array_equal(w.cpu().numpy() != 0, inside) and np.array_equal(w.cpu().numpy() == 1, inside)
    assert totals == dict(inside=int(inside.sum()), positive=int(inside.sum()), leaky_columns=0, max_abs=1)


def test_an_open_mesh_leaks_and_an_empty_one_is_outside_everywhere():
    from pvd.mesh import mesh_winding, voxelize_mesh
    _, verts, tris = _mesh("smooth", 9)
    _, totals = voxelize_mesh(_dev(verts, np.float32), _dev(tris, np.int32), 9, BMIN, BMAX, return_totals=True)
    assert totals["leaky_columns"] == _reference_lattice("smooth", 9, 9, (BMIN, BMAX))[1]["leaky_columns"] > 0
    none = torch.zeros(0, 3, dtype=torch.int32, device=DEV)
    for v in (_dev(verts, np.float32), torch.zeros(0, 3, device=DEV)):
        w, totals = voxelize_mesh(v, none, 9, BMIN, BMAX, return_totals=True)
        assert w.shape == (9, 9, 9) and not w.any() and totals == dict(inside=0, positive=0, leaky_columns=0, max_abs=0)
        p = _dev(_reference("smooth", 9, 257)[0], np.float32)
        got = mesh_winding(p, v, none).cpu().numpy()
        assert np.array_equal(got, np.where(np.isfinite(p.cpu().numpy()).all(axis=1), 0, wr.INVALID))
    assert mesh_winding(torch.zeros(0, 3, device=DEV), _dev(verts, np.float32), _dev(tris, np.int32)).shape == (0,)


def test_two_runs_give_identical_bytes():
    from pvd.mesh import mesh_winding, voxelize_mesh
    _, verts, tris = _mesh("torus", 33)
    v, t, p = _dev(verts, np.float32), _dev(tris, np.int32), _dev(_reference("torus", 33, 1000)[0], np.float32)
    a, b = voxelize_mesh(v, t, 40, *BIGGER), voxelize_mesh(v, t, 40, *BIGGER)
    assert torch.equal(a, b) and torch.equal(mesh_winding(p, v, t), mesh_winding(p, v, t))


# ------------------------------------------------------------------------------------------------------------- signed distance
def test_the_signed_distance_is_the_distance_with_the_sign_of_contains():
    from pvd.mesh import mesh_contains, mesh_distance, mesh_signed_distance
    _, verts, tris = _mesh("torus", 17)
    v, t, p = _dev(verts, np.float32), _dev(tris, np.int32), _dev(_reference("torus", 17, 1000)[0], np.float32)
    for max_dist in (10.0, 0.05):  # nothing saturated; most rows saturated
        sdf, tri = mesh_signed_distance(p, v, t, max_dist)
        dist, dtri = mesh_distance(p, v, t, max_dist)
        inside = mesh_contains(p, v, t)
        assert sdf.dtype == torch.float32 and torch.equal(tri, dtri)
        assert sdf.abs().cpu().numpy().tobytes() == dist.cpu().numpy().tobytes()  # the magnitude is mesh_distance's bits
        ok = torch.isfinite(dist) & (dist > 0)
        assert ok.sum() > 800 and torch.equal((sdf > 0)[ok], inside[ok]) and torch.equal((sdf < 0)[ok], ~inside[ok])
        assert torch.equal(torch.isnan(sdf), torch.isnan(dist)) and int(torch.isnan(sdf).sum()) == 6  # NaN rows stay NaN
        sat = dtri < 0
        sat &= torch.isfinite(dist)
        if max_dist < 1.0:
            assert (sat & inside).any() and (sat & ~inside).any()
            assert (sdf[sat & inside] == np.float32(max_dist)).all() and (sdf[sat & ~inside] == -np.float32(max_dist)).all()
        else:
            assert not sat.any()


def test_remeshing_through_the_signed_distance_stays_within_a_lattice_diagonal():
    """extract_mesh(mesh_to_sdf(mesh), 0): a new vertex lies on a lattice edge whose ends have opposite signs of an exact signed
    distance, so the old surface crosses that edge too, and an edge (of the Kuhn split: up to the cell's diagonal) is at most sqrt(3) h
    long, h the largest lattice spacing; plus one rounding term of 2^-20 of the box diagonal."""
    from pvd.mesh import extract_mesh, mesh_distance, mesh_to_sdf
    _, verts, tris = _mesh("torus", 33)
    v, t = _dev(verts, np.float32), _dev(tris, np.int32)
    R = 33
    sdf = mesh_to_sdf(v, t, R, BMIN, BMAX, max_dist=10.0, chunk=10000)  # four chunks, the last partial
    assert sdf.shape == (R, R, R) and sdf.dtype == torch.float32 and torch.isfinite(sdf).all()
    u = _mesh("torus", 33)[0]
    assert np.array_equal(sdf.cpu().numpy() > 0, u > np.float32(THRESH))  # the sign is the field's inside
    nv, nt = extract_mesh(sdf, 0.0, BMIN, BMAX)
    assert nv.shape[0] > 1000 and nt.shape[0] > 2000
    h = max((b - a) / (R - 1) for a, b in zip(BMIN, BMAX))
    diagonal = float(np.linalg.norm(np.array(BMAX) - np.array(BMIN)))
    d, tri = mesh_distance(nv, v, t, 10.0)
    print("remesh torus R=33: %d -> %d vertices, largest distance to the old mesh %.4g, bound %.4g" % (len(verts), nv.shape[0], float(d.max()), 3 ** 0.5 * h))
    assert (tri >= 0).all() and float(d.max()) <= 3 ** 0.5 * h + 2.0 ** -20 * diagonal


# --------------------------------------------------------------------------------------------------------------- volume overlap
def test_compare_meshes_reports_the_volume_overlap():
    from pvd.mesh import compare_meshes
    _, verts, tris = _mesh("sphere", 17)
    moved = (verts + np.array([0.25, 0.125, 0.0], np.float32)).astype(np.float32)
    va, vb, t = _dev(verts, np.float32), _dev(moved, np.float32), _dev(tris, np.int32)
    plain = compare_meshes(va, t, vb, t, tau=0.05)
    assert sorted(plain) == sorted(["a_to_b", "b_to_a", "chamfer", "hausdorff", "precision", "recall", "fscore", "n_a", "n_b", "saturated_a",
                                    "saturated_b"])  # without volume: today's keys
    same = compare_meshes(va, t, va, t, tau=0.05, volume=17)
    assert same["iou"] == 1.0 and same["volume_a"] == same["volume_b"] > 0.0 and same["leaky_a"] == same["leaky_b"] == 0
    got = compare_meshes(va, t, vb, t, tau=0.05, volume=17)
    assert sorted(got) == sorted(list(plain) + ["iou", "volume_a", "volume_b", "leaky_a", "leaky_b"])
    assert {k: got[k] for k in plain} == plain
    lo, hi = np.minimum(verts.min(axis=0), moved.min(axis=0)), np.maximum(verts.max(axis=0), moved.max(axis=0))
    wa, ta = wr.lattice(verts, tris, 17, lo, hi)
    wb, tb = wr.lattice(moved, tris, 17, lo, hi)
    both, either = int(((wa != 0) & (wb != 0)).sum()), int(((wa != 0) | (wb != 0)).sum())
    assert 0 < both < either and ta["inside"] > 0 and tb["inside"] > 0
    cell = 1.0
    for l, h in zip(lo.tolist(), hi.tolist()):
        cell *= (h - l) / 16
    print("compare_meshes volume=17: inside %d and %d, both %d, either %d, iou %.4f" % (ta["inside"], tb["inside"], both, either, got["iou"]))
    assert got["iou"] == both / either and got["volume_a"] == ta["inside"] * cell and got["volume_b"] == tb["inside"] * cell
    assert got["leaky_a"] == 0 and got["leaky_b"] == 0
