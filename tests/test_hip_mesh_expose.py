"""pvd_mesh_expose (csrc/mesh_expose.hip, csrc/pvd_hip_mesh_expose.h) and what pvd/mesh.py builds on it -- mesh_exposure, cull_hidden --
against the numpy restatement (tests/mesh_expose_restatement.py, pinned by tests/test_mesh_expose_restatement.py).

Tolerance.  None: counts and totals are integers decided by float64 comparisons that the device makes in the header's order and numpy
makes in the same order, so they are compared as bytes.  A differing count means a fused or reordered operation, a triangle the walk did
not test, or a lane the ballots lost.

Sizes.  The fixtures of mesh_expose_restatement (R = 9: 1616 to 2072 triangles; R = 17: 6512 to 8500).  The reference is rays x triangles
at about 0.2 microseconds a pair, so each case keeps that product near 10^7: the whole mesh at D = 1, a band of 100 triangles at D = 64 and
65 (a full wave; a second chunk with one lane), of 8 at D = 200 with S = 4 (a partial fourth chunk), and on the large meshes a band of 300
at D = 1, S = 4 and of 20 at D = 64.  A workgroup holds four triangles: every band here starts off a multiple of four and straddles
workgroup boundaries.  The cases are mesh_expose_restatement.CASES and its neighbours, so that the edge-on guard of
tests/test_mesh_expose_restatement.py runs over exactly these rays; whole meshes use the 16 directions its facts were pinned with."""
import functools

import numpy as np
import pytest
import torch

import mesh_expose_restatement as er

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(a, dt):
    return torch.from_numpy(np.array(a, dt)).to(DEV)


def _band(v, t, dirs, S, tri0, tri1, G=None, bmin=None, bmax=None):
    """(counts [tri1 - tri0, 4] int32, totals [5] int64) of one call of the entry point, as host arrays."""
    import pvd_hip
    from pvd.mesh import _ray_grid
    tv, tt = _dev(v, np.float32), _dev(t, np.int32).reshape(-1, 3)
    T, G, pairs, ws = _ray_grid(tv, tt, bmin, bmax, G)
    counts = torch.full((tri1 - tri0, 4), -7, dtype=torch.int32, device=DEV)
    totals = torch.zeros(5, dtype=torch.int64, device=DEV)
    pvd_hip.mesh_expose(_dev(dirs, np.float32).reshape(-1, 3), S, tri0, tri1, T, G, pairs, ws, counts, totals)
    return counts.cpu().numpy(), totals.cpu().numpy()


def _whole(v, t, dirs, S=1, **kw):
    from pvd.mesh import mesh_exposure
    counts, totals = mesh_exposure(_dev(v, np.float32), _dev(t, np.int32).reshape(-1, 3), None if dirs is None else _dev(dirs, np.float32), S,
                                   return_totals=True, **kw)
    assert counts.dtype == torch.int32 and counts.is_cuda and tuple(counts.shape) == (len(t), 4)
    return counts.cpu().numpy(), totals


@functools.lru_cache(maxsize=None)
def _reference(kind, R, D, S, tri0, tri1):
    v, t = er.fixture(kind, R)
    counts, totals = er.exposure(v, t, er.directions(D), S, tri0, len(t) if tri1 is None else tri1)
    counts.setflags(write=False), totals.setflags(write=False)
    return counts, totals


CASES = er.CASES  # shared with the edge-on guard of tests/test_mesh_expose_restatement.py


@pytest.mark.parametrize("kind,R,D,S,tri0,tri1", CASES)
def test_the_counts_are_the_restatements_byte_for_byte(kind, R, D, S, tri0, tri1):
    v, t = er.fixture(kind, R)
    tri1 = len(t) if tri1 is None else tri1
    ref_c, ref_t = _reference(kind, R, D, S, tri0, tri1)
    print("mesh expose %s R=%d D=%d S=%d: T=%d, band %d .. %d, totals %s" % (kind, R, D, S, len(t), tri0, tri1, ref_t.tolist()))
    assert ref_t[0] > 0
    got_c, got_t = _band(v, t, er.directions(D), S, tri0, tri1)
    bad = np.nonzero((got_c != ref_c).any(axis=1))[0]
    assert got_c.tobytes() == ref_c.tobytes(), "%d rows differ, first %d: %r against %r" % (len(bad), tri0 + bad[0], got_c[bad[0]], ref_c[bad[0]])
    assert got_t.tobytes() == ref_t.tobytes(), (got_t, ref_t)
    # the same rows out of the whole mesh, through pvd.mesh
    whole, _ = _whole(v, t, er.directions(D), S)
    assert whole[tri0:tri1].tobytes() == ref_c.tobytes()


def test_the_grid_the_box_the_banding_and_the_run_change_no_byte():
    v, t = er.fixture("hollow", 9)
    d = er.directions(er.WHOLE_D)  # the whole mesh: the guard of these rays is the restatement test's whole-mesh run
    first, totals = _whole(v, t, d)
    assert first[1001:1101].tobytes() == _reference("hollow", 9, er.WHOLE_D, 1, 1001, 1101)[0].tobytes()
    assert totals["rays_cast"] == int(first[:, [0, 2]].sum()) and totals["rays_escaped"] == int(first[:, [1, 3]].sum())
    assert totals["front_exposed"] == int((first[:, 1] > 0).sum()) and totals["back_exposed"] == 0
    assert totals["hidden"] == int((first[:, 1] == 0).sum()) > 300
    runs = [dict(), dict(grid=1), dict(grid=2), dict(grid=7), dict(grid=32), dict(bmin=(-1.5, -1.25, -2.0), bmax=(2.0, 1.5, 1.0)),
            dict(grid=7, bmin=(-1.0, -1.0, -1.0), bmax=(0.5, 1.0, 1.0)),  # the triangles beyond x = 0.5 are on the outside list
            dict(band=4), dict(band=777), dict(band=1000, grid=2)]
    for kw in runs:
        counts, tot = _whole(v, t, d, **kw)
        assert counts.tobytes() == first.tobytes() and tot == totals, kw
    # the default directions are the Fibonacci 64 (the same grid both times)
    a, ta = _whole(v, t, None)
    b, tb = _whole(v, t, er.directions(64))
    assert a.tobytes() == b.tobytes() and ta == tb and ta["rays_cast"] == 64 * len(t)
    assert a[1001:1101].tobytes() == _reference("hollow", 9, 64, 1, 1001, 1101)[0].tobytes()


def test_invalid_triangles_and_directions_take_no_part():
    v, t, d = er.invalid_case()
    for S in (1, 4):
        ref_c, ref_t = er.exposure(v, t, d, S, 1001, 1041)
        assert np.all(ref_c[[2, 9, 10]] == 0) and np.all(np.delete(ref_c, [2, 9, 10], axis=0)[:, [0, 2]].sum(axis=1) == 9 * S)
        got_c, got_t = _band(v, t, d, S, 1001, 1041, G=7)
        assert got_c.tobytes() == ref_c.tobytes() and got_t.tobytes() == ref_t.tobytes(), S


def test_no_triangles():
    from pvd.mesh import cull_hidden
    v = er.fixture("ball", 9)[0]
    counts, totals = _whole(v, np.zeros((0, 3), np.int32), er.directions(3))
    assert counts.shape == (0, 4) and set(totals.values()) == {0}
    out = cull_hidden(_dev(v, np.float32), torch.zeros(0, 3, dtype=torch.int32, device=DEV))
    assert out["triangles"].shape == (0, 3) and out["vertices"].shape == (0, 3) and out["report"]["triangles_after"] == 0


# ------------------------------------------------------------------------------------------------------------------ cull_hidden
def _cull(v, t, **kw):
    from pvd.mesh import cull_hidden
    return cull_hidden(_dev(v, np.float32), _dev(t, np.int32).reshape(-1, 3), **kw)


def _follows(out, v, t, keep, normals=None, colors=None):
    """The result is the selection `keep` [T] bool of the input: order kept, bits copied, maps consistent."""
    used = np.zeros(len(v), bool)
    used[t[keep].reshape(-1)] = True
    vmap = np.where(used, np.cumsum(used) - 1, -1).astype(np.int32)
    tmap = np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int32)
    assert out["triangle_map"].cpu().numpy().tobytes() == tmap.tobytes() and out["vertex_map"].cpu().numpy().tobytes() == vmap.tobytes()
    assert out["vertices"].cpu().numpy().tobytes() == v[used].tobytes()
    assert out["triangles"].dtype == torch.int32 and out["triangles"].cpu().numpy().tobytes() == vmap[t[keep]].astype(np.int32).tobytes()
    for name, a in (("normals", normals), ("colors", colors)):
        assert (out[name] is None) if a is None else (out[name].cpu().numpy().tobytes() == a[used].tobytes()), name
    rep = out["report"]
    assert (rep["triangles_before"], rep["triangles_after"], rep["vertices_before"], rep["vertices_after"]) == \
        (len(t), int(keep.sum()), len(v), int(used.sum()))


def test_shells_mode_keeps_the_outer_shell_of_the_nested_mesh_and_the_atlas_shrinks():
    from pvd.mesh import mesh_topology, texture_layout, voxelize_mesh
    v, t = er.fixture("nested", 9)
    rng = np.random.RandomState(2)
    normals, colors = rng.normal(size=v.shape).astype(np.float32), rng.rand(*v.shape).astype(np.float32)
    outer = er.centroid_radius(v, t)[0] > 0.7
    d = _dev(er.directions(er.WHOLE_D), np.float32)  # the directions the restatement's whole-mesh facts were pinned with
    out = _cull(v, t, normals=_dev(normals, np.float32), colors=_dev(colors, np.float32), dirs=d, band=500)
    _follows(out, v, t, outer, normals, colors)
    rep = out["report"]
    assert (rep["shells_before"], rep["shells_dropped"], rep["hidden_triangles"]) == (3, 2, int((~outer).sum()))
    assert rep["totals"]["hidden"] == int((~outer).sum()) and out["counts"].shape == (len(t), 4)
    topo = mesh_topology(out["vertices"], out["triangles"])
    assert topo["closed"] and topo["manifold"] and topo["shells"] == 1 and topo["survivors"] == int(outer.sum())
    _, tot = voxelize_mesh(out["vertices"], out["triangles"], 24, er.BMIN, er.BMAX, return_totals=True)
    assert tot["leaky_columns"] == 0 and tot["inside"] > 0
    # the atlas, by the closed form of include/pvd_hip_mesh_tex.h: C the smallest integer whose square holds ceil(T / 2) cells
    for S in (4, 8):
        before, after = texture_layout(len(t), S), texture_layout(int(outer.sum()), S)
        for lay, n in ((before, len(t)), (after, int(outer.sum()))):
            C = int(np.ceil(np.sqrt((n + 1) // 2)))
            assert lay["cells_per_row"] == C and lay["width"] == C * S
        assert after["width"] * after["height"] < before["width"] * before["height"]


def test_triangles_mode_keeps_what_the_restatement_calls_exposed():
    from pvd.mesh import mesh_topology
    v, t = er.fixture("drilled", 9)
    assert ("drilled", 9, 4) == er.CULL_TRIANGLES
    d = er.directions(4)  # the reference is the whole mesh against the whole mesh
    ref, _ = er.exposure(v, t, d, 1)
    keep = ref[:, 1] > 0
    assert 400 < keep.sum() < len(t) - 100
    out = _cull(v, t, mode="triangles", dirs=_dev(d, np.float32))
    assert out["counts"].cpu().numpy().tobytes() == ref.tobytes()
    _follows(out, v, t, keep)
    assert out["report"]["hidden_triangles"] == int((~keep).sum())
    assert mesh_topology(out["vertices"], out["triangles"])["boundary"] > 0  # this mode opens the surface
    # two escapes asked for: fewer triangles
    out2 = _cull(v, t, mode="triangles", dirs=_dev(d, np.float32), min_escaped=2)
    _follows(out2, v, t, ref[:, 1] > 1)


def test_a_ball_comes_back_unchanged_and_either_side_serves_a_flipped_mesh():
    d = _dev(er.directions(er.WHOLE_D), np.float32)
    v, t = er.fixture("ball", 9)
    for mode in ("shells", "triangles"):
        out = _cull(v, t, mode=mode, dirs=d)
        _follows(out, v, t, np.ones(len(t), bool))
        assert out["vertices"].cpu().numpy().tobytes() == v.tobytes() and out["triangles"].cpu().numpy().tobytes() == t.tobytes()
        assert out["report"]["shells_dropped"] == 0 and out["report"]["hidden_triangles"] == 0
    v, t = er.fixture("nested", 9)
    flipped = np.ascontiguousarray(t[:, [0, 2, 1]])
    for mode in ("shells", "triangles"):
        front = _cull(v, t, mode=mode, dirs=d)["triangle_map"].cpu().numpy() >= 0
        either = _cull(v, flipped, mode=mode, sides="either", dirs=d)["triangle_map"].cpu().numpy() >= 0
        wrong = _cull(v, flipped, mode=mode, dirs=d)["triangle_map"].cpu().numpy() >= 0
        assert np.array_equal(front, either) and front.sum() == (er.centroid_radius(v, t)[0] > 0.7).sum()
        assert not np.array_equal(front, wrong)  # trusting a wrong orientation: every ray that counts starts into the solid


# ------------------------------------------------------------------------------------------------------ tools/export_mesh.py
def test_export_mesh_culls_before_the_colours_and_the_atlas():
    """tools/export_mesh.py --cull-hidden: cull_surface on a model whose density is a spherical shell (two surface shells, the cavity wall
    hidden) drops the cavity wall before the colours are taken and the atlas is baked, and its report is one JSON line with the atlas
    before and after."""
    import json
    import os
    import sys
    from pvd.mesh import extract_surface, mesh_topology, texture_layout
    from test_hip_mesh_normals import _AnalyticSphere
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import export_mesh

    class Shell(_AnalyticSphere):  # sigma - 2 = 5 min(0.7 - r, r - 0.35): a wall of four lattice spacings at R = 24
        def density(self, x):
            r = torch.linalg.norm(x - torch.tensor(self.CENTRE, device=x.device), dim=1)
            return {"sigma": 2.0 + 5.0 * torch.minimum(0.7 - r, r - 0.35)}
    model, R, S = Shell(), 24, 4
    plain = extract_surface(model, resolution=R, texture=S)
    m = extract_surface(model, resolution=R, normals=True, colors=False)
    assert torch.equal(m["triangles"], plain["triangles"]) and mesh_topology(m["vertices"], m["triangles"])["shells"] == 2
    report = export_mesh.cull_surface(model, m, "shells", n_dirs=16, samples=1, colors=True, texture=S)
    assert json.loads(json.dumps(report)) == report and (report["mode"], report["directions"], report["samples"]) == ("shells", 16, 1)
    T0, T1 = int(plain["triangles"].shape[0]), int(m["triangles"].shape[0])
    assert (report["triangles_before"], report["triangles_after"], report["shells_before"], report["shells_dropped"]) == (T0, T1, 2, 1)
    radius = torch.linalg.norm(m["vertices"] - torch.tensor(model.CENTRE, device=DEV), dim=1)
    assert 0 < T1 < T0 and float(radius.min()) > 0.6  # the outer surface (0.7) is what is left
    top = mesh_topology(m["vertices"], m["triangles"])
    assert top["closed"] and top["manifold"] and top["shells"] == 1
    before, after = texture_layout(T0, S), texture_layout(T1, S)
    assert report["atlas_before"] == [before["width"], before["height"]] and report["atlas_after"] == [after["width"], after["height"]]
    assert after["width"] * after["height"] < before["width"] * before["height"]
    assert tuple(m["texture"].shape) == (after["height"], after["width"], 3) and tuple(plain["texture"].shape) == (before["height"], before["width"], 3)
    V1 = int(m["vertices"].shape[0])
    assert tuple(m["colors"].shape) == (V1, 3) and tuple(m["normals"].shape) == (V1, 3) and tuple(m["uv"].shape) == (T1, 3, 2)
    assert bool(torch.isfinite(m["colors"]).all()) and bool(torch.isfinite(m["texture"]).all())
    assert int((m["triangle_map"] >= 0).sum()) == T1 and int((m["vertex_map"] >= 0).sum()) == V1
