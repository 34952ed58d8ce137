"""pvd_mesh_nets_count / _emit / _normals (csrc/mesh_nets.hip, csrc/pvd_hip_mesh_nets.h) and extract_mesh(method="nets") of pvd/mesh.py
against the numpy restatement (tests/mesh_nets_restatement.py, pinned by tests/test_mesh_nets_restatement.py), BIT FOR BIT: the build
compiles with -ffp-contract=off and HIP's float32 division and square root are correctly rounded.  (Where the restatement has a NaN the
kernel must have one; a NaN's payload is not compared.)

Sizes, from csrc/block_scan.h (kThreads = 256 points per workgroup, kScanChunk = 1024 * 8 = 8192 workgroup sums per chunk of the one
scanning workgroup): R = 2, 3, 4 fit one workgroup (8, 27, 64 points), 7 is the first size above one (343 points), 9 .. 65 are many
workgroups in one chunk, 128^3 = 8192 * 256 is exactly one chunk of sums and 129^3 takes a second one."""
import os
import sys

import numpy as np
import pytest
import torch

import mesh_nets_restatement as sn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOX = ([-1.0, -1.0, -1.0], [1.0, 1.0, 1.0])
SHIFTED_BOX = ([1.0, -2.0, 0.5], [3.0, -1.0, 4.5])
GUARD = 5


def _t(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV)


def _run(u, thresh, box, V=None, T=None):
    """The three entry points on prefilled buffers with GUARD rows behind V and T -> (totals, vertices, triangles, normals) as numpy,
    after checking that the guard rows were not written."""
    import pvd_hip
    R = u.shape[0]
    field, lo, hi = _t(u), _t(np.float32(box[0])), _t(np.float32(box[1]))
    ws = torch.empty(pvd_hip.mesh_nets_workspace_bytes(R), dtype=torch.uint8, device=DEV)
    totals = torch.full((2,), -7, dtype=torch.int32, device=DEV)
    pvd_hip.mesh_nets_count(field, R, float(thresh), ws, totals)
    tv, tt = (int(x) for x in totals.tolist())
    V, T = tv if V is None else V, tt if T is None else T
    vertices = torch.full((V + GUARD, 3), -77.0, dtype=torch.float32, device=DEV)
    triangles = torch.full((T + GUARD, 3), -77, dtype=torch.int32, device=DEV)
    normals = torch.full((V + GUARD, 3), -77.0, dtype=torch.float32, device=DEV)
    pvd_hip.mesh_nets_emit(field, R, float(thresh), lo, hi, ws, vertices[:V], triangles[:T])
    pvd_hip.mesh_nets_normals(field, R, float(thresh), lo, hi, ws, normals[:V])
    torch.cuda.synchronize()
    assert bool((vertices[V:] == -77.0).all()) and bool((triangles[T:] == -77).all()) and bool((normals[V:] == -77.0).all())
    return (tv, tt), vertices[:V].cpu().numpy(), triangles[:T].cpu().numpy(), normals[:V].cpu().numpy()


def _same_floats(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, what
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what + ": NaN where the restatement has none, or the other way round"
    np.testing.assert_array_equal(np.where(nan, 0, got).view(np.uint32), np.where(nan, 0, want).view(np.uint32), err_msg=what)


def _check(kind, R, thresh=0.0, box=BOX):
    u = sn.field(kind, R, thresh)
    want = sn.extract(u, thresh, *box)
    totals, v, t, n = _run(u, thresh, box)
    label = "%s R=%d" % (kind, R)
    assert totals == (len(want["vertices"]), len(want["triangles"])), label
    np.testing.assert_array_equal(t, want["triangles"], err_msg=label)
    _same_floats(v, want["vertices"], label + " vertices")
    _same_floats(n, want["normals"], label + " normals")
    return want


@pytest.mark.parametrize("R", [2, 3, 4, 7, 9, 17, 33, 65])
@pytest.mark.parametrize("kind", ["sphere", "shifted", "torus", "random", "plane", "special", "inside", "outside"])
def test_bit_for_bit_against_the_restatement(kind, R):
    want = _check(kind, R)
    if kind in ("random", "plane", "special") and R >= 4:
        assert len(want["triangles"]) > 0
    if kind == "special" and R >= 9:
        assert np.isnan(want["vertices"]).any() and np.isfinite(want["vertices"]).any()
    if kind in ("inside", "outside"):
        assert len(want["vertices"]) == 0 and len(want["triangles"]) == 0


@pytest.mark.parametrize("R", [128, 129])
@pytest.mark.parametrize("kind", ["shifted", "torus", "special"])
def test_bit_for_bit_at_one_scan_chunk_and_at_two(kind, R):
    _check(kind, R)


@pytest.mark.parametrize("R", [128, 129])
def test_the_random_field_at_one_scan_chunk_and_at_two(R):
    """Nearly every cell is active: the offsets run through every workgroup sum of both chunks."""
    want = _check("random", R)
    assert len(want["vertices"]) > 0.99 * (R - 1) ** 3


@pytest.mark.parametrize("kind,R,thresh,box", [("sphere", 17, 0.25, BOX), ("random", 9, -0.5, BOX), ("special", 17, 3.0, SHIFTED_BOX),
                                               ("torus", 33, 0.0, SHIFTED_BOX), ("plane", 7, 1.5, SHIFTED_BOX), ("random", 7, 0.0, SHIFTED_BOX)])
def test_another_threshold_and_a_non_cubic_shifted_box(kind, R, thresh, box):
    _check(kind, R, thresh, box)


def test_rows_past_a_smaller_V_and_T_are_never_written_or_read():
    u = sn.field("torus", 17)
    want = sn.extract(u, 0.0, *BOX)
    V, T = len(want["vertices"]), len(want["triangles"])
    totals, v, t, n = _run(u, 0.0, BOX, V=V - 9, T=T - 5)  # (the guard rows are checked inside)
    assert totals == (V, T)
    _same_floats(v, want["vertices"][:V - 9], "vertices")
    _same_floats(n, want["normals"][:V - 9], "normals")
    # a quad with a vertex past V takes the NaN branch of the split: the first diagonal; every other row is the restatement's
    known = (want["quads"] < V - 9).all(axis=1).repeat(2)[:T - 5]
    np.testing.assert_array_equal(t[known], want["triangles"][:T - 5][known])
    _, first = sn.split_quads(np.full((V, 3), np.nan, np.float32), want["quads"])
    np.testing.assert_array_equal(t[~known], first[:T - 5][~known])


def test_two_runs_give_the_same_bits():
    u = sn.field("random", 33)
    a, b = _run(u, 0.0, SHIFTED_BOX), _run(u, 0.0, SHIFTED_BOX)
    assert a[0] == b[0]
    for x, y in zip(a[1:], b[1:]):
        assert x.tobytes() == y.tobytes()


@pytest.mark.parametrize("kind,R,euler", [("sphere", 33, 2), ("torus", 33, 0), ("shifted", 17, 2), ("torus", 17, 0)])
def test_mesh_topology_reports_a_closed_manifold_shell(kind, R, euler):
    from pvd import mesh
    u = sn.field(kind, R)
    assert sn.ambiguous_faces(u, 0.0) == 0 and sn.split_cells(u, 0.0) == 0
    v, t, n = mesh.extract_mesh(_t(u), 0.0, *BOX, with_normals=True, method="nets")
    top = mesh.mesh_topology(v, t)
    assert top["closed"] and top["manifold"] and top["euler"] == euler and top["shells"] == 1, top
    assert abs(float(torch.linalg.norm(n, dim=1).min()) - 1) < 1e-5
    # and against the marching tetrahedra of the same field: within the cell diagonal both ways
    tv, tt = mesh.extract_mesh(_t(u), 0.0, *BOX)
    assert tt.shape[0] > 2 * t.shape[0]
    diagonal = float(np.sqrt(3.0) * 2.0 / (R - 1))
    d = mesh.compare_meshes(v, t, tv, tt, tau=diagonal)
    print("%s R=%d: nets %d / %d, tetrahedra %d / %d vertices / triangles; hausdorff %.4g, cell diagonal %.4g"
          % (kind, R, v.shape[0], t.shape[0], tv.shape[0], tt.shape[0], d["hausdorff"], diagonal))
    assert d["hausdorff"] <= diagonal + 1e-6


def test_extract_mesh_methods_and_the_default_is_what_it_was():
    import pvd_hip
    from pvd import mesh
    u = _t(sn.field("shifted", 17))
    with pytest.raises(ValueError):
        mesh.extract_mesh(u, 0.0, *BOX, method="bogus")
    plain, named = mesh.extract_mesh(u, 0.0, *BOX, with_normals=True), mesh.extract_mesh(u, 0.0, *BOX, with_normals=True, method="tetrahedra")
    for a, b in zip(plain, named):
        assert torch.equal(a, b)
    R = 17  # the default path is the entry points of include/pvd_hip_mesh.h, called directly
    ws = torch.empty(pvd_hip.mesh_workspace_bytes(R), dtype=torch.uint8, device=DEV)
    totals = torch.zeros(2, dtype=torch.int32, device=DEV)
    pvd_hip.mesh_count(u, R, 0.0, ws, totals)
    assert tuple(totals.tolist()) == (plain[0].shape[0], plain[1].shape[0])
    nets = mesh.extract_mesh(u, 0.0, *BOX, method="nets")
    want = sn.extract(sn.field("shifted", 17), 0.0, *BOX)
    assert len(nets) == 2 and np.array_equal(nets[1].cpu().numpy(), want["triangles"])
    _same_floats(nets[0].cpu().numpy(), want["vertices"], "extract_mesh(method='nets')")


def test_extract_surface_with_nets_through_simplify_clean_and_texture():
    from pvd import mesh
    from test_hip_mesh_normals import _AnalyticSphere
    model, R = _AnalyticSphere(), 24
    plain = mesh.extract_surface(model, resolution=R)
    named = mesh.extract_surface(model, resolution=R, method="tetrahedra")
    assert sorted(named) == sorted(plain) == ["colors", "counts", "field", "normals", "threshold", "triangles", "vertices"]
    for key in ("vertices", "triangles", "normals", "colors", "field"):
        assert torch.equal(named[key], plain[key]), key
    with pytest.raises(ValueError):
        mesh.extract_surface(model, resolution=R, method="cubes")
    with pytest.raises(ValueError):
        mesh.extract_geometry(model, resolution=R, method="cubes")
    nets = mesh.extract_surface(model, resolution=R, method="nets")
    assert sorted(nets) == sorted(plain) and torch.equal(nets["field"], plain["field"])
    V, T = int(nets["vertices"].shape[0]), int(nets["triangles"].shape[0])
    assert 0 < T < plain["triangles"].shape[0] // 2 and tuple(nets["normals"].shape) == tuple(nets["colors"].shape) == (V, 3)
    gv, gt = mesh.extract_geometry(model, resolution=R, method="nets")
    assert torch.equal(gv, nets["vertices"]) and torch.equal(gt, nets["triangles"])
    S, G = 4, 8
    m = mesh.extract_surface(model, resolution=R, method="nets", simplify=G, clean=True, texture=S)
    V2, T2 = int(m["vertices"].shape[0]), int(m["triangles"].shape[0])
    assert m["full_counts"] == (V, T) and 0 < V2 < V and 0 < T2 < T
    assert tuple(m["normals"].shape) == tuple(m["colors"].shape) == (V2, 3) and tuple(m["vertex_map"].shape) == (V,)
    lay = mesh.texture_layout(T2, S)
    assert tuple(m["texture"].shape) == (lay["height"], lay["width"], 3) and tuple(m["uv"].shape) == (T2, 3, 2) and m["texture_cell"] == S
    for key in ("vertices", "normals", "colors", "texture", "uv"):
        assert bool(torch.isfinite(m[key]).all()), key
    assert int(m["triangles"].min()) >= 0 and int(m["triangles"].max()) < V2


def test_extract_surface_tsdf_takes_the_method():
    from pvd import mesh
    from test_hip_mesh_project import _export_model
    model = _export_model()
    kw = dict(poses=mesh.tsdf_poses(6), intrinsics=(48.0, 48.0, 24.0, 24.0), H=48, W=48, resolution=24, views_per_batch=4)
    a, b = mesh.extract_surface_tsdf(model, **kw), mesh.extract_surface_tsdf(model, method="nets", **kw)
    assert torch.equal(a["field"], b["field"]) and 0 < b["triangles"].shape[0] < a["triangles"].shape[0]
    direct = mesh.extract_mesh(-b["field"], 0.0, model.aabb_infer[:3], model.aabb_infer[3:], method="nets")
    assert torch.equal(direct[0].view(torch.int32), b["vertices"].view(torch.int32)) and torch.equal(direct[1], b["triangles"])


def test_export_mesh_with_the_nets_mesher_through_main(tmp_path, monkeypatch, capsys):
    """tools/export_mesh.py --mesher nets --normals --colors run through main() on a saved tiny checkpoint, as
    tests/test_hip_mesh_project.py does: the PLY reads back with V and T of the direct call; without the flag it is the tetrahedra's."""
    from pvd import mesh
    from pvd.checkpoint import save_checkpoint
    from test_hip_mesh_project import _export_model
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import export_mesh
    ckpt = save_checkpoint(os.path.join(str(tmp_path), "tiny.pth"), _export_model())
    monkeypatch.setattr(export_mesh, "make_model", lambda *a, **k: _export_model())
    out = os.path.join(str(tmp_path), "mesh.ply")
    common = [ckpt, "-o", out, "--model-type", "hash", "--resolution0", "64", "--resolution", "24"]
    with pytest.raises(SystemExit):
        export_mesh.main(common + ["--mesher", "cubes"])
    model = _export_model()
    # the fixture's density never reaches its own threshold: the level is the median of the volume the tool samples
    aabb = model.aabb_infer
    thresh = float(mesh.density_field(lambda x: model.density(x)["sigma"], 24, aabb[:3], aabb[3:], device=aabb.device).median())
    common += ["--threshold", repr(thresh)]
    counts = {}
    for mesher in ("nets", None):
        capsys.readouterr()
        export_mesh.main(common + ["--normals", "--colors", "--topology-report"] + (["--mesher", mesher] if mesher else []))
        text = capsys.readouterr().out
        v, t, nrm, col = mesh.read_ply(out)[:4]
        direct = mesh.extract_geometry(model, resolution=24, threshold=thresh, method=mesher or "tetrahedra")
        assert (len(v), len(t)) == (int(direct[0].shape[0]), int(direct[1].shape[0])) and len(v) > 0, mesher
        assert nrm is not None and col is not None and len(nrm) == len(col) == len(v)
        assert "%d vertices" % len(v) in text and "%d triangles" % len(t) in text
        assert ("surface nets" in text) == (mesher == "nets")
        counts[mesher] = len(t)
    assert counts["nets"] < counts[None]
