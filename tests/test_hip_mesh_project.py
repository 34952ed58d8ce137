"""pvd_mesh_project_integrate / _finalize (csrc/mesh_project.hip, csrc/pvd_hip_mesh_project.h) and project_views, view_source and
view_vertex_colors of pvd/mesh.py against the numpy restatement (tests/mesh_project_restatement.py, pinned by
tests/test_mesh_project_restatement.py), BIT FOR BIT: the build compiles with -ffp-contract=off, HIP's float32 division and square root
are correctly rounded, and the occlusion test is the float64 one of the ray cast.

Sizes.  N = 1, 63, 64, 65 (around one wave) and 257 (two workgroups of 256, the last one with one lane); V = 1, 3 and 14 (the views are
not chunked); images of 2 x 2 (one bilinear cell), 7 x 5 and 64 x 64; with and without weight; both sides and both modes; power 0, 2
and 8; the restatement's sphere at R = 9 and 17, the nested mesh of the exposure tests and no mesh at all (T = 0)."""
import os
import sys

import numpy as np
import pytest
import torch

import mesh_expose_restatement as xr
import mesh_project_restatement as pr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPHERE_KW = dict(cos_min=pr.SPHERE_COS_MIN, power=2, bias=float(np.float32(1e-3 * np.sqrt(3.0) * 2 * 0.95)))


def _t(a, dtype=torch.float32):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV)


def _bits(t):
    return t.detach().cpu().contiguous().numpy().reshape(-1).view(np.uint32)


def _same(got, want, what):
    np.testing.assert_array_equal(_bits(got), np.ascontiguousarray(want, np.float32).reshape(-1).view(np.uint32), err_msg=what)


def _grid(vertices, triangles, G, bmin=None, bmax=None):
    from pvd import mesh
    return mesh._ray_grid(_t(vertices), _t(triangles, torch.int32), bmin, bmax, G)


def _gpu_integrate(acc, points, normals, color, weight, poses, intr, grid, cos_min=0.0, power=0, bias=0.0, sides="front", mode="blend"):
    import pvd_hip
    T, G, pairs, ws = grid
    pvd_hip.mesh_project_integrate(_t(points), _t(normals), _t(color), _t(weight), _t(poses), _t(intr), T, G, pairs, ws, float(cos_min),
                                   int(power), float(bias), sides, mode, acc[0], acc[1])


def _zeros(N):
    return [torch.zeros(N, 3, dtype=torch.float32, device=DEV), torch.zeros(N, dtype=torch.float32, device=DEV)]


def _mesh(kind):
    if kind == "none":
        return np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)
    name, R = kind
    return xr.fixture(name, R)


def _scene(kind, N, V, H, W, seed):
    """points near the mesh's surface (its vertices with their radial normals, some turned, some off the surface, a few not finite),
    the first V of 14 cameras around the origin and random images with holes (NaN, inf) and a weight image with zeros"""
    import mesh_tsdf_restatement as tr
    rng = np.random.RandomState(seed)
    v, t = _mesh(kind)
    if len(v):
        pick = rng.randint(0, len(v), N)
        pts = v[pick] + rng.normal(0, 0.01, (N, 3)).astype(np.float32)
    else:
        pts = rng.normal(0, 0.5, (N, 3)).astype(np.float32)
    nrm = (pts - np.array(xr.CENTRE, np.float32)) * rng.uniform(0.5, 2.0, (N, 1)).astype(np.float32)
    nrm[1::5] = rng.normal(0, 1, nrm[1::5].shape)  # any direction
    nrm[2::11] *= -1  # inward: the cavity walls of the nested mesh face that way
    if N > 8:
        pts[7, 0], nrm[6], nrm[5, 1] = np.nan, 0.0, np.inf
    poses = tr.sphere_cameras(14, 3.2)[:V]
    focal = 0.5 * W / 0.36
    intr = np.tile(np.array([focal, focal * H / W, W / 2, H / 2], np.float32), (V, 1))
    color = rng.uniform(0, 1, (V, H, W, 3)).astype(np.float32)
    weight = rng.uniform(0.25, 2.0, (V, H, W)).astype(np.float32)
    if H * W > 4:
        holes = rng.rand(V, H, W)
        color[holes < 0.03, 1] = np.nan
        color[(holes >= 0.03) & (holes < 0.05), 2] = np.inf
        weight[rng.rand(V, H, W) < 0.05] = 0.0
    return v, t, pts.astype(np.float32), nrm.astype(np.float32), color, weight, poses, intr


CASES = [  # (mesh, N, V, H, W, weight, sides, mode, power)
    (("ball", 9), 1, 1, 2, 2, False, "front", "blend", 0),
    (("ball", 9), 63, 3, 5, 7, True, "front", "blend", 2),
    (("ball", 9), 64, 14, 64, 64, True, "both", "blend", 2),
    (("ball", 17), 65, 3, 64, 64, False, "both", "best", 8),
    (("ball", 17), 257, 3, 64, 64, True, "front", "best", 2),
    (("nested", 9), 257, 14, 64, 64, False, "both", "blend", 2),
    (("nested", 9), 65, 3, 5, 7, True, "front", "best", 0),
    ("none", 257, 3, 64, 64, True, "both", "blend", 8),
    ("none", 63, 1, 2, 2, False, "front", "best", 2),
]


@pytest.mark.parametrize("kind,N,V,H,W,weighted,sides,mode,power", CASES)
def test_integrate_is_the_restatement_bit_for_bit(kind, N, V, H, W, weighted, sides, mode, power):
    v, t, pts, nrm, color, weight, poses, intr = _scene(kind, N, V, H, W, seed=N + V + H)
    kw = dict(cos_min=0.1, power=power, bias=0.004, sides=sides, mode=mode)
    want_c, want_w, _ = pr.project(pts, nrm, color, weight if weighted else None, poses, intr, v, t, **kw)
    if H * W > 4:
        assert want_w.any()
    got = _zeros(N)
    _gpu_integrate(got, pts, nrm, color, weight if weighted else None, poses, intr, _grid(v, t, 5), **kw)
    _same(got[1], want_w, "acc_w")
    _same(got[0], want_c, "acc_c")


@pytest.mark.parametrize("kw", [dict(), dict(bias=0.5, sides="both", power=2), dict(mode="best", power=1, cos_min=0.5),
                                dict(cos_min=float(np.float32(0.8)), power=8)])
def test_the_hand_made_cases_in_one_call(kw):
    points, normals = pr.hand_points()
    color, weight, poses, intr = pr.hand_stack()
    grid = _grid(pr.HAND_VERTICES, pr.HAND_TRIANGLES, 3)
    for wt in (weight, None):
        want_c, want_w, _ = pr.project(points, normals, color, wt, poses, intr, pr.HAND_VERTICES, pr.HAND_TRIANGLES, **kw)
        got = _zeros(len(points))
        _gpu_integrate(got, points, normals, color, wt, poses, intr, grid, **kw)
        _same(got[1], want_w, "acc_w")
        _same(got[0], want_c, "acc_c")
    # and every case on its own against the values written out by hand
    if not kw:
        views = pr.hand_views()
        for name, case in pr.hand_cases().items():
            vw = views[case["view"]]
            got = _zeros(1)
            _gpu_integrate(got, case["point"][None], case["normal"][None], vw["color"][None], vw["weight"][None] if case["weighted"] else None,
                           vw["pose"][None], vw["intrinsics"][None], grid, **case["kw"])
            assert float(got[1][0]) == float(case["acc_w"]), name
            want = np.zeros(3, np.float32) if case["ramp"] is None else case["acc_w"] * pr.hand_color(case["ramp"])
            _same(got[0], want, name)


@pytest.fixture(scope="module")
def sphere():
    v, t, n = pr.sphere_mesh()
    sv = pr.sphere_views()
    ref = pr.project(v, n, sv["color"], sv["weight"], sv["poses"], sv["intrinsics"], v, t, **SPHERE_KW)  # computed once, never changed
    assert ref[2] > 1e3 * pr.DET_BOUND  # every pair is far from edge-on: the grid cannot change a byte
    return dict(v=v, t=t, n=n, sv=sv, ref=ref)


def _sphere_run(s, grid, a=0, b=14, acc=None, **kw):
    sv = s["sv"]
    acc = _zeros(len(s["v"])) if acc is None else acc
    _gpu_integrate(acc, s["v"], s["n"], sv["color"][a:b], sv["weight"][a:b], sv["poses"][a:b], sv["intrinsics"][a:b], grid, **dict(SPHERE_KW, **kw))
    return acc


def test_batches_grids_boxes_and_runs_leave_the_same_bytes(sphere):
    g4 = _grid(sphere["v"], sphere["t"], 4)
    one = _sphere_run(sphere, g4)
    _same(one[1], sphere["ref"][1], "acc_w")
    _same(one[0], sphere["ref"][0], "acc_c")
    again = _sphere_run(sphere, g4)
    two = _sphere_run(sphere, g4, 8, 14, acc=_sphere_run(sphere, g4, 0, 8))
    each = _zeros(len(sphere["v"]))
    for v in range(14):
        _sphere_run(sphere, g4, v, v + 1, acc=each)
    g1, g16 = _grid(sphere["v"], sphere["t"], 1), _grid(sphere["v"], sphere["t"], 16)
    shifted = _grid(sphere["v"], sphere["t"], 7, bmin=(-0.5, -2.0, -1.1), bmax=(1.5, 0.3, 1.0))  # part of the mesh is outside
    for other in (again, two, each, _sphere_run(sphere, g1), _sphere_run(sphere, g16), _sphere_run(sphere, shifted)):
        for a, b in zip(one, other):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    best = _sphere_run(sphere, g4, mode="best")
    best_each = _zeros(len(sphere["v"]))
    for v in range(14):
        _sphere_run(sphere, g4, v, v + 1, acc=best_each, mode="best")
    for a, b in zip(best, best_each):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("mode", pr.MODES)
def test_finalize_totals_and_untouched_fallback_rows(sphere, mode):
    import pvd_hip
    rng = np.random.RandomState(3)
    N = 2048 * 256 + 77  # more than one pass of the finalize grid, the second one partial
    acc_w = rng.choice(np.array([0.0, 0.5, 1.0, 3.0, np.nan], np.float32), N)
    acc_c = (rng.uniform(-0.5, 4.0, (N, 3)) * np.nan_to_num(acc_w)[:, None]).astype(np.float32)
    fallback = rng.uniform(0, 1, (N, 3)).astype(np.float32)
    want, want_seen, totals = pr.finalize(acc_c, acc_w, 1.0, mode, fallback)
    colors = torch.cat([_t(fallback), torch.full((3, 3), 9.0, device=DEV)])
    seen = torch.full((N + 3,), 7, dtype=torch.uint8, device=DEV)
    got = torch.full((2,), -5, dtype=torch.int64, device=DEV)
    pvd_hip.mesh_project_finalize(_t(acc_c), _t(acc_w), 1.0, mode, colors[:N], seen[:N], got)
    _same(colors[:N], want, "colors")
    assert np.array_equal(seen[:N].cpu().numpy(), want_seen) and tuple(got.tolist()) == totals and sum(totals) == N
    assert bool((colors[N:] == 9.0).all()) and bool((seen[N:] == 7).all())  # rows past N are untouched
    unseen = torch.from_numpy(want_seen == 0).to(DEV)
    assert torch.equal(colors[:N][unseen], _t(fallback)[unseen])  # the fallback rows: not a byte written


def test_project_views_through_pvd_mesh(sphere):
    """project_views at the vertices is the restatement; bake_texture(view_source(...)) reproduces project_views at texture_points; and
    render_mesh of that atlas from a held-out camera shows the pattern within the CPU test's bound."""
    from pvd import mesh
    import mesh_tsdf_restatement as tr
    sv = sphere["sv"]
    V, T = _t(sphere["v"]), _t(sphere["t"], torch.int32)
    imgs = dict(color=_t(sv["color"]), poses=_t(sv["poses"]), intrinsics=_t(sv["intrinsics"]))
    kw = dict(weight=_t(sv["weight"]), **SPHERE_KW)
    out = mesh.project_views(V, _t(sphere["n"]), V, T, views_per_batch=5, fallback=torch.full((len(sphere["v"]), 3), 0.25), **imgs, **kw)
    want, want_seen, totals = pr.finalize(sphere["ref"][0], sphere["ref"][1], 1e-6, "blend", np.full_like(sphere["ref"][0], 0.25))
    _same(out["colors"], want, "colors")
    _same(out["weight"], sphere["ref"][1], "weight")
    assert out["totals"] == dict(seen=totals[0], unseen=0) and bool(out["seen"].all())
    _same(mesh.view_vertex_colors(V, T, _t(sphere["n"]), imgs["color"], imgs["poses"], imgs["intrinsics"], **kw), want, "view_vertex_colors")
    # the default bias is 1e-3 of the box diagonal
    lo, hi = sphere["v"].min(axis=0), sphere["v"].max(axis=0)
    auto = mesh.project_views(V, _t(sphere["n"]), V, T, **imgs, weight=kw["weight"], cos_min=pr.SPHERE_COS_MIN, power=2)
    ref = mesh.project_views(V, _t(sphere["n"]), V, T, **imgs, weight=kw["weight"], cos_min=pr.SPHERE_COS_MIN, power=2,
                             bias=1e-3 * float(torch.linalg.norm(_t(hi) - _t(lo))))
    assert torch.equal(auto["colors"], ref["colors"])
    # the atlas
    S = 6
    nrm = _t(sphere["n"])
    marker = lambda x, n: torch.full_like(x, 0.125)  # noqa: E731  (the fallback: where no view sees a texel)
    baked = mesh.bake_texture(mesh.view_source(V, T, fallback=marker, **imgs, **kw), V, T, S, normals=nrm)
    x, n = mesh.texture_points(V, T, S, normals=nrm)
    good = torch.isfinite(x).all(dim=1) & torch.isfinite(n).all(dim=1)
    direct = mesh.project_views(x[good], mesh._unit_rows(n[good]), V, T, fallback=marker, **imgs, **kw)  # bake_texture hands the source unit normals
    tex = baked["texture"].reshape(-1, 3)
    assert torch.equal(tex[good], direct["colors"]) and bool((tex[~good] == 0).all())
    # a held-out camera
    pose = tr.look_at(np.array([0.5, -0.7, 0.4]) / np.linalg.norm([0.5, -0.7, 0.4]) * 3.2)
    K = tuple(float(k) for k in sv["intrinsics"][0])
    img = mesh.render_mesh(V, T, _t(pose), K, 64, 64, texture=baked["texture"], texture_cell=S)
    o, d = pr.camera_rays(pose, np.array(K), 64, 64)
    hit = img["mask"].reshape(-1).cpu().numpy()
    t_hit = img["depth"].reshape(-1).cpu().numpy().astype(np.float64) / np.linalg.norm(d.astype(np.float64), axis=1)
    from pvd.scene import get_rays
    rays = get_rays(_t(pose)[None], K, 64, 64, -1)
    xh = (rays["rays_o"].reshape(-1, 3) + img["depth"].reshape(-1, 1) * rays["rays_d"].reshape(-1, 3)).cpu().numpy()
    err = np.abs(img["color"].reshape(-1, 3).cpu().numpy().astype(np.float64) - pr.pattern(xh))[hit]
    bound = pr.sphere_bound(sv["fx"], sv["distance"])
    print("held-out view: %d pixels on the mesh, the largest |atlas - pattern| %.5f, bound %.5f; unseen texels %d of %d"
          % (int(hit.sum()), err.max(), bound, direct["totals"]["unseen"], int(good.sum())))
    assert hit.sum() > 1000 and err.max() <= bound + 1e-5 and t_hit[hit].min() > 0


def _export_model():
    from test_hip_infer_rounds import _model
    model = _model("hash")
    model.density_scale = 16  # as tests/test_hip_mesh_tsdf.py: the fixture's densities leave no ray opaque otherwise
    return model


def test_export_mesh_project_surface_on_the_tiny_model():
    """tools/export_mesh.py: project_surface on the model fixture of the depth-map tests takes the vertex colours and the atlas from
    rendered views: the seen vertices carry exactly what project_views gives for the same renders, which is not the colour head's; what
    no view sees keeps the model's own colour."""
    import math
    from pvd import mesh
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import export_mesh
    model = _export_model()
    m = mesh.extract_surface_tsdf(model, mesh.tsdf_poses(6), (48.0, 48.0, 24.0, 24.0), 48, 48, resolution=24, views_per_batch=4)  # the
    # surface tests/test_hip_mesh_tsdf.py extracts from this fixture: where its rays end
    assert int(m["vertices"].shape[0]) > 0
    own = m["colors"].clone()
    report = export_mesh.project_surface(model, m, 6, size=48, colors=True, texture=4)
    V, T = int(m["vertices"].shape[0]), int(m["triangles"].shape[0])
    assert (report["views"], report["size"], report["mode"]) == (6, 48, "blend") and report["vertices_seen"] + report["vertices_unseen"] == V
    print("export: %d vertices, %d seen by 6 views of 48 x 48" % (V, report["vertices_seen"]))
    assert report["vertices_seen"] > V // 4  # the projection sees the surface the same cameras' depth maps made
    seen = m["project_seen"]
    assert int(seen.sum()) == report["vertices_seen"]
    assert tuple(m["colors"].shape) == (V, 3) and bool(torch.isfinite(m["colors"]).all())
    assert float(m["colors"].min()) >= 0.0 and float(m["colors"].max()) <= 1.0
    # the same renders through project_views directly
    poses = mesh.tsdf_poses(6).to(DEV)
    focal = 0.5 * 48 / math.tan(math.radians(25.0))
    intr = (focal, focal, 24.0, 24.0)
    maps = mesh.render_depth_maps(model, poses, intr, 48, 48, min_opacity=0.5)
    weight = torch.where(maps["opacity"] >= 0.5, maps["opacity"], torch.zeros_like(maps["opacity"]))
    direct = mesh.project_views(m["vertices"], m["normals"], m["vertices"], m["triangles"], maps["color"], poses, intr, weight=weight)
    assert torch.equal(direct["seen"], seen) and torch.equal(direct["colors"][seen], m["colors"][seen])
    assert bool((direct["colors"][~seen] == 0).all())
    # the fallback is the model's colour head seen straight on: the unseen vertices carry it (up to the fp16 head's dependence on the
    # batch it is evaluated in), the seen ones do not
    head = mesh.vertex_colors(model, m["vertices"], mesh._unit_rows(m["normals"]))
    close = (m["colors"] - head).abs().amax(dim=1) < 4e-3
    assert bool(close[~seen].all()) and int((~close[seen]).sum()) > report["vertices_seen"] // 2
    assert not torch.equal(m["colors"], own)
    lay = mesh.texture_layout(T, 4)
    assert tuple(m["texture"].shape) == (lay["height"], lay["width"], 3) and m["texture_cell"] == 4 and bool(torch.isfinite(m["texture"]).all())
    again = dict(m)
    best = export_mesh.project_surface(model, again, 6, size=48, best=True, colors=True)
    assert best["mode"] == "best" and best["vertices_seen"] == report["vertices_seen"]


def test_export_mesh_project_views_through_main(tmp_path, monkeypatch, capsys):
    """export_mesh.py --project-views run through main() on a saved tiny checkpoint: the flag checks, the colours and the atlas taken
    from the projection and not from the model first, and the files written.  (make_model is replaced by the fixture's constructor: the
    tool builds its model from defaults that do not carry the fixture's occupancy grid and density scale; the checkpoint is loaded as
    always.)"""
    from pvd import mesh
    from pvd.checkpoint import save_checkpoint
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import export_mesh
    ckpt = save_checkpoint(os.path.join(str(tmp_path), "tiny.pth"), _export_model())
    monkeypatch.setattr(export_mesh, "make_model", lambda *a, **k: _export_model())
    straight = []
    monkeypatch.setattr(export_mesh, "bake_texture", lambda source, *a, **k: (straight.append(hasattr(source, "aabb_infer")), mesh.bake_texture(source, *a, **k))[1])
    out = os.path.join(str(tmp_path), "mesh.ply")
    common = [ckpt, "-o", out, "--model-type", "hash", "--resolution0", "64", "--resolution", "24", "--tsdf", "6", "--tsdf-res", "48x48"]
    for bad in (["--project-size", "48", "--colors"], ["--project-best", "--colors"], ["--project-views", "6"],
                ["--project-views", "6", "--colors", "--cull-hidden", "shells"], ["--project-views", "6", "--texture", "4", "--texture-sh", "2"],
                ["--project-views", "-1", "--colors"], ["--project-views", "6", "--project-data", str(tmp_path), "--colors"],
                ["--project-split", "val", "--colors"], ["--project-views", "6", "--project-size", "1", "--colors"]):
        with pytest.raises(SystemExit):
            export_mesh.main(common + bad)
    capsys.readouterr()
    export_mesh.main(common + ["--colors", "--texture", "4", "--project-views", "6", "--project-size", "48"])  # no --normals: they are taken for the projection
    text = capsys.readouterr().out
    assert "projected 6 views at 48 (blend)" in text and '"vertices_seen"' in text, text
    seen = int(text.split('"vertices_seen": ')[1].split(",")[0].split("}")[0])
    assert seen > 0
    assert straight == [False]  # one bake, from the views: the model's own atlas is not baked first
    v, t, nrm, col = mesh.read_ply(out)[:4]
    assert len(v) > 0 and col is not None and nrm is None
    for ext in (".obj", ".mtl", ".png"):
        assert os.path.exists(out[:-4] + ext), ext
