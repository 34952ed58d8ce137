"""pvd_mesh_atex_build / _points / _sample (csrc/mesh_atex.hip, csrc/pvd_hip_mesh_atex.h) and what pvd/mesh.py builds on them --
adaptive_atlas, and texture_layout, texture_uv, texture_points, bake_texture, sample_texture, render_mesh with that atlas in place of the
integer S -- against the numpy restatement (tests/mesh_atex_restatement.py, pinned by tests/test_mesh_atex_restatement.py).

Tolerance.  None for the kernels: the class of a triangle, a texel's point and a lookup are a handful of float32 operations that the
device and numpy do unfused in the same order, and the ranks are integer sums: slot, order, totals, points and samples are compared on
their bits (NaN positions included).  The one bound is the derived accuracy bound of tests/test_mesh_atex_restatement.py, for the bake
through pvd.mesh.

Sizes.  T = 0, 1, 2, 3; 255, 256, 257 (a second workgroup with one lane); the graded fixture (24 triangles, all five classes, 128 x 124
texels); a mesh with a bad index and a NaN corner; one build at T = 8192 * 256 + 257 (the scan's second chunk).  N = 1, 257, 1000."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

import mesh_atex_restatement as ar
import mesh_tex_restatement as tr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev(a, dt):
    return torch.from_numpy(np.array(a, dt)).to(DEV)


def _same(got, want, what=""):
    got, want = np.ascontiguousarray(got, F32), np.ascontiguousarray(want, F32)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=str(what))
    np.testing.assert_array_equal(np.nan_to_num(got).view(np.uint32), np.nan_to_num(want).view(np.uint32), err_msg=str(what))


@functools.lru_cache(maxsize=None)
def _triangles(T, seed=0):
    """T separate right isosceles triangles with legs 2^-k, k random in 0 .. 7 (at density 40: all five classes), read-only."""
    rng = np.random.RandomState(seed)
    legs = 2.0 ** -rng.randint(0, 8, T)
    v = rng.uniform(-1, 0, (T, 1, 3)).astype(F32) + np.zeros((T, 3, 3), F32)
    v[:, 1, 0] += legs
    v[:, 2, 1] += legs
    v, t = v.reshape(-1, 3), np.arange(3 * T, dtype=np.int64).reshape(T, 3)
    for a in (v, t):
        a.setflags(write=False)
    return v, t


@functools.lru_cache(maxsize=None)
def _graded():
    v, t = ar.graded_fixture()
    slot, order, totals = ar.build(v, t, ar.FIXTURE_DENSITY)
    for a in (v, t, slot, order, totals):
        a.setflags(write=False)
    return v, t, slot, order, totals


def _build(v, t, density, max_cell=64):
    from pvd.mesh import adaptive_atlas
    return adaptive_atlas(_dev(v, F32).reshape(-1, 3), _dev(t, np.int32).reshape(-1, 3), density, max_cell=max_cell)


def _check_build(v, t, density, max_cell=64, layout=True):
    """pvd_mesh_atex_build through the binding against the restatement; layout: adaptive_atlas's dict as well."""
    import pvd_hip
    T = len(t)
    got_slot = torch.full((T,), -1, dtype=torch.int32, device=DEV)
    got_order = torch.full((T,), -1, dtype=torch.int32, device=DEV)
    got_totals = torch.full((6,), -1, dtype=torch.int32, device=DEV)
    ws = torch.empty(pvd_hip.mesh_atex_workspace_bytes(T), dtype=torch.uint8, device=DEV)
    pvd_hip.mesh_atex_build(_dev(v, F32).reshape(-1, 3), _dev(t, np.int32).reshape(-1, 3), density, ar.CELLS.index(max_cell), ws, got_slot,
                            got_order, got_totals)
    slot, order, totals = ar.build(v, t, density, ar.CELLS.index(max_cell))
    np.testing.assert_array_equal(got_totals.cpu().numpy().view(np.uint32), totals)
    np.testing.assert_array_equal(got_slot.cpu().numpy().view(np.uint32), slot)
    np.testing.assert_array_equal(got_order.cpu().numpy().view(np.uint32), order)
    if not layout:
        return dict(counts=tuple(totals[:5].tolist()), capped=int(totals[5]))
    atlas = _build(v, t, density, max_cell)
    assert torch.equal(atlas["slot"], got_slot) and torch.equal(atlas["order"], got_order)
    assert list(atlas["counts"]) + [atlas["capped"]] == totals.tolist()
    lay = ar.layout(totals[:5])
    assert (atlas["layout"]["width"], atlas["layout"]["height"]) == (lay["Wt"], lay["Ht"]) and atlas["triangles"] == len(t)
    assert list(atlas["layout"]["y0"]) == lay["y0"] and list(atlas["layout"]["rows"]) == lay["rows"]
    assert list(atlas["layout"]["cells_per_row"]) == lay["C"] and atlas["layout"]["cell"] == ar.CELLS
    return atlas


# ------------------------------------------------------------------------------------------------ build
@pytest.mark.parametrize("T", (0, 1, 2, 3, 255, 256, 257))
def test_build_equals_the_restatement_bit_for_bit(T):
    v, t = _triangles(T)
    atlas = _check_build(v, t, 40.0)
    if T >= 255:
        assert min(atlas["counts"]) > 0
    _check_build(v, t, 40.0, max_cell=8)  # capped at class 1


def test_build_on_the_graded_fixture_and_twice_the_same_bits():
    v, t, slot, order, totals = _graded()
    a = _check_build(v, t, ar.FIXTURE_DENSITY)
    b = _build(v, t, ar.FIXTURE_DENSITY)
    assert torch.equal(a["slot"], b["slot"]) and torch.equal(a["order"], b["order"]) and a["counts"] == b["counts"] and a["capped"] == 0
    assert _check_build(v, t, 3 * ar.FIXTURE_DENSITY)["capped"] == 2 * ar.REPEAT  # legs 2 and 1 need more than 61 steps


def test_build_with_a_bad_index_and_a_nan_corner():
    v, t = (np.array(a) for a in _triangles(300, seed=5))
    t[7, 1] = len(v)
    t[200, 0] = -1
    v[3 * 100 + 2, 1] = np.nan
    v[3 * 256, 0] = np.inf
    atlas = _check_build(v, t, 40.0)
    slot = atlas["slot"].cpu().numpy().view(np.uint32)
    assert all(slot[f] >> 28 == 0 for f in (7, 100, 200, 256))


def test_build_where_the_scan_takes_a_second_chunk():
    """T = 8192 * 256 + 257: 8194 workgroup sums per class, one more than a chunk of the scan holds.  Classes from a cheap arithmetic
    pattern: triangle f = (0, 1 + f % 7, 1 + (f / 7) % 7) over eight vertices on a line, at distances 2^-k from vertex 0.  Build only:
    that many large triangles have no atlas below 16384 texels a side."""
    T = 8192 * 256 + 257
    v = np.zeros((8, 3), F32)
    v[1:, 0] = 2.0 ** -np.arange(7)
    f = np.arange(T, dtype=np.int64)
    t = np.stack([np.zeros(T, np.int64), 1 + f % 7, 1 + (f // 7) % 7], 1)
    atlas = _check_build(v, t, 40.0, layout=False)
    assert min(atlas["counts"]) > 0 and atlas["capped"] == 0
    with pytest.raises(ValueError):
        ar.layout(atlas["counts"])


# ------------------------------------------------------------------------------------------------ points
def _points(v, t, atlas, n=None, rows=None):
    from pvd.mesh import texture_points
    x, nn = texture_points(_dev(v, F32).reshape(-1, 3), _dev(t, np.int32).reshape(-1, 3), atlas, normals=None if n is None else _dev(n, F32),
                           rows=rows)
    return x.cpu().numpy(), nn.cpu().numpy()


def _check_points(v, t, density, n=None, cuts=()):
    """cuts: the atlas in bands of rows that end at these rows (those below the height)."""
    atlas = _build(v, t, density)
    order = atlas["order"].cpu().numpy().view(np.uint32)
    Ht = atlas["layout"]["height"]
    edges = sorted({0, Ht} | {c for c in cuts if c < Ht})
    for row0, row1 in zip(edges[:-1], edges[1:]):
        x, nn = _points(v, t, atlas, n, rows=(row0, row1))
        wx, wn = ar.points(v, t, atlas["counts"], order, normals=n, row0=row0, row1=row1)
        _same(x, wx, ("x", row0, row1))
        _same(nn, wn, ("n", row0, row1))
    return atlas


@pytest.mark.parametrize("with_normals", (False, True))
def test_points_on_the_graded_fixture_equal_the_restatement_bit_for_bit(with_normals):
    v, t = _graded()[:2]
    n = np.random.RandomState(6).randn(len(v), 3).astype(F32) if with_normals else None
    atlas = _check_points(v, t, ar.FIXTURE_DENSITY, n)
    # row bands that cut through the class boundaries (y0 = 0, 4, 12, 28, 60), the last row alone, and an empty band
    assert atlas["layout"]["y0"] == (0, 4, 12, 28, 60) and atlas["layout"]["height"] == 124
    _check_points(v, t, ar.FIXTURE_DENSITY, n, cuts=(3, 13, 59, 61, 123))
    assert _points(v, t, atlas, n, rows=(13, 13))[0].shape == (0, 3)
    x, _ = _points(v, t, atlas)
    assert 0 < np.isnan(x).all(1).sum() < len(x)  # unowned texels: six NaNs


def test_points_on_a_one_class_mesh_and_with_an_empty_middle_class():
    v, t = _triangles(257)
    one = _check_points(v * F32(1e-3), t, 40.0)  # every edge below 1 / density: class 0 only
    assert one["counts"][1:] == (0, 0, 0, 0)
    legs = ar.classes(v, t, 40.0)[0]
    keep = np.array(t)[legs != 2]  # no triangle of class 2
    gap = _check_points(v, keep, 40.0)
    assert gap["counts"][2] == 0 and min(gap["counts"][:2] + gap["counts"][3:]) > 0
    y0 = gap["layout"]["y0"]
    assert y0[2] == y0[3]  # the empty band has no rows: classes 1 and 3 meet
    _check_points(v, keep, 40.0, cuts=(y0[3] - 1, y0[3] + 1, y0[4] + 5))


def test_points_of_invalid_triangles_are_nan():
    v, t = (np.array(a) for a in _triangles(40, seed=8))
    t[5, 2] = len(v) + 3
    v[3 * 11, 2] = np.nan
    n = np.random.RandomState(9).randn(len(v), 3).astype(F32)
    n[3 * 20 + 1, 0] = np.inf  # valid for the class, invalid for its texels when normals are given
    for normals in (None, n):
        atlas = _check_points(v, t, 40.0, normals)
        f = ar.owners(atlas["counts"], atlas["order"].cpu().numpy().view(np.uint32))[0].reshape(-1)
        x, nn = _points(v, t, atlas, normals)
        bad = [5, 11] + ([20] if normals is not None else [])
        assert np.isnan(x[np.isin(f, bad)]).all() and np.isnan(nn[np.isin(f, bad)]).all()
        assert np.isfinite(x[(f >= 0) & ~np.isin(f, bad)]).all()


# ------------------------------------------------------------------------------------------------ sample
def _lookups(T, N, seed):
    """tri and bary with everything the header names: -1, >= T, corners, the hypotenuse, outside [0, 1], NaN."""
    rng = np.random.RandomState(seed)
    tri = rng.randint(0, T, N).astype(np.int32)
    bary = rng.rand(N, 2).astype(F32)
    flip = bary.sum(1) > 1
    bary[flip] = F32(1) - bary[flip]
    kind = np.arange(N) % 10
    tri[kind == 1], tri[kind == 2] = -1, T + (np.arange(N)[kind == 2] % 3)
    bary[kind == 3] = [0, 0]
    bary[kind == 4] = [1, 0]
    bary[kind == 5] = [0, 1]
    bary[kind == 6, 1] = F32(1) - bary[kind == 6, 0]  # on the hypotenuse
    bary[kind == 7] = rng.uniform(-2, 3, ((kind == 7).sum(), 2)).astype(F32)
    bary[kind == 8, 0] = np.nan
    return tri, bary


@pytest.mark.parametrize("N", (1, 257, 1000))
def test_sample_equals_the_restatement_bit_for_bit(N):
    from pvd.mesh import sample_texture
    v, t, slot, order, totals = _graded()
    atlas = _build(v, t, ar.FIXTURE_DENSITY)
    lay = ar.layout(totals[:5])
    tex = np.random.RandomState(10).rand(lay["Ht"], lay["Wt"], 3).astype(F32)
    tri, bary = _lookups(len(t), N, 11 + N)
    if N == 1:
        tri[0], bary[0] = 1, [0.25, 0.5]
    got = sample_texture(_dev(tex, F32), atlas, len(t), _dev(tri, np.int32), _dev(bary, F32), bg_color=(0.25, 0.5, 0.75)).cpu().numpy()
    _same(got, ar.sample(tex, len(t), totals[:5], slot, tri, bary, (0.25, 0.5, 0.75)), N)
    # NaN everywhere but in the cells of the looked-up triangles: no read leaves the triangle's own cell, whatever bary holds
    some = np.where((tri >= 0) & (tri < len(t)), tri, 0) % 8 != 0  # (not the triangles of the leg 2: their cells are left NaN)
    tri2 = np.where(some, tri, -1).astype(np.int32)
    f_of = ar.owners(totals[:5], order)[0]
    rank = (slot & 0x0fffffff).astype(np.int64)
    by_cell = {(int(slot[f] >> 28), int(rank[f]) // 2) for f in set(tri2[(tri2 >= 0) & (tri2 < len(t))].tolist())}
    keep = np.zeros(f_of.shape, bool)
    for f in range(len(t)):
        if (int(slot[f] >> 28), int(rank[f]) // 2) in by_cell:
            keep |= f_of == f
    for c, k in by_cell:  # the unowned half of a half-used cell belongs to the cell too
        S, C, y0 = ar.CELLS[c], lay["C"][c], lay["y0"][c]
        keep[y0 + (k // C) * S:y0 + (k // C + 1) * S, (k % C) * S:(k % C + 1) * S] = True
    holed = np.where(keep[:, :, None], tex, F32(np.nan))
    got = sample_texture(_dev(holed, F32), atlas, len(t), _dev(tri2, np.int32), _dev(bary, F32), bg_color=0.0).cpu().numpy()
    assert np.isfinite(got).all()
    _same(got, ar.sample(tex, len(t), totals[:5], slot, tri2, bary, (0, 0, 0)), (N, "holed"))


# ------------------------------------------------------------------------------------------------ through pvd.mesh
def _wave(x, n):
    k = torch.tensor(ar.WAVE_K, dtype=torch.float64, device=x.device)
    s = x.to(torch.float64) @ k
    return (0.5 + 0.5 * torch.sin(s[:, None] + torch.tensor([0.0, 1.0, 2.0], dtype=torch.float64, device=x.device)[None, :])).to(torch.float32)


def test_bake_then_sample_stays_within_the_derived_bound_and_uv_sits_on_the_corner_texels():
    """The bound of tests/test_mesh_atex_restatement.py (0.02 from the density, plus its float32 term), on the device."""
    from pvd import mesh
    from test_mesh_atex_restatement import BOUND
    v, t, slot, order, totals = _graded()
    dv, dt = _dev(v, F32), _dev(t, np.int32)
    atlas = mesh.adaptive_atlas(dv, dt, ar.FIXTURE_DENSITY)
    baked = mesh.bake_texture(_wave, dv, dt, atlas)
    lay = ar.layout(totals[:5])
    assert baked["texture_cell"] is atlas and tuple(baked["texture"].shape) == (lay["Ht"], lay["Wt"], 3)
    assert baked["layout"] == mesh.texture_layout(len(t), atlas) and baked["layout"]["width"] == lay["Wt"]
    tri, bary = ar.random_lookups(len(t), 200, 0)
    got = mesh.sample_texture(baked["texture"], atlas, len(t), _dev(tri, np.int32), _dev(bary, F32)).cpu().numpy().astype(np.float64)
    err = np.abs(got - ar.wave_colour(ar.lookup_points(v, t, tri, bary))).max()
    print("bake_texture + sample_texture on the adaptive atlas: max error %.6f, bound %.6f" % (err, BOUND))
    assert err <= BOUND
    # uv: every corner on the centre of the texel that holds the corner's baked value
    uv = baked["uv"].cpu().numpy().astype(np.float64)
    np.testing.assert_allclose(uv, ar.uv(totals[:5], slot), rtol=0, atol=2.0 ** -23)
    ct = ar.corner_texels(totals[:5], slot)
    assert np.array_equal(np.floor(uv[..., 0] * lay["Wt"]).astype(np.int64), ct[..., 0])
    assert np.array_equal(np.floor((1.0 - uv[..., 1]) * lay["Ht"]).astype(np.int64), ct[..., 1])
    at_corner = baked["texture"].cpu().numpy()[ct[..., 1], ct[..., 0]]
    want = _wave(dv[dt.long().reshape(-1)], None).cpu().numpy().reshape(len(t), 3, 3)
    np.testing.assert_array_equal(at_corner, want)  # the corner's texel point is the corner, bit for bit
    assert np.array_equal(mesh.texture_uv(len(t), atlas, device=DEV).cpu().numpy(), baked["uv"].cpu().numpy())
    with pytest.raises(ValueError):
        mesh.texture_layout(len(t) + 1, atlas)


def test_render_mesh_returns_sample_textures_bits_at_the_casts_hits():
    from pvd import mesh
    v, t = _graded()[:2]
    dv, dt = _dev(v, F32), _dev(t, np.int32)
    atlas = mesh.adaptive_atlas(dv, dt, ar.FIXTURE_DENSITY)
    baked = mesh.bake_texture(_wave, dv, dt, atlas)
    pose = np.eye(4, dtype=F32)
    pose[:3, 3] = [0.1, -0.05, -3.0]
    out = mesh.render_mesh(dv, dt, pose, (90.0, 90.0, 32.0, 32.0), 64, 64, bg_color=(0.1, 0.2, 0.3), texture=baked["texture"],
                           texture_cell=baked["texture_cell"])
    assert int(out["mask"].sum()) > 500
    want = mesh.sample_texture(baked["texture"], atlas, len(t), out["tri"], out["bary"], bg_color=(0.1, 0.2, 0.3))
    assert torch.equal(out["color"], want)
    host = ar.sample(baked["texture"].cpu().numpy(), len(t), atlas["counts"], atlas["slot"].cpu().numpy().view(np.uint32),
                     out["tri"].cpu().numpy().reshape(-1), out["bary"].cpu().numpy().reshape(-1, 2), (0.1, 0.2, 0.3))
    _same(out["color"].cpu().numpy().reshape(-1, 3), host)
    rep = mesh.evaluate_mesh_views(dv, dt, None, [pose], (90.0, 90.0, 32.0, 32.0), 64, 64, out["color"][None], bg_color=(0.1, 0.2, 0.3),
                                   texture=baked["texture"], texture_cell=atlas)
    assert rep["coverage"] == float(out["mask"].sum()) / (64 * 64) and "psnr" in rep


def test_an_integer_cell_edge_does_what_it_did():
    """With an integer S every touched function returns the uniform atlas's bits (tests/mesh_tex_restatement.py), and no new key."""
    from pvd import mesh
    v, t = _triangles(257)
    dv, dt = _dev(v, F32), _dev(t, np.int32)
    T, S = len(t), 8
    C, rows, Wt, Ht = tr.layout(T, S)
    assert mesh.texture_layout(T, S) == dict(cells_per_row=C, rows=rows, width=Wt, height=Ht, cell=S, triangles=T)
    x, n = mesh.texture_points(dv, dt, S)
    wx, wn = tr.points(v, t, S)
    _same(x.cpu().numpy(), wx)
    _same(n.cpu().numpy(), wn)
    np.testing.assert_array_equal(mesh.texture_uv(T, S).numpy(), tr.uv(T, S).astype(F32))
    baked = mesh.bake_texture(_wave, dv, dt, S)
    assert sorted(baked) == ["layout", "texture", "uv"]
    tex = np.where(np.isnan(wx), 0, _wave(torch.from_numpy(np.nan_to_num(wx)).to(DEV), None).cpu().numpy()).reshape(Ht, Wt, 3)
    np.testing.assert_array_equal(baked["texture"].cpu().numpy(), tex)
    tri, bary = _lookups(T, 1000, 12)
    got = mesh.sample_texture(baked["texture"], S, T, _dev(tri, np.int32), _dev(bary, F32), bg_color=0.5).cpu().numpy()
    _same(got, tr.sample(tex, T, S, tri, bary, (0.5, 0.5, 0.5)))


def test_sh_atlases_refuse_an_adaptive_atlas():
    from pvd import mesh
    v, t = _graded()[:2]
    dv, dt = _dev(v, F32), _dev(t, np.int32)
    atlas = mesh.adaptive_atlas(dv, dt, ar.FIXTURE_DENSITY)
    with pytest.raises(ValueError):
        mesh.bake_sh_texture(lambda x, d: x, dv, dt, atlas, degree=2)
    with pytest.raises(ValueError):
        mesh.sample_sh_texture(torch.zeros(124, 128, 4, 3, device=DEV), atlas, len(t), _dev([0], np.int32), _dev([[0.2, 0.2]], F32),
                               _dev([[0, 0, 1]], F32))
    with pytest.raises(ValueError):
        mesh.render_mesh(dv, dt, np.eye(4, dtype=F32), (90.0, 90.0, 8.0, 8.0), 16, 16, texture=torch.zeros(124, 128, 4, 3, device=DEV),
                         texture_cell=atlas)


# ------------------------------------------------------------------------------------------------ tools/export_mesh.py
def test_export_mesh_texture_density_through_main(tmp_path, monkeypatch, capsys):
    """export_mesh.py --simplify G --clean --texture-density D run through main() on a saved tiny checkpoint (the fixture pattern of
    tests/test_hip_mesh_project.py): the flag checks, the line with the class counts, an OBJ whose vt lines are texture_uv(atlas) and a PNG
    of Wt x Ht."""
    from pvd import mesh
    from pvd.checkpoint import save_checkpoint
    from test_hip_mesh_project import _export_model
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import export_mesh
    ckpt = save_checkpoint(os.path.join(str(tmp_path), "tiny.pth"), _export_model())
    monkeypatch.setattr(export_mesh, "make_model", lambda *a, **k: _export_model())
    atlases = []
    real = mesh.adaptive_atlas
    monkeypatch.setattr(mesh, "adaptive_atlas", lambda *a, **k: (atlases.append(real(*a, **k)), atlases[-1])[1])
    out = os.path.join(str(tmp_path), "mesh.ply")
    common = [ckpt, "-o", out, "--model-type", "hash", "--resolution0", "64", "--resolution", "24", "--tsdf", "6", "--tsdf-res", "48x48",
              "--simplify", "6", "--clean"]
    for bad in (["--texture-density", "-1"], ["--texture-density", "nan"], ["--texture-density", "30", "--texture", "12"],
                ["--texture-density", "30", "--texture", "16", "--texture-sh", "2"]):
        with pytest.raises(SystemExit):
            export_mesh.main(common + bad)
    capsys.readouterr()
    export_mesh.main(common + ["--texture-density", "12", "--texture", "16", "--render-check", "1"])
    text = capsys.readouterr().out
    assert "adaptive texture" in text and "capped" in text and "fill" in text and "textured mesh" in text, text
    atlas = atlases[0]
    assert atlas["counts"][4] == 0 and atlas["counts"][3] == 0 and sum(atlas["counts"]) == atlas["triangles"] > 0  # --texture 16 caps the class
    obj = mesh.read_obj(out[:-4] + ".obj")
    t, uv = obj["triangles"], obj["uv"]
    totals = ar.build(obj["vertices"].numpy(), t.numpy(), 12.0, max_class=2)[2]  # the OBJ's floats come back bit for bit
    assert list(atlas["counts"]) + [atlas["capped"]] == totals.tolist()
    print("export: classes %s, %d capped" % (atlas["counts"], atlas["capped"]))
    want = mesh.texture_uv(atlas["triangles"], atlas).cpu().numpy()
    assert len(t) == atlas["triangles"]
    np.testing.assert_allclose(np.asarray(uv, np.float64).reshape(-1, 2), want.reshape(-1, 2).astype(np.float64), rtol=0, atol=1e-6)
    png = mesh.read_png(out[:-4] + ".png")
    assert tuple(png.shape[:2]) == (atlas["layout"]["height"], atlas["layout"]["width"])
