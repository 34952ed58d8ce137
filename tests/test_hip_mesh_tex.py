"""pvd_mesh_tex_points / pvd_mesh_tex_sample (csrc/mesh_tex.hip, include/pvd_hip_mesh_tex.h) and what pvd/mesh.py builds on them --
texture_points, bake_texture, sample_texture, render_mesh(texture=...), evaluate_mesh_views(texture=...), extract_surface(texture=S) --
against the numpy restatement (tests/mesh_tex_restatement.py, pinned by tests/test_mesh_tex_restatement.py).

Tolerance.  None: a texel's point and a lookup are a handful of float32 operations that the device and numpy do unfused in the same
order, so the results are compared on their bits (assert_array_equal, NaN positions included).  A difference means a fused or reordered
operation, a texel given to the wrong triangle, or a read outside the cell.

Sizes.  Meshes: the fixtures of mesh_dist_restatement.FIXTURES at R = 9 and 17 through extract_mesh (some 300 to 2 500 triangles; at
S = 16 up to 36 x 36 cells, three workgroups along x).  S = 4 (m = 1: every texel but three per triangle is extrapolated), 5, 8, 16.
T as extracted, T - 1 (odd: the last cell half owned), 1, 0.  N = 1, 257 (a second workgroup with one lane), 1000."""
import functools

import numpy as np
import pytest
import torch

import mesh_dist_restatement as md
import mesh_normals_restatement as nr
import mesh_tex_restatement as tr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BMIN, BMAX, THRESH = md.BMIN, md.BMAX, md.THRESH
MESHES = tuple(f for f in md.FIXTURES if f[1] in (9, 17))
CELLS = (4, 5, 8, 16)
F32 = np.float32


def _dev(a, dt):
    return torch.from_numpy(np.array(a, dt)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _mesh(kind, R):
    """(vertices, triangles, normals) as extract_mesh returns them, as read-only host arrays."""
    from pvd.mesh import extract_mesh
    u = np.array(nr.field(kind, R, THRESH))
    v, t, n = (a.cpu().numpy() for a in extract_mesh(torch.from_numpy(u).to(DEV), THRESH, BMIN, BMAX, with_normals=True))
    assert np.array_equal(t, md.fixture(kind, R)[1]) and np.all(np.isfinite(n))
    for a in (v, t, n):
        a.setflags(write=False)
    return v, t, n


def _points(v, t, S, n=None, rows=None):
    from pvd.mesh import texture_points
    x, nn = texture_points(_dev(v, F32).reshape(-1, 3), _dev(t, np.int32).reshape(-1, 3), S, normals=None if n is None else _dev(n, F32), rows=rows)
    return x.cpu().numpy(), nn.cpu().numpy()


def _same(got, want, what):
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=str(what))
    np.testing.assert_array_equal(_bits(np.nan_to_num(got)), _bits(np.nan_to_num(want)), err_msg=str(what))
    np.testing.assert_array_equal(got, want, err_msg=str(what))


@pytest.mark.parametrize("kind,R", MESHES)
@pytest.mark.parametrize("S", CELLS)
def test_points_equal_the_restatement_bit_for_bit(kind, R, S):
    v, t, n = _mesh(kind, R)
    for normals in (None, n):
        wx, wn = tr.points(v, t, S, normals)
        gx, gn = _points(v, t, S, normals)
        _same(gx, wx, (kind, R, S, normals is not None, "x"))
        _same(gn, wn, (kind, R, S, normals is not None, "n"))
    assert np.isfinite(wx).any() and (len(t) % 2 == 0 or np.isnan(wx).any())


@pytest.mark.parametrize("S", CELLS)
def test_points_for_an_odd_count_one_triangle_and_none(S):
    v, t, n = _mesh("sphere", 9)
    for T in (len(t) - 1, 1, 0):
        assert T <= 1 or T % 2 == 1  # the last cell is half owned
        for normals in (None, n):
            wx, wn = tr.points(v, t[:T], S, normals)
            gx, gn = _points(v, t[:T], S, normals)
            assert gx.shape == wx.shape == (tr.layout(T, S)[2] * tr.layout(T, S)[3], 3)
            _same(gx, wx, (T, S, "x"))
            _same(gn, wn, (T, S, "n"))
        if T == 0:
            assert gx.shape == (S * S, 3) and np.all(np.isnan(gx)) and np.all(np.isnan(gn))
        if T % 2 == 1:
            f = tr.owners(T, S)[0].reshape(-1)
            assert np.all(np.isnan(gx[f >= T])) and np.all(np.isfinite(gx[f < T])) and (f >= T).sum() >= S * (S - 1) // 2
    # an empty vertex array under triangles that point nowhere: every texel is a NaN, nothing is read
    gx, gn = _points(np.zeros((0, 3), F32), t[:5], S)
    assert np.all(np.isnan(gx)) and np.all(np.isnan(gn))


def test_points_of_a_mesh_with_a_bad_index_a_nan_corner_and_a_nan_normal():
    v, t, n = (np.array(a) for a in _mesh("torus", 17))
    t = t[:301].copy()
    t[7, 2] = len(v)  # out of range
    t[8, 0] = -1
    v[t[40, 1], 0] = np.nan  # a corner
    v[t[41, 2], 2] = np.inf
    n[t[100, 0], 1] = np.nan  # a normal: invalid only when normals are given
    for S in (5, 8):
        for normals in (None, n):
            ok = tr.valid(v, t, normals)
            assert not ok[7] and not ok[8] and not ok[40] and not ok[41] and ok[100] == (normals is None) and ok.sum() > 250
            wx, wn = tr.points(v, t, S, normals)
            gx, gn = _points(v, t, S, normals)
            _same(gx, wx, (S, "x"))
            _same(gn, wn, (S, "n"))
            f = tr.owners(len(t), S)[0].reshape(-1)
            bad = (f >= len(t)) | ~ok[np.minimum(f, len(t) - 1)]
            assert np.array_equal(np.isnan(gx).all(1), bad) and np.array_equal(np.isnan(gn).all(1), bad) and np.array_equal(np.isnan(gx).any(1), bad)


@pytest.mark.parametrize("S", (5, 16))
def test_points_in_row_bands(S):
    import pvd_hip
    v, t, n = _mesh("sphere", 17)
    C, rows, Wt, Ht = tr.layout(len(t), S)
    wx, wn = tr.points(v, t, S, n)
    dv, dt, dn = _dev(v, F32), _dev(t, np.int32), _dev(n, F32)
    for r0, r1 in ((0, Ht), (S + 1, S + 2), (S - 2, 2 * S + 3), (Ht - 1, Ht), (7, 7), (Ht, Ht)):
        gx, gn = _points(v, t, S, n, rows=(r0, r1))
        assert gx.shape == ((r1 - r0) * Wt, 3)
        _same(gx, wx[r0 * Wt:r1 * Wt], (S, r0, r1, "x"))
        _same(gn, wn[r0 * Wt:r1 * Wt], (S, r0, r1, "n"))
    # a band writes its own rows and nothing after them
    r0, r1 = S - 1, S + 1
    x = torch.full(((r1 - r0) * Wt + 64, 3), 7.0, device=DEV)
    nn = torch.full(((r1 - r0) * Wt + 64, 3), 7.0, device=DEV)
    pvd_hip.mesh_tex_points(dv, dt, dn, S, r0, r1, x[:(r1 - r0) * Wt], nn[:(r1 - r0) * Wt])
    assert bool((x[(r1 - r0) * Wt:] == 7.0).all()) and bool((nn[(r1 - r0) * Wt:] == 7.0).all())
    _same(x[:(r1 - r0) * Wt].cpu().numpy(), wx[r0 * Wt:r1 * Wt], "guarded band")
    for bad in ((3, 2), (0, Ht + 1)):
        with pytest.raises(pvd_hip.PvdHipError):
            pvd_hip.mesh_tex_points(dv, dt, dn, S, bad[0], bad[1], x[:0], nn[:0])


def _lookups(T, S, N, seed):
    """(tri [N] int32, bary [N,2] f32): a seeded mix of interior weights, the three corners, edges, beta + gamma = 1 + 2^-23, negative
    weights, NaN and inf, with tri = -1 and tri >= T mixed in.  N = 1: one interior lookup."""
    rng = np.random.RandomState(seed)
    r1, r2 = np.sqrt(rng.rand(N)), rng.rand(N)
    bary = np.stack([r1 * (1 - r2), r1 * r2], 1).astype(F32)
    tri = rng.randint(0, max(T, 1), N).astype(np.int32)
    if N >= 100:
        m = S - 3
        special = [(0, 0), (1, 0), (0, 1), (0.5, 0), (0, 0.25), (0.5, 0.5), (0.25, 0.75), (F32(0.5), F32(0.5) + F32(2.0 ** -23)),
                   (F32(1.0 + 2.0 ** -23), 0), (-0.25, 0.5), (0.5, -1e-3), (-2, -2), (np.nan, 0.5), (0.5, np.nan), (np.nan, np.nan),
                   (np.inf, 0), (0, -np.inf), (np.inf, np.inf), (3.0, 5.0), (1e30, -1e30), (1.0 / m, 1.0 - 1.0 / m), (2.0 ** -149, 0)]
        for e, b in enumerate(special * 2):  # once on an even and once on an odd triangle (where T allows)
            bary[3 * e] = b
            tri[3 * e] = min(2 * (e % 7) + e // len(special), max(T - 1, 0))
        tri[1::10] = -1
        tri[4::25] = T
        tri[5::50] = 2 ** 31 - 1
        tri[6::50] = -2 ** 31
    return tri, bary


@pytest.mark.parametrize("S", CELLS)
@pytest.mark.parametrize("N", (1, 257, 1000))
def test_sample_equals_the_restatement_bit_for_bit(S, N):
    from pvd.mesh import sample_texture
    v, t, _ = _mesh("two_spheres", 17)
    for T in (len(t), len(t) - 1, 1):
        C, rows, Wt, Ht = tr.layout(T, S)
        tex = np.random.RandomState(S + T).rand(Ht, Wt, 3).astype(F32)
        tri, bary = _lookups(T, S, N, 31 * N + S)
        bg = (0.25, 1.0, 0.5)
        want = tr.sample(tex, T, S, tri, bary, bg)
        got = sample_texture(_dev(tex, F32), S, T, _dev(tri, np.int32), _dev(bary, F32), bg_color=bg).cpu().numpy()
        assert got.shape == (N, 3) and np.all(np.isfinite(want))
        np.testing.assert_array_equal(_bits(got), _bits(want), err_msg=str((S, N, T)))
        out = (tri < 0) | (tri >= T)
        assert np.array_equal(got[out], np.tile(np.array(bg, F32), (out.sum(), 1)))
    # a shaped request keeps its shape, and a scalar background spreads
    img = sample_texture(_dev(tex, F32), S, T, _dev(tri[:1], np.int32).reshape(1, 1), _dev(bary[:1], F32).reshape(1, 1, 2), bg_color=0.5)
    assert tuple(img.shape) == (1, 1, 3)


def test_sample_with_no_rows_and_no_triangles():
    from pvd.mesh import sample_texture
    tex = torch.rand(4, 4, 3, device=DEV)
    out = sample_texture(tex, 4, 0, torch.tensor([0, -1, 7], dtype=torch.int32, device=DEV), torch.zeros(3, 2, device=DEV), bg_color=(0.0, 0.5, 1.0))
    assert out.cpu().tolist() == [[0.0, 0.5, 1.0]] * 3
    none = sample_texture(tex, 4, 1, torch.zeros(0, dtype=torch.int32, device=DEV), torch.zeros(0, 2, device=DEV))
    assert tuple(none.shape) == (0, 3)


@pytest.mark.parametrize("S", CELLS)
def test_unowned_texels_are_never_read(S):
    """The unowned tail of the atlas -- the upper half of the last cell of an odd T, and the cells after it -- is filled with NaN: no
    lookup of a valid tri comes back NaN.  The weights are those of _lookups -- corners, edges, beta + gamma = 1 + 2^-23, negative, NaN
    and inf among them -- but for the few that still lie outside the triangle after the header's clamp to [0, m] ((3, 5), (inf, inf)):
    those may read the other half of their own cell, as the header says, and are put on the corner c here."""
    from pvd.mesh import sample_texture
    v, t, _ = _mesh("sphere", 9)
    T = len(t) - 1
    Wt, Ht = tr.layout(T, S)[2:]
    f = tr.owners(T, S)[0]
    tex = np.random.RandomState(S).rand(Ht, Wt, 3).astype(F32)
    tex[f >= T] = np.nan
    assert np.isnan(tex).any()
    tri, bary = _lookups(T, S, 1000, S)
    tri[::3] = T - 1  # the half-owned cell's triangle, often
    clamped = np.clip(np.nan_to_num(bary.astype(np.float64), nan=0.0, posinf=1.0, neginf=0.0), 0.0, 1.0)
    outside = clamped.sum(1) > 1.0 + 2.0 ** -22
    assert 0 < outside.sum() < 10
    bary[outside] = (0.0, 1.0)
    got = sample_texture(_dev(tex, F32), S, T, _dev(tri, np.int32), _dev(bary, F32), bg_color=0.0).cpu().numpy()
    assert not np.isnan(got).any()
    np.testing.assert_array_equal(_bits(got), _bits(tr.sample(tex, T, S, tri, bary, (0, 0, 0))))


# what the CPU restatement of the job gives (tests/mesh_tex_restatement.py: job_on_the_host; profiles/mesh_tex.txt): the mean squared
# error of the vertex-coloured render over that of the textured one
RECORDED_RATIO = 10478.7


def test_a_baked_texture_follows_a_colour_field_the_vertex_colours_cannot():
    """The job, end to end: bake the sphere fixture (R = 17) at S = 16 from 0.5 + 0.5 sin(20 x), render 64 x 64 with the texture and
    with vertex colours, compare both with the analytic colour at the hit points.  The textured error must be below the
    vertex-coloured one by half the ratio the CPU restatement recorded -- a margin for the render's different hit set, nothing else."""
    from pvd.mesh import bake_texture, render_mesh
    v, t, n = _mesh("sphere", tr.JOB_R)
    dv, dt, dn = _dev(v, F32), _dev(t, np.int32), _dev(n, F32)

    def source(x, nrm):
        assert x.shape == nrm.shape and bool(torch.isfinite(x).all()) and bool((torch.linalg.norm(nrm, dim=1) - 1).abs().max() < 1e-5)
        return 0.5 + 0.5 * torch.sin(tr.JOB_K * x)
    baked = bake_texture(source, dv, dt, tr.JOB_S, normals=dn, chunk=20000)  # several bands
    lay = baked["layout"]
    assert tuple(baked["texture"].shape) == (lay["height"], lay["width"], 3) and tuple(baked["uv"].shape) == (len(t), 3, 2)
    assert lay["height"] > 3 * (20000 // lay["width"]) > 0  # more than three bands
    tex = baked["texture"]
    assert bool(torch.isfinite(tex).all()) and 0.0 <= float(tex.min()) and float(tex.max()) <= 1.0
    whole = bake_texture(source, dv, dt, tr.JOB_S, normals=dn)
    assert torch.equal(whole["texture"], tex)  # the bands do not show
    col = (0.5 + 0.5 * torch.sin(tr.JOB_K * dv)).contiguous()
    pose = torch.from_numpy(tr.JOB_POSE).to(DEV)
    hw = tr.JOB_HW
    textured = render_mesh(dv, dt, pose, tr.JOB_INTRINSICS, hw, hw, texture=tex, texture_cell=tr.JOB_S)
    coloured = render_mesh(dv, dt, pose, tr.JOB_INTRINSICS, hw, hw, colors=col)
    assert torch.equal(textured["tri"], coloured["tri"]) and torch.equal(textured["bary"], coloured["bary"])
    assert bool((textured["color"][~textured["mask"]] == 1.0).all())
    o, d = tr.job_rays()
    t_hit = torch.where(textured["mask"], textured["depth"], torch.zeros_like(textured["depth"])).cpu().numpy()
    e_tex, e_vc, hits = tr.job_errors(v, t, t_hit, textured["tri"].cpu().numpy(), None, textured["color"].cpu().numpy(),
                                      coloured["color"].cpu().numpy(), o, d)
    print("textured mse %.3e, vertex-coloured mse %.3e, ratio %.1f (recorded on the host: %.1f), %d pixels hit"
          % (e_tex, e_vc, e_vc / e_tex, RECORDED_RATIO, hits))
    assert hits > 1500
    assert e_tex * (RECORDED_RATIO / 2) <= e_vc


def test_the_defaults_return_what_they_returned():
    """render_mesh and evaluate_mesh_views without a texture, and extract_surface(texture=0): the same call with and without the new
    keywords, bit for bit; and extract_surface(texture=S) adds its three entries to an otherwise identical dict."""
    from pvd.mesh import evaluate_mesh_views, extract_surface, render_mesh, texture_layout
    from test_hip_mesh_normals import _AnalyticSphere
    v, t, n = _mesh("sphere", 17)
    dv, dt, dn = _dev(v, F32), _dev(t, np.int32), _dev(n, F32)
    col = (0.5 + 0.4 * dn).clamp(0.0, 1.0)
    pose = torch.from_numpy(tr.JOB_POSE).to(DEV)
    intr, hw = tr.JOB_INTRINSICS, 32
    for kw in (dict(), dict(normals=dn), dict(colors=col, bg_color=(1.0, 0.0, 0.5)), dict(normals=dn, colors=col, grid=5)):
        a = render_mesh(dv, dt, pose, intr, hw, hw, **kw)
        b = render_mesh(dv, dt, pose, intr, hw, hw, texture=None, texture_cell=None, **kw)
        assert sorted(a) == sorted(b) == ["bary", "color", "depth", "mask", "normal", "tri"]
        for key in a:
            assert (a[key] is None and b[key] is None) or torch.equal(a[key], b[key]), key
    empty = render_mesh(dv, dt[:0], pose, intr, hw, hw)
    assert empty["color"] is None
    lay = texture_layout(0, 4)
    blank = render_mesh(dv, dt[:0], pose, intr, hw, hw, texture=torch.zeros(lay["height"], lay["width"], 3, device=DEV), texture_cell=4, bg_color=0.25)
    assert bool((blank["color"] == 0.25).all())
    with pytest.raises(ValueError):
        render_mesh(dv, dt, pose, intr, hw, hw, texture=torch.zeros(4, 4, 3, device=DEV))
    poses = pose[None]
    truth = torch.full((1, hw, hw, 3), 0.5, device=DEV)
    ra = evaluate_mesh_views(dv, dt, col, poses, intr, hw, hw, truth, keep_images=True)
    rb = evaluate_mesh_views(dv, dt, col, poses, intr, hw, hw, truth, keep_images=True, texture=None, texture_cell=None)
    assert sorted(ra) == sorted(rb) and torch.equal(ra["images"][0], rb["images"][0])
    assert all(ra[k] == rb[k] for k in ra if k != "images")
    # with a texture the colours may be None, and a texture baked from the vertex-colour interpolation's own corners scores close to it
    S = 8
    flat = torch.full((texture_layout(len(t), S)["height"], texture_layout(len(t), S)["width"], 3), 0.5, device=DEV)
    rt = evaluate_mesh_views(dv, dt, None, poses, intr, hw, hw, truth, bg_color=0.5, texture=flat, texture_cell=S)
    assert rt["psnr"] == float("inf") and rt["coverage"] == ra["coverage"]
    model, R = _AnalyticSphere(), 24
    plain = extract_surface(model, resolution=R)
    zero = extract_surface(model, resolution=R, texture=0)
    assert sorted(zero) == sorted(plain) == ["colors", "counts", "field", "normals", "threshold", "triangles", "vertices"]
    for key in ("vertices", "triangles", "normals", "colors", "field"):
        assert torch.equal(zero[key], plain[key]), key
    m = extract_surface(model, resolution=R, texture=5)
    assert sorted(m) == sorted(list(plain) + ["texture", "texture_cell", "uv"]) and m["texture_cell"] == 5
    for key in ("vertices", "triangles", "normals", "colors", "field"):
        assert torch.equal(m[key], plain[key]), key
    T = int(m["triangles"].shape[0])
    lay = texture_layout(T, 5)
    assert tuple(m["texture"].shape) == (lay["height"], lay["width"], 3) and tuple(m["uv"].shape) == (T, 3, 2)
    assert bool(torch.isfinite(m["texture"]).all()) and 0.0 <= float(m["texture"].min()) and float(m["texture"].max()) <= 1.0
    # the texel at a corner holds what the model's colour head gives at that vertex along its normal: the vertex colour
    ct = tr.corner_texels(T, 5)
    tri = m["triangles"].cpu().numpy()
    at_corner = m["texture"].cpu().numpy()[ct[:, 0, 1], ct[:, 0, 0]]
    assert np.abs(at_corner - m["colors"].cpu().numpy()[tri[:, 0]]).max() <= 2e-3
    small = extract_surface(model, resolution=R, simplify=4, clean=True, texture=4)  # baked last, on the final mesh
    assert tuple(small["uv"].shape) == (int(small["triangles"].shape[0]), 3, 2)
    assert tuple(small["texture"].shape)[:2] == tuple(texture_layout(int(small["triangles"].shape[0]), 4)[k] for k in ("height", "width"))
