"""pvd_mesh_shtex_basis / _dirs / _project / _sample (csrc/mesh_shtex.hip, csrc/pvd_hip_mesh_shtex.h) and what pvd/mesh.py builds on them
-- sh_basis, bake_sh_texture, sample_sh_texture, render_mesh with a 4-D texture, extract_surface(texture_sh=L) -- against the numpy
restatement (tests/mesh_shtex_restatement.py, pinned by tests/test_mesh_shtex_restatement.py).

Tolerance.  None for the kernels: the header orders every float32 operation and fuses none, the device and numpy do the same ones, so
the results are compared on their bytes.  A difference means a fused or reordered operation, a wrong texel or a wrong coefficient.  The
two end-to-end cases carry the CPU test's bound (planar recovery) and an ordering (the curved case).

Sizes.  The smallest at which each kernel takes every path: one lane, one wave, one wave and a lane, a second workgroup with one lane
(257), N = 4099 for the sample; T = 1, 2, 3, 5, 200 (one cell, a half-owned last cell, several rows of cells); S = 4, 5, 16."""
import functools

import numpy as np
import pytest
import torch

import mesh_dist_restatement as md
import mesh_normals_restatement as nr
import mesh_shtex_restatement as sr
import mesh_tex_restatement as tr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
BANDS = (1, 2, 3, 4)


def _dev(a, dt):
    return torch.from_numpy(np.array(a, dt)).to(DEV)


def _same(got, want, what):
    got, want = np.ascontiguousarray(got, F32), np.ascontiguousarray(want, F32)
    assert got.shape == want.shape, what
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32), err_msg=str(what))


def _directions(N, seed):
    """[N,3] f32: random unit directions, with the six axes, (0,0,0) and a vector that is not unit where N has room for them."""
    rng = np.random.RandomState(seed)
    d = rng.normal(size=(N, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    special = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [0, 0, 0], [0.3, -1.7, 2.2]], float)
    if N >= 63:
        d[5:5 + len(special)] = special
    return d.astype(F32)


# ------------------------------------------------------------------------------------------------ the basis
@pytest.mark.parametrize("L", BANDS)
@pytest.mark.parametrize("N", (1, 63, 64, 65, 257))
def test_the_basis_equals_the_restatement_bit_for_bit(L, N):
    import pvd_hip
    from pvd.mesh import sh_basis
    d = _directions(N, 3 * N + L)
    want = sr.basis(d, L)
    _same(sh_basis(_dev(d, F32), L).cpu().numpy(), want, (L, N))
    out = torch.full((N + 5, L * L), 7.0, device=DEV)  # rows past N are not written
    pvd_hip.mesh_shtex_basis(_dev(d, F32), L, out[:N])
    assert bool((out[N:] == 7.0).all())
    _same(out[:N].cpu().numpy(), want, (L, N, "guarded"))


# ------------------------------------------------------------------------------------------------ the mirrored directions
def _normals(M, seed):
    """[M,3] f32: unnormalised normals over several magnitudes; from M = 255 on with a zero, a NaN, an inf, one that underflows, one
    in the plane z = 0 (tangent to the axis the test puts among the directions: s == 0), and one along the first fitting direction
    (averted) and one against it (facing)."""
    rng = np.random.RandomState(seed)
    n = (rng.normal(size=(M, 3)) * np.exp(rng.uniform(-4, 4, size=(M, 1)))).astype(F32)
    if M >= 255:
        u = tr_dirs()[0].astype(np.float64)
        n[3:11] = np.array([[0, 0, 0], [np.nan, 1, 0], [0, np.inf, 0], [1e-30, 0, 0], [2, -3, 0], 2.5 * u, -0.5 * u, [0, 0, 3.0]], F32)
    return n


def tr_dirs():
    from pvd.mesh import exposure_directions
    return exposure_directions(64).numpy()


@pytest.mark.parametrize("M", (1, 255, 256, 257))
@pytest.mark.parametrize("J", (1, 3, 8))
def test_the_query_directions_equal_the_restatement_bit_for_bit(M, J):
    import pvd_hip
    n = _normals(M, 7 * M + J)
    U = tr_dirs()[:J].copy()
    if J == 8:
        U[5] = (0.0, 0.0, 1.0)  # an axis: s == 0 against every normal in the plane z = 0
    want = sr.mirrored(n, U)
    d = torch.full((J * M + 3, 3), 7.0, device=DEV)
    pvd_hip.mesh_shtex_dirs(_dev(n, F32), _dev(U, F32), d[:J * M].view(J, M, 3))
    assert bool((d[J * M:] == 7.0).all())
    got = d[:J * M].view(J, M, 3).cpu().numpy()
    _same(got, want, (M, J))
    assert not np.isnan(got).any()  # a NaN normal leaves the direction as it is
    if M >= 255:
        keep = np.broadcast_to(U[:, None, :], got.shape)
        for row in (3, 4, 5, 6):  # zero, NaN, inf, underflow: d = u as bits
            _same(got[:, row], keep[:, row], (M, J, row))
        if J == 8:
            _same(got[5, 7], U[5], "tangent: s == 0")
            _same(got[5, 10], np.array([0, 0, -1], F32), "the axis mirrored in the plane z = 0")
        _same(got[0, 9], U[0], "facing")
        assert got[0, 8].tobytes() != U[0].tobytes() and float(np.dot(got[0, 8].astype(np.float64), n[8])) < 0  # averted: mirrored


# ------------------------------------------------------------------------------------------------ the projection
@pytest.mark.parametrize("L", BANDS)
@pytest.mark.parametrize("M", (1, 255, 256, 257))
def test_the_projection_equals_the_restatement_and_ignores_the_batch_split(L, M):
    import pvd_hip
    rng = np.random.RandomState(11 * M + L)
    D, K = 7, L * L
    rgb = rng.rand(D, M, 3).astype(F32)
    P = rng.normal(size=(K, D)).astype(F32)
    want = sr.project(rgb, P)
    drgb, dP = _dev(rgb, F32), _dev(P, F32)
    results = []
    for split in ((7,), (3, 4), (1,) * 7):
        buf = torch.full((M * K * 3 + 64,), 7.0, device=DEV)  # prefilled: first=1 must ignore it; and a guard after coef
        coef = buf[:M * K * 3].view(M, K, 3)
        j0 = 0
        for J in split:
            pvd_hip.mesh_shtex_project(drgb[j0:j0 + J].contiguous(), dP[:, j0:j0 + J].contiguous(), L, coef, j0 == 0)
            j0 += J
        assert bool((buf[M * K * 3:] == 7.0).all()), split
        results.append(coef.cpu().numpy())
        _same(results[-1], want, (L, M, split))
    assert results[0].tobytes() == results[1].tobytes() == results[2].tobytes()
    _same(want, sr.project_batched(rgb, P, 3), "the restatement's own split")
    # first = 0 continues from what coef holds
    start = rng.rand(M, K, 3).astype(F32)
    coef = _dev(start, F32)
    pvd_hip.mesh_shtex_project(drgb, dP, L, coef, False)
    _same(coef.cpu().numpy(), sr.project(rgb, P, start), (L, M, "continued"))


def test_the_projection_with_nothing_to_do_leaves_coef_alone():
    import pvd_hip
    coef = torch.full((4, 9, 3), 7.0, device=DEV)
    pvd_hip.mesh_shtex_project(torch.zeros(0, 4, 3, device=DEV), torch.zeros(9, 0, device=DEV), 3, coef, True)
    assert bool((coef == 7.0).all())
    pvd_hip.mesh_shtex_project(torch.zeros(2, 0, 3, device=DEV), torch.zeros(9, 2, device=DEV), 3, coef[:0], True)
    pvd_hip.mesh_shtex_dirs(torch.zeros(0, 3, device=DEV), torch.ones(2, 3, device=DEV), torch.zeros(2, 0, 3, device=DEV))
    with pytest.raises(pvd_hip.PvdHipError):
        pvd_hip.mesh_shtex_project(torch.zeros(2, 4, 3, device=DEV), torch.zeros(9, 2, device=DEV), 5, coef, True)


# ------------------------------------------------------------------------------------------------ the sample
def _lookups(T, S, N, seed):
    """(tri [N] int32, bary [N,2] f32, dirs [N,3] f32): random interior points and unit directions; from N = 64 on also the three
    corners, every whole point of the hypotenuse (on the odd triangle 1 where T > 1: the weight-zero read of the tex header), a NaN
    bary, tri = -1 and tri = T."""
    rng = np.random.RandomState(seed)
    r1, r2 = np.sqrt(rng.rand(N)), rng.rand(N)
    bary = np.stack([r1 * (1 - r2), r1 * r2], 1).astype(F32)
    tri = rng.randint(0, T, N).astype(np.int32)
    dirs = _directions(N, seed + 1)
    if N >= 64:
        m = S - 3
        odd = 1 if T > 1 else 0
        special = [(0, 0), (1, 0), (0, 1)] + [(F32(i) / F32(m), F32(m - i) / F32(m)) for i in range(m + 1)] + [(np.nan, 0.5), (np.nan, np.nan)]
        for e, b in enumerate(special):
            bary[20 + e], tri[20 + e] = b, odd
        for e, b in enumerate(special[:3]):
            bary[40 + e], tri[40 + e] = b, 0
        tri[1::10] = -1
        tri[4::25] = T
    return tri, bary, dirs


@pytest.mark.parametrize("L", BANDS)
@pytest.mark.parametrize("S", (4, 5, 16))
def test_the_sample_equals_the_restatement_bit_for_bit(L, S):
    import pvd_hip
    from pvd.mesh import sample_sh_texture
    K = L * L
    bg = (0.25, 1.0, 0.5)
    for T in (1, 2, 3, 5, 200):
        C, rows, Wt, Ht = tr.layout(T, S)
        tex = (np.random.RandomState(100 * S + T + L).rand(Ht, Wt, K, 3) * 8.0 - 3.0).astype(F32)  # sums leave [0, 1] on both sides
        dtex = _dev(tex, F32)
        for N in (1, 64, 4099):
            tri, bary, dirs = _lookups(T, S, N, 31 * N + S + T)
            want = sr.sample(tex, T, S, L, tri, bary, dirs, bg)
            got = sample_sh_texture(dtex, S, T, _dev(tri, np.int32), _dev(bary, F32), _dev(dirs, F32), bg_color=bg).cpu().numpy()
            _same(got, want, (L, S, T, N))
            out = (tri < 0) | (tri >= T)
            assert np.array_equal(got[out], np.tile(np.array(bg, F32), (out.sum(), 1)))  # the background is not clamped away
            assert np.all((got[~out] >= 0) & (got[~out] <= 1))
            if N == 4099 and T == 200:
                assert (got[~out] == 0).any() and (got[~out] == 1).any() and ((got[~out] > 0) & (got[~out] < 1)).any()
        # rows past N are untouched
        color = torch.full((N + 7, 3), 7.0, device=DEV)
        pvd_hip.mesh_shtex_sample(dtex, T, S, L, _dev(tri, np.int32), _dev(bary, F32), _dev(dirs, F32), _dev(bg, F32), color[:N])
        assert bool((color[N:] == 7.0).all())
        _same(color[:N].cpu().numpy(), want, (L, S, T, "guarded"))


def test_the_sample_turns_a_nan_into_zero_and_keeps_its_shape():
    from pvd.mesh import sample_sh_texture
    lay = tr.layout(2, 4)
    tex = torch.full((lay[3], lay[2], 4, 3), float("nan"), device=DEV)
    tri = torch.tensor([[0, 1, -1]], dtype=torch.int32, device=DEV)
    out = sample_sh_texture(tex, 4, 2, tri, torch.full((1, 3, 2), 0.25, device=DEV), torch.ones(1, 3, 3, device=DEV), bg_color=0.5)
    assert tuple(out.shape) == (1, 3, 3) and out.cpu().tolist() == [[[0.0] * 3, [0.0] * 3, [0.5] * 3]]
    none = sample_sh_texture(tex, 4, 2, tri[:, :0], torch.zeros(1, 0, 2, device=DEV), torch.zeros(1, 0, 3, device=DEV))
    assert tuple(none.shape) == (1, 0, 3)


@pytest.mark.parametrize("S", (4, 16))
def test_one_band_is_the_flat_lookup_of_the_first_coefficient(S):
    """At L = 1 the sample is pvd_mesh_tex_sample's of coef[0] * Y_0, clamped: the two kernels agree bit for bit."""
    from pvd.mesh import sample_sh_texture, sample_texture
    T = 200
    C, rows, Wt, Ht = tr.layout(T, S)
    tex = _dev((np.random.RandomState(S).rand(Ht, Wt, 1, 3) * 6.0 - 1.0).astype(F32), F32)
    tri, bary, dirs = _lookups(T, S, 4099, S)
    a = sample_sh_texture(tex, S, T, _dev(tri, np.int32), _dev(bary, F32), _dev(dirs, F32), bg_color=0.5)
    flat = (tex[:, :, 0, :] * torch.tensor(0.282094806, device=DEV)).contiguous()
    b = sample_texture(flat, S, T, _dev(tri, np.int32), _dev(bary, F32), bg_color=0.5).clamp(0.0, 1.0)
    assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ end to end
def test_a_bake_on_a_plane_recovers_a_function_in_the_span():
    """The CPU test's planar case on the device: bake_sh_texture from the callable, render_mesh from two oblique views at 32 x 32; at
    every hit the colour lies within the CPU test's bound (fit_bound carried through the dot: sample_bound) of f at the ray's
    direction."""
    from pvd.mesh import bake_sh_texture, exposure_directions, render_mesh
    from pvd.scene import get_rays
    dv, dt = _dev(sr.PLANE_V, F32), _dev(sr.PLANE_T, np.int32)
    A, B, Cc = (torch.from_numpy(a).to(DEV) for a in (sr.PLANE_A, sr.PLANE_B, sr.PLANE_C))
    asked = []

    def source(x, d):
        asked.append(d.clone())
        d = d.double()
        return (A[None] + B[None] * (d[:, 2] ** 2)[:, None] + Cc[None] * d[:, 0][:, None]).float()
    baked = bake_sh_texture(source, dv, dt, 8, degree=3, batch=8)
    assert baked["degree"] == 3 and tuple(baked["texture"].shape) == (8, 8, 9, 3) and tuple(baked["diffuse"].shape) == (8, 8, 3)
    assert len(asked) == 8 and all(bool((d[:, 2] <= 0).all()) for d in asked)  # 64 directions in batches of 8, none from behind
    tex = baked["texture"].cpu().numpy()
    owned = tr.owners(2, 8)[0] < 2
    assert np.all(tex[~owned] == 0) and np.all(tex[owned] == tex[0, 0])
    U = exposure_directions(64).numpy()
    P = sr.fit_matrix(U, 3)
    rgb = sr.plane_colour(sr.mirrored(np.array([[0, 0, 1]], F32), U)[:, 0]).astype(F32)
    # the device's bake is the restatement's, as bytes, up to the callable's own float64 arithmetic
    assert np.abs(tex[0, 0].astype(np.float64) - sr.project(rgb[:, None, :], P)[0]).max() <= 1e-6
    _same(baked["diffuse"].cpu().numpy(), sr.clamp01(tex[:, :, 0, :] * F32(0.282094806)), "diffuse")
    bound_k = sr.fit_bound(P, rgb, 64)
    intr, hw, worst, hits = (40.0, 40.0, 16.0, 16.0), 32, 0.0, 0
    for eye in ((1.4, 0.2, 0.9), (-0.3, 1.1, 0.5)):
        pose = torch.from_numpy(sr.look_at(eye, (0.5, 0.5, 0.0))).to(DEV)
        out = render_mesh(dv, dt, pose, intr, hw, hw, texture=baked["texture"], texture_cell=8)
        d = get_rays(pose[None], intr, hw, hw, -1)["rays_d"].reshape(-1, 3).cpu().numpy()
        mask = out["mask"].reshape(-1).cpu().numpy()
        col = out["color"].reshape(-1, 3).cpu().numpy()
        assert mask.sum() > 100 and np.all(col[~mask] == 1.0) and np.all(d[mask][:, 2] < 0)
        bound = sr.sample_bound(bound_k, tex[0, 0], sr.basis(d[mask], 3))
        err = np.abs(col[mask].astype(np.float64) - sr.plane_colour(d[mask]))
        worst, hits = max(worst, float((err / bound).max())), hits + int(mask.sum())
        assert np.all(err <= bound)
    print("planar recovery: %d hits, largest error over its bound %.3f" % (hits, worst))


@functools.lru_cache(maxsize=None)
def _sphere(R):
    from pvd.mesh import extract_mesh
    u = np.array(nr.field("sphere", R, md.THRESH))
    return tuple(a.contiguous() for a in extract_mesh(torch.from_numpy(u).to(DEV), md.THRESH, md.BMIN, md.BMAX, with_normals=True))


def test_on_a_sphere_the_sh_atlas_follows_the_view_and_the_flat_one_cannot():
    """The mesh of the sphere field at R = 16, the source clamp(0.5 + 0.4 (d . a)) for a fixed a, four views at 48 x 48: the mean
    absolute error of the L = 3 SH render against the source at the hits is strictly below that of the flat bake_texture render, which
    cannot follow d at all.  The ordering is the assertion; the ratio is printed (profiles/mesh_shtex.txt has it)."""
    from pvd.mesh import bake_sh_texture, bake_texture, render_mesh
    from pvd.scene import get_rays
    dv, dt, dn = _sphere(16)
    a = torch.tensor([0.48, -0.6, 0.64], device=DEV)

    def f(d):
        return (0.5 + 0.4 * (d @ a))[:, None].expand(-1, 3).clamp(0.0, 1.0)
    S = 8
    sh = bake_sh_texture(lambda x, d: f(d), dv, dt, S, degree=3, normals=dn)
    flat = bake_texture(lambda x, n: f(-n), dv, dt, S, normals=dn)  # the colour seen straight on, as the vertex colours are taken
    assert bool(torch.isfinite(sh["texture"]).all()) and tuple(sh["texture"].shape)[2:] == (9, 3)
    centre = dv.mean(dim=0).cpu().numpy().astype(np.float64)
    radius = float(torch.linalg.norm(dv - dv.mean(dim=0), dim=1).max())
    intr, hw = (60.0, 60.0, 24.0, 24.0), 48
    e_sh = e_flat = 0.0
    hits = 0
    for direction in ((1, 0.2, 0.1), (-0.3, 1, 0.4), (0.2, -0.5, -1), (-1, -0.4, 0.6)):
        eye = centre + 3.0 * radius * np.array(direction) / np.linalg.norm(direction)
        pose = torch.from_numpy(sr.look_at(eye, centre)).to(DEV)
        with_sh = render_mesh(dv, dt, pose, intr, hw, hw, texture=sh["texture"], texture_cell=S)
        with_flat = render_mesh(dv, dt, pose, intr, hw, hw, texture=flat["texture"], texture_cell=S)
        assert torch.equal(with_sh["tri"], with_flat["tri"])
        mask = with_sh["mask"].reshape(-1)
        truth = f(get_rays(pose[None], intr, hw, hw, -1)["rays_d"].reshape(-1, 3))[mask]
        e_sh += float((with_sh["color"].reshape(-1, 3)[mask] - truth).abs().sum())
        e_flat += float((with_flat["color"].reshape(-1, 3)[mask] - truth).abs().sum())
        hits += int(mask.sum())
    assert hits > 4 * 400
    e_sh, e_flat = e_sh / (3 * hits), e_flat / (3 * hits)
    print("curved case: mean |error| SH (L = 3) %.4f, flat %.4f, flat / SH = %.2f over %d hits" % (e_sh, e_flat, e_flat / e_sh, hits))
    assert e_sh < e_flat


def test_a_flat_texture_keeps_its_path_and_extract_surface_its_keys():
    """render_mesh with a 3-D texture returns the bytes of sample_texture on its own hits (the old path is not rerouted);
    extract_surface(texture=8) has no new keys; texture_sh adds the degree and the diffuse atlas and puts the 4-D atlas under texture."""
    from pvd.mesh import evaluate_mesh_views, extract_surface, render_mesh, sample_texture, texture_layout
    from test_hip_mesh_normals import _AnalyticSphere
    dv, dt, dn = _sphere(16)
    T, S = int(dt.shape[0]), 5
    lay = texture_layout(T, S)
    tex = torch.rand(lay["height"], lay["width"], 3, device=DEV)
    pose = torch.from_numpy(tr.JOB_POSE).to(DEV)
    out = render_mesh(dv, dt, pose, tr.JOB_INTRINSICS, 32, 32, texture=tex, texture_cell=S, bg_color=0.25)
    assert int(out["mask"].sum()) > 100
    assert torch.equal(out["color"], sample_texture(tex, S, T, out["tri"], out["bary"], bg_color=0.25))
    model, R = _AnalyticSphere(), 24
    plain = extract_surface(model, resolution=R)
    m = extract_surface(model, resolution=R, texture=8)
    assert sorted(m) == sorted(list(plain) + ["texture", "texture_cell", "uv"]) and m["texture"].dim() == 3
    assert sorted(extract_surface(model, resolution=R, texture_sh=2)) == sorted(plain)  # texture_sh needs texture=S
    s = extract_surface(model, resolution=R, texture=5, texture_sh=2)
    assert sorted(s) == sorted(list(m) + ["texture_degree", "texture_diffuse"]) and s["texture_degree"] == 2 and s["texture_cell"] == 5
    lay = texture_layout(int(s["triangles"].shape[0]), 5)
    assert tuple(s["texture"].shape) == (lay["height"], lay["width"], 4, 3) and tuple(s["texture_diffuse"].shape) == (lay["height"], lay["width"], 3)
    assert bool(torch.isfinite(s["texture"]).all()) and torch.equal(s["vertices"], plain["vertices"])
    # evaluate_mesh_views takes the 4-D atlas as it takes the flat one
    truth = torch.full((1, 32, 32, 3), 0.5, device=DEV)
    rep = evaluate_mesh_views(s["vertices"], s["triangles"], None, pose[None], tr.JOB_INTRINSICS, 32, 32, truth, texture=s["texture"],
                              texture_cell=5)
    assert np.isfinite(rep["psnr"]) and 0.0 <= rep["coverage"] <= 1.0
