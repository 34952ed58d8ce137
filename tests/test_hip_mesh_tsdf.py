"""pvd_mesh_tsdf_integrate / _finalize / _sample_color (csrc/mesh_tsdf.hip, csrc/pvd_hip_mesh_tsdf.h) and the depth-map fusion of
pvd/mesh.py against the float32 numpy restatement (tests/mesh_tsdf_restatement.py, pinned by tests/test_mesh_tsdf_restatement.py),
BIT FOR BIT: the build compiles with -ffp-contract=off and HIP's float32 division and square root are correctly rounded.

Sizes.  R = 2 (one cell), 9, 20 (no power of two: the lattice coordinates round; 8000 voxels are 32 workgroups of 256, the last one
partial) and 33; V = 1, 3 and 14 (the views are not chunked); images of 1 x 1, 7 x 5 and 64 x 64; with and without colour and
weight."""
import numpy as np
import pytest
import torch

import mesh_tsdf_restatement as tr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _t(a, dtype=torch.float32):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV)


def _bits(t):
    return t.detach().cpu().contiguous().numpy().reshape(-1).view(np.uint32)


def _same(got, want, what):
    np.testing.assert_array_equal(_bits(got), np.ascontiguousarray(want, np.float32).reshape(-1).view(np.uint32), err_msg=what)


def _gpu_integrate(acc, depth, color, weight, poses, intr, R, lo, hi, tau):
    import pvd_hip
    pvd_hip.mesh_tsdf_integrate(_t(depth), _t(color), _t(weight), _t(poses), _t(intr), R, _t(lo), _t(hi), float(tau), acc[0], acc[1],
                                acc[2] if color is not None else None)


def _zeros(R, color=True):
    z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=DEV)  # noqa: E731
    return [z(R ** 3), z(R ** 3), z(R ** 3, 3) if color else None]


@pytest.fixture(scope="module")
def sphere():
    fx = tr.sphere_fixture()
    rng = np.random.RandomState(5)
    fx["weight"] = rng.uniform(0.25, 2.0, fx["depth"].shape).astype(np.float32)
    fx["weight"][rng.rand(*fx["depth"].shape) < 0.05] = 0.0
    # the reference of the finalize, sample and end-to-end tests: computed once, never changed.  It is UNWEIGHTED (w = 1); the weight
    # image above is used by the batch test only, and weighted sums are compared in test_integrate_is_the_restatement_bit_for_bit
    fx["ref"] = tr.fuse(fx, np.float32)
    return fx


def _scene(R, V, HW, seed):
    """a generic scene: the sphere's cameras (the first V of 14) over an off-centre box, depth maps of the sphere with holes (NaN, 0)
    and rays that miss it (+inf), a weight and a colour per pixel"""
    fx = tr.sphere_fixture(R=R, HW=HW, n=14)
    rng = np.random.RandomState(seed)
    out = {k: fx[k][:V] for k in ("poses", "intrinsics", "depth", "color")}
    depth = out["depth"].copy()
    holes = rng.rand(*depth.shape)
    depth[holes < 0.05] = np.nan
    depth[(holes >= 0.05) & (holes < 0.08)] = 0.0
    out["depth"] = depth
    out["weight"] = rng.uniform(0.5, 1.5, depth.shape).astype(np.float32)
    out.update(R=R, bmin=np.array([-0.9, -1.0, -0.7], np.float32), bmax=np.array([1.0, 0.8, 0.9], np.float32),
               tau=np.float32(0.3 if R < 9 else 3 * 2.0 / (R - 1)))
    return out


@pytest.mark.parametrize("R,V,HW", [(2, 1, 64), (9, 3, 64), (20, 14, 64), (33, 3, 64), (20, 3, 1)])
@pytest.mark.parametrize("color,weight", [(True, True), (True, False), (False, True), (False, False)])
def test_integrate_is_the_restatement_bit_for_bit(R, V, HW, color, weight):
    sc = _scene(R, V, HW, seed=R + V)
    want = [np.zeros(R ** 3, np.float32), np.zeros(R ** 3, np.float32), np.zeros((R ** 3, 3), np.float32) if color else None]
    args = (sc["depth"], sc["color"] if color else None, sc["weight"] if weight else None, sc["poses"], sc["intrinsics"], R, sc["bmin"],
            sc["bmax"], sc["tau"])
    tr.integrate(want[0], want[1], want[2], *args)
    assert want[1].any()
    got = _zeros(R, color)
    _gpu_integrate(got, *args)
    _same(got[0], want[0], "acc_d")
    _same(got[1], want[1], "acc_w")
    if color:
        _same(got[2], want[2], "acc_c")


def test_the_hand_made_skip_cases_in_one_call():
    views = list(tr.hand_views().values())
    depth, color, weight, poses, intr = tr.stack_views(views)
    assert depth.shape == (len(views), 5, 7)
    want = [np.zeros(27, np.float32), np.zeros(27, np.float32), np.zeros((27, 3), np.float32)]
    tr.integrate(*want, depth, color, weight, poses, intr, 3, tr.HAND_BMIN, tr.HAND_BMAX, tr.HAND_TAU)
    got = _zeros(3)
    _gpu_integrate(got, depth, color, weight, poses, intr, 3, tr.HAND_BMIN, tr.HAND_BMAX, tr.HAND_TAU)
    for g, w, name in zip(got, want, ("acc_d", "acc_w", "acc_c")):
        _same(g, w, name)
    # and the 1 x 1 image
    depth, color, weight, poses, intr = tr.stack_views([tr.hand_view_1x1()])
    want = [np.zeros(27, np.float32), np.zeros(27, np.float32), np.zeros((27, 3), np.float32)]
    tr.integrate(*want, depth, color, weight, poses, intr, 3, tr.HAND_BMIN, tr.HAND_BMAX, tr.HAND_TAU)
    got = _zeros(3)
    _gpu_integrate(got, depth, color, weight, poses, intr, 3, tr.HAND_BMIN, tr.HAND_BMAX, tr.HAND_TAU)
    for g, w, name in zip(got, want, ("acc_d", "acc_w", "acc_c")):
        _same(g, w, name + " (1 x 1)")
    assert float(got[1].sum()) == 2.0 * 22  # 27 voxels less the five of the plane q_z = 2 that land on x = W or y = H


def test_batches_leave_the_bits_of_one_call(sphere):
    args = lambda a, b: (sphere["depth"][a:b], sphere["color"][a:b], sphere["weight"][a:b], sphere["poses"][a:b],  # noqa: E731
                         sphere["intrinsics"][a:b], 33, sphere["bmin"], sphere["bmax"], sphere["tau"])
    one = _zeros(33)
    _gpu_integrate(one, *args(0, 14))
    two = _zeros(33)
    _gpu_integrate(two, *args(0, 8))
    _gpu_integrate(two, *args(8, 14))
    each = _zeros(33)
    for v in range(14):
        _gpu_integrate(each, *args(v, v + 1))
    for a, b, c in zip(one, two, each):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(a.view(torch.int32), c.view(torch.int32))
    want = [np.zeros(33 ** 3, np.float32), np.zeros(33 ** 3, np.float32), np.zeros((33 ** 3, 3), np.float32)]
    tr.integrate(*want, *args(0, 14))
    for g, w, name in zip(one, want, ("acc_d", "acc_w", "acc_c")):
        _same(g, w, name)


@pytest.mark.parametrize("min_weight", [1.0, 3.0])
@pytest.mark.parametrize("unknown", [-1.0, 1.0])
def test_finalize_is_the_restatement(sphere, min_weight, unknown):
    import pvd_hip
    acc_d, acc_w, _ = sphere["ref"]
    n = 33 ** 3
    cases = {"sphere": (acc_d, acc_w), "all unknown": (np.zeros(n, np.float32), np.zeros(n, np.float32)),
             "all observed": (acc_d, (acc_w + np.float32(3)).astype(np.float32))}
    for name, (d, w) in cases.items():
        want, totals = tr.finalize(d, w, min_weight, unknown)
        field = torch.full((n,), 7.0, device=DEV)
        got = torch.full((3,), -5, dtype=torch.int64, device=DEV)
        pvd_hip.mesh_tsdf_finalize(_t(d), _t(w), 33, min_weight, unknown, field, got)
        _same(field, want, name)
        assert tuple(got.tolist()) == totals, name
        if name == "all unknown":
            assert totals == (0, 0, n)
        if name == "all observed":
            assert totals[0] == n and totals[2] == 0


def test_finalize_walks_a_volume_larger_than_its_grid():
    """The finalize pass runs at most 2048 workgroups of 256 lanes and strides over the rest: R = 81 has 531441 voxels, 7153 more than
    one pass of the grid holds, so the second pass is a partial one."""
    import pvd_hip
    n = 81 ** 3
    assert 2048 * 256 < n < 2 * 2048 * 256
    rng = np.random.RandomState(81)
    w = rng.randint(0, 4, n).astype(np.float32)
    d = (w * rng.uniform(-1.0, 1.0, n)).astype(np.float32)
    want, totals = tr.finalize(d, w, 2.0, -1.0)
    field = torch.full((n + 64,), 7.0, device=DEV)
    got = torch.zeros(3, dtype=torch.int64, device=DEV)
    pvd_hip.mesh_tsdf_finalize(_t(d), _t(w), 81, 2.0, -1.0, field[:n], got)
    _same(field[:n], want, "field")
    assert tuple(got.tolist()) == totals and totals[0] + totals[2] == n and bool((field[n:] == 7.0).all())


@pytest.mark.parametrize("N", [1, 257, 1000])
def test_sample_color_is_the_restatement(sphere, N):
    import pvd_hip
    _, acc_w, acc_c = sphere["ref"]
    lo, hi = sphere["bmin"], sphere["bmax"]
    rng = np.random.RandomState(N)
    lattice = tr.lattice(33, lo, hi)
    pts = rng.uniform(-1.0, 1.0, (N, 3)).astype(np.float32)  # cells with 0 (deep inside), some and 8 observed corners
    pts[1::7] = lattice[rng.randint(0, 33 ** 3, len(pts[1::7]))]  # lattice points themselves
    pts[2::7, 0] = rng.choice(np.array([-1.0, 1.0], np.float32), len(pts[2::7]))  # on the faces of the box
    pts[3::7] *= np.float32(1.2)  # partly outside
    pts[4::7] = (pts[4::7] * np.float32(0.1))  # around the centre: no observed corner
    one = np.argwhere(tr.observed_corners(acc_w, 33, 1.0) == 1)  # cells at the rim of the unobserved ball: ONE observed corner
    idx = np.arange(8, N, 13)
    pick = one[rng.randint(0, len(one), len(idx))]
    pts[idx] = (-1.0 + (pick + rng.uniform(0.05, 0.95, (len(idx), 3))) / 16.0).astype(np.float32)
    pts[5::31, 1] = np.nan
    pts[6::31, 2] = np.inf
    if N == 1:
        pts[0] = (0.5, 0.1, -0.2)
    want = tr.sample_color(acc_c, acc_w, 33, lo, hi, 1.0, pts)
    if N > 1:
        seen = (acc_w >= 1).reshape(33, 33, 33)
        cell = np.clip(np.floor((np.nan_to_num(pts, posinf=0) + 1) * 16).astype(int), 0, 31)
        corners = sum(seen[cell[:, 0] + a, cell[:, 1] + b, cell[:, 2] + c].astype(int) for a in (0, 1) for b in (0, 1) for c in (0, 1))
        assert (corners == 0).any() and (corners == 1).any() and (corners == 8).any() and ((corners > 1) & (corners < 8)).any()
        assert (want.any(axis=1)).any() and (~want.any(axis=1)).any()
    out = torch.full((N + 3, 3), 9.0, device=DEV)
    pvd_hip.mesh_tsdf_sample_color(_t(acc_c), _t(acc_w), 33, _t(lo), _t(hi), 1.0, _t(pts), out[:N])
    _same(out[:N], want, "colors")
    assert bool((out[N:] == 9.0).all())  # rows past N are untouched


def test_sample_color_with_exactly_one_observed_corner():
    """The hand-made volume with a single observed voxel: every point's cell has exactly one observed corner, and the blend divides by
    that corner's weight alone -- 1e-9 and 2^-60 next to the opposite corner, 0 (colour 0) exactly on it."""
    import pvd_hip
    case = tr.single_corner_case()
    pts = case["points"]
    want = tr.sample_color(case["acc_c"], case["acc_w"], case["R"], case["bmin"], case["bmax"], 1.0, pts)
    assert want[~case["exact_zero"]].all() and not want[case["exact_zero"]].any()
    out = torch.full((len(pts) + 2, 3), 9.0, device=DEV)
    pvd_hip.mesh_tsdf_sample_color(_t(case["acc_c"]), _t(case["acc_w"]), case["R"], _t(case["bmin"]), _t(case["bmax"]), 1.0, _t(pts),
                                   out[:len(pts)])
    _same(out[:len(pts)], want, "colors")
    assert bool((out[len(pts):] == 9.0).all())


def test_the_sphere_end_to_end(sphere):
    """The fixture of the CPU geometry check through pvd/mesh.py: tsdf_volume, tsdf_integrate, tsdf_field, extract_mesh(-field, 0),
    mesh_topology, mesh_winding, tsdf_vertex_colors."""
    from pvd import mesh
    lo, hi = sphere["bmin"], sphere["bmax"]
    vol = mesh.tsdf_volume(33, lo, hi, device=torch.device(DEV))
    assert abs(vol.tau - float(sphere["tau"])) < 1e-7
    mesh.tsdf_integrate(vol, sphere["depth"][:8], sphere["poses"][:8], sphere["intrinsics"][0], color=sphere["color"][:8])
    mesh.tsdf_integrate(vol, sphere["depth"][8:], sphere["poses"][8:], sphere["intrinsics"][8:], color=sphere["color"][8:])
    assert vol.views == 14
    field, totals = mesh.tsdf_field(vol, return_totals=True)
    d, w, c = sphere["ref"]
    want, want_totals = tr.finalize(d, w, 1.0, -1.0)
    _same(field, want, "field")
    assert totals == dict(observed=want_totals[0], observed_inside=want_totals[1], unknown=want_totals[2])
    verts, tris, normals = mesh.extract_mesh(-field, 0.0, lo, hi, with_normals=True)
    topo = mesh.mesh_topology(verts, tris)
    print("sphere: %d vertices, %d triangles, topology %s" % (verts.shape[0], tris.shape[0], topo))
    assert topo["closed"] and topo["manifold"] and topo["shells"] == 1
    radius = torch.linalg.norm(verts, dim=1)
    assert float((radius - 0.5).abs().max()) < sphere["spacing"]
    assert int(mesh.mesh_winding(torch.zeros(1, 3, device=DEV), verts, tris)[0]) == 1
    assert float((normals * verts / radius[:, None]).sum(dim=1).min()) > 0.8  # outward
    colors = mesh.tsdf_vertex_colors(vol, verts)
    _same(colors, tr.sample_color(c, w, 33, lo, hi, 1.0, verts.cpu().numpy()), "vertex colours")
    assert bool((colors.sum(dim=1) > 0).all())  # every vertex of the surface has an observed corner


# ------------------------------------------------------------------------------------------------------ the model's own depth maps
# measured on the fixture below with the operators as they were before this file existed (march_rays_train + composite_rays_train
# against the inference render): the largest difference over the opaque pixels, their number, and the tolerance -- twice the former
RENDER_MEASURED, RENDER_PIXELS = 0.030699, 296
RENDER_TOL = 2 * RENDER_MEASURED


@pytest.fixture(scope="module")
def model():
    from test_hip_infer_rounds import _model
    m = _model("hash")
    m.density_scale = 16  # the fixture's densities leave no ray above an opacity of 0.9; at 16 times that, 296 of the view's 2500 end
    return m


def _view():
    from pvd.scene import synthetic_poses
    pose = torch.from_numpy(synthetic_poses(np.random.RandomState(2))[9:10]).to(DEV)
    return pose, (69.44375, 69.44375, 25.0, 25.0), 50, 50  # the 200 x 200 view of tests/test_hip_infer_rounds.py at a quarter of its size


def _both_depths(model):
    """(render_depth_maps' dict, the inference render's depth as a distance: near + unit * (far - near)) of one 50 x 50 view"""
    from pvd import mesh
    from pvd.scene import get_rays
    pose, intr, H, W = _view()
    maps = mesh.render_depth_maps(model, pose, intr, H, W, ray_batch=1024)  # three ray batches, the last one partial
    rays = get_rays(pose, intr, H, W)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        out = model.render(rays["rays_o"], rays["rays_d"], staged=False, bg_color=1, perturb=False, dt_gamma=0, max_steps=1024)
    o, d = rays["rays_o"].reshape(-1, 3).contiguous(), rays["rays_d"].reshape(-1, 3).contiguous()
    nears, fars = model.rm.near_far_from_aabb(o, d, model.aabb_infer, model.min_near)
    return maps, (nears + out["depth"].float().view(-1) * (fars - nears)).view(H, W)


def test_render_depth_maps_agrees_with_the_inference_render_where_the_ray_ends(model):
    """Where opacity >= 0.99 the returned depth (near + sum w (t - near) / sum w over the training marcher's samples) agrees with the
    inference render's near + unit * (far - near) (the sum w t of the inference marcher, not divided by the opacity, which also stops
    a ray at a transmittance of 1e-4).  The tolerance is what these two existing paths show against each other on this fixture: the
    measured maximum is 0.030699 world units over 296 opaque pixels (the inference sum may lack up to 1 % of a
    depth of about 3); the tolerance is twice that, 0.061398.  Pixels under free_opacity are +inf, those in between NaN."""
    maps, infer = _both_depths(model)
    depth, opacity = maps["depth"], maps["opacity"]
    assert tuple(depth.shape) == (1, 50, 50) and tuple(maps["color"].shape) == (1, 50, 50, 3)
    opaque = opacity[0] >= 0.99
    diff = (depth[0] - infer)[opaque].abs()
    print("opaque pixels: %d of 2500; the largest |depth - inference depth| %.6f" % (int(opaque.sum()), float(diff.max())))
    assert int(opaque.sum()) >= RENDER_PIXELS // 2 and float(diff.max()) <= RENDER_TOL
    free, solid = opacity < 0.05, opacity >= 0.5
    assert bool(free.any()) and bool(torch.isposinf(depth[free]).all())
    assert bool(torch.isfinite(depth[solid]).all()) and bool((depth[solid] > 0).all())
    assert bool(torch.isnan(depth[~free & ~solid]).all())
    assert bool((maps["color"][~solid] == 0).all()) and float(maps["color"].max()) <= 1.0 and float(maps["color"][solid].max()) > 0.0


def test_extract_surface_tsdf_returns_the_documented_dict(model):
    from pvd import mesh
    poses = mesh.tsdf_poses(6)
    intr = (48.0, 48.0, 24.0, 24.0)
    m = mesh.extract_surface_tsdf(model, poses, intr, 48, 48, resolution=24, views_per_batch=4)
    assert sorted(m) == ["colors", "counts", "field", "normals", "threshold", "triangles", "tsdf_totals", "vertices", "views"]
    assert m["threshold"] == 0.0 and m["views"] == 6 and m["counts"] is None and m["tsdf_totals"]["observed"] + m["tsdf_totals"]["unknown"] == 24 ** 3
    V, T = int(m["vertices"].shape[0]), int(m["triangles"].shape[0])
    assert V > 0 and T > 0 and tuple(m["normals"].shape) == (V, 3) and tuple(m["colors"].shape) == (V, 3)
    assert tuple(m["field"].shape) == (24, 24, 24) and float(m["field"].abs().max()) <= 1.0
    assert float(m["colors"].min()) >= 0.0 and float(m["colors"].max()) <= 1.0
    # the same views in one batch: the same bits
    one = mesh.extract_surface_tsdf(model, poses, intr, 48, 48, resolution=24, views_per_batch=6)
    for key in ("vertices", "triangles", "normals", "colors", "field"):
        assert torch.equal(one[key], m[key]), key
    # simplify and texture pass through the functions extract_surface uses
    s = mesh.extract_surface_tsdf(model, poses, intr, 48, 48, resolution=24, views_per_batch=4, simplify=6, texture=4)
    assert s["full_counts"] == (V, T) and int(s["triangles"].shape[0]) < T and s["texture_cell"] == 4
    assert tuple(s["uv"].shape) == (int(s["triangles"].shape[0]), 3, 2) and s["texture"].dim() == 3 and tuple(s["vertex_map"].shape) == (V,)
    small = mesh.simplify_mesh(m["vertices"], m["triangles"], 6, bmin=model.aabb_infer[:3], bmax=model.aabb_infer[3:], normals=m["normals"],
                               colors=m["colors"])
    assert torch.equal(small["vertices"], s["vertices"]) and torch.equal(small["triangles"], s["triangles"])


def test_extract_surface_is_what_it_was(model):
    """extract_surface's tail moved into a helper that extract_surface_tsdf shares: the same bits as the steps it is made of, called
    here one by one as extract_surface called them before."""
    from pvd import mesh
    R = 24
    got = mesh.extract_surface(model, resolution=R, simplify=6, smooth=2)
    lo, hi = model.aabb_infer[:3], model.aabb_infer[3:]
    thresh = mesh.default_threshold(model)
    u = mesh.density_field(lambda x: model.density(x)["sigma"], R, lo, hi, device=lo.device)
    verts, tris, nrm = mesh.extract_mesh(u, thresh, lo, hi, with_normals=True)
    col = mesh.vertex_colors(model, verts, nrm)
    verts = mesh.smooth_mesh(verts, tris, iterations=2, lam=0.5, mu=-0.53, bmin=lo, bmax=hi)
    nrm = mesh.face_vertex_normals(verts, tris)
    small = mesh.simplify_mesh(verts, tris, 6, bmin=lo, bmax=hi, normals=nrm, colors=col)
    assert sorted(got) == ["colors", "counts", "field", "full_counts", "normals", "smoothed", "threshold", "triangles", "vertex_map", "vertices"]
    assert torch.equal(got["field"], u) and got["threshold"] == float(thresh) and got["full_counts"] == (verts.shape[0], tris.shape[0])
    for key in ("vertices", "triangles", "normals", "colors", "vertex_map"):
        assert torch.equal(got[key], small[key]), key
    plain = mesh.extract_surface(model, resolution=R)
    assert sorted(plain) == ["colors", "counts", "field", "normals", "threshold", "triangles", "vertices"]
