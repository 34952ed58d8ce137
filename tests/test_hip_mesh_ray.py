"""pvd_mesh_ray_count / _build / _cast (csrc/mesh_ray.hip, include/pvd_hip_mesh_ray.h) and what pvd/mesh.py builds on them -- mesh_raycast,
render_mesh, evaluate_mesh_views -- against the numpy restatement (tests/mesh_ray_restatement.py, pinned by
tests/test_mesh_ray_restatement.py).

Tolerance.  None: the device evaluates the watertight test in unfused float64 in the header's order and so does numpy, so t, tri and
bary are compared as bytes.  A differing bit means a fused or reordered operation in the kernel, or a triangle the walk did not test.

Sizes.  Meshes: the fixtures of mesh_dist_restatement.FIXTURES through extract_mesh (R = 9, 17, 33; 648 to about 11 000 triangles: one
to 44 workgroups in the per-triangle passes).  N = 1 (one lane), 257 (a second workgroup with one lane) and 1000.  G = 1 (one cell:
brute force), 2, 7 (343 cells: a second, partial workgroup in the per-cell passes) and 32 (128 workgroups of cells).  The reference
matrix is N x T, so N = 1000 goes with the small meshes."""
import functools

import numpy as np
import pytest
import torch

import mesh_dist_restatement as md
import mesh_normals_restatement as nr
import mesh_ray_restatement as rr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BMIN, BMAX, THRESH = md.BMIN, md.BMAX, md.THRESH
CENTRE = tuple((a + b) / 2 for a, b in zip(BMIN, BMAX))


@functools.lru_cache(maxsize=None)
def _mesh(kind, R):
    """(vertices, triangles) as extract_mesh returns them, as read-only host arrays."""
    from pvd.mesh import extract_mesh
    v, t = extract_mesh(torch.from_numpy(np.array(nr.field(kind, R, THRESH))).to(DEV), THRESH, BMIN, BMAX)
    v, t = v.cpu().numpy(), t.cpu().numpy()
    assert np.array_equal(t, md.fixture(kind, R)[1])
    v.setflags(write=False), t.setflags(write=False)
    return v, t


def rays_of(verts, which, N, seed):
    """Seeded rays (origins, dirs) [N,3] f32 for a mesh inside BMIN .. BMAX: "camera" -- the pixels of two 24 x 24 get_rays views from
    pose_spherical poses (in get_rays' axes: nerf_matrix_to_ngp), moved so that they look at the box's centre --, "own" -- aimed at
    the mesh's own vertices from three box lengths out, directions not normalised --, "inside" -- from uniform points of the box in uniform directions --, "miss" -- rays
    that never enter the box."""
    from pvd.scene import get_rays, nerf_matrix_to_ngp, pose_spherical
    rng = np.random.RandomState(seed)
    lo, hi = np.array(BMIN), np.array(BMAX)
    L = np.linalg.norm(hi - lo)
    if which == "camera":
        o, d = [], []
        for theta, phi in ((30.0, -30.0), (200.0, -70.0)):
            pose = nerf_matrix_to_ngp(pose_spherical(theta, phi, 4.0), scale=1.0)  # the axes get_rays expects
            pose[:3, 3] += np.array(CENTRE, np.float32)
            r = get_rays(torch.from_numpy(pose)[None], (40.0, 40.0, 12.0, 12.0), 24, 24, -1)
            o.append(r["rays_o"].reshape(-1, 3).numpy()), d.append(r["rays_d"].reshape(-1, 3).numpy())
        o, d = np.concatenate(o), np.concatenate(d)
        pick = np.sort(rng.permutation(len(o))[:N])  # row-major pixel order is kept
        o, d = o[pick], d[pick]
    elif which == "own":
        target = verts[rng.permutation(len(verts))[:N]].astype(np.float64)
        u = rng.normal(size=target.shape)
        o = (np.array(CENTRE) + 3.0 * L * u / np.linalg.norm(u, axis=1, keepdims=True)).astype(np.float32)
        d = target - o
    elif which == "inside":
        o = rng.uniform(lo, hi, (N, 3))
        d = rng.normal(size=(N, 3))
    else:
        o = rng.uniform(hi + 0.1 * (hi - lo), hi + (hi - lo), (N, 3))
        d = np.abs(rng.normal(size=(N, 3))) * np.where(rng.rand(N, 1) < 0.5, 1.0, [1.0, 0.0, 1.0])  # away from the box, some along a plane
    o, d = np.ascontiguousarray(o, np.float32), np.ascontiguousarray(d, np.float32)
    assert o.shape == d.shape == (N, 3)
    return o, d


@functools.lru_cache(maxsize=None)
def _reference(kind, R, which, N):
    """(origins, dirs, hit matrices, ref t, ref tri, ref bary) -- computed once, read-only."""
    v, t = _mesh(kind, R)
    o, d = rays_of(v, which, N, 1000 * R + N + len(which))
    M = rr.hit_matrix(o, d, v, t)
    ref = rr.first_hit(o, d, v, t, M=M)
    for a in (o, d) + M + ref:
        a.setflags(write=False)
    return (o, d, M) + ref


def _cast(o, d, verts, tris, t_min=0.0, t_max=float("inf"), G=None, bmin=BMIN, bmax=BMAX):
    from pvd.mesh import mesh_raycast
    dev = lambda a, dt: torch.from_numpy(np.array(a, dt)).to(DEV)  # noqa: E731
    t, tri, bary = mesh_raycast(dev(o, np.float32).reshape(-1, 3), dev(d, np.float32).reshape(-1, 3), dev(verts, np.float32), dev(tris, np.int32),
                                t_min, t_max, bmin, bmax, G)
    n = len(np.asarray(o).reshape(-1, 3))
    assert t.dtype == torch.float32 and tri.dtype == torch.int32 and bary.dtype == torch.float32 and t.is_cuda and tri.is_cuda and bary.is_cuda
    assert t.shape == tri.shape == (n,) and bary.shape == (n, 2)
    return t.cpu().numpy(), tri.cpu().numpy(), bary.cpu().numpy()


def _same(got, ref, label):
    for g, r, name in zip(got, ref, ("t", "tri", "bary")):
        if g.tobytes() != r.tobytes():
            bad = np.nonzero((g.view(np.int32) != np.asarray(r).view(np.int32)).reshape(len(g), -1).any(axis=1))[0]
            raise AssertionError("%s: %s differs in %d rows, first %d: %r against %r" % (label, name, len(bad), bad[0], g[bad[0]], r[bad[0]]))


# ------------------------------------------------------------------------------------------------------------------------- bits
CASES = [("sphere", 9, "camera", 1000), ("sphere", 9, "own", 257), ("sphere", 9, "inside", 1000), ("sphere", 9, "miss", 257),
         ("sphere", 17, "inside", 1), ("torus", 17, "camera", 257), ("torus", 17, "own", 257), ("torus", 33, "camera", 257),
         ("torus", 33, "inside", 257), ("two_spheres", 17, "own", 257), ("two_spheres", 17, "miss", 1), ("smooth", 9, "camera", 1000),
         ("smooth", 17, "own", 257), ("smooth", 17, "inside", 257)]


@pytest.mark.parametrize("kind,R,which,N", CASES)
def test_the_first_hit_is_the_restatements_bit_for_bit(kind, R, which, N):
    verts, tris = _mesh(kind, R)
    o, d, _, rt, rtri, rbary = _reference(kind, R, which, N)
    hits = int((rtri >= 0).sum())
    print("mesh ray %s R=%d %s: T=%d N=%d, %d hit" % (kind, R, which, len(tris), N, hits))
    assert hits == 0 if which == "miss" else (hits > N // 8 or N == 1)
    _same(_cast(o, d, verts, tris, G=None if which != "own" else 7), (rt, rtri, rbary), "%s R=%d %s" % (kind, R, which))
    # the box defaults to the bounding box of the vertices: another box, the same bits
    from pvd.mesh import mesh_raycast
    got = mesh_raycast(torch.from_numpy(np.array(o)).to(DEV), torch.from_numpy(np.array(d)).to(DEV), torch.from_numpy(np.array(verts)).to(DEV),
                       torch.from_numpy(np.array(tris)).to(DEV))
    _same(tuple(a.cpu().numpy() for a in got), (rt, rtri, rbary), "%s R=%d %s, default box" % (kind, R, which))


def test_the_scan_of_the_cell_counts_carries_into_a_second_chunk():
    """G = 129: 2 146 689 cells are 8386 per-workgroup sums, one chunk of 8192 and a second one that starts from the first one's
    carry.  The cell index is x-major, so cell 8192 * 256 lies in the x-layer 126 of 129: in the box of the other tests the sphere
    (x = -0.6 .. 0.6 of -1 .. 1) stays below it, so this box is the same one stretched to x = -30, which puts x = 0 into that layer and
    still holds the whole mesh.  The reference does not depend on the box."""
    G, lo, hi = 129, (-30.0,) + BMIN[1:], (0.7,) + BMAX[1:]
    assert 8192 < -(-G ** 3 // 256) <= 2 * 8192
    verts, tris = _mesh("sphere", 9)
    x = (verts.astype(np.float64)[:, 0][tris] - lo[0]) * (G / (hi[0] - lo[0]))  # [T,3]: the corners' x in cells
    layer = 8192 * 256 // G ** 2
    assert layer == 126 and (x.max(axis=1) < layer - 0.5).sum() > 50 and (x.min(axis=1) > layer + 1.5).sum() > 50  # both sides
    o, d, _, rt, rtri, rbary = _reference("sphere", 9, "camera", 1000)
    _same(_cast(o, d, verts, tris, G=G, bmin=lo, bmax=hi), (rt, rtri, rbary), "sphere R=9 camera, G=129")


def test_the_hand_made_cube_with_exact_zeros():
    o, d = [c[0] for c in rr.CUBE_RAYS], [c[1] for c in rr.CUBE_RAYS]
    ref = rr.first_hit(o, d, rr.CUBE_V, rr.CUBE_T)
    assert ref[0].tolist() == [c[2] for c in rr.CUBE_RAYS] and ref[1].tolist() == [c[3] for c in rr.CUBE_RAYS]
    for G, lo, hi in ((1, (0.0,) * 3, (1.0,) * 3), (2, (0.0,) * 3, (1.0,) * 3), (4, (0.0,) * 3, (1.0,) * 3), (3, (-1.0,) * 3, (2.0,) * 3),
                      (5, (0.25,) * 3, (0.75,) * 3), (4, (0.0, 0.0, 0.0), (1.0, 1.0, 0.0))):
        _same(_cast(o, d, rr.CUBE_V, rr.CUBE_T, G=G, bmin=lo, bmax=hi), ref, "cube G=%d %s" % (G, lo))
    for kw in (dict(t_min=2.0), dict(t_max=2.0), dict(t_min=2.5), dict(t_min=0.5, t_max=1.0)):
        _same(_cast(o, d, rr.CUBE_V, rr.CUBE_T, G=2, bmin=(0.0,) * 3, bmax=(1.0,) * 3, **kw), rr.first_hit(o, d, rr.CUBE_V, rr.CUBE_T, **kw),
              "cube %s" % kw)


# ------------------------------------------------------------------------------------------------------------- grid independence
def _grid_independent(label, o, d, verts, tris, boxes, ref, **kw):
    for lo, hi in boxes:
        for G in (1, 2, 7, 32):
            for run in range(2 if G == 7 else 1):
                _same(_cast(o, d, verts, tris, G=G, bmin=lo, bmax=hi, **kw), ref, "%s G=%d %s %s run %d" % (label, G, lo, hi, run))


BOXES = [(BMIN, BMAX),
         ((0.1, 0.6, 1.0), (0.2, 0.7, 1.1)),  # much smaller than the mesh: most triangles go to the outside list
         (tuple(a * s for a, s in zip(BMIN, (1, 1, 0.01))), tuple(a * s for a, s in zip(BMAX, (1, 1, 0.01)))),  # squashed along z
         ((5.0, 5.0, 5.0), (6.0, 6.0, 6.0)),   # away from the mesh altogether: every triangle is outside
         ((-1.0, -0.5, 0.25), (1.0, -0.5, 0.0))]  # one flat axis and one of negative extent


@pytest.mark.parametrize("which", ["camera", "inside"])
def test_the_result_does_not_depend_on_the_grid_or_the_box(which):
    verts, tris = _mesh("torus", 17)
    o, d, _, rt, rtri, rbary = _reference("torus", 17, which, 257)
    _grid_independent("torus R=17 " + which, o, d, verts, tris, BOXES, (rt, rtri, rbary))


def test_one_triangle_spanning_the_box_next_to_thousands_of_small_ones():
    v0, t0 = _mesh("sphere", 17)
    big = np.array([(-1.0, -0.5, 0.3), (1.0, 1.5, 0.3), (1.0, -0.5, 1.9)], np.float32)
    verts = np.concatenate([v0, big])
    tris = np.concatenate([t0, np.array([[len(v0), len(v0) + 1, len(v0) + 2]], np.int32)])
    o, d = rays_of(v0, "inside", 257, 5)
    ref = rr.first_hit(o, d, verts, tris)
    assert 20 < (ref[1] == len(t0)).sum() < 237  # the big one wins for a good share of the rays, not for all
    _grid_independent("sphere R=17 + one big triangle", o, d, verts, tris, [(BMIN, BMAX)], ref)


# ------------------------------------------------------------------------------------------------------------------ the interval
def test_t_max_saturates_and_t_min_skips_the_first_surface():
    """The interval is compared on the float64 t: `nearer` below means a float64 t below t_max, whatever it rounds to.  One more
    triangle in the plane x = t_max beside the box (so it is on the outside list), and a ray along x from x = 0 towards it, make a
    hit at exactly t_max: its U, V, W are -3 or 3 and det 9 or -9, so t = 9 t_max / 9 without a rounding."""
    v0, t0 = _mesh("smooth", 17)
    o, d, _, rt0, rtri0, _ = _reference("smooth", 17, "own", 257)
    hit0 = rtri0 >= 0
    m = float(np.sort(rt0[hit0])[hit0.sum() // 2])  # the (upper) median of the hit distances
    verts = np.concatenate([v0, np.array([(m, 9.0, -1.0), (m, 12.0, -1.0), (m, 9.0, 2.0)], np.float32)])
    tris = np.concatenate([t0, np.array([[len(v0), len(v0) + 1, len(v0) + 2]], np.int32)])
    o = np.concatenate([o, np.array([(0.0, 10.0, 0.0)], np.float32)])
    d = np.concatenate([d, np.array([(1.0, 0.0, 0.0)], np.float32)])
    M = rr.hit_matrix(o, d, verts, tris)
    rt, rtri, rbary = rr.first_hit(o, d, verts, tris, M=M)
    assert rtri[-1] == len(t0) and rt[-1] == np.float32(m) and M[0][-1, len(t0)] == m  # the hit at exactly t_max
    hit = rtri >= 0
    t64 = M[0][np.arange(len(o)), np.maximum(rtri, 0)]
    below = hit & (t64 < m)
    assert 50 < below.sum() < hit.sum() and not below[-1]
    for G in (1, 7, 32):
        _same(_cast(o, d, verts, tris, G=G), (rt, rtri, rbary), "no t_max, G=%d" % G)
        t, tri, bary = _cast(o, d, verts, tris, t_max=m, G=G)
        _same((t[below], tri[below], bary[below]), (rt[below], rtri[below], rbary[below]), "t_max, G=%d" % G)
        assert np.all(t[~below] == np.float32(m)) and np.all(tri[~below] == -1) and np.all(bary[~below] == 0), G
        _same((t, tri, bary), rr.first_hit(o, d, verts, tris, t_max=m, M=M), "t_max against the reference, G=%d" % G)
    # past the first surface: the second one
    t_min = float(np.nextafter(np.float32(m), np.float32(np.inf)))
    ref = rr.first_hit(o, d, verts, tris, t_min=t_min, M=M)
    assert ((ref[1] >= 0) & (ref[1] != rtri)).sum() > 50 and np.min(rt[hit]) < t_min
    for G in (1, 7, 32):
        _same(_cast(o, d, verts, tris, t_min=t_min, G=G), ref, "t_min, G=%d" % G)


# ----------------------------------------------------------------------------------------------------------------- invalid input
def test_invalid_triangles_and_rays_and_rows_past_n():
    import pvd_hip
    v0, t0 = _mesh("sphere", 9)
    o, d, _, rt, rtri, rbary = _reference("sphere", 9, "own", 257)
    verts = np.concatenate([v0, np.array([(np.nan, 0.0, 1.0), (0.0, np.inf, 1.0)], np.float32)])
    V = len(verts)
    planted = np.array([[0, 1, len(v0)], [len(v0) + 1, 2, 3], [0, 1, V], [0, -1, 2], [-2 ** 31, 1, 2], [2 ** 31 - 1, 1, 2]], np.int32)
    where = [0, 100, 100, 300, len(t0), len(t0)]
    tris = np.insert(t0, where, planted, axis=0)
    keep = np.ones(len(tris), bool)
    keep[np.array(where) + np.arange(len(where))] = False
    assert np.array_equal(tris[keep], t0) and md.valid_triangles(verts, tris).tolist() == keep.tolist()
    original = np.nonzero(keep)[0]  # index in the new array of every original triangle
    shifted = np.where(rtri >= 0, original[np.maximum(rtri, 0)], -1).astype(np.int32)
    for G in (1, 7):
        _same(_cast(o, d, verts, tris, G=G), (rt, shifted, rbary), "planted, G=%d" % G)
    # rays that are not finite or have no direction: (NaN, -1, (0, 0)), and their neighbours are untouched
    o2, d2 = o.copy(), d.copy()
    o2[3, 1], o2[200, 0], d2[64, 2], d2[256, 0], d2[100] = np.nan, np.inf, -np.inf, np.nan, 0.0
    t, tri, bary = _cast(o2, d2, v0, t0)
    bad = np.zeros(257, bool)
    bad[[3, 200, 64, 256, 100]] = True
    assert np.all(np.isnan(t[bad])) and np.all(tri[bad] == -1) and np.all(bary[bad] == 0)
    _same((t[~bad], tri[~bad], bary[~bad]), (rt[~bad], rtri[~bad], rbary[~bad]), "neighbours of invalid rays")
    _same((t, tri, bary), rr.first_hit(o2, d2, v0, t0), "invalid rays against the reference")
    # no triangles, no vertices: misses
    for vv, tt in ((v0, t0[:0]), (v0[:0], t0), (v0[:0], t0[:0])):
        t, tri, bary = _cast(o, d, vv, tt, t_max=3.5, bmin=BMIN, bmax=BMAX)
        assert np.all(t == np.float32(3.5)) and np.all(tri == -1) and np.all(bary == 0)
    t, tri, bary = _cast(o, d, v0, t0[:0])
    assert np.all(np.isposinf(t)) and np.all(tri == -1)
    # rows past N are never written
    vt, tt = torch.from_numpy(np.array(v0)).to(DEV), torch.from_numpy(np.array(t0)).to(DEV)
    T, G = len(t0), 7
    lo, hi = torch.tensor(BMIN, device=DEV), torch.tensor(BMAX, device=DEV)
    totals = torch.zeros(2, dtype=torch.int64, device=DEV)
    pvd_hip.mesh_ray_count(vt, tt, lo, hi, G, totals)
    pairs, outside = totals.tolist()
    assert pairs >= T and outside == 0
    ws = torch.empty(pvd_hip.mesh_ray_workspace_bytes(T, G, pairs), dtype=torch.uint8, device=DEV)
    pvd_hip.mesh_ray_build(vt, tt, lo, hi, G, pairs, ws)
    ot, dt = torch.from_numpy(np.array(o)).to(DEV), torch.from_numpy(np.array(d)).to(DEV)
    t = torch.full((257,), 7.0, device=DEV)
    tri = torch.full((257,), -7, dtype=torch.int32, device=DEV)
    bary = torch.full((257, 2), 7.0, device=DEV)
    inf = float("inf")
    pvd_hip.mesh_ray_cast(ot[:100], dt[:100], T, G, pairs, ws, 0.0, inf, t[:100], tri[:100], bary[:100])
    assert bool((t[100:] == 7.0).all()) and bool((tri[100:] == -7).all()) and bool((bary[100:] == 7.0).all())
    _same((t[:100].cpu().numpy(), tri[:100].cpu().numpy(), bary[:100].cpu().numpy()), (rt[:100], rtri[:100], rbary[:100]), "rows below N")
    pvd_hip.mesh_ray_cast(ot[:0], dt[:0], T, G, pairs, ws, 0.0, inf, t[:0], tri[:0], bary[:0])  # N == 0: PVD_OK, no launch
    for args in ((ot, dt, T, G, pairs, ws[:-1], 0.0, inf, t, tri, bary), (ot, dt, T, G, pairs, ws, -1.0, inf, t, tri, bary),
                 (ot, dt, T, G, pairs, ws, 1.0, 1.0, t, tri, bary), (ot, dt, T, G, pairs, ws, 0.0, float("nan"), t, tri, bary),
                 (ot, dt, T, G, pairs, ws, 0.0, inf, t[:100], tri, bary), (ot.double(), dt, T, G, pairs, ws, 0.0, inf, t, tri, bary),
                 (ot, dt[:100], T, G, pairs, ws, 0.0, inf, t, tri, bary), (ot, dt, T, G, pairs, ws[1:], 0.0, inf, t, tri, bary),
                 (ot, dt, T, G, pairs, ws, 0.0, inf, t, tri.long(), bary), (ot, dt, T, G, pairs + 1, ws, 0.0, inf, t, tri, bary)):
        with pytest.raises(pvd_hip.PvdHipError):
            pvd_hip.mesh_ray_cast(*args)
    with pytest.raises(pvd_hip.PvdHipError):
        pvd_hip.mesh_ray_build(vt, tt.long(), lo, hi, G, pairs, ws)
    with pytest.raises(pvd_hip.PvdHipError):
        pvd_hip.mesh_ray_build(vt.reshape(-1), tt, lo, hi, G, pairs, ws)
    with pytest.raises(pvd_hip.PvdHipError):
        pvd_hip.mesh_ray_count(vt, tt, lo, hi, G, totals.int())


# ------------------------------------------------------------------------------------------------------------------ render_mesh
@functools.lru_cache(maxsize=None)
def _analytic_sphere(radius=0.4, R=33):
    """The analytic density of tests/test_hip_mesh_dist.py (sigma = 2 on the sphere around (0.1, -0.05, 0)), meshed at R^3."""
    from pvd.mesh import density_field, extract_mesh
    centre = torch.tensor([0.1, -0.05, 0.0], device=DEV)
    u = density_field(lambda x: 2.0 + 5.0 * (radius - torch.linalg.norm(x - centre, dim=1)), R, (-1.0,) * 3, (1.0,) * 3,
                      device=torch.device(DEV))
    return extract_mesh(u, 2.0, (-1.0,) * 3, (1.0,) * 3, with_normals=True)


INTRINSICS, HW = (40.0, 40.0, 16.0, 16.0), 32


def test_render_mesh_on_the_analytic_sphere():
    from pvd.mesh import render_mesh
    from pvd.scene import get_rays, nerf_matrix_to_ngp, pose_spherical
    v, t, n = _analytic_sphere()
    pose = torch.from_numpy(nerf_matrix_to_ngp(pose_spherical(40.0, -25.0, 2.0), scale=1.0)).to(DEV)
    out = render_mesh(v, t, pose, INTRINSICS, HW, HW)
    assert sorted(out) == ["bary", "color", "depth", "mask", "normal", "tri"] and out["color"] is None
    assert out["depth"].shape == (HW, HW) and out["depth"].dtype == torch.float32 and out["mask"].dtype == torch.bool
    assert out["tri"].shape == (HW, HW) and out["tri"].dtype == torch.int32 and out["bary"].shape == (HW, HW, 2)
    assert out["normal"].shape == (HW, HW, 3)
    r = get_rays(pose[None], INTRINSICS, HW, HW, -1)
    o, d = r["rays_o"].reshape(-1, 3).cpu().numpy(), r["rays_d"].reshape(-1, 3).cpu().numpy()
    rt, rtri, rbary = rr.first_hit(o, d, v.cpu().numpy(), t.cpu().numpy())
    mask = out["mask"].cpu().numpy().reshape(-1)
    assert np.array_equal(mask, rtri >= 0) and 100 < mask.sum() < HW * HW - 100
    assert out["tri"].cpu().numpy().reshape(-1).tobytes() == rtri.tobytes()
    depth = out["depth"].cpu().numpy().reshape(-1)
    assert depth[mask].tobytes() == rt[mask].tobytes() and np.all(depth[~mask] == 0)
    # the analytic distance to the sphere of radius 0.4 around c, in float64: within one lattice spacing at the pixels the ray meets it
    o64, d64, c = o.astype(np.float64), d.astype(np.float64), np.array([0.1, -0.05, 0.0])
    b = ((o64 - c) * d64).sum(axis=1)
    disc = b * b - (((o64 - c) ** 2).sum(axis=1) - 0.4 ** 2)
    both = mask & (disc > 0)
    assert both.sum() > 100
    # every hit pixel, silhouette included: the mesh lies within a lattice spacing of the sphere, so a ray that hits it passes within
    # radius + spacing of the centre, and one that passes within radius - spacing cannot miss it; the pixels that hit the mesh while
    # the analytic ray misses the sphere can only lie in that ring
    closest = np.sqrt(np.maximum(((o64 - c) ** 2).sum(axis=1) - b * b, 0.0))
    stray = mask & ~(disc > 0)
    print("render_mesh: %d hit pixels outside the analytic silhouette, largest distance from the centre %.4f" % (stray.sum(), closest[mask].max()))
    assert np.all(closest[mask] <= 0.4 + 2.0 / 32) and np.all(mask[(closest <= 0.4 - 2.0 / 32) & (b < 0)])
    tangent = -b[stray]  # the parameter of the closest approach: a stray hit, within radius + spacing of the centre, is within the
    assert np.all(np.abs(depth[stray] - tangent) <= np.sqrt((0.4 + 2.0 / 32) ** 2 - 0.4 ** 2))  # ring's half chord of it
    exact = -b[both] - np.sqrt(disc[both])
    print("render_mesh: %d pixels hit, largest |depth - analytic| = %.4f (lattice spacing %.4f)" % (
        mask.sum(), np.abs(depth[both] - exact).max(), 2.0 / 32))
    assert np.all(np.abs(depth[both] - exact) <= 2.0 / 32)
    # without vertex normals: the face normal, unit, towards the camera; (0,0,0) off the mesh
    nrm = out["normal"].cpu().numpy().reshape(-1, 3).astype(np.float64)
    assert np.all((nrm[mask] * -d64[mask]).sum(axis=1) > 0) and np.all(np.abs(np.linalg.norm(nrm[mask], axis=1) - 1) <= 1e-5)
    assert np.all(nrm[~mask] == 0)
    # with vertex normals: unit length, and outwards (the extraction's normals point out of the sphere)
    col = torch.tensor([0.25, 0.5, 0.75], device=DEV).expand(v.shape[0], 3).contiguous()
    out2 = render_mesh(v, t, pose, INTRINSICS, HW, HW, normals=n, colors=col, bg_color=(1.0, 0.0, 0.5), grid=5)
    assert torch.equal(out2["mask"], out["mask"]) and torch.equal(out2["depth"], out["depth"]) and torch.equal(out2["tri"], out["tri"])
    n2 = out2["normal"].cpu().numpy().reshape(-1, 3).astype(np.float64)
    assert np.all(np.abs(np.linalg.norm(n2[mask], axis=1) - 1) <= 1e-5) and np.all(n2[~mask] == 0)
    point = o64[mask] + depth[mask, None] * d64[mask]
    assert np.all((n2[mask] * (point - c)).sum(axis=1) > 0)
    c2 = out2["color"].cpu().numpy().reshape(-1, 3)
    assert np.all(np.abs(c2[mask] - np.array([0.25, 0.5, 0.75], np.float32)) <= 2e-7)  # three weights that sum to 1 within 2^-23
    assert np.all(c2[~mask] == np.array([1.0, 0.0, 0.5], np.float32))
    # an empty mesh renders the background
    empty = render_mesh(v, t[:0], pose, INTRINSICS, HW, HW, colors=col, bg_color=0.5)
    assert not bool(empty["mask"].any()) and bool((empty["color"] == 0.5).all()) and bool((empty["normal"] == 0).all())


def test_evaluate_mesh_views_against_its_own_renders():
    from pvd.mesh import evaluate_mesh_views, render_mesh
    from pvd.scene import nerf_matrix_to_ngp, pose_spherical
    v, t, n = _analytic_sphere()
    col = (0.5 + 0.4 * n).clamp(0.0, 1.0)
    poses = torch.from_numpy(np.stack([nerf_matrix_to_ngp(pose_spherical(a, -30.0, 2.0), scale=1.0) for a in (0.0, 120.0, 240.0)])).to(DEV)
    truth = torch.stack([render_mesh(v, t, p, INTRINSICS, HW, HW, colors=col)["color"] for p in poses])
    rep = evaluate_mesh_views(v, t, col, poses, INTRINSICS, HW, HW, truth)
    assert rep["n"] == 3 and rep["psnr"] == float("inf") and abs(rep["ssim"] - 1.0) <= 1e-6  # MSE exactly 0
    assert 0.05 < rep["coverage"] < 0.95
    # against a different truth the score is finite, and a callable truth is asked with the view's rays
    seen = []

    def white(rays_o, rays_d):
        seen.append(tuple(rays_o.shape))
        return torch.ones(HW * HW, 3, device=DEV)
    rep2 = evaluate_mesh_views(v, t, col, poses, INTRINSICS, HW, HW, white, keep_images=True)
    assert 0 < rep2["psnr"] < 40 and rep2["coverage"] == rep["coverage"] and len(rep2["images"]) == 3 and seen == [(1, HW * HW, 3)] * 3
    assert torch.equal(rep2["images"][1], truth[1])
