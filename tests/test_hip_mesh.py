"""pvd_mesh_count / pvd_mesh_emit (csrc/mesh.hip, include/pvd_hip_mesh.h) and pvd/mesh.py against the numpy restatement of marching
tetrahedra on the Kuhn split (tests/mesh_restatement.py, pinned by tests/test_mesh_restatement.py).

Sizes.  R = 2 (one cell), 3, 9 and 17 (a workgroup's 256 points end inside a row / a plane), 33 (141 workgroups: the scan of the
per-workgroup sums and the add pass really carry offsets between workgroups).  The scan of the per-workgroup sums walks them in
chunks of 8192 with a carry; a second chunk needs more than 8192 * 256 lattice points, i.e. R >= 129, so one more case runs at
R = 129 with two small spheres, one in the first chunk and one that reaches into the second -- which is only the last two
x-layers there -- (the restatement only loops over the cells the surface crosses).

Topology (V, T, every index of `triangles`) must be identical.  Positions are compared with the float64 restatement on the same
float32 inputs, per axis, under a bound derived from the kernel's operation chain (eps = 2^-24, E = |bmax - bmin|,
B = max(|bmin|, |bmax|) of the axis):
    t   = (thresh - u_a) / (u_b - u_a)   two rounded differences and one rounded division: relative error 3 eps, t <= 1  -> 3 eps
    l   = p + t                          one rounded sum of magnitude <= R - 1                                        -> (R - 1) eps
    w   = l / (R - 1) * (bmax - bmin)    three roundings (division, extent, product) of a value <= E: 3 eps E, and the error of l
                                         scaled by E / (R - 1)                                     -> eps E (3 + 1 + 3 / (R - 1))
    out = w + bmin                       one rounded sum of magnitude <= B                                            -> eps B
    bound = eps * (E * (4 + 3 / (R - 1)) + B) * 1.001      (the factor covers the terms of order eps^2, which are ~1e-6 of it)
A vertex whose edge ends in a NaN has NaN coordinates in both; every other coordinate of every case is under the bound."""
import functools
import os

import numpy as np
import pytest
import torch

import mesh_restatement as mr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
THRESH = 0.125
BMIN, BMAX = (-1.0, -0.5, 0.25), (1.0, 1.5, 2.0)
SIZES = (2, 3, 9, 17, 33)
EPS = 2.0 ** -24


def _smooth(R, seed):
    rng = np.random.RandomState(seed)
    X, Y, Z = mr.grid(R)
    u = np.zeros_like(X)
    for _ in range(4):
        f, ph = rng.uniform(0.5, 3.0, 3), rng.uniform(0, 2 * np.pi, 3)
        u += rng.uniform(0.3, 1.0) * np.sin(f[0] * X + ph[0]) * np.sin(f[1] * Y + ph[1]) * np.sin(f[2] * Z + ph[2])
    return u.astype(np.float32)


def _field(kind, R):
    if kind == "sphere":
        u = mr.sphere_field(R)
    elif kind == "torus":
        u = mr.torus_field(R)
    elif kind == "two_spheres":
        u = mr.two_spheres_field(R)
    elif kind == "smooth":
        u = _smooth(R, 7)
    elif kind == "plane":  # u == thresh on the whole layer i = (R - 1) // 2: outside, and t = 0 on every edge that leaves it
        i = np.arange(R, dtype=np.float32)[:, None, None]
        return np.broadcast_to((i - (R - 1) // 2) * np.float32(0.5) + np.float32(THRESH), (R, R, R)).astype(np.float32).copy()
    elif kind == "nan":
        u = _smooth(R, 11)
        u[np.random.RandomState(R).uniform(size=u.shape) < 0.02] = np.nan
    elif kind == "all_inside":
        u = np.ones((R, R, R), np.float32)
    elif kind == "all_outside":
        u = -np.ones((R, R, R), np.float32)
    elif kind == "far_spheres":  # two small spheres, near the first lattice points and cut by the face x = 1, where the last ones are
        u = mr.two_spheres_field(R, 0.12, (-0.8, -0.75, -0.7), (1.0, 0.75, 0.7))
    else:
        raise KeyError(kind)
    return (u + np.float32(THRESH)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _reference(kind, R):
    """(field, float64 vertices, triangles) -- computed once, read-only."""
    u = _field(kind, R)
    verts, tris = mr.extract(u, THRESH, BMIN, BMAX, np.float64)
    for a in (u, verts, tris):
        a.setflags(write=False)
    return u, verts, tris


def _bound(R, bmin=BMIN, bmax=BMAX):
    lo, hi = np.asarray(bmin, np.float32).astype(np.float64), np.asarray(bmax, np.float32).astype(np.float64)
    return EPS * ((hi - lo) * (4.0 + 3.0 / (R - 1)) + np.maximum(np.abs(lo), np.abs(hi))) * 1.001


def _extract(u, thresh=THRESH, bmin=BMIN, bmax=BMAX):
    from pvd.mesh import extract_mesh
    v, t = extract_mesh(torch.from_numpy(np.array(u, np.float32)).to(DEV), thresh, bmin, bmax)
    assert v.dtype == torch.float32 and t.dtype == torch.int32 and v.shape[1:] == (3,) and t.shape[1:] == (3,)
    return v.cpu().numpy(), t.cpu().numpy()


def _compare(label, R, verts, tris, ref_verts, ref_tris, bmin=BMIN, bmax=BMAX):
    assert verts.shape == ref_verts.shape and tris.shape == ref_tris.shape, (label, verts.shape, ref_verts.shape, tris.shape, ref_tris.shape)
    assert np.array_equal(tris, ref_tris), label
    assert np.array_equal(np.isnan(verts), np.isnan(ref_verts)), label
    if len(verts):
        err = np.nan_to_num(np.abs(verts.astype(np.float64) - ref_verts), nan=0.0).max(axis=0)
        bound = _bound(R, bmin, bmax)
        print("%s R=%d: V=%d T=%d, position error per axis %s, bound %s" % (label, R, len(verts), len(tris), err, bound))
        assert np.all(err <= bound), (label, err, bound)


@pytest.mark.parametrize("R", SIZES)
@pytest.mark.parametrize("kind", ["sphere", "torus", "two_spheres", "smooth", "plane", "nan"])
def test_the_mesh_is_the_restatements(kind, R):
    u, ref_verts, ref_tris = _reference(kind, R)
    verts, tris = _extract(u)
    _compare(kind, R, verts, tris, ref_verts, ref_tris)
    if R >= 9:
        assert len(tris) > 100
    # a second run gives the same bits
    verts2, tris2 = _extract(u)
    assert verts.tobytes() == verts2.tobytes() and tris.tobytes() == tris2.tobytes()


def test_the_plane_case_is_degenerate_as_meant():
    u, ref_verts, ref_tris = _reference("plane", 9)
    assert (u == np.float32(THRESH)).sum() == 81 and len(ref_tris) > 0
    x = BMIN[0] + 4 / 8 * (BMAX[0] - BMIN[0])
    assert np.all(ref_verts[:, 0] == x)  # t = 0: every vertex lies in the layer itself


def test_the_nan_case_has_nan_vertices():
    _, ref_verts, _ = _reference("nan", 17)
    assert np.isnan(ref_verts).any() and np.isfinite(ref_verts).any()


@pytest.mark.parametrize("R", SIZES)
@pytest.mark.parametrize("kind", ["all_inside", "all_outside"])
def test_a_field_without_a_surface_gives_empty_tensors(kind, R):
    import pvd_hip
    u = torch.from_numpy(_field(kind, R)).to(DEV)
    ws = torch.empty(pvd_hip.mesh_workspace_bytes(R), dtype=torch.uint8, device=DEV)
    totals = torch.full((2,), -1, dtype=torch.int32, device=DEV)
    pvd_hip.mesh_count(u, R, THRESH, ws, totals)
    assert totals.tolist() == [0, 0]
    lo, hi = torch.tensor(BMIN, device=DEV), torch.tensor(BMAX, device=DEV)
    pvd_hip.mesh_emit(u, R, THRESH, lo, hi, ws, torch.empty(0, 3, device=DEV), torch.empty(0, 3, dtype=torch.int32, device=DEV))  # PVD_OK
    verts, tris = _extract(u.cpu().numpy())
    assert verts.shape == (0, 3) and tris.shape == (0, 3)


def test_the_block_sum_scan_carries_into_a_second_chunk():
    R = 129
    assert -(-R ** 3 // 256) > 8192  # more per-workgroup sums than one chunk of the scan
    u, ref_verts, ref_tris = _reference("far_spheres", R)
    assert len(np.unique(mr.components(len(ref_verts), ref_tris))) == 2
    owners = mr.topology(u, THRESH)[0]
    assert owners.min() // 256 < 8192 and (owners // 256 >= 8192).sum() > 100  # vertices on both sides of the chunk boundary
    verts, tris = _extract(u)
    _compare("far_spheres", R, verts, tris, ref_verts, ref_tris)


def test_rows_past_the_totals_are_never_written():
    """mesh_emit with V and T smaller than the totals stays inside the tensors it was given."""
    import pvd_hip
    R = 9
    u_np, ref_verts, ref_tris = _reference("sphere", R)
    u = torch.from_numpy(np.array(u_np)).to(DEV)
    ws = torch.empty(pvd_hip.mesh_workspace_bytes(R), dtype=torch.uint8, device=DEV)
    totals = torch.zeros(2, dtype=torch.int32, device=DEV)
    pvd_hip.mesh_count(u, R, THRESH, ws, totals)
    V, T = totals.tolist()
    assert (V, T) == (len(ref_verts), len(ref_tris))
    verts = torch.full((V, 3), 7.0, device=DEV)
    tris = torch.full((T, 3), -7, dtype=torch.int32, device=DEV)
    lo, hi = torch.tensor(BMIN, device=DEV), torch.tensor(BMAX, device=DEV)
    pvd_hip.mesh_emit(u, R, THRESH, lo, hi, ws, verts[:V // 2], tris[:T // 2])
    assert bool((verts[V // 2:] == 7.0).all()) and bool((tris[T // 2:] == -7).all())
    assert np.array_equal(tris[:T // 2].cpu().numpy(), ref_tris[:T // 2])


class _AnalyticSphere:
    """What extract_geometry needs of a model: density(), density_thresh, aabb_infer (no occupancy grid)."""
    cuda_ray = False
    density_thresh = 2.0

    def __init__(self):
        self.aabb_infer = torch.tensor([-1.0, -1.0, -1.0, 1.0, 1.0, 1.0], device=DEV)

    def density(self, x):
        assert x.is_cuda and x.shape[1] == 3
        return {"sigma": 4.0 - 5.0 * torch.linalg.norm(x - torch.tensor([0.1, -0.05, 0.0], device=x.device), dim=1)}  # = 2 at radius 0.4


def test_extract_geometry_end_to_end_on_an_analytic_density():
    from pvd.mesh import extract_geometry
    R = 24
    verts, tris, u = extract_geometry(_AnalyticSphere(), resolution=R, return_field=True)
    assert u.shape == (R, R, R) and u.is_cuda and u.dtype == torch.float32
    box = ((-1.0,) * 3, (1.0,) * 3)
    ref_verts, ref_tris = mr.extract(u.cpu().numpy(), 2.0, *box, np.float64)
    _compare("analytic sphere", R, verts.cpu().numpy(), tris.cpu().numpy(), ref_verts, ref_tris, *box)
    # the field is the density at the lattice points, and the mesh is the sphere
    X, Y, Z = mr.grid(R)
    truth = 4.0 - 5.0 * np.sqrt((X - 0.1) ** 2 + (Y + 0.05) ** 2 + Z ** 2)
    assert np.abs(u.cpu().numpy() - truth).max() < 1e-5
    radius = np.linalg.norm(ref_verts - np.array([0.1, -0.05, 0.0]), axis=1)
    assert np.abs(radius - 0.4).max() < 0.02 and mr.signed_volume(verts.cpu().numpy(), tris.cpu().numpy()) > 0
    # chunked filling gives the same field
    from pvd.mesh import density_field
    u2 = density_field(lambda x: _AnalyticSphere().density(x)["sigma"], R, *box, chunk=1000, device=torch.device(DEV))
    assert torch.equal(u, u2)


def test_extract_geometry_of_a_randomly_initialised_hash_model():
    from pvd.config import PVDConfig
    from pvd.mesh import default_threshold, density_field, extract_geometry
    from pvd.ops import hip_ops
    from pvd.workload import make_model
    torch.manual_seed(3)
    model = make_model(hip_ops(), PVDConfig(model_type="hash"), "hash", True, torch.device(DEV)).eval()
    assert model.mean_density == 0 and default_threshold(model) == float(model.density_thresh)  # no occupancy statistics yet
    model.mean_density = torch.tensor(3.5, device=DEV)  # as update_extra_state leaves it: on the device
    assert default_threshold(model) == 3.5 < float(model.density_thresh)
    model.mean_density = 1e9
    assert default_threshold(model) == float(model.density_thresh)
    R = 16
    u = density_field(lambda x: model.density(x)["sigma"], R, model.aabb_infer[:3], model.aabb_infer[3:])
    thresh = float(u.median())
    verts, tris = extract_geometry(model, resolution=R, threshold=thresh)
    V = verts.shape[0]
    assert V > 0 and tris.shape[0] > 0
    assert bool(torch.isfinite(verts).all())
    assert bool((verts >= model.aabb_infer[:3]).all()) and bool((verts <= model.aabb_infer[3:]).all())
    assert int(tris.min()) >= 0 and int(tris.max()) < V
    ref_verts, ref_tris = mr.extract(u.cpu().numpy(), thresh, model.aabb_infer[:3].cpu().numpy(), model.aabb_infer[3:].cpu().numpy(), np.float64)
    assert np.array_equal(tris.cpu().numpy(), ref_tris) and verts.shape == ref_verts.shape


def _read_ply(path):
    """Binary little-endian PLY with float x y z vertices and uchar-counted int faces -> (vertices, triangles)."""
    with open(path, "rb") as f:
        assert f.readline() == b"ply\n" and f.readline() == b"format binary_little_endian 1.0\n"
        counts, line = {}, f.readline()
        while line != b"end_header\n":
            words = line.split()
            if words[0] == b"element":
                counts[words[1].decode()] = int(words[2])
            line = f.readline()
        verts = np.frombuffer(f.read(12 * counts["vertex"]), "<f4").reshape(-1, 3)
        faces = np.frombuffer(f.read(13 * counts["face"]), np.dtype([("n", "u1"), ("v", "<i4", (3,))]))
        assert f.read() == b"" and np.all(faces["n"] == 3)
    return verts, faces["v"]


def test_write_ply_round_trips(tmp_path):
    from pvd.mesh import write_ply
    u, _, _ = _reference("two_spheres", 17)
    v, t = (torch.from_numpy(a).to(DEV) for a in _extract(u))
    path = write_ply(os.path.join(str(tmp_path), "mesh.ply"), v, t)
    verts, tris = _read_ply(path)
    assert verts.tobytes() == v.cpu().numpy().tobytes() and np.array_equal(tris, t.cpu().numpy())
