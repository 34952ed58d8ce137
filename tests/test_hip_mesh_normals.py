"""pvd_mesh_normals (csrc/mesh.hip, include/pvd_hip_mesh_attr.h) and the attribute functions of pvd/mesh.py -- extract_mesh's
with_normals, vertex_colors, extract_surface, write_ply with normals and colours -- against the numpy restatement
(tests/mesh_normals_restatement.py, pinned by tests/test_mesh_normals_restatement.py).

Sizes.  R = 2 (only one-sided differences), 3 (mixed), 9 and 17 (a workgroup's 256 points end inside a row / a plane), 33 (141
workgroups, so the first vertex index carries between workgroups; the smooth field and the far spheres cross the faces of the box,
so vertices owned by border points take the c == 0 and c == R-1 branches).  The box is the non-cubic one of tests/test_hip_mesh.py:
every axis has its own inv_h.

The zero rows ((0,0,0): a NaN in a stencil or in t, or a gradient of length 0) must be exactly the restatement's.  Every other
component is compared with the float64 restatement on the same float32 inputs under a bound derived from the kernel's operation
chain, per vertex and per axis (eps = 2^-24; relative errors add to first order, the factor at the end covers the rest):
    d_a      one rounded difference (the * 0.5 is exact)                                                     rel eps
    inv_h_a  rounded extent, rounded division                                                                rel 2 eps
    g_a      = d_a * inv_h_a, one product                                                                    rel 4 eps
    t        = (thresh - u_A) / (u_B - u_A): two rounded differences, one division (tests/test_hip_mesh.py)  rel 3 eps, t <= 1
    G_a      = g_a(A) + t * (g_a(B) - g_a(A)), with S_a = |g_a(A)| + |g_a(B)| >= every magnitude in it: the difference carries its
             inputs' 4 eps S_a and its own rounding, 5 eps S_a, which t <= 1 does not enlarge; the product adds t's 3 eps and its
             own eps, 4 eps S_a; the sum adds g_a(A)'s 4 eps S_a and its own eps S_a:
                                                                              |dG_a| <= (5 + 4 + 4 + 1) eps S_a = 14 eps S_a
    len      = sqrt(G_x^2 + G_y^2 + G_z^2): |d len| <= |dG|_2 + (squares, two sums, square root: 2.5 eps len)
                                                                              <= 14 eps |S|_2 + 2.5 eps len
    n_a      = -G_a / len: |dn_a| <= |dG_a| / len + |n_a| |d len| / len + eps |n_a|, with |n_a| <= 1:
                                                                   |dn_a| <= eps * ((14 S_a + 14 |S|_2) / len + 4)
    bound_a  = that * 1.001
It is derived, not measured; it grows where the two endpoint gradients cancel (len small against S).  No vertex is left out."""
import functools
import os

import numpy as np
import pytest
import torch

import mesh_normals_restatement as nr
import mesh_restatement as mr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
THRESH = 0.125
BMIN, BMAX = (-1.0, -0.5, 0.25), (1.0, 1.5, 2.0)
SIZES = (2, 3, 9, 17, 33)
KINDS = ("sphere", "torus", "two_spheres", "smooth", "plane", "nan")


@functools.lru_cache(maxsize=None)
def _reference(kind, R):
    """(field, float64 normals, S, len, bound) -- computed once, read-only."""
    u = nr.field(kind, R, THRESH)
    n, S, length = nr.normals(u, THRESH, BMIN, BMAX, np.float64)
    bound = nr.bound(S, length)
    for a in (u, n, S, length, bound):
        a.setflags(write=False)
    return u, n, S, length, bound


def _extract(u, **kw):
    from pvd.mesh import extract_mesh
    return extract_mesh(torch.from_numpy(np.array(u, np.float32)).to(DEV), THRESH, BMIN, BMAX, **kw)


def _compare(label, R, normals, ref, bound):
    assert normals.shape == ref.shape, (label, normals.shape, ref.shape)
    assert np.all(np.isfinite(normals)), label
    zero, ref_zero = np.all(normals == 0, axis=1), np.all(ref == 0, axis=1)
    assert np.array_equal(zero, ref_zero), (label, int(zero.sum()), int(ref_zero.sum()))
    live = ~ref_zero
    if live.any():
        err = np.abs(normals[live].astype(np.float64) - ref[live])
        ratio = err / bound[live]
        print("%s R=%d: V=%d (%d zero rows), largest error %.3g, largest bound %.3g, largest error / bound %.4f"
              % (label, R, len(ref), int(ref_zero.sum()), err.max(), bound[live].max(), ratio.max()))
        assert np.all(err <= bound[live]), (label, float(ratio.max()))


@pytest.mark.parametrize("R", SIZES)
@pytest.mark.parametrize("kind", KINDS)
def test_the_normals_are_the_restatements(kind, R):
    u, ref, _, _, bound = _reference(kind, R)
    verts0, tris0 = _extract(u)
    verts, tris, normals = _extract(u, with_normals=True)
    assert normals.dtype == torch.float32 and normals.is_cuda and normals.shape == (verts0.shape[0], 3)
    # the keyword changes neither vertices nor triangles (NaN coordinates included: compare the bits)
    assert verts.cpu().numpy().tobytes() == verts0.cpu().numpy().tobytes() and torch.equal(tris, tris0)
    _compare(kind, R, normals.cpu().numpy(), ref, bound)
    if kind == "nan" and R >= 9:
        assert np.all(ref == 0, axis=1).any()
    # a second run gives the same bits
    normals2 = _extract(u, with_normals=True)[2]
    assert normals.cpu().numpy().tobytes() == normals2.cpu().numpy().tobytes()


def test_vertices_owned_by_border_points_take_the_one_sided_branches():
    """far_spheres at R = 33: one sphere is cut by the face x = 1, so points of the last x-layer own vertices."""
    R = 33
    u, ref, _, _, bound = _reference("far_spheres", R)
    owners = mr.topology(u, THRESH)[0]
    assert (owners // (R * R) == R - 1).sum() > 10
    _compare("far_spheres", R, _extract(u, with_normals=True)[2].cpu().numpy(), ref, bound)
    # and the smooth field's surface leaves the box through several faces: owners with an index 0 and with an index R - 1
    p = np.stack(np.unravel_index(mr.topology(_reference("smooth", R)[0], THRESH)[0], (R, R, R)), axis=1)
    assert (p == 0).any() and (p == R - 1).any()


def test_rows_past_v_are_never_written():
    import pvd_hip
    R = 17
    u_np, ref, _, _, bound = _reference("torus", R)
    u = torch.from_numpy(np.array(u_np)).to(DEV)
    ws = torch.empty(pvd_hip.mesh_workspace_bytes(R), dtype=torch.uint8, device=DEV)
    totals = torch.zeros(2, dtype=torch.int32, device=DEV)
    pvd_hip.mesh_count(u, R, THRESH, ws, totals)
    V = int(totals[0])
    assert V == len(ref)
    lo, hi = torch.tensor(BMIN, device=DEV), torch.tensor(BMAX, device=DEV)
    normals = torch.full((V, 3), 7.0, device=DEV)
    pvd_hip.mesh_normals(u, R, THRESH, lo, hi, ws, normals[:V // 2])
    assert bool((normals[V // 2:] == 7.0).all())
    _compare("torus, first half", R, normals[:V // 2].cpu().numpy(), ref[:V // 2], bound[:V // 2])
    pvd_hip.mesh_normals(u, R, THRESH, lo, hi, ws, normals[:0])  # V == 0: PVD_OK, no launch
    with pytest.raises(pvd_hip.PvdHipError):
        pvd_hip.mesh_normals(u, R, THRESH, lo, hi, ws, torch.zeros(4, device=DEV))  # not [V,3]
    with pytest.raises(pvd_hip.PvdHipError):
        pvd_hip.mesh_normals(u, R, THRESH, lo, hi, ws[:-1], normals)  # short workspace


# ---------------------------------------------------------------------------------------------------------------- vertex_colors
def _stub_colour(x, d):
    return 0.5 + 0.3 * d + 0.1 * torch.sin(x)  # in [0.1, 0.9]


class _StubModel:
    """What vertex_colors needs of a model: __call__(x, d) -> (sigma, rgb) and aabb_infer.  Never sees a non-finite input."""

    def __init__(self):
        self.aabb_infer = torch.tensor([BMIN + BMAX], device=DEV).reshape(6)
        self.calls = []

    def __call__(self, x, d):
        assert x.is_cuda and d.is_cuda and x.shape == d.shape and x.shape[1] == 3
        assert x.dtype == torch.float32 and d.dtype == torch.float32
        assert bool(torch.isfinite(x).all()) and bool(torch.isfinite(d).all())
        assert not torch.is_grad_enabled()
        self.calls.append(int(x.shape[0]))
        return torch.zeros(x.shape[0], device=x.device), _stub_colour(x, d)


def test_vertex_colors_of_a_closed_form_model():
    from pvd.mesh import vertex_colors
    verts, _, normals = _extract(_reference("sphere", 17)[0], with_normals=True)
    V = verts.shape[0]
    assert V > 1000
    model = _StubModel()
    colours = vertex_colors(model, verts, normals)
    assert colours.shape == (V, 3) and colours.dtype == torch.float32 and colours.is_cuda and model.calls == [V]
    assert torch.equal(colours, _stub_colour(verts, -normals))
    for autocast in (True, False):
        model = _StubModel()
        assert torch.equal(vertex_colors(model, verts, normals, chunk=1000, autocast=autocast), colours)
        assert model.calls == [1000] * (V // 1000) + [V % 1000]
    # planted rows: a NaN position, an infinite normal -> colour 0 (the model is given the centre of its box instead);
    # a zero normal -> seen along (0, 0, -1)
    v2, n2 = verts.clone(), normals.clone()
    v2[5, 1] = float("nan")
    n2[9, 0] = float("inf")
    n2[7] = 0.0
    got = vertex_colors(_StubModel(), v2, n2, chunk=1000)
    want = colours.clone()
    want[5] = 0.0
    want[9] = 0.0
    want[7] = _stub_colour(verts[7:8], torch.tensor([[0.0, 0.0, -1.0]], device=DEV))[0]
    assert torch.equal(got, want)
    # no vertices: an empty tensor, and the model is not called
    model = _StubModel()
    empty = vertex_colors(model, verts[:0], normals[:0])
    assert empty.shape == (0, 3) and empty.dtype == torch.float32 and model.calls == []


@pytest.mark.parametrize("model_type", ["hash", "vm"])
def test_vertex_colors_of_a_randomly_initialised_model(model_type):
    from pvd.config import PVDConfig
    from pvd.mesh import density_field, extract_mesh, vertex_colors
    from pvd.ops import hip_ops
    from pvd.workload import make_model
    torch.manual_seed(3)
    opt = PVDConfig(model_type=model_type, resolution0=64) if model_type == "vm" else PVDConfig(model_type=model_type)
    model = make_model(hip_ops(), opt, model_type, model_type == "hash", torch.device(DEV)).eval()
    R = 16
    lo, hi = model.aabb_infer[:3], model.aabb_infer[3:]
    u = density_field(lambda x: model.density(x)["sigma"], R, lo, hi)
    verts, tris, normals = extract_mesh(u, float(u.median()), lo, hi, with_normals=True)
    V = verts.shape[0]
    assert V > 100 and bool(torch.isfinite(verts).all()) and bool(torch.isfinite(normals).all())
    chunk = 1 + V // 3  # three calls, the last one shorter
    colours = vertex_colors(model, verts, normals, chunk=chunk)
    assert colours.shape == (V, 3) and colours.dtype == torch.float32
    assert bool(torch.isfinite(colours).all()) and float(colours.min()) >= 0.0 and float(colours.max()) <= 1.0
    zero = (normals == 0).all(dim=1, keepdim=True)
    d = torch.where(zero, torch.tensor([0.0, 0.0, -1.0], device=DEV), -normals)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        direct = torch.cat([model(verts[s:s + chunk].clone(), d[s:s + chunk].clone())[1].float() for s in range(0, V, chunk)])
    assert torch.equal(colours, direct)
    assert float(colours.std()) > 0  # not one constant colour


# -------------------------------------------------------------------------------------------------------------- extract_surface
class _AnalyticSphere:
    """The analytic density of tests/test_hip_mesh.py (sigma = 2 on the sphere of radius 0.4 around CENTRE), with a forward."""
    cuda_ray = False
    density_thresh = 2.0
    CENTRE = (0.1, -0.05, 0.0)

    def __init__(self):
        self.aabb_infer = torch.tensor([-1.0, -1.0, -1.0, 1.0, 1.0, 1.0], device=DEV)

    def density(self, x):
        assert x.is_cuda and x.shape[1] == 3
        return {"sigma": 4.0 - 5.0 * torch.linalg.norm(x - torch.tensor(self.CENTRE, device=x.device), dim=1)}

    def __call__(self, x, d):
        assert bool(torch.isfinite(x).all()) and bool(torch.isfinite(d).all())
        return self.density(x)["sigma"], _stub_colour(x, d)


def test_extract_surface_end_to_end_on_an_analytic_density():
    from pvd.mesh import extract_geometry, extract_surface
    R = 24
    model = _AnalyticSphere()
    m = extract_surface(model, resolution=R)
    assert sorted(m) == ["colors", "counts", "field", "normals", "threshold", "triangles", "vertices"]
    assert m["threshold"] == 2.0 and m["counts"] is None and m["field"].shape == (R, R, R)
    verts, tris = extract_geometry(model, resolution=R)
    assert torch.equal(m["vertices"], verts) and torch.equal(m["triangles"], tris)
    V = verts.shape[0]
    assert m["normals"].shape == (V, 3) and m["colors"].shape == (V, 3)
    radial = verts - torch.tensor(model.CENTRE, device=DEV)
    radial = radial / torch.linalg.norm(radial, dim=1, keepdim=True)
    off = float((m["normals"] - radial).abs().max())
    print("analytic sphere R=%d: V=%d, largest |n - radial| component %.4f" % (R, V, off))
    assert off <= 0.02
    assert torch.equal(m["colors"], _stub_colour(verts, -m["normals"]))
    # colours without normals: computed along the normals all the same; neither: geometry only
    only = extract_surface(model, resolution=R, normals=False)
    assert only["normals"] is None and torch.equal(only["colors"], m["colors"])
    bare = extract_surface(model, resolution=R, normals=False, colors=False)
    assert bare["normals"] is None and bare["colors"] is None and torch.equal(bare["vertices"], verts)
    half = extract_surface(model, resolution=R, colors=False)
    assert half["colors"] is None and torch.equal(half["normals"], m["normals"])
    # with filtering, counts is (components found, components kept, points kept)
    kept = extract_surface(model, resolution=R, largest_only=True)
    assert kept["counts"][:2] == (1, 1) and kept["counts"][2] > 0 and torch.equal(kept["vertices"], verts)


# -------------------------------------------------------------------------------------------------------------------- write_ply
def _read_ply(path):
    """Binary little-endian PLY with float / uchar vertex properties and uchar-counted int faces -> ({name: column}, triangles)."""
    kinds = {b"float": "<f4", b"uchar": "u1"}
    with open(path, "rb") as f:
        assert f.readline() == b"ply\n" and f.readline() == b"format binary_little_endian 1.0\n"
        counts, fields, element, line = {}, [], None, f.readline()
        while line != b"end_header\n":
            words = line.split()
            if words[0] == b"element":
                element = words[1]
                counts[element.decode()] = int(words[2])
            elif words[0] == b"property" and element == b"vertex":
                fields.append((words[2].decode(), kinds[words[1]]))
            else:
                assert line == b"property list uchar int vertex_indices\n", line
            line = f.readline()
        dt = np.dtype(fields)
        rows = np.frombuffer(f.read(dt.itemsize * counts["vertex"]), dt)
        faces = np.frombuffer(f.read(13 * counts["face"]), np.dtype([("n", "u1"), ("v", "<i4", (3,))]))
        assert f.read() == b"" and np.all(faces["n"] == 3)
    return rows, faces["v"]


def test_write_ply_with_normals_and_colours_round_trips(tmp_path):
    from pvd.mesh import write_ply
    v, t, n = _extract(_reference("two_spheres", 17)[0], with_normals=True)
    c = _stub_colour(v, -n)
    c[0] = torch.tensor([-0.5, 1.5, 0.5], device=DEV)  # clamped: 0, 255, round(127.5) = 128
    path = write_ply(os.path.join(str(tmp_path), "full.ply"), v, t, normals=n, colors=c)
    rows, tris = _read_ply(path)
    assert rows.dtype.names == ("x", "y", "z", "nx", "ny", "nz", "red", "green", "blue") and rows.dtype.itemsize == 27
    vn, nn, cn = v.cpu().numpy(), n.cpu().numpy(), c.cpu().numpy()
    assert np.array_equal(np.stack([rows["x"], rows["y"], rows["z"]], axis=1), vn)
    assert np.array_equal(np.stack([rows["nx"], rows["ny"], rows["nz"]], axis=1), nn)
    want = np.round(np.clip(cn, 0.0, 1.0) * 255.0).astype(np.uint8)
    assert np.array_equal(np.stack([rows["red"], rows["green"], rows["blue"]], axis=1), want) and tuple(want[0]) == (0, 255, 128)
    assert np.array_equal(tris, t.cpu().numpy())
    # one attribute at a time
    rows, _ = _read_ply(write_ply(os.path.join(str(tmp_path), "n.ply"), v, t, normals=n))
    assert rows.dtype.names == ("x", "y", "z", "nx", "ny", "nz") and np.array_equal(rows["nz"], nn[:, 2])
    rows, _ = _read_ply(write_ply(os.path.join(str(tmp_path), "c.ply"), v, t, colors=c))
    assert rows.dtype.names == ("x", "y", "z", "red", "green", "blue") and np.array_equal(rows["blue"], want[:, 2])
    # without them the file is what it was: the header of three properties, 12 bytes per vertex, 13 per face
    plain = open(write_ply(os.path.join(str(tmp_path), "plain.ply"), v, t), "rb").read()
    assert plain == open(write_ply(os.path.join(str(tmp_path), "none.ply"), v, t, normals=None, colors=None), "rb").read()
    header = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
              "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % (len(vn), len(tris))).encode("ascii")
    faces = np.empty(len(tris), dtype=[("n", "u1"), ("v", "<i4", (3,))])
    faces["n"], faces["v"] = 3, t.cpu().numpy()
    assert plain == header + vn.astype("<f4").tobytes() + faces.tobytes()
