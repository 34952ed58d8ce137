"""csrc/mesh_simplify.hip against tests/mesh_simplify_restatement.py (numpy, from include/pvd_hip_mesh_simplify.h), BIT FOR BIT:
new vertices, new attributes, new triangles, vertex_map and the two totals.  Every sum of the definition is an integer sum, so there
is no tolerance anywhere; the one inequality is the Hausdorff distance of the public path against the header's displacement bound.

Sizes.  The scans of the implementation work on workgroups of 256 flags and, in one workgroup, on chunks of 8192 workgroup sums (2^21
flags).  Only cells and triangles are scanned; vertices are merely spread over workgroups of 256.  So: T and V = 255, 256, 257 (one
workgroup, exactly one, two) and 65 537 (257 workgroup sums); G = 7 (343 cells: two workgroups, the second partly filled), G = 41
(68 921 cells, 270 workgroup sums), G = 129 (2 146 689 cells: 8386 workgroup sums, two chunks of the one-workgroup scan), T = 2^21 +
257 (8194 sums: two chunks), and G = 512 (2^27 cells, the largest table) with a handful of vertices."""
import functools
import os

import numpy as np
import pytest
import torch

import mesh_restatement as mr
import mesh_simplify_restatement as sr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(a, dtype):
    return torch.from_numpy(np.array(a, dtype)).to(DEV)  # a copy: the shared inputs are read-only


def _kernels(v, t, lo, hi, G, attrs=None):
    """The two entry points through the binding, as simplify_mesh drives them -> dict of host arrays and the totals."""
    import pvd_hip
    V, T, K = len(v), len(t), 0 if attrs is None else attrs.shape[1]
    dv, dt, dlo, dhi = _dev(v, np.float32).reshape(V, 3), _dev(t, np.int32).reshape(T, 3), _dev(lo, np.float32), _dev(hi, np.float32)
    da = None if attrs is None else _dev(attrs, np.float32)
    ws = torch.empty(pvd_hip.mesh_simplify_workspace_bytes(V, T, G, K), dtype=torch.uint8, device=DEV)
    totals = torch.full((2,), -7, dtype=torch.int32, device=DEV)
    pvd_hip.mesh_simplify_count(dv, dt, dlo, dhi, G, K, ws, totals)
    Vn, Tn = (int(x) for x in totals.tolist())
    assert 0 <= Vn <= min(V, G ** 3) and 0 <= Tn <= T
    # one guard row behind each output: rows past V' / T' are never written
    out_v = torch.full((Vn + 1, 3), 123.0, device=DEV)
    out_t = torch.full((Tn + 1, 3), -9, dtype=torch.int32, device=DEV)
    out_a = torch.full((Vn + 1, K), 123.0, device=DEV) if K else None
    vmap = torch.full((V + 1,), -9, dtype=torch.int32, device=DEV)
    pvd_hip.mesh_simplify_emit(dv, dt, da, dlo, dhi, G, ws, out_v[:Vn], None if out_a is None else out_a[:Vn], out_t[:Tn], vmap[:V])
    torch.cuda.synchronize()
    assert bool((out_v[Vn] == 123.0).all()) and bool((out_t[Tn] == -9).all()) and int(vmap[V]) == -9
    assert out_a is None or bool((out_a[Vn] == 123.0).all())
    return dict(vertices=out_v[:Vn].cpu(), triangles=out_t[:Tn].cpu(), attrs=None if out_a is None else out_a[:Vn].cpu(),
                vertex_map=vmap[:V].cpu(), totals=(Vn, Tn))


def _same_bits(label, got, ref):
    """torch.equal on the bits (floats as int32: -0.0 is not 0.0, and NaN would equal NaN)."""
    assert got["totals"] == (len(ref["vertices"]), len(ref["triangles"])), (label, got["totals"], len(ref["vertices"]), len(ref["triangles"]))
    assert torch.equal(got["vertex_map"], torch.from_numpy(ref["vertex_map"])), label + ": vertex_map"
    assert torch.equal(got["triangles"], torch.from_numpy(ref["triangles"]).reshape(-1, 3)), label + ": triangles"
    assert got["vertices"].dtype == torch.float32
    assert torch.equal(got["vertices"].view(torch.int32), torch.from_numpy(ref["vertices"]).view(torch.int32)), label + ": vertices"
    assert (got["attrs"] is None) == (ref["attrs"] is None)
    if ref["attrs"] is not None:
        assert torch.equal(got["attrs"].view(torch.int32), torch.from_numpy(ref["attrs"]).view(torch.int32)), label + ": attrs"


def _check(label, v, t, lo, hi, G, attrs=None):
    ref = sr.simplify(v, t, lo, hi, G, attrs=attrs)
    got = _kernels(v, t, lo, hi, G, attrs=attrs)
    print("%s: V=%d T=%d G=%d K=%d -> V'=%d T'=%d" % (label, len(v), len(t), G, 0 if attrs is None else attrs.shape[1], *got["totals"]))
    _same_bits(label, got, ref)
    return got, ref


@functools.lru_cache(maxsize=None)
def _sphere():
    v, t, lo, hi = sr.sphere_mesh(12)
    for a in (v, t, lo, hi):
        a.setflags(write=False)
    return v, t, lo, hi


@pytest.mark.parametrize("K", [0, 3, 6])
@pytest.mark.parametrize("G", [1, 2, 3, 5, 8])
def test_the_sphere(G, K):
    v, t, lo, hi = _sphere()
    got, _ = _check("sphere", v, t, lo, hi, G, attrs=sr.sphere_attrs(v, K))
    if G == 1:
        assert got["totals"] == (0, 0) and bool((got["vertex_map"] == -1).all())
    else:
        assert got["totals"][0] > 0 and got["totals"][1] > 0 and bool((got["vertex_map"] >= 0).all())


def test_a_dirty_soup():
    """Indices -1 and V, NaN / +-inf vertices, attributes that are not finite or out of range; vertices outside a given box; a flat
    axis; the default box of simplify_mesh against the same box given explicitly."""
    from pvd.mesh import simplify_mesh
    v, t, a = sr.soup(1000, 3000, seed=0, K=4)
    lo, hi = sr.finite_box(v)
    for G in (2, 7, 41):
        _check("soup, its own box", v, t, lo, hi, G, attrs=a)
    _check("soup, a smaller box", v, t, np.float32([-0.5, -0.75, -1.0]), np.float32([0.5, 0.25, 0.0]), 7, attrs=a)
    got, _ = _check("soup, a flat axis", v, t, np.float32([-1, 0.25, -1]), np.float32([1, 0.25, 1]), 7, attrs=a)
    assert bool((got["vertices"][:, 1] == 0.25).all())
    _check("soup, an inverted axis (flat)", v, t, np.float32([-1, 1, -1]), np.float32([1, -1, 1]), 7)
    # the public path: six attributes (normals and colours), the default box against the explicit one
    nrm, col = a[:, :3], np.abs(a[:, 1:4])
    dv, dt = _dev(v, np.float32), _dev(t, np.int32)
    default = simplify_mesh(dv, dt, 7, normals=_dev(nrm, np.float32), colors=_dev(col, np.float32))
    explicit = simplify_mesh(dv, dt, 7, bmin=lo, bmax=hi, normals=_dev(nrm, np.float32), colors=_dev(col, np.float32))
    ref = sr.simplify(v, t, lo, hi, 7, attrs=np.concatenate([nrm, col], axis=1))
    for m in (default, explicit):
        assert torch.equal(m["vertices"].cpu().view(torch.int32), torch.from_numpy(ref["vertices"]).view(torch.int32))
        assert torch.equal(m["triangles"].cpu(), torch.from_numpy(ref["triangles"]))
        assert torch.equal(m["vertex_map"].cpu(), torch.from_numpy(ref["vertex_map"]))
        assert torch.equal(m["colors"].cpu(), torch.from_numpy(ref["attrs"][:, 3:]).clamp(0.0, 1.0))
        length = np.linalg.norm(ref["attrs"][:, :3].astype(np.float64), axis=1)
        got_len = torch.linalg.norm(m["normals"].double(), dim=1).cpu().numpy()
        assert np.all(np.abs(got_len[length > 0] - 1.0) <= 1e-6) and np.all(got_len[length == 0] == 0.0)


@pytest.mark.parametrize("N", [255, 256, 257, 65537])
def test_chunk_boundaries_in_the_triangles_and_the_vertices(N):
    v, t, a = sr.soup(1000, N, seed=N, K=1)
    _check("T at a boundary", v, t, *sr.finite_box(v), 7, attrs=a)
    v, t, a = sr.soup(N, 3000, seed=N + 1, K=1)
    _check("V at a boundary", v, t, *sr.finite_box(v), 7, attrs=a)


@pytest.mark.parametrize("G", [7, 41, 129])
def test_chunk_boundaries_in_the_cells(G):
    v, t, a = sr.soup(4000, 9000, seed=G, K=2)
    got, _ = _check("cells at a boundary", v, t, *sr.finite_box(v), G, attrs=a)
    assert got["totals"][0] > 256


def test_two_chunks_of_the_one_workgroup_scan_over_the_triangles():
    v, t, _ = sr.soup(5000, (1 << 21) + 257, seed=21)
    got, _ = _check("T = 2^21 + 257", v, t, *sr.finite_box(v), 5)
    assert got["totals"][1] > (1 << 20)


def test_the_largest_table():
    v = np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 1], [1, 1, 1 - 2.0 ** -12], [np.nan, 0, 0], [0.5, 0.5, 0.5]])
    t = np.int32([[0, 1, 2], [1, 2, 3], [4, 5, 3], [4, 4, 0], [6, 0, 1], [2, 3, 4]])
    got, _ = _check("G = 512", v, t, np.zeros(3, np.float32), np.ones(3, np.float32), 512, attrs=v[:, :2].copy())
    assert got["totals"] == (5, 3)  # vertices 4 and 5 share the last cell; vertex 7 is in a cell no triangle touches
    assert got["vertex_map"].tolist() == [0, 3, 2, 1, 4, 4, -1, -1]  # ascending linear index: x slowest, z fastest


def test_contention_in_eight_cells():
    """2^17 vertices in a 2^3 grid: about 16 384 members per cell and 64-bit atomics from every wave into the same eight rows.  The
    sums are integers: bits equal to the restatement's, and equal again on a second call."""
    rng = np.random.default_rng(17)
    N = 1 << 17
    v = rng.uniform(-1.0, 1.0, (N, 3)).astype(np.float32)
    a = rng.uniform(-1.0, 1.0, (N, 3)).astype(np.float32)
    t = rng.integers(0, N, (1000, 3)).astype(np.int32)
    lo, hi = np.float32([-1, -1, -1]), np.float32([1, 1, 1])
    first, ref = _check("contention", v, t, lo, hi, 2, attrs=a)
    assert first["totals"][0] == 8 and int(ref["n"].sum()) == N
    second = _kernels(v, t, lo, hi, 2, attrs=a)
    for key in ("vertices", "attrs", "triangles", "vertex_map"):
        assert torch.equal(first[key], second[key]), key
    # the sums themselves, against Python integers, through the outputs they determine
    _, q, _, _ = sr.quantise(v, lo, hi)
    for i in range(8):
        members = ref["vertex_map"] == i
        S = sum(int(x) for x in q[members, 0])
        assert first["vertices"][i, 0].item() == float(np.float32(-1.0 + (float(S) / float(int(members.sum()))) * (2.0 * 2.0 ** -30)))


def test_empty_inputs():
    lo, hi = np.zeros(3, np.float32), np.ones(3, np.float32)
    none_v, none_t = np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)
    v, t, a = sr.soup(100, 50, seed=2, dirty=False, K=3)
    for label, vv, tt, aa in (("V = 0, T = 0", none_v, none_t, None), ("V = 0, T > 0", none_v, t, None), ("T = 0", v, none_t, a),
                              ("all triangles invalid", v, np.full((50, 3), 100, np.int32), a),
                              ("all triangles in one cell", v, np.zeros((50, 3), np.int32), a)):
        got, _ = _check(label, vv, tt, lo, hi, 4, attrs=aa)
        assert got["totals"] == (0, 0) and bool((got["vertex_map"] == -1).all())
    from pvd.mesh import simplify_mesh
    m = simplify_mesh(torch.zeros(0, 3, device=DEV), torch.zeros(0, 3, dtype=torch.int32, device=DEV), 4)
    assert m["vertices"].shape == (0, 3) and m["triangles"].shape == (0, 3) and m["vertex_map"].shape == (0,)
    assert m["normals"] is None and m["colors"] is None


def test_simplify_mesh_stays_within_the_cell_diagonal_of_the_original():
    """extract_mesh of an analytic sphere (R = 33), simplify_mesh at G = 8 over the extraction box.  Every original vertex is mapped
    (tests/test_mesh_simplify_restatement.py shows it on the CPU; asserted here again), so every vertex of either mesh has a vertex
    of the other within the per-axis bound of the header on every axis: the Hausdorff distance over the vertices is at most the
    length of the bound vector -- the cell diagonal plus the header's slack -- and it is not 0."""
    from pvd.mesh import compare_meshes, extract_mesh, simplify_mesh
    R, G = 33, 8
    lo, hi = np.full(3, -1.0, np.float32), np.full(3, 1.0, np.float32)
    verts, tris, normals = extract_mesh(_dev(mr.sphere_field(R), np.float32), 0.0, lo, hi, with_normals=True)
    m = simplify_mesh(verts, tris, G, bmin=lo, bmax=hi, normals=normals)
    assert bool((m["vertex_map"] >= 0).all())
    ref = sr.simplify(verts.cpu().numpy(), tris.cpu().numpy(), lo, hi, G, attrs=normals.cpu().numpy())
    assert torch.equal(m["vertices"].cpu().view(torch.int32), torch.from_numpy(ref["vertices"]).view(torch.int32))
    assert torch.equal(m["triangles"].cpu(), torch.from_numpy(ref["triangles"]))
    limit = float(np.linalg.norm(sr.bound(lo, hi, G)))
    d = compare_meshes(verts, tris, m["vertices"], m["triangles"], tau=limit)
    print("R=%d G=%d: %d -> %d vertices, %d -> %d triangles; hausdorff %.6f, chamfer %.6f, limit %.6f (cell diagonal %.6f)"
          % (R, G, verts.shape[0], m["vertices"].shape[0], tris.shape[0], m["triangles"].shape[0], d["hausdorff"], d["chamfer"], limit,
             float(np.linalg.norm((hi - lo) / G))))
    assert d["saturated_a"] == 0 and d["saturated_b"] == 0
    assert 0.0 < d["hausdorff"] <= limit
    assert m["triangles"].shape[0] < tris.shape[0] // 4 and m["vertices"].shape[0] < verts.shape[0] // 4
    length = torch.linalg.norm(m["normals"], dim=1)
    assert bool(((length - 1.0).abs() <= 1e-6).all())  # a sphere: no cell's normals cancel
    radial = m["vertices"] / torch.linalg.norm(m["vertices"], dim=1, keepdim=True)
    assert float((m["normals"] * radial).sum(dim=1).min()) > 0.9


def test_extract_surface_with_and_without_simplify():
    from pvd.mesh import extract_surface
    from test_hip_mesh_normals import _AnalyticSphere
    R, G = 24, 8
    model = _AnalyticSphere()
    plain = extract_surface(model, resolution=R)
    zero = extract_surface(model, resolution=R, simplify=0)
    assert sorted(zero) == sorted(plain) == ["colors", "counts", "field", "normals", "threshold", "triangles", "vertices"]
    for key in ("vertices", "triangles", "normals", "colors", "field"):
        assert torch.equal(zero[key], plain[key]), key
    m = extract_surface(model, resolution=R, simplify=G)
    assert sorted(m) == ["colors", "counts", "field", "full_counts", "normals", "threshold", "triangles", "vertex_map", "vertices"]
    assert m["full_counts"] == (plain["vertices"].shape[0], plain["triangles"].shape[0])
    Vn, Tn = m["vertices"].shape[0], m["triangles"].shape[0]
    assert 0 < Vn < plain["vertices"].shape[0] and 0 < Tn < plain["triangles"].shape[0]
    assert m["vertex_map"].shape == (m["full_counts"][0],) and int(m["vertex_map"].max()) == Vn - 1
    assert m["normals"].shape == (Vn, 3) and m["colors"].shape == (Vn, 3) and torch.equal(m["field"], plain["field"])
    length = torch.linalg.norm(m["normals"], dim=1)
    assert bool((((length - 1.0).abs() <= 1e-6) | (length == 0)).all())
    assert float(m["colors"].min()) >= 0.0 and float(m["colors"].max()) <= 1.0
    assert int(m["triangles"].min()) >= 0 and int(m["triangles"].max()) < Vn
    ref = sr.simplify(plain["vertices"].cpu().numpy(), plain["triangles"].cpu().numpy(), model.aabb_infer[:3].cpu().numpy(),
                      model.aabb_infer[3:].cpu().numpy(), G,
                      attrs=torch.cat([plain["normals"], plain["colors"]], dim=1).cpu().numpy())
    assert torch.equal(m["vertices"].cpu().view(torch.int32), torch.from_numpy(ref["vertices"]).view(torch.int32))
    assert torch.equal(m["triangles"].cpu(), torch.from_numpy(ref["triangles"]))
    assert torch.equal(m["colors"].cpu(), torch.from_numpy(ref["attrs"][:, 3:]).clamp(0.0, 1.0))
    bare = extract_surface(model, resolution=R, normals=False, colors=False, simplify=G)
    assert bare["normals"] is None and bare["colors"] is None and torch.equal(bare["vertices"], m["vertices"])


def test_a_simplified_mesh_round_trips_through_ply(tmp_path):
    from pvd.mesh import read_ply, simplify_mesh, write_ply
    v, t, lo, hi = _sphere()
    a = sr.sphere_attrs(v, 6)
    m = simplify_mesh(_dev(v, np.float32), _dev(t, np.int32), 5, bmin=_dev(lo, np.float32), bmax=_dev(hi, np.float32),
                      normals=_dev(a[:, :3], np.float32), colors=_dev(a[:, 3:], np.float32))
    path = write_ply(os.path.join(str(tmp_path), "small.ply"), m["vertices"], m["triangles"], normals=m["normals"], colors=m["colors"])
    rv, rt, rn, rc = read_ply(path)
    assert torch.equal(rv, m["vertices"].cpu()) and torch.equal(rt, m["triangles"].cpu()) and torch.equal(rn, m["normals"].cpu())
    assert torch.equal(rc, torch.round(m["colors"].cpu() * 255.0) / 255.0)
