"""tests/mesh_simplify_restatement.py -- the numpy restatement of include/pvd_hip_mesh_simplify.h that the GPU tests compare bits
with -- pinned on its own first, without a GPU: the displacement bound of the header, order and orientation of the survivors, index
ranges, the degenerate grids, exact sums in a crowded cell, and that the sphere inputs of the GPU tests leave no vertex unmapped."""
import numpy as np
import pytest

import mesh_simplify_restatement as sr


@pytest.fixture(scope="module")
def sphere():
    return sr.sphere_mesh(12)


def _check_bound(v, vmap, out, lo, hi, G):
    b = sr.bound(lo, hi, G)
    lo64, hi64 = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    m = vmap >= 0
    d = np.abs(v[m].astype(np.float64) - out[vmap[m]].astype(np.float64))
    inside = (v[m] >= lo64) & (v[m] <= hi64) & (b > 0)
    worst = np.where(inside, d - b, -np.inf).max(axis=0) if m.any() else np.full(3, -np.inf)
    print("G=%d: largest (displacement - bound) per axis %s, bound %s" % (G, worst, b))
    assert np.all(d[inside] <= np.broadcast_to(b, d.shape)[inside])
    return int(inside.sum())


def test_the_bound_is_read_from_the_header():
    assert sr.header_bound_terms() == (2.0 ** -30, 2.0 ** -23)
    b = sr.bound([-1, 0, 2], [1, 4, 2], 4)
    assert b[0] == 0.5 + 2.0 ** -29 + 2.0 ** -23 and b[1] == 1.0 + 2.0 ** -28 + 2.0 ** -21 and b[2] == 0.0


@pytest.mark.parametrize("G", [1, 2, 3, 5, 6, 8, 16, 64])
def test_the_displacement_bound_holds_per_axis_on_the_sphere(sphere, G):
    v, t, lo, hi = sphere
    r = sr.simplify(v, t, lo, hi, G)
    checked = _check_bound(v, r["vertex_map"], r["vertices"], lo, hi, G)
    assert checked > 0 or G == 1
    # the mean of a cell's members never leaves the cell: the new vertex quantises into the cell it stands for
    if len(r["vertices"]):
        _, q, _, _ = sr.quantise(v, lo, hi)
        cell_of_new = np.full(len(r["vertices"]), -1, np.int64)
        cell_of_new[r["vertex_map"][r["vertex_map"] >= 0]] = sr.cells(q, G)[r["vertex_map"] >= 0]
        mean_q = r["S"] // r["n"][:, None]  # floor of the exact mean: in the members' interval
        assert np.array_equal(sr.cells(mean_q, G), cell_of_new)


@pytest.mark.parametrize("seed", [0, 1])
def test_the_displacement_bound_holds_on_random_soups(seed):
    v, t, _ = sr.soup(seed=seed)
    for lo, hi in (sr.finite_box(v), (np.float32([-1, -1, -1]), np.float32([1, 1, 1])), (np.float32([-1, 0.5, -1]), np.float32([1, 0.5, 3]))):
        for G in (2, 7, 41):
            r = sr.simplify(v, t, lo, hi, G)
            assert _check_bound(v, r["vertex_map"], r["vertices"], lo, hi, G) > 0


def test_survivors_keep_their_order_and_orientation(sphere):
    v, t, lo, hi = sphere
    r = sr.simplify(v, t, lo, hi, 6)
    s = r["survives"]
    assert 0 < s.sum() < len(t)
    assert np.array_equal(r["triangles"], r["vertex_map"][t[s]])  # input order, corner order
    assert (r["triangles"] >= 0).all()

    def outward(verts, tris):
        p = verts.astype(np.float64)[tris]
        n = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
        return np.einsum("ij,ij->i", n, p.mean(axis=1))
    before, after = outward(v, t[s]), outward(r["vertices"], r["triangles"])
    assert (before > 0).all()  # the extraction winds outwards; the sphere is centred
    assert (after > 0).all(), "%d of %d surviving triangles turned" % ((after <= 0).sum(), len(after))


@pytest.mark.parametrize("G", [2, 3, 5, 8])
def test_indices_are_in_range_and_every_new_vertex_is_referenced(sphere, G):
    v, t, lo, hi = sphere
    for verts, tris in ((v, t), sr.soup(seed=3)[:2]):
        r = sr.simplify(verts, tris, lo, hi, G)
        Vn = len(r["vertices"])
        assert Vn > 0 and r["triangles"].min() >= 0 and r["triangles"].max() < Vn
        assert np.array_equal(np.unique(r["triangles"]), np.arange(Vn))
        assert r["vertex_map"].max() == Vn - 1 and (r["n"] >= 1).all()
        for row in r["triangles"]:
            assert len(set(row)) == 3


def test_one_cell_keeps_nothing(sphere):
    v, t, lo, hi = sphere
    r = sr.simplify(v, t, lo, hi, 1, attrs=sr.sphere_attrs(v, 3))
    assert r["vertices"].shape == (0, 3) and r["triangles"].shape == (0, 3) and r["attrs"].shape == (0, 3)
    assert r["vertex_map"].shape == (len(v),) and (r["vertex_map"] == -1).all()


def test_the_sums_of_a_crowded_cell_are_exact():
    """2^17 members in one cell of a G = 2 grid, next to the three single vertices that make its triangle survive: n, S and A against
    Python integers, and the outputs against the same expressions on those integers."""
    rng = np.random.default_rng(5)
    N = 1 << 17
    v = np.concatenate([rng.uniform(0.0, 1.0, (N, 3)), [[-0.5, 0.5, 0.5], [0.5, -0.5, 0.5]]]).astype(np.float32)
    a = rng.uniform(-1.0, 1.0, (N + 2, 2)).astype(np.float32)
    t = np.array([[0, N, N + 1]], np.int32)
    lo, hi = np.float32([-1, -1, -1]), np.float32([1, 1, 1])
    r = sr.simplify(v, t, lo, hi, 2, attrs=a)
    big = int(r["vertex_map"][0])
    assert (r["vertex_map"][:N] == big).all() and int(r["n"][big]) == N and len(r["n"]) == 3
    _, q, _, _ = sr.quantise(v, lo, hi)
    qa = sr.quantise_attrs(a)
    for axis in range(3):
        S = sum(int(x) for x in q[:N, axis])
        assert int(r["S"][big, axis]) == S
        assert r["vertices"][big, axis] == np.float32(-1.0 + (float(S) / float(N)) * (2.0 * 2.0 ** -30))
    for j in range(2):
        A = sum(int(x) for x in qa[:N, j])
        assert int(r["A"][big, j]) == A and r["attrs"][big, j] == np.float32((float(A) / float(N)) * 2.0 ** -30)


def test_dirty_rows_are_left_out():
    v, t, a = sr.soup(K=4)
    lo, hi = sr.finite_box(v)
    r = sr.simplify(v, t, lo, hi, 5, attrs=a)
    assert (r["vertex_map"][[3, 5, 7, 9]] == -1).all()
    assert not r["survives"][[0, 1, 2, 4, 6, 8]].any()
    assert np.isfinite(r["vertices"]).all() and np.isfinite(r["attrs"]).all() and np.abs(r["attrs"]).max() <= 1.0
    # a flat axis: every new vertex sits on bmin there
    flat = sr.simplify(v, t, np.float32([-1, 0.25, -1]), np.float32([1, 0.25, 1]), 5)
    assert len(flat["vertices"]) and (flat["vertices"][:, 1] == np.float32(0.25)).all()
    # outside a given box: projected onto it, so inside it afterwards
    small = sr.simplify(v, t, np.float32([-0.5, -0.5, -0.5]), np.float32([0.5, 0.5, 0.5]), 5)
    assert np.abs(small["vertices"]).max() <= 0.5


@pytest.mark.parametrize("R,G", [(12, 2), (12, 3), (12, 5), (12, 8), (33, 8)])
def test_the_spheres_of_the_gpu_tests_leave_no_vertex_unmapped(R, G):
    """The GPU Hausdorff check measures all vertices of the original against the simplified mesh; that is covered by the displacement
    bound only when every vertex is mapped.  Condition: 0 unmapped."""
    v, t, lo, hi = sr.sphere_mesh(R)
    r = sr.simplify(v, t, lo, hi, G)
    unmapped = int((r["vertex_map"] < 0).sum())
    print("R=%d G=%d: V=%d T=%d -> V'=%d T'=%d, unmapped %d" % (R, G, len(v), len(t), len(r["vertices"]), len(r["triangles"]), unmapped))
    assert unmapped == 0
