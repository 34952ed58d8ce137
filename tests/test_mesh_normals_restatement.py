"""tests/mesh_normals_restatement.py -- the numpy restatement of include/pvd_hip_mesh_attr.h that tests/test_hip_mesh_normals.py
compares pvd_mesh_normals with -- is pinned here on fields whose normals are known: radial on the sphere, agreeing with the outward
face normals the winding of include/pvd_hip_mesh.h gives, (-1,0,0) on the plane, zero exactly where a NaN is touched; and its float32
evaluation stays inside the error bound the GPU test uses.  No GPU, no library."""
import numpy as np
import pytest

import mesh_normals_restatement as nr
import mesh_restatement as mr

BOX = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
THRESH = 0.125
BMIN, BMAX = (-1.0, -0.5, 0.25), (1.0, 1.5, 2.0)  # the non-cubic box of the GPU tests
KINDS = ("sphere", "torus", "two_spheres", "smooth", "plane", "nan")
SIZES = (2, 3, 9, 17, 33)


@pytest.fixture(scope="module")
def sphere():
    u = mr.sphere_field(33)
    owners, slots, tris = mr.topology(u, 0.0)
    verts = mr.positions(u, 0.0, owners, slots, *BOX, np.float64)[0]
    n, S, length = nr.normals(u, 0.0, *BOX, np.float64)
    return dict(u=u, verts=verts, tris=tris, n=n, S=S, length=length)


def test_the_normals_of_a_sphere_are_radial_and_of_unit_length(sphere):
    v, n = sphere["verts"], sphere["n"]
    assert n.shape == v.shape and len(v) > 1000
    assert np.abs(np.linalg.norm(n, axis=1) - 1.0).max() < 1e-12
    dots = (n * v / np.linalg.norm(v, axis=1, keepdims=True)).sum(axis=1)
    print("sphere R=33: smallest n . x/|x| = %.6f over %d vertices" % (dots.min(), len(v)))
    assert dots.min() >= 0.9999


def test_the_normals_agree_with_the_outward_face_normals(sphere):
    """Ties the sign of the normals to the winding pvd_hip_mesh.h promises (a closed component has positive signed volume)."""
    v, tris, n = sphere["verts"], sphere["tris"].astype(np.int64), sphere["n"]
    assert mr.signed_volume(v, tris) > 0
    face = np.cross(v[tris[:, 1]] - v[tris[:, 0]], v[tris[:, 2]] - v[tris[:, 0]])
    area2 = np.linalg.norm(face, axis=1)
    keep = area2 > 1e-12  # a triangle of two coinciding vertices has no normal
    assert keep.sum() > 0.9 * len(tris)
    face = face[keep] / area2[keep, None]
    dots = np.einsum("tcj,tj->tc", n[tris[keep]], face)
    print("sphere R=33: smallest vertex normal . face normal = %.4f over %d triangles" % (dots.min(), keep.sum()))
    assert dots.min() >= 0.99


@pytest.mark.parametrize("R", SIZES)
def test_the_normals_of_the_plane_point_down_the_x_axis(R):
    u = nr.field("plane", R, THRESH)
    for dtype in (np.float32, np.float64):
        n, S, length = nr.normals(u, THRESH, BMIN, BMAX, dtype)
        assert len(n) > 0
        n64, S64, len64 = nr.normals(u, THRESH, BMIN, BMAX, np.float64)
        assert np.all(np.abs(n - np.array([-1.0, 0.0, 0.0])) <= nr.bound(S64, len64))
        assert np.all(n[:, 1:] == 0)


def _touches_nan(u, thresh):
    """Per vertex: a NaN among the values the definition reads -- the two endpoints (t) and both gradient stencils."""
    R = u.shape[0]
    bad = np.isnan(u)
    stencil = np.zeros_like(bad)
    for a in range(3):
        b = np.moveaxis(bad, a, 0)
        s = np.zeros_like(b)
        s[0] = b[0] | b[1]
        s[R - 1] = b[R - 1] | b[R - 2]
        if R > 2:
            s[1:R - 1] = b[2:] | b[:R - 2]
        stencil |= np.moveaxis(s, 0, a)
    owners, slots, _ = mr.topology(u, thresh)
    d = np.asarray(mr.SLOTS, np.int64)[slots].reshape(-1, 3)
    p = np.stack([owners // (R * R), (owners // R) % R, owners % R], axis=1)
    other = (p + d) @ np.array([R * R, R, 1])
    hit = (bad | stencil).reshape(-1)
    return hit[owners] | hit[other]


@pytest.mark.parametrize("R", (9, 17, 33))
def test_the_zero_rows_are_the_rows_that_touch_a_nan(R):
    u = nr.field("nan", R, THRESH)
    hit = _touches_nan(u, THRESH)
    assert hit.any() and not hit.all()
    for dtype in (np.float32, np.float64):
        n, _, length = nr.normals(u, THRESH, BMIN, BMAX, dtype)
        zero = np.all(n == 0, axis=1)
        assert np.array_equal(zero, hit)
        assert np.all(np.isfinite(n)) and np.all(np.abs(np.linalg.norm(n[~zero].astype(np.float64), axis=1) - 1.0) < 1e-6)


def test_the_one_sided_and_the_mixed_paths_run():
    """R = 2: every difference is one-sided, so the gradient is that of the trilinear cell; R = 3: the middle index is central."""
    u = np.arange(8, dtype=np.float32).reshape(2, 2, 2)  # u = 4 i + 2 j + k
    inv_h = np.array([1.0, 1.0, 1.0])
    assert np.array_equal(nr.lattice_gradient(u, inv_h, np.float64), np.broadcast_to([4.0, 2.0, 1.0], (2, 2, 2, 3)))
    n, S, length = nr.normals(u, 3.5, (0, 0, 0), (1, 1, 1), np.float64)
    assert len(n) > 0 and np.allclose(n, -np.array([4.0, 2.0, 1.0]) / np.sqrt(21.0)) and np.allclose(length, np.sqrt(21.0))
    i = np.arange(3, dtype=np.float32)
    u = np.broadcast_to((i * i)[:, None, None], (3, 3, 3)).copy()  # 0 1 4 along x: differences 1 (one-sided), 2 (central), 3 (one-sided)
    g = nr.lattice_gradient(u, inv_h, np.float64)
    assert np.array_equal(g[:, 0, 0, 0], [1.0, 2.0, 3.0]) and np.all(g[..., 1:] == 0)
    for kind in KINDS:
        for R in (2, 3):
            n, _, _ = nr.normals(nr.field(kind, R, THRESH), THRESH, BMIN, BMAX, np.float32)
            assert n.dtype == np.float32 and n.shape[1] == 3


def test_a_non_cubic_box_tilts_the_normal():
    u = np.arange(8, dtype=np.float32).reshape(2, 2, 2)
    n, _, _ = nr.normals(u, 3.5, (0, 0, 0), (1, 2, 4), np.float64)  # inv_h = 1, 1/2, 1/4
    assert np.allclose(n, -np.array([4.0, 1.0, 0.25]) / np.sqrt(17.0625))


@pytest.mark.parametrize("R", SIZES)
@pytest.mark.parametrize("kind", KINDS + ("far_spheres",))
def test_float32_stays_inside_the_bound_of_the_gpu_test(kind, R):
    """The bound is derived (tests/test_hip_mesh_normals.py); numpy's float32 evaluation of the same chain uses a small part of it,
    and it stays a small number for every vertex of the fields the GPU test runs."""
    u = nr.field(kind, R, THRESH)
    n64, S, length = nr.normals(u, THRESH, BMIN, BMAX, np.float64)
    n32, _, _ = nr.normals(u, THRESH, BMIN, BMAX, np.float32)
    assert n32.dtype == np.float32 and n32.shape == n64.shape
    zero = np.all(n64 == 0, axis=1)
    assert np.array_equal(zero, np.all(n32 == 0, axis=1))
    if kind != "nan":
        assert not zero.any()
    if (~zero).any():
        b = nr.bound(S, length)[~zero]
        err = np.abs(n32[~zero].astype(np.float64) - n64[~zero])
        print("%s R=%d: V=%d, largest bound %.3g, largest error / bound %.4f" % (kind, R, len(n64), b.max(), (err / b).max()))
        assert np.all(err <= b)
        # the bound grows where the two endpoint gradients cancel (len small against S); on these fields it never gets vacuous:
        # against components of a unit vector it is at most 7.3e-6 on the five finite fields, 7.7e-6 on far_spheres (R = 9) and
        # 2.3e-5 on the field with NaNs (R = 3)
        assert b.max() < 1e-4
