"""tests/mesh_shtex_restatement.py -- csrc/pvd_hip_mesh_shtex.h in numpy -- pinned without a GPU: the basis against the spherical
harmonics' definition in float64, the mirrored direction's three properties, the fit matrix of pvd.mesh.sh_fit_matrix, the exact
recovery of a function in the span on a planar mesh, and the batch independence of the projection."""
import numpy as np
import pytest
import torch

import mesh_shtex_restatement as sr
from pvd.mesh import exposure_directions, sh_basis, sh_fit_matrix

F32 = np.float32
EPS = 2.0 ** -24  # half an ulp of 1: the relative error of one float32 rounding


def _directions():
    rng = np.random.default_rng(5)
    d = rng.normal(size=(500, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    axes = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [0, 0, 0], [0.3, -1.7, 2.2], [3, 4, 12]], float)
    return np.concatenate([d, axes, exposure_directions(64).numpy()]).astype(F32)


# ------------------------------------------------------------------------------------------------ the basis
@pytest.mark.parametrize("L", [1, 2, 3, 4])
def test_the_basis_is_the_real_spherical_harmonics_within_8_ulps_of_the_largest_monomial(L):
    """The bound from the operation count of the header.  A polynomial there is at most two monomials A, B of one sign before their
    difference, so |A - B| <= max(|A|, |B|) =: M.  Every rounding (a product, a difference, a float32 literal) adds at most 2^-24 of
    the quantity it rounds.  The worst cases are Y_9 = c (y (3 xx - yy)) and Y_15: on A's way xx and 3 xx (2), on B's yy (1), and on
    the way of the difference the difference itself, the product with y, the product with c and the literal c (4 of at most M each):
    7 * 2^-24 M to first order.  Y_11 .. Y_14: 6; Y_6, Y_8: 5; single monomials at most 4.  ulp(M) > 2^-24 M, so 8 ulps of the
    largest monomial hold with the second-order terms included.  The float64 value is the harmonics' definition (Legendre), evaluated
    at the float32 direction as given -- unit or not."""
    d = _directions()
    Y = sr.basis(d, L)
    Y64, largest = sr.basis64_terms(d, L)
    bound = 8.0 * np.spacing(largest.astype(F32)).astype(np.float64)
    err = np.abs(Y.astype(np.float64) - Y64)
    print("L = %d: largest error %.2f ulps of the largest monomial" % (L, (err / np.spacing(largest.astype(F32))).max()))
    assert np.all(err <= bound)
    assert np.all(Y[len(d) - 64 - 3] == sr.basis(np.zeros((1, 3), F32), L))  # (0, 0, 0): Y_0, -0.315.. and zeros
    # the lower bands are a prefix of the higher ones, bit for bit
    assert sr.basis(d, 4)[:, :L * L].tobytes() == Y.tobytes()
    # pvd.mesh.sh_basis on a host tensor is the same operations
    assert sh_basis(torch.from_numpy(d), L).numpy().tobytes() == Y.tobytes()


def test_the_basis_is_orthonormal_by_quadrature():
    """(4 pi / N) sum_i Y_a(d_i) Y_b(d_i) over the 4096 Fibonacci directions is the identity to the accuracy of that quadrature, which
    the float64 harmonics give: their own Gram matrix misses the identity by q; the float32 basis may miss it by q plus the basis'
    rounding (8 ulps of values below 1.2, summed with weights that add up to 4 pi times 2 |Y| <= 2.4)."""
    d = exposure_directions(4096).numpy()
    Y = sr.basis(d, 4).astype(np.float64)
    Y64, _ = sr.basis64_terms(d, 4)
    w = 4.0 * np.pi / len(d)
    q = np.abs(w * Y64.T @ Y64 - np.eye(16)).max()
    print("quadrature error of the float64 harmonics: %.3g" % q)
    assert q < 5e-3  # the rule is good enough to tell an orthonormal basis from one that is not
    tol = q + 4.0 * np.pi * 2.4 * 8 * 2.0 ** -23 * 1.2
    assert np.abs(w * Y.T @ Y - np.eye(16)).max() <= tol
    assert np.abs(w * Y.T @ Y - w * Y64.T @ Y64).max() <= tol - q


# ------------------------------------------------------------------------------------------------ the mirrored direction
def test_the_mirrored_direction_never_looks_from_behind_and_keeps_its_length():
    """With exact arithmetic d . n = -|s| and |d| = |u|.  In float32: s and q carry 3 roundings each, r two more, every component of d
    two; collected, d . n <= (-s) + 17 * 2^-24 |u| |n| (asserted with 20), and |d|^2 - |u|^2 = 2 dr (r q - s) + ... stays below
    32 * 2^-24 |u|^2, so | |d| - |u| | <= 16 * 2^-24 |u|: eight ulps."""
    rng = np.random.default_rng(7)
    n = (rng.normal(size=(400, 3)) * np.exp(rng.uniform(-6, 6, size=(400, 1)))).astype(F32)  # unnormalised, over many magnitudes
    U = exposure_directions(64).numpy()
    d = sr.mirrored(n, U).astype(np.float64)  # [J,M,3]
    n64, U64 = n.astype(np.float64), U.astype(np.float64)
    ln, lu = np.linalg.norm(n64, axis=1), np.linalg.norm(U64, axis=1)
    dn = (d * n64[None]).sum(-1)
    assert np.all(dn <= 20 * EPS * lu[:, None] * ln[None, :])
    assert np.all(np.abs(np.linalg.norm(d, axis=2) - lu[:, None]) <= 16 * EPS * lu[:, None])
    s = U64 @ n64.T
    behind = s > 20 * EPS * lu[:, None] * ln[None, :]
    assert behind.any() and (~behind).any()
    assert np.all(dn[behind] < 0)
    front = s < -20 * EPS * lu[:, None] * ln[None, :]
    assert np.all(d[front] == np.broadcast_to(U64[:, None, :], d.shape)[front])  # a direction that sees the surface is kept


def test_tangent_null_and_nan_normals_keep_the_direction_as_bits():
    U = np.array([[0.6, 0.0, 0.8], [0.0, -1.0, 0.0], [-0.0, 0.28, -0.96]], F32)
    n = np.array([[0.0, 5.0, 0.0],        # tangent to U[0]: s == 0
                  [0.0, 0.0, 0.0],        # q == 0
                  [np.nan, 1.0, 0.0],     # a NaN normal (an unowned texel)
                  [np.inf, 0.0, 0.0],     # q is not finite
                  [1e-30, 0.0, 0.0],      # q underflows to 0
                  [3e19, 3e19, 3e19]], F32)  # q overflows
    d = sr.mirrored(n, U)
    keep = np.ones((3, 6), bool)
    keep[2, 0] = False  # U[2] . (0, 5, 0) = 1.4 > 0: mirrored; U[1] . (0, 5, 0) = -5 sees the surface and is kept as well
    want = np.broadcast_to(U[:, None, :], d.shape)
    assert d[keep].tobytes() == want[keep].tobytes()
    assert d[2, 0].tobytes() != U[2].tobytes() and d[2, 0, 1] < 0


# ------------------------------------------------------------------------------------------------ the fit matrix
@pytest.mark.parametrize("L", [1, 2, 3, 4])
def test_the_fit_matrix_inverts_the_basis(L):
    U = exposure_directions(64)
    P = sh_fit_matrix(U, L)
    assert P.dtype == torch.float32 and tuple(P.shape) == (L * L, 64)
    Y = sr.basis(U.numpy(), L).astype(np.float64)
    assert np.abs(P.numpy().astype(np.float64) @ Y - np.eye(L * L)).max() <= 1e-5
    assert P.numpy().tobytes() == sr.fit_matrix(U.numpy(), L).tobytes()


def test_the_fit_matrix_refuses_too_few_and_degenerate_directions():
    with pytest.raises(ValueError):
        sh_fit_matrix(exposure_directions(8), 3)  # D < K
    a = np.linspace(0.0, 2.0 * np.pi, 64, endpoint=False)
    ring = torch.from_numpy(np.stack([np.cos(a), np.sin(a), np.zeros(64)], 1).astype(F32))  # all in the plane z = 0
    with pytest.raises(ValueError):
        sh_fit_matrix(ring, 2)  # Y_2 = c z vanishes on the whole set
    with pytest.raises(ValueError):
        sh_fit_matrix(ring, 5)  # more bands than the header has
    assert tuple(sh_fit_matrix(exposure_directions(9), 3).shape) == (9, 9)  # D == K is enough where the set is not degenerate


# ------------------------------------------------------------------------------------------------ exact recovery, batch independence
@pytest.fixture(scope="module")
def plane():
    """The planar case baked on the host at L = 3, S = 8, D = 64: the texture, P, the colours the source returned and the float64 fit."""
    U = exposure_directions(64).numpy()
    seen = []

    def source(x, d):
        seen.append(np.array(d))
        return sr.plane_colour(d).astype(F32)
    tex = sr.bake(source, sr.PLANE_V, sr.PLANE_T, 8, 3, U, batch=8)
    P = sr.fit_matrix(U, 3)
    rgb = sr.plane_colour(np.stack([s[0] for s in seen]))  # [D,3]: every texel asks for the same d_j
    fit64 = np.linalg.pinv(sr.basis(U, 3).astype(np.float64)) @ rgb
    return dict(U=U, tex=tex, P=P, rgb=rgb, fit64=fit64, seen=seen)


def test_the_restated_bake_recovers_a_function_in_the_span(plane):
    tex, P, rgb, fit64 = plane["tex"], plane["P"], plane["rgb"], plane["fit64"]
    # no colour is taken from behind the plane, and every texel asked for the same 64 directions
    assert all(np.all(s[:, 2] <= 0) and np.all(s == s[0]) for s in plane["seen"]) and len(plane["seen"]) == 64
    f, p, q = sr.mt.owners(2, 8)
    owned = f < 2
    assert np.all(tex[~owned] == 0)
    coef = tex[owned]  # [n,9,3]
    assert np.all(coef == coef[0])  # one plane, one normal: one set of coefficients
    bound = sr.fit_bound(P, rgb.astype(F32), 64)
    err = np.abs(coef[0].astype(np.float64) - fit64)
    print("largest coefficient error over its bound: %.3f" % (err / bound).max())
    assert np.all(err <= bound)
    # the float64 fit is the function's own expansion: a + b / 3 on Y_0, b on Y_6, c on Y_3, nothing elsewhere
    want = np.zeros((9, 3))
    want[0] = (sr.PLANE_A + sr.PLANE_B / 3.0) / 0.28209479177387814
    want[6] = sr.PLANE_B / 0.9461746957575601
    want[3] = sr.PLANE_C / -0.4886025119029199
    assert np.abs(fit64 - want).max() < 1e-5


def test_the_restated_sample_returns_the_function_at_interior_hits(plane):
    tex, P, rgb = plane["tex"], plane["P"], plane["rgb"]
    rng = np.random.default_rng(11)
    N = 300
    tri = rng.integers(0, 2, N).astype(np.int32)
    b = rng.uniform(0.02, 0.96, (N, 2))
    bary = np.where((b.sum(1) > 0.98)[:, None], 0.49 * b, b).astype(F32)  # strictly inside
    dirs = rng.normal(size=(N, 3))
    dirs[:, 2] = -np.abs(dirs[:, 2]) - 0.05  # a ray that sees the plane travels downwards
    dirs = (dirs / np.linalg.norm(dirs, axis=1, keepdims=True)).astype(F32)
    out = sr.sample(tex, 2, 8, 3, tri, bary, dirs, (1.0, 1.0, 1.0))
    coef = tex[0, 0]
    bound = sr.sample_bound(sr.fit_bound(P, rgb.astype(F32), 64), coef, sr.basis(dirs, 3))
    err = np.abs(out.astype(np.float64) - sr.plane_colour(dirs))
    print("largest sample error over its bound: %.3f" % (err / bound).max())
    assert np.all(err <= bound)


@pytest.mark.parametrize("L", [1, 2, 3, 4])
def test_the_projection_does_not_depend_on_the_batch_split(L):
    rng = np.random.default_rng(13)
    D, M = 64, 37
    rgb = rng.uniform(0, 1, (D, M, 3)).astype(F32)
    P = sr.fit_matrix(exposure_directions(D).numpy(), L)
    whole = sr.project_batched(rgb, P, D)
    assert whole.dtype == F32 and whole.shape == (M, L * L, 3)
    for batch in (1, 3):
        assert sr.project_batched(rgb, P, batch).tobytes() == whole.tobytes()
    # and it is the sum in the header's order, from +0
    acc = np.zeros((M, L * L, 3), F32)
    for j in range(D):
        acc = acc + (P[:, j][None, :, None] * rgb[j][:, None, :]).astype(F32)
    assert acc.tobytes() == whole.tobytes()
    assert np.abs(whole.astype(np.float64) - np.einsum("kj,jmc->mkc", P.astype(np.float64), rgb.astype(np.float64))).max() < 1e-5
