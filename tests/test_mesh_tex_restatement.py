"""tests/mesh_tex_restatement.py pinned against what include/pvd_hip_mesh_tex.h promises of the atlas: one owner per texel, the texel counts
of a lower and an upper half, corners that come back bit for bit, texture coordinates on texel centres, a bilinear lookup that stays
with its triangle, and a baked-then-sampled linear function that comes back within a derived bound.  No GPU."""
import numpy as np
import pytest

import mesh_dist_restatement as md
import mesh_tex_restatement as tr

F32 = np.float32
SIZES = tuple(range(4, 10))
COUNTS = (0, 1, 2, 7, 50)


@pytest.mark.parametrize("S", SIZES)
@pytest.mark.parametrize("T", COUNTS)
def test_every_texel_of_a_used_cell_has_one_owner_and_the_halves_have_their_counts(T, S):
    C, rows, Wt, Ht = tr.layout(T, S)
    cells = (T + 1) // 2
    assert C >= 1 and C * C >= cells and (C == 1 or (C - 1) * (C - 1) < cells)
    assert rows == max(1, -(-cells // C)) and (Wt, Ht) == (C * S, rows * S)
    f, p, q = tr.owners(T, S)
    assert f.shape == (Ht, Wt)
    # f is a function of the texel: every texel has exactly one candidate; it is an owner iff f < T
    y, x = np.meshgrid(np.arange(Ht), np.arange(Wt), indexing="ij")
    k = (y // S) * C + x // S
    assert np.all((f == 2 * k) | (f == 2 * k + 1)) and np.all((p >= 0) & (p < S) & (q >= 0) & (q < S))
    used = k < cells
    full = 2 * k + 1 < T  # cells both of whose halves are owned
    assert np.all(f[used & full] < T) and np.all(f[~used] >= T)
    count = np.bincount(f.reshape(-1), minlength=max(T, 1))
    for t in range(T):
        assert count[t] == (S * (S + 1) // 2 if t % 2 == 0 else S * (S - 1) // 2), (t, count[t])
        # (p, q) is one-to-one inside a triangle
        own = f == t
        assert len(set(zip(p[own].tolist(), q[own].tolist()))) == count[t]
        assert np.all(p[own] + q[own] <= (S - 1 if t % 2 == 0 else S - 2))
    if T == 0:
        assert (C, rows) == (1, 1) and np.all(f >= T)


def test_the_layout_refuses_what_the_header_refuses():
    for T, S in ((5, 3), (5, 65), (5, 0), (2 * 4096 * 4096 + 1, 4), (2 * 256 * 256 + 1, 64)):
        with pytest.raises(ValueError):
            tr.layout(T, S)
    assert tr.layout(2 * 4096 * 4096, 4) == (4096, 4096, 16384, 16384) and tr.layout(2 * 256 * 256, 64) == (256, 256, 16384, 16384)
    assert tr.layout(3, 4) == (2, 1, 8, 4)  # two cells in one row: rows is not C


@pytest.mark.parametrize("S", (4, 5, 8, 9))
@pytest.mark.parametrize("with_normals", (False, True))
def test_the_texel_at_a_corner_returns_the_corner_bit_for_bit(S, with_normals):
    v, t = md.fixture("sphere", 9)
    assert not np.any(np.signbit(v) & (v == 0))  # no -0: 1 * A + 0 * B + 0 * C is A bit for bit
    T = len(t)
    rng = np.random.RandomState(S)
    nrm = rng.randn(len(v), 3).astype(F32) if with_normals else None
    _, _, Wt, Ht = tr.layout(T, S)
    x, n = tr.points(v, t, S, nrm)
    x, n = x.reshape(Ht, Wt, 3), n.reshape(Ht, Wt, 3)
    ct = tr.corner_texels(T, S)  # [T,3,2]
    f, p, q = tr.owners(T, S)
    m = S - 3
    for c, (pc, qc) in enumerate(((0, 0), (m, 0), (0, m))):
        xs, ys = ct[:, c, 0], ct[:, c, 1]
        assert np.array_equal(f[ys, xs], np.arange(T)) and np.all(p[ys, xs] == pc) and np.all(q[ys, xs] == qc)
        assert np.array_equal(x[ys, xs].view(np.uint32), v[t[:, c]].view(np.uint32))
        if with_normals:
            got, want = n[ys, xs], nrm[t[:, c]]
            assert np.array_equal(got, want)  # (-0 + 0 is +0: values, not bits)
    if not with_normals:  # one face normal per triangle
        own = f < T
        a, b, c = (v[t[:, e]] for e in range(3))
        u, w = b - a, c - a
        face = np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2], u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], 1)
        assert np.array_equal(n[own].view(np.uint32), face[f[own]].view(np.uint32))
    assert np.all(np.isnan(x[f >= T])) and np.all(np.isnan(n[f >= T])) and np.all(np.isfinite(x[f < T]))


def test_invalid_triangles_and_bands():
    v, t = (np.array(a) for a in md.fixture("sphere", 9))
    t = t[:41].copy()
    nrm = np.random.RandomState(0).randn(len(v), 3).astype(F32)
    t[3, 1] = len(v)
    t[4, 0] = -1
    v[t[10, 2], 1] = np.nan
    nrm[t[20, 0], 2] = np.inf
    S = 5
    _, _, Wt, Ht = tr.layout(len(t), S)
    f = tr.owners(len(t), S)[0].reshape(-1)
    for normals in (None, nrm):
        ok = tr.valid(v, t, normals)
        assert not ok[3] and not ok[4] and not ok[10] and ok[20] == (normals is None) and ok[0]
        x, n = tr.points(v, t, S, normals)
        bad = (f >= len(t)) | ~ok[np.minimum(f, len(t) - 1)]
        assert np.array_equal(np.isnan(x).all(1), bad) and np.array_equal(np.isnan(n).all(1), bad)
        assert np.array_equal(np.isnan(x).any(1), bad)
        for r0, r1 in ((0, Ht), (3, 4), (S - 2, S + 2), (7, 7)):
            xb, nb = tr.points(v, t, S, normals, r0, r1)
            assert xb.shape == ((r1 - r0) * Wt, 3)
            np.testing.assert_array_equal(xb, x[r0 * Wt:r1 * Wt])
            np.testing.assert_array_equal(nb, n[r0 * Wt:r1 * Wt])


@pytest.mark.parametrize("S", SIZES)
@pytest.mark.parametrize("T", COUNTS)
def test_texture_uv_corners_land_on_texel_centres(T, S, hip_lib_built):
    from pvd.mesh import texture_uv
    C, rows, Wt, Ht = tr.layout(T, S)
    uv = texture_uv(T, S).numpy().astype(np.float64)
    assert uv.shape == (T, 3, 2)
    if T == 0:
        return
    # back to continuous texel units: the float32 of a uv moves a coordinate by at most 2^-24 of the side, far below half a texel
    X, Y = uv[..., 0] * Wt, (1.0 - uv[..., 1]) * Ht
    want = tr.corner_coordinates(T, S)
    assert np.abs(X - want[..., 0]).max() <= Wt * 2.0 ** -23 and np.abs(Y - want[..., 1]).max() <= Ht * 2.0 ** -23
    np.testing.assert_allclose(uv, tr.uv(T, S), rtol=0, atol=2.0 ** -23)
    ct = tr.corner_texels(T, S)
    assert np.array_equal(np.floor(X).astype(np.int64), ct[..., 0]) and np.array_equal(np.floor(Y).astype(np.int64), ct[..., 1])
    f = tr.owners(T, S)[0]
    assert np.array_equal(f[ct[..., 1], ct[..., 0]], np.repeat(np.arange(T)[:, None], 3, 1))
    m = S - 3
    assert np.array_equal(np.abs(ct[:, 1, 0] - ct[:, 0, 0]), np.full(T, m)) and np.array_equal(np.abs(ct[:, 2, 1] - ct[:, 0, 1]), np.full(T, m))


@pytest.mark.parametrize("S", SIZES)
@pytest.mark.parametrize("T", COUNTS)
def test_on_a_barycentric_lattice_the_lookup_stays_with_its_triangle(T, S):
    """Lattice of step 1 / (4 m) over every triangle, closed edges and corners included.  Every texel the lookup reads lies in the
    triangle's own cell.  Every texel it reads WITH A WEIGHT THAT IS NOT ZERO is owned by the triangle, and for an even triangle (a lower
    half, the closed diagonal included) all four are.  The header names the one case left: at a lattice point of the hypotenuse where
    beta m and gamma m are both whole (the corners b and c among them) the fourth texel (i0 + 1, j0 + 1) lies on the cell's diagonal,
    p + q = S - 1, which the lower half owns; an odd triangle reads it there from its cell's even triangle, multiplied by tx = ty = 0.
    This test asserts that this is the only such read."""
    if T == 0:
        xs, ys, w, _ = tr.touched(0, S, np.array([0, -1, 5]), np.zeros((3, 2), F32))
        assert np.all(xs == -1) and np.all(w == 0)
        return
    m = S - 3
    a, b = np.meshgrid(np.arange(4 * m + 1), np.arange(4 * m + 1), indexing="ij")
    keep = a + b <= 4 * m
    a, b = a[keep], b[keep]
    bary = np.stack([a.astype(F32) / F32(4 * m), b.astype(F32) / F32(4 * m)], 1)
    C = tr.layout(T, S)[0]
    f, p, q = tr.owners(T, S)
    exceptions = 0
    for t in range(T):
        xs, ys, w, (tx, ty) = tr.touched(T, S, np.full(len(bary), t), bary)
        k = t // 2
        assert np.all(xs // S == k % C) and np.all(ys // S == k // C)  # the own cell
        own = f[ys, xs] == t
        assert np.all(own[w != 0])
        assert np.all((w >= 0) & (w <= 1)) and np.all(np.abs(w.sum(1) - 1) <= 4 * 2.0 ** -24)
        if t % 2 == 0:
            assert np.all(own)
        else:
            rows, cols = np.nonzero(~own)
            assert np.all(cols == 3)  # only c11
            assert np.all(tx[rows] == 0) and np.all(ty[rows] == 0) and np.all(a[rows] + b[rows] == 4 * m)
            assert np.all(p[ys[rows, 3], xs[rows, 3]] + q[ys[rows, 3], xs[rows, 3]] == S - 1) and np.all(f[ys[rows, 3], xs[rows, 3]] == t - 1)
            exceptions += len(rows)
    assert exceptions == (T // 2) * (m + 1)  # the m + 1 whole points of each odd triangle's hypotenuse


def test_whatever_bary_holds_the_lookup_stays_inside_the_cell():
    T, S = 7, 6
    C = tr.layout(T, S)[0]
    vals = np.array([0, 1, -1, 0.5, 2, -3, np.nan, np.inf, -np.inf, 1 + 2.0 ** -23, 1e30, -1e30, 1 / 3], F32)
    bary = np.stack(np.meshgrid(vals, vals, indexing="ij"), -1).reshape(-1, 2)
    for t in range(T):
        xs, ys, w, _ = tr.touched(T, S, np.full(len(bary), t), bary)
        assert np.all(xs // S == (t // 2) % C) and np.all(ys // S == (t // 2) // C) and np.all(np.isfinite(w))
    tex = np.random.RandomState(1).rand(*tr.layout(T, S)[3:1:-1], 3).astype(F32)
    out = tr.sample(tex, T, S, np.array([-1, T, 2 ** 31 - 1, 0]), np.zeros((4, 2), F32), (0.25, 0.5, 0.75))
    assert np.array_equal(out[:3], np.tile(np.array([0.25, 0.5, 0.75], F32), (3, 1)))
    assert np.array_equal(out[3], tex[0, 0])  # the corner a of triangle 0: the texel (0, 0)


@pytest.mark.parametrize("kind,R", (("sphere", 9), ("torus", 17)))
@pytest.mark.parametrize("S", (4, 5, 8, 16))
def test_baked_positions_come_back_through_the_lookup(kind, R, S):
    """The float32 positions themselves are the "colour".  Sampled at random interior bary they reproduce alpha A + beta B + gamma C
    (float64, alpha = 1 - beta - gamma, from the same float32 bary) within 81 * 2^-24 * M, M the largest |coordinate| of the triangle's
    corners.  With u = 2^-24, fu = beta m, fv = gamma m, and L(p, q) the exact plane A + (p / m)(B - A) + (q / m)(Cc - A):
      - the lookup reads texels with 0 <= p, q <= m + 1, extrapolated ones included: beta', gamma' <= (m + 1) / m <= 2 and
        -3 <= alpha' <= 1, so the weights' absolute values sum to at most 7 and |L| <= 7 M, as does every intermediate;
      - a texel: beta', gamma' carry one rounding each (<= 2 u), alpha' two more of numbers <= 3 plus theirs (<= 10 u): 14 u M through
        the weights; three products whose sizes sum to <= 7 M (7 u M) and two sums <= 7 M (14 u M): a texel is within 35 u M of L;
      - bilinear interpolation of a linear function is exact, and a mean of texel errors is no larger than the largest: 35 u M;
      - fu and fv carry one rounding each, <= u m, and L changes by |B - A| / m <= 2 M / m per texel: 4 u M; tx = fu - i0 is exact;
      - 1 - tx and 1 - ty carry one rounding (<= u), so a lerp's weights miss 1 by u: 7 u M for the x lerps, 7 u M for the y lerp;
      - each lerp rounds two products whose sizes sum to <= 7 M and one sum <= 7 M: 14 u M for the x lerps (a mean of two), 14 u M for
        the y lerp.
    35 + 4 + 14 + 28 = 81.  The float64 reference's own roundings (2^-53) are not counted.  Not tuned."""
    v, t = md.fixture(kind, R)
    T = len(t)
    _, _, Wt, Ht = tr.layout(T, S)
    tex = tr.points(v, t, S)[0].reshape(Ht, Wt, 3)
    tex = np.where(np.isnan(tex), F32(0), tex)
    rng = np.random.RandomState(R + S)
    N = 4000
    tri = rng.randint(0, T, N)
    r1, r2 = np.sqrt(rng.rand(N)), rng.rand(N)
    bary = np.stack([r1 * (1 - r2), r1 * r2], 1).astype(F32)
    keep = (bary[:, 0].astype(np.float64) + bary[:, 1].astype(np.float64)) <= 1.0  # interior, after the rounding to float32
    tri, bary = tri[keep], bary[keep]
    got = tr.sample(tex, T, S, tri, bary, (0, 0, 0)).astype(np.float64)
    A, B, Cc = (v[t[tri, e]].astype(np.float64) for e in range(3))
    be, ga = bary[:, :1].astype(np.float64), bary[:, 1:].astype(np.float64)
    want = (1.0 - be - ga) * A + be * B + ga * Cc
    M = np.abs(np.stack([A, B, Cc], 1)).max(axis=(1, 2))
    err = np.abs(got - want).max(axis=1)
    print("S=%d %s %d: largest error / (2^-24 M) = %.2f of 81" % (S, kind, R, (err / (2.0 ** -24 * M)).max()))
    assert np.all(err <= 81 * 2.0 ** -24 * M)
