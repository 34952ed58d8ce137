"""tests/mesh_atex_restatement.py pinned against what csrc/pvd_hip_mesh_atex.h promises of the area-adaptive atlas: the class boundaries
to the ulp, stable ranks, the layout identities, one owner per texel and the texel counts of the halves, the graded fixture's classes, and
a baked-then-sampled colour field that comes back within a bound derived from the density.  No GPU."""
import numpy as np
import pytest

import mesh_atex_restatement as ar
import mesh_tex_restatement as tr

F32 = np.float32
# right triangles with whole sides whose hypotenuse is m_c = 5, 13, 29, 61; for m_0 = 1 an isosceles one with the base 1
PYTHAGOREAN = {1: (1.0, 0.5), 5: (3.0, 4.0), 13: (5.0, 12.0), 29: (20.0, 21.0), 61: (11.0, 60.0)}


def _right_triangle(a, b, outward=False):
    """A = 0, B = (a, 0, 0), Cc = (0, b, 0); outward: Cc one ulp further out.  (m = 1, where b < a: Cc = (a / 2, b, 0), the longest edge
    is AB = 1, and B moves.)"""
    v = np.array([[0, 0, 0], [a, 0, 0], [a / 2 if b < a else 0, b, 0]], F32)
    if outward:
        if b < a:
            v[1, 0] = np.nextafter(F32(a), F32(np.inf))
        else:
            v[2, 1] = np.nextafter(F32(b), F32(np.inf))
    return v, np.array([[0, 1, 2]], np.int64)


@pytest.mark.parametrize("c, m", list(enumerate(ar.STEPS)))
def test_the_class_boundaries_are_exact_to_the_ulp(c, m):
    """q = m_c^2 exactly is still class c; one ulp further out it is class c + 1 -- or, past 3721, class 4 and capped."""
    a, b = PYTHAGOREAN[m]
    cls, capped, q = ar.classes(*_right_triangle(a, b), 1.0)
    assert q[0] == F32(m * m) and cls[0] == c and not capped[0]
    cls, capped, q = ar.classes(*_right_triangle(a, b, outward=True), 1.0)
    assert q[0] > F32(m * m)
    if c < 4:
        assert cls[0] == c + 1 and not capped[0]
    else:
        assert cls[0] == 4 and capped[0]
    # under max_class: on the boundary of class c the cap c keeps it uncapped, the cap c - 1 does not; past it the cap c caps
    cls, capped, _ = ar.classes(*_right_triangle(a, b), 1.0, max_class=c)
    assert cls[0] == c and not capped[0]
    if c > 0:
        cls, capped, _ = ar.classes(*_right_triangle(a, b), 1.0, max_class=c - 1)
        assert cls[0] == c - 1 and capped[0]
    cls, capped, _ = ar.classes(*_right_triangle(a, b, outward=True), 1.0, max_class=c)
    assert cls[0] == c and capped[0]
    # the density scales the edge: twice the density on half the triangle is the same q
    cls2, _, q2 = ar.classes(_right_triangle(a / 2, b / 2)[0], [[0, 1, 2]], 2.0)
    assert q2[0] == F32(m * m) and cls2[0] == c


def test_an_invalid_triangle_has_class_zero_and_is_not_capped_and_a_bad_density_is_refused():
    v = np.array([[0, 0, 0], [100, 0, 0], [0, 100, 0], [np.nan, 0, 0], [np.inf, 0, 0]], F32)
    t = np.array([[0, 1, 2], [0, 1, 5], [0, -1, 2], [0, 1, 3], [0, 4, 2]], np.int64)
    cls, capped, _ = ar.classes(v, t, 1.0)
    assert cls.tolist() == [4, 0, 0, 0, 0] and capped.tolist() == [True, False, False, False, False]
    slot, order, totals = ar.build(v, t, 1.0)
    assert totals.tolist() == [4, 0, 0, 0, 1, 1] and order.tolist() == [1, 2, 3, 4, 0]
    for bad in (0.0, -1.0, float("nan"), float("inf"), 1e30, 1e-30):  # rho2 overflows or underflows in float32
        with pytest.raises(ValueError):
            ar.classes(v, t, bad)
    with pytest.raises(ValueError):
        ar.classes(v, t, 1.0, max_class=5)


def test_ranks_are_stable_and_order_inverts_slot():
    rng = np.random.RandomState(1)
    T = 1000
    legs = 2.0 ** -rng.randint(0, 8, T)
    v = np.zeros((T, 3, 3), F32)
    v[:, 1, 0] = legs
    v[:, 2, 1] = legs
    t = np.arange(3 * T, dtype=np.int64).reshape(T, 3)
    slot, order, totals = ar.build(v.reshape(-1, 3), t, 40.0)
    cls = ar.classes(v.reshape(-1, 3), t, 40.0)[0]
    assert len(set(cls.tolist())) == 5 and totals[:5].sum() == T
    assert sorted(order.tolist()) == list(range(T))
    base = np.concatenate([[0], np.cumsum(totals[:5])[:4]]).astype(np.int64)
    c, rank = (slot >> 28).astype(np.int64), (slot & 0x0fffffff).astype(np.int64)
    assert np.array_equal(c, cls) and np.array_equal(order[base[c] + rank], np.arange(T))
    for k in range(5):  # stable: inside a class the ranks ascend with f, and are 0 .. count - 1
        assert np.array_equal(rank[cls == k], np.arange(totals[k]))
    for f in (0, 17, T - 1):  # the definition, the slow way
        assert rank[f] == np.sum(cls[:f] == cls[f])


COUNTS = [(0, 0, 0, 0, 0), (1, 0, 0, 0, 0), (0, 0, 0, 0, 1), (1, 0, 0, 0, 1), (5, 0, 3, 0, 2), (33, 17, 9, 5, 3), (0, 700, 0, 0, 0),
          (1000, 1, 1, 1, 1)]


@pytest.mark.parametrize("counts", COUNTS)
def test_the_layout_identities_and_one_owner_per_texel(counts):
    lay = ar.layout(counts)
    Wt, Ht, A = lay["Wt"], lay["Ht"], lay["area"]
    assert Wt % 64 == 0 and Wt * Wt >= A and (Wt == 64 or (Wt - 64) ** 2 < A)
    y = 0
    for c, S in enumerate(ar.CELLS):  # the bands are disjoint, in order, and cover [0, Ht)
        cells = (counts[c] + 1) // 2
        assert lay["y0"][c] == y and lay["C"][c] * S == Wt and lay["rows"][c] == -(-cells // lay["C"][c])
        assert (lay["rows"][c] == 0) == (counts[c] == 0)
        y += lay["rows"][c] * S
    assert Ht == (y if sum(counts) else 4)
    assert ar.layout_words(counts) == [Wt, Ht] + lay["y0"] + lay["rows"] + lay["C"]
    T = sum(counts)
    order = np.random.RandomState(2).permutation(T)
    f, p, q, S = ar.owners(counts, order)
    assert f.shape == (Ht, Wt) and f.max(initial=-1) < T
    owned = np.bincount(f[f >= 0], minlength=T)
    cls = np.repeat(np.arange(5), counts)  # of order[i]
    rank = np.concatenate([np.arange(n) for n in counts]) if T else np.zeros(0, np.int64)
    Sc = np.asarray(ar.CELLS)[cls]
    want = np.where(rank % 2 == 0, Sc * (Sc + 1) // 2, Sc * (Sc - 1) // 2)
    assert np.array_equal(owned[order], want)  # every triangle owns S (S + 1) / 2 or S (S - 1) / 2 texels, and so every one is placed
    assert np.all((p[f >= 0] >= 0) & (p[f >= 0] < S[f >= 0]) & (q[f >= 0] >= 0) & (q[f >= 0] < S[f >= 0]))


def test_the_layout_refuses_a_side_above_16384():
    assert ar.layout((0, 0, 0, 0, 2 * 256 * 256))["Wt"] == 16384
    for bad in ((0, 0, 0, 0, 2 * 256 * 256 + 1), (2 ** 28, 0, 0, 0, 0), (2 * 4096 * 4096 + 1, 0, 0, 0, 0)):
        with pytest.raises(ValueError):
            ar.layout(bad)
    with pytest.raises(ValueError):  # the width fits, the stacked bands do not: 16384 x 16384 of class 4 and one more row of class 0
        ar.layout((1, 0, 0, 0, 2 * 256 * 256))


def test_the_graded_fixture_has_its_classes_and_every_triangle_its_density():
    v, t = ar.graded_fixture()
    assert len(t) == 8 * ar.REPEAT and np.abs(v).max() <= 1.0
    cls, capped, _ = ar.classes(v, t, ar.FIXTURE_DENSITY)
    assert not capped.any()
    assert [int(cls[f]) for f in range(len(t))] == [ar.LEG_CLASSES[ar.fixture_leg(f)] for f in range(len(t))]
    assert np.all(cls[1:] != cls[:-1])  # the classes alternate along f
    # the header's consequence, in float64: m_c >= density * (the longest edge)
    c = v.astype(np.float64)[t]
    L = np.sqrt(np.max([((c[:, 1] - c[:, 0]) ** 2).sum(1), ((c[:, 2] - c[:, 0]) ** 2).sum(1), ((c[:, 2] - c[:, 1]) ** 2).sum(1)], axis=0))
    assert np.all(np.asarray(ar.STEPS)[cls] >= ar.FIXTURE_DENSITY * L)
    slot, order, totals = ar.build(v, t, ar.FIXTURE_DENSITY)
    assert totals.tolist() == [2 * ar.REPEAT, 2 * ar.REPEAT, ar.REPEAT, 2 * ar.REPEAT, ar.REPEAT, 0]


def test_corners_come_back_bit_for_bit_and_uv_sits_on_their_texels():
    v, t = ar.graded_fixture()
    slot, order, totals = ar.build(v, t, ar.FIXTURE_DENSITY)
    counts = totals[:5]
    lay = ar.layout(counts)
    x, _ = ar.points(v, t, counts, order)
    x = x.reshape(lay["Ht"], lay["Wt"], 3)
    ct = ar.corner_texels(counts, slot)
    for k in range(3):
        assert np.array_equal(x[ct[:, k, 1], ct[:, k, 0]].view(np.uint32), v[t[:, k]].view(np.uint32))
    uv = ar.uv(counts, slot)
    assert np.array_equal(np.floor(uv[..., 0] * lay["Wt"]).astype(np.int64), ct[..., 0])
    assert np.array_equal(np.floor((1.0 - uv[..., 1]) * lay["Ht"]).astype(np.int64), ct[..., 1])
    # a lookup at a corner returns the corner's texel, and no lookup reads outside its triangle's cell
    tri = np.repeat(np.arange(len(t), dtype=np.int32), 3)
    bary = np.tile(np.array([[0, 0], [1, 0], [0, 1]], F32), (len(t), 1))
    tex = np.random.RandomState(3).rand(lay["Ht"], lay["Wt"], 3).astype(F32)
    out = ar.sample(tex, len(t), counts, slot, tri, bary, (0, 0, 0))
    assert np.array_equal(out, tex[ct[..., 1].reshape(-1), ct[..., 0].reshape(-1)])
    f_of = ar.owners(counts, order)[0]
    wild = np.random.RandomState(4).uniform(-2, 3, (len(tri), 2)).astype(F32)
    xs, ys, _ = ar.touched(len(t), counts, slot, tri, wild)
    S = np.asarray(ar.CELLS)[slot[tri] >> 28]
    pair = f_of[ys, xs]  # the owners of what was read: the triangle or the one that shares its cell
    rank = (slot & 0x0fffffff).astype(np.int64)
    mate_rank = rank[tri] ^ 1
    assert np.all((xs // S[:, None]) == (xs[:, :1] // S[:, None]))
    for e in range(4):
        mine = pair[:, e] == tri
        other = pair[:, e] >= 0
        assert np.all(mine | ~other | ((slot[np.maximum(pair[:, e], 0)] >> 28 == slot[tri] >> 28) & (rank[np.maximum(pair[:, e], 0)] == mate_rank)))


# ------------------------------------------------------------------------------------------------ the derived accuracy bound
OMEGA = 8.0
# Bilinear interpolation of a function whose second directional derivatives are at most M on a parallelogram cell with edges h1, h2 is off
# by at most (M / 8) (h1^2 + h2^2).  Here M = 0.5 omega^2 and h1, h2 <= 1 / density (the header's consequence): 0.5 * 64 * 2 / (8 * 400).
BOUND_INTERPOLATION = 0.5 * OMEGA ** 2 * 2.0 / (8.0 * ar.FIXTURE_DENSITY ** 2)
# float32: a texel's point has per component three products and two sums of numbers of magnitude <= 2 (|weights| <= 2, |coordinates| <= 1),
# each rounded once, and weights that are themselves rounded (beta, gamma: one rounding; alpha: two): at most 16 ulp(1) = 16 * 2^-23 per
# component, sqrt 3 of that in length, times the colour's Lipschitz constant 0.5 omega.  The texture is stored in float32 (2^-24) and the
# blend is two nested lerps of values <= 1 with rounded weights and tx, ty computed from beta * m with one rounding: 16 * 2^-24 covers it.
BOUND_FLOAT32 = 0.5 * OMEGA * np.sqrt(3.0) * 16 * 2.0 ** -23 + 16 * 2.0 ** -24
BOUND = BOUND_INTERPOLATION + BOUND_FLOAT32


def baked_lookup_errors():
    """(adaptive maximum error, uniform maximum error, adaptive texels, uniform S, uniform texels): the colour field baked on the graded
    fixture through both restatements and looked up at 200 random points inside every triangle, against the field at the float64
    point."""
    v, t = ar.graded_fixture()
    T = len(t)
    slot, order, totals = ar.build(v, t, ar.FIXTURE_DENSITY)
    counts = totals[:5]
    lay = ar.layout(counts)
    tri, bary = ar.random_lookups(T, 200, 0)
    truth = ar.wave_colour(ar.lookup_points(v, t, tri, bary))

    def bake(x, Ht, Wt):
        return np.where(np.isnan(x), 0.0, ar.wave_colour(np.nan_to_num(x))).astype(F32).reshape(Ht, Wt, 3)
    tex = bake(ar.points(v, t, counts, order)[0], lay["Ht"], lay["Wt"])
    adaptive = np.abs(ar.sample(tex, T, counts, slot, tri, bary, (1, 1, 1)).astype(np.float64) - truth)
    texels = lay["Ht"] * lay["Wt"]
    S = next(s for s in range(tr.MIN_S, tr.MAX_S + 1) if tr.layout(T, s)[2] * tr.layout(T, s)[3] >= texels)
    _, _, Wu, Hu = tr.layout(T, S)
    uniform = np.abs(tr.sample(bake(tr.points(v, t, S)[0], Hu, Wu), T, S, tri, bary, (1, 1, 1)).astype(np.float64) - truth)
    return adaptive, uniform, texels, S, Wu * Hu, tri


def test_a_baked_colour_field_comes_back_within_the_bound_derived_from_the_density():
    """|k| = omega = 8, density 20: every lookup is within 0.02 + 1.4e-5 (BOUND above) of the field at the float64 point, in every
    triangle of every class.  The uniform atlas with at least as many texels (S = 37: 148 x 111 against 128 x 124) is measured on the
    same lookups and recorded, not bounded: measured maxima 0.004702 (adaptive) and 0.013699 (uniform), profiles/mesh_atex_checks.txt;
    the adaptive maximum is the smaller one."""
    assert abs(np.linalg.norm(ar.WAVE_K) - OMEGA) < 1e-12 and abs(BOUND_INTERPOLATION - 0.02) < 1e-15 and BOUND_FLOAT32 < 5e-5
    adaptive, uniform, texels, S, texels_u, tri = baked_lookup_errors()
    per_leg = [float(adaptive[np.isin(tri % 8, [k for k in range(8) if ar.LEG_ORDER[k] == i])].max()) for i in range(8)]
    print("adaptive: %d texels, max error %.6f (per leg 2 .. 1/64: %s); uniform S = %d: %d texels, max error %.6f; bound %.6f"
          % (texels, adaptive.max(), " ".join("%.6f" % e for e in per_leg), S, texels_u, uniform.max(), BOUND))
    assert texels_u >= texels
    assert adaptive.max() <= BOUND
    assert adaptive.max() < uniform.max()
