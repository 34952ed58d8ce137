"""tests/mesh_expose_restatement.py pinned on the CPU: the facts below hold for the reference alone, so the GPU tests
(tests/test_hip_mesh_expose.py) cannot hide behind them.  Whole meshes at R = 9 with 16 directions of the Fibonacci sphere (the
reference is rays x triangles: 16 directions keep a fixture near ten seconds); R = 17 is checked on a band."""
import functools

import numpy as np
import pytest

import mesh_expose_restatement as er
import mesh_restatement as mr

D16 = er.directions(er.WHOLE_D)
RATIOS = {}  # label -> smallest det_ratio of a ray set


@functools.lru_cache(maxsize=None)
def _whole(kind):
    v, t = er.fixture(kind, 9)
    counts, totals, ratio = er.exposure(v, t, D16, 1, with_ratio=True)
    counts.setflags(write=False)
    RATIOS["%s R=9 whole D=%d S=1" % (kind, er.WHOLE_D)] = ratio
    return v, t, counts, totals


def test_the_fixtures_are_what_they_are_named():
    for R in er.SIZES:
        shells = {kind: len(np.unique(mr.components(len(er.fixture(kind, R)[0]), er.fixture(kind, R)[1]))) for kind in er.KINDS}
        assert shells == dict(ball=1, hollow=2, nested=3, drilled=2), (R, shells)
        for kind in er.KINDS:
            v, t = er.fixture(kind, R)
            a, b, c = (v[t[:, k]].astype(np.float64) for k in range(3))
            assert np.linalg.norm(np.cross(b - a, c - a), axis=1).min() > 0, (kind, R)  # no triangle without area
            assert mr.signed_volume(v, t) > 0  # outward
    assert len(er.fixture("ball", 9)[1]) == 1616 and 8000 < len(er.fixture("drilled", 17)[1]) < 11000


def test_a_ball_is_seen_from_outside_only():
    v, t, counts, totals = _whole("ball")
    assert np.all(counts[:, 1] > 0) and np.all(counts[:, 3] == 0)
    assert np.all(counts[:, 0] + counts[:, 2] == 16)  # no s == 0 among these
    assert totals.tolist() == [16 * len(t), int(counts[:, 1].sum()), len(t), 0, 0]


@pytest.mark.parametrize("kind", ["hollow", "nested"])
def test_the_inner_shells_are_hidden_and_the_outer_one_is_not(kind):
    v, t, counts, totals = _whole(kind)
    inner = er.centroid_radius(v, t)[0] < 0.7  # the cavity wall (0.5) and the ball (0.12) against the outer surface (0.95)
    assert 300 < inner.sum() < len(t) // 2
    assert np.all(counts[inner, 1] == 0) and np.all(counts[~inner, 1] > 0) and np.all(counts[:, 3] == 0)
    assert totals[4] == inner.sum() and totals[2] == (~inner).sum()


def test_the_drill_exposes_the_cavity():
    v, t, counts, _ = _whole("drilled")
    r, rho, x = er.centroid_radius(v, t)
    cavity = (r < 0.6) & ~((x > 0) & (rho < 0.45))  # the cavity wall and the ball, without the mouth of the drill
    print("drilled: %d cavity triangles, %d exposed" % (cavity.sum(), (counts[cavity, 1] > 0).sum()))
    assert (counts[cavity, 1] > 0).sum() >= 1 and (counts[cavity, 1] == 0).sum() >= 1


def test_the_counts_add_up_and_do_not_depend_on_any_order():
    v, t = er.fixture("nested", 9)
    rng = np.random.RandomState(5)
    band = (700, 740)
    d = np.concatenate([er.directions(7), [[0, 0, 0], [np.nan, 1, 0], [np.inf, 0, 0]]]).astype(np.float32)
    for S in (1, 4):
        c, tot = er.exposure(v, t, d, S, *band)
        assert np.all(c[:, 0] + c[:, 2] == 7 * S) and np.all(c[:, 1] <= c[:, 0]) and np.all(c[:, 3] <= c[:, 2])  # the three bad ones cast nothing
        assert tot[0] == c[:, [0, 2]].sum() and tot[1] == c[:, [1, 3]].sum()
        # the directions in another order
        c2, tot2 = er.exposure(v, t, d[rng.permutation(len(d))], S, *band)
        assert c2.tobytes() == c.tobytes() and tot2.tolist() == tot.tolist()
    # the triangles in another order: the band's rows move with them
    perm = rng.permutation(len(t))
    inv = np.argsort(perm)
    c, _ = er.exposure(v, t, d, 1, *band)
    whole = {int(f): er.exposure(v, t[perm], d, 1, int(inv[f]), int(inv[f]) + 1)[0][0].tolist() for f in range(band[0], band[0] + 6)}
    assert [whole[f] for f in sorted(whole)] == c[:6].tolist()
    # a direction in the plane of a triangle: s == 0, not cast
    tri = np.array([[0, 1, 2]], np.int32)
    flat = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    c, tot = er.exposure(flat, tri, np.array([[1, 1, 0], [0, 0, 1], [0, 0, -2]], np.float32), 4)
    assert c.tolist() == [[4, 4, 4, 4]] and tot.tolist() == [8, 8, 1, 1, 0]


def test_a_duplicate_blocks_its_twin_and_an_invalid_triangle_does_nothing():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [np.nan, 0, 0]], np.float32)
    d = np.array([[0.1, 0.2, 1.0], [0.1, -0.2, -1.0]], np.float32)
    one, _ = er.exposure(v, np.array([[0, 1, 2]], np.int32), d, 4)
    assert one.tolist() == [[4, 4, 4, 4]]
    t = np.array([[0, 1, 2], [0, 1, 2], [0, 1, 3], [0, 1, 7], [-1, 1, 2]], np.int32)
    c, tot = er.exposure(v, t, d, 4)
    assert c.tolist() == [[4, 0, 4, 0], [4, 0, 4, 0], [0] * 4, [0] * 4, [0] * 4] and tot.tolist() == [16, 0, 0, 0, 2]
    # the other orientation: its twin's front is its back, and they still block each other
    c, _ = er.exposure(v, np.array([[0, 1, 2], [0, 2, 1]], np.int32), d, 1)
    assert c.tolist() == [[1, 0, 1, 0], [1, 0, 1, 0]]


def test_the_fixtures_stay_clear_of_the_edge_on_exception():
    """For every (ray, triangle) pair that steps 5 and 6 do not miss, over EXACTLY the ray sets tests/test_hip_mesh_expose.py compares
    with this restatement or across grids -- er.CASES, the whole meshes at directions(er.WHOLE_D), er.CULL_TRIANGLES and er.invalid_case()
    -- det is not rounding noise: |det| >= 2^-34 L^2 (mesh_expose_restatement.det_ratio derives the 2^-44 L^2 a det can be off by).
    (A mesh with every triangle turned over has the same |det|: the flipped nested mesh of the GPU tests is covered by the nested one.
    The default 64 directions on the whole hollow mesh are compared there only with the same 64 on the same grid.)"""
    for kind in er.KINDS:
        _whole(kind)
    for kind, R, D, S, tri0, tri1 in er.CASES:
        v, t = er.fixture(kind, R)
        RATIOS["%s R=%d D=%d S=%d band %s .. %s" % (kind, R, D, S, tri0, tri1)] = er.exposure(v, t, er.directions(D), S, tri0, tri1, True)[2]
    RATIOS["hollow R=9 D=%d band 1001 .. 1101" % er.WHOLE_D] = er.exposure(*er.fixture("hollow", 9), D16, 1, 1001, 1101, True)[2]
    kind, R, D = er.CULL_TRIANGLES
    RATIOS["%s R=%d whole D=%d S=1" % (kind, R, D)] = er.exposure(*er.fixture(kind, R), er.directions(D), 1, with_ratio=True)[2]
    v, t, d = er.invalid_case()
    for S in (1, 4):
        RATIOS["invalid case S=%d" % S] = er.exposure(v, t, d, S, *er.INVALID_BAND, with_ratio=True)[2]
    for label in sorted(RATIOS):
        print("%s: smallest |det| / L^2 = 2^%.1f" % (label, np.log2(RATIOS[label])))
    smallest = min(RATIOS.values())
    print("smallest of all: 2^%.1f, bound 2^%.1f" % (np.log2(smallest), np.log2(er.DET_BOUND)))
    assert len(RATIOS) == 4 + len(er.CASES) + 1 + 1 + 2 and smallest >= er.DET_BOUND
