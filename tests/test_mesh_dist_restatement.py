"""tests/mesh_dist_restatement.py pinned before anything is compared with it (tests/test_hip_mesh_dist.py): closed forms for one
triangle in all seven regions, repeated-corner and collinear triangles, a dense barycentric sampling of random triangles (never
nearer than the restated distance, and within the sampling step of it), the min / tie / saturation / validity rules, and the
precondition of the GPU tolerance on every mesh fixture the GPU test uses.  No GPU."""
import numpy as np
import pytest

import mesh_dist_restatement as md

A, B, C = (0.0, 0.0, 0.0), (2.0, 0.0, 0.0), (0.0, 1.0, 0.0)
VERTS = np.array([A, B, C], np.float32)
TRI = np.array([[0, 1, 2]], np.int32)


def _d(points, verts=VERTS, tris=TRI):
    return md.distance_matrix(np.asarray(points, np.float32), verts, tris).astype(np.float64)


def test_closed_forms_in_the_seven_regions_of_one_triangle():
    s5 = np.sqrt(5.0)
    cases = [
        ((0.5, 0.25, 0.75), 0.75), ((0.5, 0.25, -0.75), 0.75), ((0.5, 0.25, 0.0), 0.0),  # above, below, in the interior
        ((1.0, -0.5, 0.0), 0.5), ((1.0, -0.3, 0.4), 0.5),                                 # beyond edge ab
        ((-0.25, 0.5, 0.0), 0.25), ((-0.3, 0.5, -0.4), 0.5),                              # beyond edge ac
        ((2.0, 1.0, 0.0), 2.0 / s5), ((1.0 + 1.0 / s5, 0.5 + 2.0 / s5, 2.0), np.sqrt(5.0)),  # beyond edge bc (normal (1,2)/sqrt 5)
        ((-3.0, -4.0, 0.0), 5.0), ((-1.0, -2.0, 2.0), 3.0),                               # corner a
        ((5.0, -4.0, 0.0), 5.0), ((3.0, -0.5, 0.0), np.sqrt(1.25)),                       # corner b
        ((-1.0, 3.0, 2.0), 3.0), ((0.5, 3.0, 0.0), np.sqrt(4.25)),                        # corner c
        (A, 0.0), (B, 0.0), (C, 0.0), ((1.0, 0.0, 0.0), 0.0), ((1.0, 0.5, 0.0), 0.0),     # on a corner, on an edge
    ]
    got = _d([p for p, _ in cases])[:, 0]
    want = np.array([w for _, w in cases])
    assert np.all(np.abs(got - want) <= 1e-7 * (1.0 + want)), (got, want)  # (the points are float32: 1 + 1/sqrt 5 is rounded)
    exact = [i for i, (p, w) in enumerate(cases) if w == float(np.float32(w)) and all(float(np.float32(x)) == x for x in p)]
    assert len(exact) >= 12 and np.all(got[exact] == want[exact])
    # the order of the corners does not matter
    for perm in ((1, 2, 0), (2, 0, 1), (0, 2, 1)):
        assert np.array_equal(_d([p for p, _ in cases], tris=np.array([perm], np.int32))[:, 0] == 0, want == 0)
        assert np.allclose(_d([p for p, _ in cases], tris=np.array([perm], np.int32))[:, 0], want, rtol=1e-7, atol=1e-12)


def test_repeated_corners_and_collinear_corners_are_their_segments():
    pts = [(1.0, 1.0, 0.0), (-1.0, 0.0, 0.0), (3.0, 4.0, 0.0), (0.5, 0.0, 0.0)]
    seg = np.array([1.0, 1.0, np.sqrt(17.0), 0.0])  # to the segment (0,0,0) -> (2,0,0)
    for tri in ([0, 1, 1], [0, 0, 1], [1, 0, 1]):  # a repeated corner
        assert np.allclose(_d(pts, tris=np.array([tri], np.int32))[:, 0], seg, rtol=1e-15)
    assert np.allclose(_d(pts, tris=np.array([[0, 0, 0]], np.int32))[:, 0], [np.sqrt(2.0), 1.0, 5.0, 0.5], rtol=1e-15)  # a point
    line = np.array([(0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (2.0, 0.0, 0.0), (0.5, 0.0, 0.0)], np.float32)  # exactly collinear
    for tri in ([0, 1, 2], [0, 2, 1], [1, 0, 2], [3, 0, 2]):
        assert np.allclose(_d(pts, line, np.array([tri], np.int32))[:, 0], seg, rtol=1e-15)
    # the switch itself: sin^2 just below and just above 2^-40 -- a sliver of height e over a base of 1 has sin^2 ~ e^2 / ...
    for e, flat in ((2.0 ** -21, True), (2.0 ** -19, False)):
        v = np.array([(0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (1.0, e, 0.0)], np.float32)
        a, b, c, _ = md.corners(v, TRI)
        assert bool(md.sin2(a, b, c)[0] <= md.DEGENERATE) == flat
        assert md.precondition(v, TRI)[0] == 1  # and both sit in the band the GPU fixtures must stay out of


def test_a_dense_sampling_of_random_triangles_never_beats_the_restatement():
    rng = np.random.RandomState(5)
    K = 96  # barycentric step 1 / K
    i, j = np.meshgrid(np.arange(K + 1), np.arange(K + 1), indexing="ij")
    keep = i + j <= K
    w = np.stack([i[keep], j[keep], K - i[keep] - j[keep]], axis=1).astype(np.float64) / K
    for trial in range(12):
        v = rng.uniform(-1.0, 1.0, (3, 3)).astype(np.float32)
        if trial % 4 == 3:
            v[2] = v[0] + (v[1] - v[0]) * 0.3 + rng.uniform(-1e-3, 1e-3, 3).astype(np.float32)  # a thin one
        pts = rng.uniform(-2.0, 2.0, (40, 3)).astype(np.float32)
        ref = _d(pts, v, TRI)[:, 0]
        surface = w @ v.astype(np.float64)
        sampled = np.linalg.norm(pts.astype(np.float64)[:, None, :] - surface[None], axis=2).min(axis=1)
        step = max(np.linalg.norm(v[q].astype(np.float64) - v[(q + 1) % 3]) for q in range(3)) / K
        assert np.all(sampled >= ref - 1e-12), trial
        assert np.all(sampled <= ref + step), trial


def test_min_tie_saturation_and_validity_rules():
    v = np.array([A, B, C, (0.0, 0.0, 1.0), (np.nan, 0.0, 0.0)], np.float32)
    t = np.array([[0, 1, 3], [0, 1, 2], [0, 1, 2], [0, 1, 4], [0, 1, 5], [0, -1, 2]], np.int32)
    assert md.valid_triangles(v, t).tolist() == [True, True, True, False, False, False]
    pts = np.array([(1.0, 0.0, 0.0), (0.5, 0.25, -2.0), (0.5, 0.25, -0.5), (np.inf, 0.0, 0.0), (0.0, np.nan, 0.0)], np.float32)
    D = md.distance_matrix(pts, v, t)
    assert np.all(np.isinf(D[:3, 3:])) and np.all(np.isnan(D[3:]))
    dist, tri = md.nearest(pts, v, t, 1.0, D)
    assert tri.tolist() == [0, -1, 1, -1, -1]  # a tie between 0, 1 and 2 on the shared edge; 1 and 2 are the same triangle
    assert dist[0] == 0 and dist[1] == 1.0 and dist[2] == 0.5 and np.isnan(dist[3]) and np.isnan(dist[4])
    dist, tri = md.nearest(pts, v, t, 0.5, D)  # best == max_dist is saturated
    assert tri.tolist() == [0, -1, -1, -1, -1] and dist[2] == 0.5
    dist, tri = md.nearest(pts, v, t[:0], 2.0)
    assert tri.tolist() == [-1] * 5 and dist[:3].tolist() == [2.0] * 3 and np.isnan(dist[3:]).all()
    dist, tri = md.nearest(pts, v, t[3:], 2.0)  # only invalid triangles
    assert tri.tolist() == [-1] * 5 and dist[:3].tolist() == [2.0] * 3
    assert md.spread(pts[:3], v, t, np.array([0, -1, 1])).tolist() == [1.0, 0.0, 1.5]


@pytest.mark.parametrize("kind,R", md.FIXTURES)
def test_the_fixtures_meet_the_precondition_of_the_gpu_tolerance(kind, R):
    v, t = md.fixture(kind, R)
    near, degenerate = md.precondition(v, t)
    print("%s R=%d: V=%d T=%d, triangles with 0 < sin^2 < 2^-36: %d, degenerate share %.4f" % (kind, R, len(v), len(t), near, degenerate))
    assert len(t) > 100 and md.valid_triangles(v, t).all()
    assert near == 0
    assert degenerate <= 0.01


def test_the_fixtures_cover_three_kinds_at_two_sizes():
    kinds = {}
    for kind, R in md.FIXTURES:
        kinds.setdefault(kind, set()).add(R)
    assert sum(len(s) >= 2 for s in kinds.values()) >= 3 and max(R for _, R in md.FIXTURES) == 33
    assert len(md.fixture("torus", 33)[1]) > 9000
