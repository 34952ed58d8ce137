"""tests/mesh_smooth_restatement.py pinned on the CPU before csrc/mesh_smooth.hip is compared with it: a pass computed by hand, the
invariants of include/pvd_hip_mesh_smooth.h, and what the filter is for -- the noise of a noisy sphere goes, its radius stays."""
import numpy as np

import mesh_simplify_restatement as sr
import mesh_smooth_restatement as mr

ONE = 1 << 30


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def test_one_pass_on_a_tetrahedron_by_hand():
    """Box [0, 1]^3, vertices on the 2^30 lattice: q is the coordinate times 2^30.  Every vertex of a closed tetrahedron has the other
    three as neighbours, each twice (n = 6).  One pass with w = 0.5 and w = 0: q' = q + rint(0.5 (mean of the others - q))."""
    v = np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 0.5]])
    t = np.int32([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]])
    lo, hi = np.zeros(3, np.float32), np.ones(3, np.float32)
    valid, q, e, flat, tri, n = mr.rows(v, t, lo, hi)
    assert valid.all() and not flat.any() and len(tri) == 4 and n.tolist() == [6, 6, 6, 6]
    assert q.tolist() == [[0, 0, 0], [ONE, 0, 0], [0, ONE, 0], [0, 0, ONE // 2]]
    q1 = mr.one_pass(q, tri, n, np.ones(4, bool), 0.5)
    # vertex 0: the others sum to (2^30, 2^30, 2^29), twice: S / 6 = (2^30 / 3, 2^30 / 3, 2^29 / 3); half of that, rounded
    third = ONE / 3.0
    assert q1[0].tolist() == [int(np.rint(0.5 * third)), int(np.rint(0.5 * third)), int(np.rint(0.5 * (third / 2.0)))]
    assert q1[0].tolist() == [178956971, 178956971, 89478485]
    # vertex 1: the others sum to (0, 2^30, 2^29): x moves half the way to 0, y and z as vertex 0's
    assert q1[1].tolist() == [ONE // 2, 178956971, 89478485]
    # vertex 3: the others sum to (2^30, 2^30, 0): z moves half the way to 0
    assert q1[3].tolist() == [178956971, 178956971, ONE // 4]
    # the whole function: one iteration with mu = 0 is that pass, mapped back into the box; exact in f32 for vertex 1's x
    out = mr.smooth(v, t, lo, hi, 0.5, 0.0, 1)
    assert out[1, 0] == np.float32(0.5) and out[3, 2] == np.float32(0.25)
    assert out[0, 0] == np.float32(178956971 * 2.0 ** -30)
    # a clamp: w = 1 and then w = -1 can leave the box; nothing leaves 0 .. 2^30
    _, st = mr.smooth(v, t, lo, hi, 1.0, -1.0, 3, return_state=True)
    assert st["q"].min() >= 0 and st["q"].max() <= ONE


def test_pinned_invalid_and_isolated_vertices_keep_their_bits():
    v, t, _ = sr.soup(400, 900, seed=3, dirty=True)
    v = np.concatenate([v, np.float32([[0.3, 0.3, 0.3], [np.nan, 1, 2]])])  # two vertices no triangle refers to
    v[9].view(np.int32)[0] = 0x7fc01234  # a NaN with a payload
    rng = np.random.default_rng(4)
    pinned = (rng.uniform(size=len(v)) < 0.3).astype(np.uint8)
    lo, hi = sr.finite_box(v)
    out, st = mr.smooth(v, t, lo, hi, 0.5, -0.53, 4, pinned=pinned, return_state=True)
    keep = ~st["movable"]
    assert keep[-1] and keep[-2] and keep[3] and keep[5] and keep[7] and keep[9] and keep[pinned != 0].all()
    assert np.array_equal(_bits(out[keep]), _bits(v[keep]))
    assert st["movable"].sum() > 100 and not np.array_equal(_bits(out[st["movable"]]), _bits(v[st["movable"]]))
    # a triangle with a repeated index, an index out of range or a corner that is not finite is in no row
    assert st["totals"][0] == 6 * len(mr.rows(v, t, lo, hi)[4]) and len(mr.rows(v, t, lo, hi)[4]) < len(t)
    # iterations == 0: the input bits, whatever else is given
    assert np.array_equal(_bits(mr.smooth(v, t, lo, hi, 0.5, -0.53, 0, pinned=pinned)), _bits(v))


def test_zero_weights_stay_within_the_bound_of_the_header():
    v, t, _ = sr.soup(1000, 3000, seed=5, dirty=False)
    for lo, hi in (sr.finite_box(v), (np.float32([-3, -2, -1.5]), np.float32([1.5, 2, 5])), (np.float32([100, 100, 100]), np.float32([101, 103, 104]))):
        vv = v if lo[0] < 50 else (v + np.float32(102.0)).astype(np.float32)
        vv = np.clip(vv, lo, hi)
        out, st = mr.smooth(vv, t, lo, hi, 0.0, 0.0, 3, return_state=True)
        assert st["movable"].sum() > 900
        err = np.abs(out.astype(np.float64) - vv.astype(np.float64))[st["movable"]].max(axis=0)
        limit = mr.bound(lo, hi)
        print("round trip", err, "bound", limit)
        assert np.all(err <= limit) and np.all(limit < 1e-4)
    assert mr.header_bound_terms() == (2.0 ** -30, 2.0 ** -23)


def test_a_vertex_permutation_permutes_the_output():
    v, t, lo, hi = mr.noisy_sphere(seed=1)
    rng = np.random.default_rng(6)
    perm = rng.permutation(len(v))  # new index i holds old vertex perm[i]
    inv = np.argsort(perm)
    pinned = (rng.uniform(size=len(v)) < 0.1).astype(np.uint8)
    a = mr.smooth(v, t, lo, hi, 0.5, -0.53, 5, pinned=pinned)
    b = mr.smooth(v[perm], inv[t].astype(np.int32)[rng.permutation(len(t))], lo, hi, 0.5, -0.53, 5, pinned=pinned[perm])
    assert np.array_equal(_bits(b), _bits(a[perm]))


def test_the_noisy_sphere_loses_its_noise_and_keeps_its_radius():
    v, t, lo, hi = mr.noisy_sphere(seed=0, amplitude=0.03)
    assert v.shape == (614, 3) and t.shape == (1224, 3)
    _, st = mr.smooth(v, t, lo, hi, 0.5, -0.53, 1, return_state=True)
    assert st["movable"].all() and st["totals"][0] == 6 * 1224  # closed: every vertex has a row
    taubin = mr.smooth(v, t, lo, hi, 0.5, -0.53, 10)
    laplace = mr.smooth(v, t, lo, hi, 0.5, 0.0, 10)
    print("radius (mean, std): before %s, taubin %s, laplace %s" % (mr.radii(v), mr.radii(taubin), mr.radii(laplace)))
    mr.check_noisy_sphere_figures(mr.noisy_sphere_figures(v, taubin, laplace))
