"""tests/components_restatement.py -- the numpy union-find the GPU labelling is compared with -- pinned on the CPU: against
scipy.ndimage.label with the 15-cell structure of the 14 offsets (relabelled to the smallest linear index), on the direction pairs
that tell the Kuhn connectivity from 6- and 26-connectivity, and through the mesh identity (tests/mesh_restatement.py): the mesh of
the filtered field is the mesh of the field without the shells of the dropped components, vertex bits included.  Every comparison
is exact."""
import functools

import numpy as np
import pytest
from scipy import ndimage

import components_restatement as cr
import mesh_restatement as mr

THRESH = 0.5
RANDOM_CASES = ((9, 0.1), (17, 0.2), (33, 0.15), (33, 0.5))


def random_field(R, p, seed=0):
    """1 where a uniform sample is below p (inside at THRESH), 0 elsewhere."""
    return (np.random.RandomState(seed).uniform(size=(R, R, R)) < p).astype(np.float32)


def structure(offsets):
    s = np.zeros((3, 3, 3), bool)
    s[1, 1, 1] = True
    for d in offsets:
        s[1 + d[0], 1 + d[1], 1 + d[2]] = True
    return s


def scipy_labels(u, thresh):
    """labels as the header defines them, from scipy.ndimage.label + scipy.ndimage.minimum over the linear index."""
    ins = cr.inside(u, thresh)
    lab, n = ndimage.label(ins, structure=structure(cr.OFFSETS))
    lin = np.arange(ins.size, dtype=np.int64).reshape(ins.shape)
    out = np.full(ins.shape, -1, np.int32)
    if n:
        smallest = np.asarray(ndimage.minimum(lin, lab, index=np.arange(1, n + 1))).astype(np.int64)
        out[ins] = smallest[lab[ins] - 1]
    return out, n


def check_against_scipy(label_fn, cases=RANDOM_CASES):
    """Raises AssertionError where label_fn's labels, sizes or stats are not what scipy's labelling gives."""
    for R, p in cases:
        u = random_field(R, p)
        labels, sizes, stats = label_fn(u, THRESH)
        want, n = scipy_labels(u, THRESH)
        assert labels.dtype == np.int32 and sizes.dtype == np.uint32 and stats.dtype == np.uint32
        assert np.array_equal(labels, want), (R, p)
        counts = np.bincount(want[want >= 0], minlength=R ** 3).reshape(R, R, R)
        assert np.array_equal(sizes, counts), (R, p)
        big = int(np.argmax(counts))
        assert stats.tolist() == [n, int((want >= 0).sum()), int(counts.reshape(-1)[big]), big], (R, p)


def test_the_structure_has_15_cells_and_the_offsets_are_the_meshers():
    assert structure(cr.OFFSETS).sum() == 15 and len(set(cr.OFFSETS)) == 14
    assert cr.SLOTS == mr.SLOTS
    assert len(cr.OFFSETS_6) == 6 and len(cr.OFFSETS_26) == 26
    assert set(cr.OFFSETS) | set(cr.NOT_NEIGHBOURS) | {tuple(-c for c in d) for d in cr.NOT_NEIGHBOURS} == set(cr.OFFSETS_26)


def test_the_restatement_is_scipys_labelling():
    check_against_scipy(cr.label)


def test_the_random_fields_have_many_small_components_and_one_that_percolates():
    found = [cr.label(random_field(R, p), THRESH)[2] for R, p in RANDOM_CASES]
    for (R, p), st in zip(RANDOM_CASES, found):
        print("R=%d p=%.2f: components %d, inside %d, largest %d at %d" % ((R, p) + tuple(int(v) for v in st)))
    assert all(st[0] > 30 for st in found[:3])                      # many small components
    assert found[2][0] > 1000 and found[2][2] < 0.05 * found[2][1]  # p = 0.15: below the percolation threshold
    assert found[3][2] > 0.99 * found[3][1]                         # p = 0.5: one component crosses everything


def _pair(d, R=5):
    u = np.zeros((R, R, R), np.float32)
    a = tuple(1 if c >= 0 else 2 for c in d)
    u[a] = 1.0
    u[tuple(x + c for x, c in zip(a, d))] = 1.0
    return u


@pytest.mark.parametrize("d", cr.SLOTS)
def test_two_points_along_a_kuhn_direction_are_one_component(d):
    u = _pair(d)
    labels, sizes, stats = cr.label(u, THRESH)
    assert stats.tolist()[:3] == [1, 2, 2] and scipy_labels(u, THRESH)[1] == 1
    assert sorted(set(labels[labels >= 0].tolist())) == [int(stats[3])] == [int(np.flatnonzero(u.reshape(-1))[0])]


@pytest.mark.parametrize("d", cr.NOT_NEIGHBOURS)
def test_two_points_along_another_cube_diagonal_stay_two_components(d):
    u = _pair(d)
    labels, sizes, stats = cr.label(u, THRESH)
    assert stats.tolist()[:3] == [2, 2, 1] and scipy_labels(u, THRESH)[1] == 2
    assert np.array_equal(np.flatnonzero(sizes.reshape(-1)), np.flatnonzero(u.reshape(-1)))


def test_a_6_connected_checker_is_caught():
    assert cr.label(_pair((1, 1, 1)), THRESH, offsets=cr.OFFSETS_6)[2][0] == 2  # splits what a Kuhn edge joins
    with pytest.raises(AssertionError):
        check_against_scipy(lambda u, t: cr.label(u, t, offsets=cr.OFFSETS_6))


def test_a_26_connected_checker_is_caught():
    assert cr.label(_pair((1, -1, 0)), THRESH, offsets=cr.OFFSETS_26)[2][0] == 1  # joins what no Kuhn edge joins
    with pytest.raises(AssertionError):
        check_against_scipy(lambda u, t: cr.label(u, t, offsets=cr.OFFSETS_26))


def test_a_label_that_is_not_the_minimum_is_caught():
    def largest_index(u, t):
        labels, sizes, stats = cr.label(u, t)
        lin = np.arange(labels.size, dtype=np.int64).reshape(labels.shape)
        ids = np.flatnonzero(sizes.reshape(-1))
        top = np.asarray(ndimage.maximum(lin, labels, index=ids)).astype(np.int32)
        out = labels.copy()
        out[labels >= 0] = top[np.searchsorted(ids, labels[labels >= 0])]
        return out, sizes, stats
    with pytest.raises(AssertionError):
        check_against_scipy(largest_index)


def test_nan_and_the_threshold_itself_are_outside():
    u = np.ones((5, 5, 5), np.float32)
    u[2, :, :] = np.nan
    u[:, 2, :] = THRESH
    labels, sizes, stats = cr.label(u, THRESH)
    assert stats.tolist()[:3] == [4, 4 * 2 * 2 * 5, 20] and np.all(labels[2] == -1) and np.all(labels[:, 2] == -1)
    out, kept = cr.filter_field(u, THRESH, labels, sizes, stats, min_points=21)
    assert kept.tolist() == [0, 0] and np.all(np.isnan(out[2][[0, 1, 3, 4]])) and np.all(out[~np.isnan(out)] == np.float32(THRESH))


def test_the_filter_rule_and_the_tie():
    u = np.zeros((9, 9, 9), np.float32)
    u[1, 1, 1:4] = 1.0  # three points, label 91
    u[5, 5, 2:5] = 1.0  # three points: a tie, the larger label
    u[7, 7, 7] = 1.0
    labels, sizes, stats = cr.label(u, THRESH)
    first = (1 * 9 + 1) * 9 + 1
    assert stats.tolist() == [3, 7, 3, first]
    for min_points, want in ((2, [2, 6]), (3, [2, 6]), (4, [0, 0]), (0, [3, 7]), (1, [3, 7])):
        out, kept = cr.filter_field(u, THRESH, labels, sizes, stats, min_points=min_points)
        assert kept.tolist() == want and int((out > THRESH).sum()) == want[1]
    out, kept = cr.filter_field(u, THRESH, labels, sizes, stats, largest_only=True)
    assert kept.tolist() == [1, 3] and np.array_equal(np.flatnonzero(out.reshape(-1) > THRESH), first + np.arange(3))
    empty = np.zeros((3, 3, 3), np.float32)
    labels, sizes, stats = cr.label(empty, THRESH)
    assert stats.tolist() == [0, 0, 0, 0] and np.all(labels == -1) and not sizes.any()
    assert cr.filter_field(empty, THRESH, labels, sizes, stats, 5, True)[1].tolist() == [0, 0]


# ------------------------------------------------------------------ the mesh identity
MESH_R = 17
BOX = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))


@functools.lru_cache(maxsize=None)
def _sphere_plus_noise():
    """A sphere (radius 0.45) and seeded floaters of one to a few points around it, none nearer than two points to the box."""
    R = MESH_R
    u = mr.sphere_field(R, 0.45).astype(np.float32)  # threshold 0
    noise = np.random.RandomState(5).uniform(size=u.shape) < 0.03
    noise[:2] = noise[-2:] = noise[:, :2] = noise[:, -2:] = noise[:, :, :2] = noise[:, :, -2:] = False
    u[noise & (u < -0.1)] = np.float32(0.3)
    u.setflags(write=False)
    return u


def _shells(verts, tris):
    comp = mr.components(len(verts), tris)
    return [tris[comp[tris[:, 0]] == c] for c in np.unique(comp[tris.reshape(-1)])]


def _closed(tris):
    e = mr.directed_edges(tris)
    fwd = set(map(tuple, e.tolist()))
    return len(fwd) == len(e) and all((b, a) in fwd for a, b in fwd)


def _bits(verts):
    return set(map(bytes, np.ascontiguousarray(verts, np.float32).view(np.uint8).reshape(len(verts), 12)))


@pytest.mark.parametrize("min_points,largest_only", [(2, False), (4, False), (0, True)])
def test_the_filtered_fields_mesh_is_the_mesh_minus_the_dropped_shells(min_points, largest_only):
    u = _sphere_plus_noise()
    labels, sizes, stats, out, kept = cr.components(u, 0.0, min_points, largest_only)
    assert stats[0] > 20 and 1 <= kept[0] < stats[0] and stats[2] > 150  # floaters, and the sphere (about 4/3 pi 3.6^3 points)
    verts, tris = mr.extract(u, 0.0, *BOX)
    fverts, ftris = mr.extract(out, 0.0, *BOX)
    # only the dropped components: the kept ones moved outside by the same rule, outside points as they were
    drop = cr.dropped_mask(labels, sizes, stats, min_points, largest_only)
    only = np.where((labels >= 0) & ~drop, np.float32(0.0), u).astype(np.float32)
    dverts, dtris = mr.extract(only, 0.0, *BOX)
    assert len(ftris) == len(tris) - len(dtris) and len(fverts) == len(verts) - len(dverts) and len(dtris) > 0
    all_bits = _bits(verts)
    assert _bits(fverts) <= all_bits and _bits(dverts) <= all_bits and not _bits(fverts) & _bits(dverts)
    shells = _shells(fverts, ftris)
    assert len(shells) == int(kept[0])  # no cavities here: one closed surface per kept component
    for t in shells:
        assert _closed(t) and mr.signed_volume(fverts, t) > 0
    if largest_only:
        assert len(shells) == 1 and int(kept[1]) == int(stats[2])
