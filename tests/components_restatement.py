"""Connected components of the inside set of a density volume, restated in plain numpy from the text of
include/pvd_hip_components.h (not from the kernel): what csrc/components.hip is compared with in tests/test_hip_components.py, and
what tests/test_components_restatement.py pins first (against scipy.ndimage.label, and through the mesh identity).

Field u [R,R,R] f32, x-major.  Inside iff u > thresh (NaN, u == thresh: outside).  Two inside points are neighbours when they differ
by one of OFFSETS: the seven owned-edge directions of the mesher and their negatives.  The label of a component is the smallest
linear index of its points; outside points carry -1.  sizes[q] = points of the component labelled q, at q; 0 elsewhere.
stats = (components, inside points, size of the largest, its label), ties to the smaller label, zeros for an empty inside set.

The union-find: `parent` over linear indices; every round compresses all paths (pointer jumping), then hangs, for every edge whose
ends have different roots, the larger root under the smallest root it met.  Roots only move down, so at the fixed point the root of
a component is its smallest index.
"""
import numpy as np

SLOTS = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1))
OFFSETS = SLOTS + tuple(tuple(-c for c in d) for d in SLOTS)
# what a 6- or a 26-connected implementation would use (for the mutation tests)
OFFSETS_6 = tuple(d for d in OFFSETS if sum(abs(c) for c in d) == 1)
OFFSETS_26 = tuple((a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1) if (a, b, c) != (0, 0, 0))
# the six cube diagonals that are NOT Kuhn edges (and their negatives are not either)
NOT_NEIGHBOURS = ((1, -1, 0), (1, 0, -1), (0, 1, -1), (1, 1, -1), (1, -1, 1), (-1, 1, 1))


def inside(u, thresh):
    with np.errstate(invalid="ignore"):
        return np.asarray(u, np.float32) > np.float32(thresh)


def _window(R, c):
    """Slices (of the point, of the point + c) along one axis."""
    return (slice(0, R - c), slice(c, R)) if c >= 0 else (slice(-c, R), slice(0, R + c))


def edges(ins, offsets=OFFSETS):
    """Linear indices (a, b) of every pair of inside points with b = a + d, d in offsets."""
    R = ins.shape[0]
    lin = np.arange(R ** 3, dtype=np.int64).reshape(R, R, R)
    A, B = [], []
    for d in offsets:
        (ax, bx), (ay, by), (az, bz) = (_window(R, c) for c in d)
        both = ins[ax, ay, az] & ins[bx, by, bz]
        A.append(lin[ax, ay, az][both])
        B.append(lin[bx, by, bz][both])
    return np.concatenate(A), np.concatenate(B)


def label(u, thresh, offsets=OFFSETS):
    """labels [R,R,R] int32, sizes [R,R,R] uint32, stats [4] uint32."""
    u = np.asarray(u, np.float32)
    R = u.shape[0]
    assert u.shape == (R, R, R) and R >= 2
    ins = inside(u, thresh)
    A, B = edges(ins, offsets)
    parent = np.arange(R ** 3, dtype=np.int64)
    while True:
        while True:  # full path compression
            pp = parent[parent]
            if np.array_equal(pp, parent):
                break
            parent = pp
        ra, rb = parent[A], parent[B]
        differ = ra != rb
        if not differ.any():
            break
        np.minimum.at(parent, np.maximum(ra, rb)[differ], np.minimum(ra, rb)[differ])
    flat = ins.reshape(-1)
    labels = np.where(flat, parent, -1).astype(np.int32)
    sizes = np.bincount(labels[flat], minlength=R ** 3).astype(np.uint32)
    stats = np.zeros(4, np.uint32)
    if flat.any():
        big = int(np.argmax(sizes))  # the first maximum: ties go to the smaller label
        stats[:] = (np.count_nonzero(sizes), np.count_nonzero(flat), sizes[big], big)
    return labels.reshape(R, R, R), sizes.reshape(R, R, R), stats


def dropped_mask(labels, sizes, stats, min_points=0, largest_only=False):
    """True at the inside points whose component is dropped: size < min_points, or (largest_only and label != stats[3])."""
    lab = labels.reshape(-1)
    ins = lab >= 0
    size_of = np.where(ins, sizes.reshape(-1)[np.where(ins, lab, 0)], 0)
    drop = ins & (size_of < min_points)
    if largest_only:
        drop |= ins & (lab != int(stats[3]))
    return drop.reshape(labels.shape)


def filter_field(u, thresh, labels, sizes, stats, min_points=0, largest_only=False):
    """(out [R,R,R] f32, kept [2] uint32 = (components kept, points kept)): u with the points of dropped components set to thresh."""
    u = np.asarray(u, np.float32)
    drop = dropped_mask(labels, sizes, stats, min_points, largest_only)
    out = u.copy()
    out[drop] = np.float32(thresh)
    keep = (labels >= 0) & ~drop
    roots = keep & (labels == np.arange(labels.size, dtype=np.int64).reshape(labels.shape))
    return out, np.array([np.count_nonzero(roots), np.count_nonzero(keep)], np.uint32)


def components(u, thresh, min_points=0, largest_only=False, offsets=OFFSETS):
    """Everything at once: labels, sizes, stats, filtered field, kept."""
    labels, sizes, stats = label(u, thresh, offsets)
    out, kept = filter_field(u, thresh, labels, sizes, stats, min_points, largest_only)
    return labels, sizes, stats, out, kept
