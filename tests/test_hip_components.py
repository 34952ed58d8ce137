"""pvd_components_label / pvd_components_filter (csrc/components.hip, include/pvd_hip_components.h) and pvd/mesh.py against the numpy
union-find of tests/components_restatement.py (pinned by tests/test_components_restatement.py).  labels, sizes, stats, out and kept
must equal the restatement's element for element: the definition of a label leaves no freedom, so there is no tolerance anywhere.

Sizes.  R = 2 (8 points, an eighth of a wave), 3, 9 (729 points: a few workgroups), 17 and 33 (35 937 points: 141 workgroups of
the merge pass, 36 of the flatten pass).  The kernel's tiles are ranges of the LINEAR index -- 64 (a wave: the init pass joins the
runs along k inside it), 256 (a workgroup of the init, merge and filter passes) and 1024 (a workgroup of the flatten pass, which
merges the waves' leading runs before it adds to a size) --, so "across a tile boundary" means p < B <= q for B = 64, 256, 1024,
and the 7 + 6 direction pairs move along every axis.  One case at R = 129 (2.1 M points) puts more increments on one size than a
wave or a workgroup holds.  The serpentine has R^3 / 4 points, not R^3 / 2: two populated neighbouring x-planes always touch through
(1,0,0), so every other plane carries a single connecting point."""
import functools

import numpy as np
import pytest
import torch

import components_restatement as cr
import mesh_restatement as mr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
THRESH = 0.125
SIZES = (2, 3, 9, 17, 33)
TILES = (64, 256, 1024)
MARGIN = 96  # sentinel elements on both sides of every output
IN, OUT = np.float32(1.0), np.float32(-1.0)


# ------------------------------------------------------------------ fields
def _from_mask(mask):
    return np.where(mask, IN, OUT).astype(np.float32)


def _plane_serpentine(R, j0=0, j1=None, k0=0, k1=None):
    """[R,R] mask over (j, k): full rows at j0, j0 + 2, ..., joined alternately at k1 and k0; ((start), (end)) of the path."""
    j1 = R - 1 if j1 is None else j1
    k1 = R - 1 if k1 is None else k1
    m = np.zeros((R, R), bool)
    rows = list(range(j0, j1 + 1, 2))
    for n, j in enumerate(rows):
        m[j, k0:k1 + 1] = True
        if j + 2 <= j1:
            m[j + 1, k1 if n % 2 == 0 else k0] = True
    end = (rows[-1], k1 if len(rows) % 2 == 1 else k0)
    return m, (j0, k0), end


def _serpentine(R):
    """One path: a serpentine in every even x-plane, run forwards and backwards in turn, single points in the odd planes between
    their ends.  Its smallest index, point 0, is one end of the path."""
    m = np.zeros((R, R, R), bool)
    plane, start, end = _plane_serpentine(R)
    for n, i in enumerate(range(0, R, 2)):
        m[i] = plane
        if i + 1 < R and i + 2 < R:
            m[(i + 1,) + (end if n % 2 == 0 else start)] = True
    return m


def _two_serpentines(R):
    """Two combs of serpentines that never touch through a Kuhn edge: A in the planes i = 0 mod 4 over the rows j <= R - 3, hung on
    the column (j, k) = (0, 0); B in the planes i = 2 mod 4 over the rows j >= 2, hung on the column (R - 1, R - 1)."""
    a, b = np.zeros((R, R, R), bool), np.zeros((R, R, R), bool)
    pa = _plane_serpentine(R, 0, R - 3)[0]
    pb = pa[::-1, ::-1]  # the same turned round: rows R - 1, R - 3, ... >= 2, starting at (R - 1, R - 1)
    assert not pb[:2].any() and not pa[R - 2:].any()
    last_a, last_b = (R - 1) // 4 * 4, 2 + (R - 3) // 4 * 4
    a[:last_a + 1, 0, 0] = True
    b[2:last_b + 1, R - 1, R - 1] = True
    for i in range(0, R, 4):
        a[i] |= pa
    for i in range(2, R, 4):
        b[i] |= pb
    return a, b


def _field(kind, R):
    rng = np.random.RandomState(1000 + R)
    if kind == "all_outside":
        u = _from_mask(np.zeros((R, R, R), bool))
    elif kind == "all_inside":
        u = _from_mask(np.ones((R, R, R), bool))
    elif kind.startswith("corner"):
        c = int(kind[6:])
        m = np.zeros((R, R, R), bool)
        m[(R - 1) * (c >> 2), (R - 1) * ((c >> 1) & 1), (R - 1) * (c & 1)] = True
        u = _from_mask(m)
    elif kind == "checkerboard":
        i, j, k = np.indices((R, R, R))
        u = _from_mask((i + j + k) % 2 == 0)
    elif kind.startswith("random"):
        u = _from_mask(rng.uniform(size=(R, R, R)) < float(kind[6:]))
        u *= rng.uniform(0.5, 2.0, size=u.shape).astype(np.float32)  # not two values only
    elif kind == "serpentine":
        u = _from_mask(_serpentine(R))
    elif kind == "two_serpentines":
        a, b = _two_serpentines(R)
        u = _from_mask(a | b)
    elif kind == "nan_blob":  # a ball with NaN and u == thresh points in it: both are outside, and cut it up
        u = (mr.sphere_field(R, 0.8) > 0).astype(np.float32) * 2 - 1
        r = rng.uniform(size=u.shape)
        u[r < 0.25] = np.nan
        u[(r >= 0.25) & (r < 0.5)] = 0.0  # becomes THRESH below
    else:
        raise KeyError(kind)
    return (u + np.float32(THRESH)).astype(np.float32)


KINDS = ["all_outside", "all_inside"] + ["corner%d" % c for c in range(8)] + ["checkerboard", "random0.1", "random0.2", "random0.5",
                                                                             "serpentine", "two_serpentines", "nan_blob"]


@functools.lru_cache(maxsize=None)
def _reference(kind, R):
    """(field, labels, sizes, stats) -- computed once, read-only."""
    u = _field(kind, R)
    out = (u,) + cr.label(u, THRESH)
    for a in out:
        a.setflags(write=False)
    return out


# ------------------------------------------------------------------ running the kernels
def _guarded(n, dtype, garbage, sentinel):
    t = torch.full((n + 2 * MARGIN,), sentinel, dtype=dtype, device=DEV)
    t[MARGIN:MARGIN + n] = garbage
    return t


def _run(u, thresh=THRESH, min_points=0, largest_only=False, in_place=False):
    """labels, sizes, stats, out, kept as numpy arrays, from buffers prefilled with garbage between sentinel margins."""
    import pvd_hip
    R, N = u.shape[0], u.size
    field = torch.from_numpy(np.array(u, np.float32)).to(DEV)
    labels, sizes = _guarded(N, torch.int32, 0x5A5A5A5A, -77), _guarded(N, torch.int32, 0x3C3C3C3C, -78)
    out = _guarded(N, torch.float32, float("inf"), -79.0)
    stats, kept = _guarded(4, torch.int32, -5, -80), _guarded(2, torch.int32, -6, -81)
    inner = [t[MARGIN:t.numel() - MARGIN] for t in (labels, sizes, out, stats, kept)]
    pvd_hip.components_label(field, R, thresh, inner[0], inner[1], inner[3])
    if in_place:
        inner[2].copy_(field.view(-1))
        pvd_hip.components_filter(inner[2], inner[0], inner[1], inner[3], R, thresh, min_points, largest_only, inner[2], inner[4])
    else:
        pvd_hip.components_filter(field, inner[0], inner[1], inner[3], R, thresh, min_points, largest_only, inner[2], inner[4])
    assert field.cpu().numpy().tobytes() == np.asarray(u, np.float32).tobytes()  # the input is not written
    for t, s in ((labels, -77), (sizes, -78), (out, -79.0), (stats, -80), (kept, -81)):
        assert bool((t[:MARGIN] == s).all()) and bool((t[-MARGIN:] == s).all()), "a sentinel margin was written"
    lab, siz, o, st, kp = (t.cpu().numpy() for t in inner)
    return lab.reshape(u.shape), siz.view(np.uint32).reshape(u.shape), st.view(np.uint32), o.reshape(u.shape), kp.view(np.uint32)


def _same(label, got, want):
    names = ("labels", "sizes", "stats", "out", "kept")
    for name, g, w in zip(names, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (label, name, g.dtype, w.dtype, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), (label, name, int((g.view(np.uint32) != w.view(np.uint32)).sum()), "elements differ")


def _check(label, u, ref=None, **kw):
    labels, sizes, stats = ref if ref is not None else cr.label(u, THRESH)
    want = (labels, sizes, stats) + cr.filter_field(u, THRESH, labels, sizes, stats, kw.get("min_points", 0), kw.get("largest_only", False))
    got = _run(u, **kw)
    _same(label, got, want)
    return got


# ------------------------------------------------------------------ tests
# (the two combs need a box of 9 points per edge to stay apart)
CASES = [(kind, R) for kind in KINDS for R in SIZES if not (kind == "two_serpentines" and R < 9)]


@pytest.mark.parametrize("kind,R", CASES)
def test_labels_sizes_and_stats_are_the_restatements(kind, R):
    u, labels, sizes, stats = _reference(kind, R)
    # filtered with a rule that depends on the case, so that kept differs from the totals where it can
    min_points = int(stats[2]) if stats[0] > 1 else 0
    got = _check("%s R=%d" % (kind, R), u, (labels, sizes, stats), min_points=min_points)
    again = _run(u, min_points=min_points)
    for a, b in zip(got, again):  # a second run gives the same bits
        assert a.tobytes() == b.tobytes()


def test_the_cases_are_what_they_are_meant_to_be():
    for R in (9, 17, 33):
        m = _serpentine(R)
        st = _reference("serpentine", R)[3]
        assert st.tolist() == [1, int(m.sum()), int(m.sum()), 0] and m.sum() > R ** 3 // 5
        assert _run(_reference("serpentine", R)[0])[2].tolist() == st.tolist()  # and the kernel finds the one path
        a, b = _two_serpentines(R)
        st = _reference("two_serpentines", R)[3]
        assert st[0] == 2 and st[1] == a.sum() + b.sum() and st[2] == max(a.sum(), b.sum()) and min(a.sum(), b.sum()) > R ** 3 // 12
        assert _reference("nan_blob", R)[3][0] >= 2 and np.isnan(_reference("nan_blob", R)[0]).sum() > R ** 3 // 20
    assert _reference("checkerboard", 9)[3][0] == 1 and _reference("all_inside", 33)[3].tolist() == [1, 33 ** 3, 33 ** 3, 0]
    assert _reference("random0.1", 33)[3][0] > 500 and _reference("random0.5", 33)[3][2] > 0.99 * _reference("random0.5", 33)[3][1]


def _coords(p, R):
    return (p // (R * R), (p // R) % R, p % R)


def _pairs(R):
    """[(p, q)] linear indices, q = p + d: for each of the 7 + 6 directions, one pair across each tile boundary that the lattice
    has (p < B <= q) and one between the last two points of every axis."""
    out = []
    for d in cr.SLOTS + cr.NOT_NEIGHBOURS:
        e = d if (d[0] * R + d[1]) * R + d[2] > 0 else tuple(-c for c in d)  # from the point with the smaller index

        def valid(p):
            c = [x + y for x, y in zip(_coords(p, R), e)]
            return all(0 <= x < R for x in c)
        off = (e[0] * R + e[1]) * R + e[2]
        for B in TILES:
            hit = [p for p in range(max(B - off, 0), min(B, R ** 3)) if valid(p) and p + off >= B and p + off < R ** 3]
            if hit:
                out.append((d, hit[-1], hit[-1] + off))
        p = tuple(R - 2 if c >= 0 else R - 1 for c in e)
        lin = (p[0] * R + p[1]) * R + p[2]
        out.append((d, lin, lin + off))
    return out


@pytest.mark.parametrize("R", SIZES)
def test_direction_pairs_across_tile_boundaries_and_at_the_far_faces(R):
    pairs = _pairs(R)
    assert len(pairs) >= 13 and (R < 9 or any(p < 256 <= q for _, p, q in pairs))
    for d, p, q in pairs:
        u = np.full(R ** 3, OUT + np.float32(THRESH), np.float32)
        u[[p, q]] = IN
        u = u.reshape(R, R, R)
        got = _check("pair %s at %d, %d, R=%d" % (d, p, q, R), u)
        assert got[2].tolist() == ([1, 2, 2, p] if d in cr.SLOTS else [2, 2, 1, p])


def test_min_points_around_the_size_of_a_known_component():
    R = 17
    u = np.full((R, R, R), OUT, np.float32)
    u[2:5, 2:5, 2:5] = IN      # 27 points
    u[8, 8, 3:15] = IN         # 12 points, crossing a wave's end
    u[12:14, 12:14, 12:14] = IN  # 8 points
    u[15, 1, 1] = IN
    u += np.float32(THRESH)
    ref = cr.label(u, THRESH)
    assert ref[2].tolist() == [4, 48, 27, (2 * R + 2) * R + 2]
    for size in (12, 27):
        for min_points, in_place in ((size - 1, False), (size, True), (size + 1, False), (size + 1, True)):
            got = _check("min_points %d" % min_points, u, ref, min_points=min_points, in_place=in_place)
            want_points = sum(s for s in (27, 12, 8, 1) if s >= min_points)
            assert got[4].tolist() == [sum(1 for s in (27, 12, 8, 1) if s >= min_points), want_points]
            assert int((got[3] > THRESH).sum()) == want_points
    got = _check("largest", u, ref, largest_only=True, in_place=True)
    assert got[4].tolist() == [1, 27]


def test_largest_only_with_a_tie_keeps_the_smaller_label():
    R = 9
    u = np.full((R, R, R), OUT, np.float32)
    u[6, 1, 1:5] = IN
    u[1, 6, 3:7] = IN  # the same size, the smaller label
    u[4, 4, 4] = IN
    u += np.float32(THRESH)
    first = (1 * R + 6) * R + 3
    for in_place in (False, True):
        got = _check("tie", u, largest_only=True, in_place=in_place)
        assert got[2].tolist() == [3, 9, 4, first] and got[4].tolist() == [1, 4]
        assert np.array_equal(np.flatnonzero(got[3].reshape(-1) > THRESH), first + np.arange(4))
    got = _check("tie and min_points", u, largest_only=True, min_points=5)
    assert got[4].tolist() == [0, 0] and not (got[3] > THRESH).any()


def test_an_empty_inside_set():
    for R in (2, 9):
        u = _field("all_outside", R)
        for kw in ({}, {"min_points": 3}, {"largest_only": True, "in_place": True}):
            got = _check("empty", u, **kw)
            assert got[2].tolist() == [0, 0, 0, 0] and got[4].tolist() == [0, 0] and np.all(got[0] == -1) and not got[1].any()
            assert got[3].tobytes() == u.tobytes()


def test_more_increments_on_one_size_than_a_workgroup_holds():
    R = 129
    u = _from_mask(np.random.RandomState(0).uniform(size=(R, R, R)) < 0.2) + np.float32(THRESH)
    ref = cr.label(u, THRESH)
    print("R=129 p=0.2: components %d, inside %d, largest %d at %d" % tuple(int(v) for v in ref[2]))
    assert ref[2][0] > 30000 and ref[2][2] > 250000 > 1024
    got = _check("R=129", u, ref, min_points=10)
    again = _run(u, min_points=10)
    for a, b in zip(got, again):
        assert a.tobytes() == b.tobytes()


def test_label_components_and_drop_components():
    from pvd.mesh import drop_components, label_components
    u, labels, sizes, stats = _reference("random0.2", 17)
    field = torch.from_numpy(np.array(u)).to(DEV)
    lab, siz, st = label_components(field, THRESH)
    assert lab.shape == siz.shape == (17, 17, 17) and lab.dtype == siz.dtype == torch.int32 and lab.is_cuda
    assert st == tuple(int(v) for v in stats) and np.array_equal(lab.cpu().numpy(), labels)
    assert np.array_equal(siz.cpu().numpy().view(np.uint32), sizes)
    for kw in ({"min_points": 3}, {"largest_only": True}, {}):
        out, kept = drop_components(field, THRESH, **kw)
        want, want_kept = cr.filter_field(u, THRESH, labels, sizes, stats, **kw)
        assert out.data_ptr() != field.data_ptr() and np.array_equal(field.cpu().numpy(), u)
        assert out.cpu().numpy().tobytes() == want.tobytes() and kept == tuple(int(v) for v in want_kept)
    with pytest.raises(ValueError):
        label_components(field[:, :, :5], THRESH)


class _SphereAndFloaters:
    """What extract_geometry needs of a model: density(), density_thresh, aabb_infer (no occupancy grid)."""
    cuda_ray = False
    density_thresh = 2.0
    blobs = ((0.1, -0.05, 0.0, 0.4), (-0.7, -0.7, -0.6, 0.1), (0.7, 0.6, -0.7, 0.13), (0.65, -0.7, 0.7, 0.06), (-0.6, 0.7, 0.7, 0.16))

    def __init__(self):
        self.aabb_infer = torch.tensor([-1.0, -1.0, -1.0, 1.0, 1.0, 1.0], device=DEV)

    def density(self, x):
        assert x.is_cuda and x.shape[1] == 3
        s = [2.0 + 5.0 * (b[3] - torch.linalg.norm(x - torch.tensor(b[:3], device=x.device), dim=1)) for b in self.blobs]
        return {"sigma": torch.stack(s).max(dim=0).values}


def test_extract_geometry_filters_between_the_field_and_the_mesh():
    from pvd.mesh import density_field, extract_geometry, extract_mesh
    R, model, box = 24, _SphereAndFloaters(), ((-1.0,) * 3, (1.0,) * 3)
    u = density_field(lambda x: model.density(x)["sigma"], R, *box, device=torch.device(DEV))
    labels, sizes, stats = cr.label(u.cpu().numpy(), 2.0)
    small = sorted(int(s) for s in sizes[sizes > 0])
    assert stats[0] >= 4 and small[-1] > 200 and small[-2] < small[-1] // 4  # a sphere and much smaller floaters
    # the defaults: exactly today's calls
    verts, tris, field = extract_geometry(model, resolution=R, return_field=True)
    v0, t0 = extract_mesh(u, 2.0, *box)
    assert torch.equal(field, u) and torch.equal(verts, v0) and torch.equal(tris, t0)
    for kw in ({"min_points": small[-2] + 1}, {"min_points": small[0] + 1}, {"largest_only": True}):
        want, want_kept = cr.filter_field(u.cpu().numpy(), 2.0, labels, sizes, stats, **kw)
        vw, tw = extract_mesh(torch.from_numpy(want).to(DEV), 2.0, *box)
        verts, tris, field, counts = extract_geometry(model, resolution=R, return_field=True, return_counts=True, **kw)
        assert field.cpu().numpy().tobytes() == want.tobytes()
        assert verts.cpu().numpy().tobytes() == vw.cpu().numpy().tobytes() and torch.equal(tris, tw)
        assert counts == (int(stats[0]), int(want_kept[0]), int(want_kept[1]))
        assert 0 < tris.shape[0] < t0.shape[0]
        # the identity: every surviving vertex keeps its bits
        rows = set(map(bytes, v0.cpu().numpy().view(np.uint8).reshape(-1, 12)))
        assert set(map(bytes, verts.cpu().numpy().view(np.uint8).reshape(-1, 12))) <= rows
    assert len(np.unique(mr.components(len(verts), tris.cpu().numpy()))) == 1  # largest_only: one closed surface
