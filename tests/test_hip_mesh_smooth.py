"""csrc/mesh_smooth.hip against tests/mesh_smooth_restatement.py (numpy, from include/pvd_hip_mesh_smooth.h), BIT FOR BIT: the
smoothed vertices (floats viewed as int32) and the two totals.  Every sum of the definition is an integer sum, so there is no
tolerance anywhere; the inequalities are those of the noisy sphere, asserted next to the equality.

Sizes.  The scan works on workgroups of 256 row sizes and, in one workgroup, on chunks of 8192 workgroup sums: V = 255, 256, 257
(one workgroup, exactly one, two) and 65 537 (257 workgroup sums).  A row of more than 64 entries is summed by a wavefront whose lanes
stride it by 64: hub rows of 62, 64 and 66 entries (lane, lane, wavefront), of 126, 128 and 130 (two strides, the second nearly full,
full, and a third begun), of 63, 64 and 65 strides, and one of 2^18 entries."""
import functools
import os

import numpy as np
import pytest
import torch

import mesh_simplify_restatement as sr
import mesh_smooth_restatement as mr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LAM, MU = 0.5, -0.53


def _dev(a, dtype):
    return torch.from_numpy(np.array(a, dtype)).to(DEV)  # a copy: the shared inputs are read-only


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


class _Built:
    """pvd_mesh_smooth_build through the binding; run() may be called again and again on it."""

    def __init__(self, v, t, lo, hi, pinned=None):
        import pvd_hip
        self.V, self.T = len(v), len(t)
        self.v, self.t = _dev(v, np.float32).reshape(self.V, 3), _dev(t, np.int32).reshape(self.T, 3)
        self.lo, self.hi = _dev(lo, np.float32), _dev(hi, np.float32)
        self.ws = torch.empty(pvd_hip.mesh_smooth_workspace_bytes(self.V, self.T), dtype=torch.uint8, device=DEV)
        totals = torch.full((2,), -7, dtype=torch.int64, device=DEV)  # a sentinel
        pvd_hip.mesh_smooth_build(self.v, self.t, self.lo, self.hi, None if pinned is None else _dev(pinned, np.uint8), self.ws, totals)
        self.totals = tuple(int(x) for x in totals.tolist())

    def run(self, lam, mu, iterations):
        import pvd_hip
        out = torch.full((self.V + 1, 3), 123.0, device=DEV)  # one guard row behind the output
        pvd_hip.mesh_smooth_run(self.v, self.T, self.lo, self.hi, self.ws, lam, mu, iterations, out[:self.V])
        torch.cuda.synchronize()
        assert bool((out[self.V] == 123.0).all())
        return out[:self.V].cpu().numpy()


def _check(label, v, t, lo, hi, iterations=3, pinned=None, lam=LAM, mu=MU):
    ref, st = mr.smooth(v, t, lo, hi, lam, mu, iterations, pinned=pinned, return_state=True)
    b = _Built(v, t, lo, hi, pinned=pinned)
    got = b.run(lam, mu, iterations)
    print("%s: V=%d T=%d iterations=%d -> entries %d, largest row %d, movable %d"
          % (label, len(v), len(t), iterations, b.totals[0], b.totals[1], int(st["movable"].sum())))
    assert b.totals == st["totals"], (label, b.totals, st["totals"])
    assert got.dtype == np.float32 and np.array_equal(_bits(got), _bits(ref)), label
    return got, st, b


@functools.lru_cache(maxsize=None)
def _sphere():
    v, t, lo, hi = mr.noisy_sphere(seed=0)
    for a in (v, t, lo, hi):
        a.setflags(write=False)
    return v, t, lo, hi


@pytest.mark.parametrize("iterations", [1, 2, 10])
def test_the_sphere(iterations):
    v, t, lo, hi = _sphere()
    got, st, _ = _check("sphere", v, t, lo, hi, iterations)
    assert st["movable"].all() and not np.array_equal(_bits(got), _bits(v))
    # the clean sphere too
    cv, ct, _, _ = sr.sphere_mesh(12)
    _check("clean sphere", cv, ct, lo, hi, iterations)


def test_a_second_run_and_a_fresh_build_give_the_same_bits():
    v, t, lo, hi = _sphere()
    first, _, b = _check("sphere", v, t, lo, hi, 4)
    again = b.run(LAM, MU, 4)
    other = b.run(LAM, 0.0, 2)  # another run in between leaves the build as it was
    again2 = b.run(LAM, MU, 4)
    fresh = _Built(v, t, lo, hi).run(LAM, MU, 4)
    assert np.array_equal(_bits(again), _bits(first)) and np.array_equal(_bits(again2), _bits(first))
    assert np.array_equal(_bits(fresh), _bits(first))
    assert np.array_equal(_bits(other), _bits(mr.smooth(v, t, lo, hi, LAM, 0.0, 2)))


def test_a_dirty_soup():
    """Indices -1 and V, NaN / +-inf vertices, repeated indices inside a triangle; its own box, a smaller box (projection), a flat
    axis and an inverted axis; a random pinned mask."""
    v, t, _ = sr.soup(1000, 3000, seed=0)
    v[9].view(np.int32)[0] = 0x7fc01234  # a NaN with a payload: copied, not recomputed
    t[20], t[21], t[22] = (5, 5, 5), (30, 31, 30), (40, 41, 41)
    pinned = (np.random.default_rng(1).uniform(size=len(v)) < 0.25).astype(np.uint8)
    lo, hi = sr.finite_box(v)
    got, st, _ = _check("soup, its own box", v, t, lo, hi)
    assert got[9].view(np.int32)[0] == 0x7fc01234 and not st["movable"][[3, 5, 7, 9]].any()
    got, st, _ = _check("soup, its own box, pinned", v, t, lo, hi, pinned=pinned)
    assert np.array_equal(_bits(got[pinned != 0]), _bits(v[pinned != 0]))
    _check("soup, a smaller box", v, t, np.float32([-0.5, -0.75, -1.0]), np.float32([0.5, 0.25, 0.0]), pinned=pinned)
    got, st, _ = _check("soup, a flat axis", v, t, np.float32([-1, 0.25, -1]), np.float32([1, 0.25, 1]))
    assert bool((got[st["movable"], 1] == 0.25).all())
    _check("soup, an inverted axis (flat)", v, t, np.float32([-1, 1, -1]), np.float32([1, -1, 1]), pinned=pinned)
    _check("soup, the clamp", v, t, lo, hi, iterations=4, lam=1.0, mu=-1.0)
    # zero weights: the round trip of the header's bound, for the movable vertices (all inside their own box)
    got, st, _ = _check("soup, zero weights", v, t, lo, hi, iterations=2, lam=0.0, mu=0.0)
    m = st["movable"]
    assert np.all(np.abs(got[m].astype(np.float64) - v[m].astype(np.float64)).max(axis=0) <= mr.bound(lo, hi))


@pytest.mark.parametrize("V", [255, 256, 257, 65537])
def test_scan_boundaries(V):
    v, t, _ = sr.soup(V, 3000, seed=V)
    _check("V at a boundary", v, t, *sr.finite_box(v), iterations=2)


@pytest.mark.parametrize("k", [31, 32, 33, 63, 64, 65, 32 * 63, 32 * 64, 32 * 65])
def test_row_lengths_around_the_wavefront_threshold(k):
    """A hub of k triangles has a row of 2 k entries: 62, 64, 66 around the threshold of 64; 126, 128, 130 around two strides of the
    wavefront; 63, 64 and 65 whole strides.  Open and closed fans, and two hubs in one mesh."""
    for closed in (False, True):
        v, t = mr.fan(k, seed=k, closed=closed)
        got, st, b = _check("fan of %d, closed=%s" % (k, closed), v, t, *sr.finite_box(v), iterations=3)
        assert b.totals[1] == 2 * k and st["n"][0] == 2 * k
        assert not np.array_equal(_bits(got[0]), _bits(v[0]))
    v2, t2 = mr.fan(k + 1, seed=k + 100, closed=True)
    both_v, both_t = np.concatenate([v, v2 + np.float32(0.5)]), np.concatenate([t, t2 + len(v)]).astype(np.int32)
    pinned = np.zeros(len(both_v), np.uint8)
    pinned[len(v)] = 1  # the second hub is pinned: a long row that is not movable
    _check("two fans", both_v, both_t, *sr.finite_box(both_v), iterations=3)
    got, _, _ = _check("two fans, one hub pinned", both_v, both_t, *sr.finite_box(both_v), iterations=3, pinned=pinned)
    assert np.array_equal(_bits(got[len(v)]), _bits(both_v[len(v)]))


def test_one_hub_of_2_to_the_17_triangles():
    """A row of 2^18 entries, summed by one wavefront.  One pass with weight 1 puts the hub at the mean of its row: the int64 sums
    against Python integers, through the output they determine."""
    k = 1 << 17
    v, t = mr.fan(k, seed=17, closed=True)
    lo, hi = sr.finite_box(v)
    got, st, b = _check("hub", v, t, lo, hi, iterations=1, lam=1.0, mu=0.0)
    assert b.totals == (6 * k, 2 * k)
    _, q, e, _ = sr.quantise(v, lo, hi)
    for a in range(3):
        S = 2 * sum(int(x) for x in q[1:, a])  # every rim vertex is in two of the hub's triangles
        qa = int(q[0, a])
        moved = min(max(qa + int(np.rint(1.0 * (float(S) / float(2 * k) - float(qa)))), 0), 1 << 30)
        assert got[0, a] == np.float32(float(lo[a]) + float(moved) * (float(e[a]) * 2.0 ** -30)), a
    _check("hub, three iterations", v, t, lo, hi, iterations=3)


def test_empty_and_degenerate_inputs():
    import pvd_hip
    lo, hi = np.zeros(3, np.float32), np.ones(3, np.float32)
    none_v, none_t = np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)
    v, t, _ = sr.soup(100, 50, seed=2, dirty=False)
    got, st, b = _check("T = 0", v, none_t, lo, hi)
    assert b.totals == (0, 0) and np.array_equal(_bits(got), _bits(v))
    got, st, b = _check("all triangles invalid", v, np.full((50, 3), 100, np.int32), lo, hi)
    assert b.totals == (0, 0) and np.array_equal(_bits(got), _bits(v))
    got, st, b = _check("all triangles repeat an index", v, np.stack([t[:, 0], t[:, 0], t[:, 2]], axis=1), lo, hi)
    assert b.totals == (0, 0) and np.array_equal(_bits(got), _bits(v))
    got, st, b = _check("all vertices pinned", v, t, lo, hi, pinned=np.ones(100, np.uint8))
    assert b.totals[0] > 0 and np.array_equal(_bits(got), _bits(v))
    got, _, _ = _check("iterations = 0", v, t, lo, hi, iterations=0)
    assert np.array_equal(_bits(got), _bits(v))
    # V = 0: nothing is launched and the totals are not written
    ws = torch.empty(pvd_hip.mesh_smooth_workspace_bytes(0, 50), dtype=torch.uint8, device=DEV)
    totals = torch.full((2,), -7, dtype=torch.int64, device=DEV)
    dv, dt, dlo, dhi = _dev(none_v, np.float32), _dev(t, np.int32), _dev(lo, np.float32), _dev(hi, np.float32)
    pvd_hip.mesh_smooth_build(dv, dt, dlo, dhi, None, ws, totals)
    pvd_hip.mesh_smooth_run(dv, 50, dlo, dhi, ws, LAM, MU, 3, torch.empty(0, 3, device=DEV))
    torch.cuda.synchronize()
    assert totals.tolist() == [-7, -7]
    from pvd.mesh import smooth_mesh
    assert smooth_mesh(dv, _dev(none_t, np.int32)).shape == (0, 3)


def test_smooth_mesh_the_public_path():
    from pvd.mesh import face_vertex_normals, smooth_mesh
    v, t, _ = sr.soup(1000, 3000, seed=0)
    lo, hi = sr.finite_box(v)
    dv, dt = _dev(v, np.float32), _dev(t, np.int32)
    pinned = (np.random.default_rng(1).uniform(size=len(v)) < 0.25)
    default = smooth_mesh(dv, dt, pinned=torch.from_numpy(pinned).to(DEV))
    explicit, totals = smooth_mesh(dv, dt, bmin=lo, bmax=hi, pinned=torch.from_numpy(pinned.astype(np.uint8)).to(DEV), return_totals=True)
    ref, st = mr.smooth(v, t, lo, hi, 0.5, -0.53, 10, pinned=pinned, return_state=True)
    assert np.array_equal(_bits(default.cpu().numpy()), _bits(ref)) and np.array_equal(_bits(explicit.cpu().numpy()), _bits(ref))
    assert tuple(totals.tolist()) == st["totals"]
    zero = smooth_mesh(dv, dt, iterations=0)
    assert zero.data_ptr() != dv.data_ptr() and np.array_equal(_bits(zero.cpu().numpy()), _bits(v))
    # face normals of a sphere point outwards and have unit length
    sv, stri, _, _ = sr.sphere_mesh(12)
    n = face_vertex_normals(_dev(sv, np.float32), _dev(stri, np.int32)).cpu().numpy().astype(np.float64)
    assert np.all(np.abs(np.linalg.norm(n, axis=1) - 1.0) <= 1e-6)
    assert np.min((n * (sv / np.linalg.norm(sv, axis=1, keepdims=True))).sum(axis=1)) > 0.9
    n = face_vertex_normals(dv, dt).cpu().numpy()  # the soup: indices out of range, corners that are not finite
    length = np.linalg.norm(n.astype(np.float64), axis=1)
    assert np.isfinite(n).all() and np.all((np.abs(length - 1.0) <= 1e-6) | (length == 0))


def test_extract_surface_with_and_without_smooth():
    from pvd.mesh import extract_surface
    from test_hip_mesh_normals import _AnalyticSphere
    R = 24
    model = _AnalyticSphere()
    plain = extract_surface(model, resolution=R)
    zero = extract_surface(model, resolution=R, smooth=0)
    assert sorted(zero) == sorted(plain) == ["colors", "counts", "field", "normals", "threshold", "triangles", "vertices"]
    for key in ("vertices", "triangles", "normals", "colors", "field"):
        assert torch.equal(zero[key], plain[key]), key
    assert zero["threshold"] == plain["threshold"] and zero["counts"] == plain["counts"]
    m = extract_surface(model, resolution=R, smooth=5)
    assert sorted(m) == ["colors", "counts", "field", "normals", "smoothed", "threshold", "triangles", "vertices"] and m["smoothed"] == 5
    assert torch.equal(m["triangles"], plain["triangles"]) and not torch.equal(m["vertices"], plain["vertices"])
    assert torch.equal(m["colors"], plain["colors"])  # evaluated at the unsmoothed vertices
    length = torch.linalg.norm(m["normals"], dim=1)
    assert bool(((length - 1.0).abs() <= 1e-6).all())
    radial = m["vertices"] / torch.linalg.norm(m["vertices"], dim=1, keepdim=True)
    assert float((m["normals"] * radial).sum(dim=1).min()) > 0.9
    ref = mr.smooth(plain["vertices"].cpu().numpy(), plain["triangles"].cpu().numpy(), model.aabb_infer[:3].cpu().numpy(),
                    model.aabb_infer[3:].cpu().numpy(), 0.5, -0.53, 5)
    assert np.array_equal(_bits(m["vertices"].cpu().numpy()), _bits(ref))
    both = extract_surface(model, resolution=R, smooth=5, simplify=8)  # the simplification sees the smoothed vertices
    assert both["smoothed"] == 5 and both["full_counts"] == (plain["vertices"].shape[0], plain["triangles"].shape[0])
    small = sr.simplify(ref, plain["triangles"].cpu().numpy(), model.aabb_infer[:3].cpu().numpy(), model.aabb_infer[3:].cpu().numpy(), 8)
    assert np.array_equal(_bits(both["vertices"].cpu().numpy()), _bits(small["vertices"]))
    bare = extract_surface(model, resolution=R, normals=False, colors=False, smooth=5)
    assert bare["normals"] is None and bare["colors"] is None and torch.equal(bare["vertices"], m["vertices"])


def test_a_smoothed_mesh_round_trips_through_ply(tmp_path):
    from pvd.mesh import face_vertex_normals, read_ply, smooth_mesh, write_ply
    v, t, lo, hi = _sphere()
    dt = _dev(t, np.int32)
    sv = smooth_mesh(_dev(v, np.float32), dt, iterations=3)
    nrm = face_vertex_normals(sv, dt)
    path = write_ply(os.path.join(str(tmp_path), "smooth.ply"), sv, dt, normals=nrm)
    rv, rt, rn, rc = read_ply(path)
    assert torch.equal(rv, sv.cpu()) and torch.equal(rt, dt.cpu()) and torch.equal(rn, nrm.cpu()) and rc is None


def test_the_noisy_sphere_on_the_device():
    """The conditions of tests/test_mesh_smooth_restatement.py through smooth_mesh: they hold because the bits are the
    restatement's."""
    from pvd.mesh import smooth_mesh
    v, t, lo, hi = _sphere()
    dv, dt, dlo, dhi = _dev(v, np.float32), _dev(t, np.int32), _dev(lo, np.float32), _dev(hi, np.float32)
    taubin = smooth_mesh(dv, dt, iterations=10, lam=0.5, mu=-0.53, bmin=dlo, bmax=dhi).cpu().numpy()
    laplace = smooth_mesh(dv, dt, iterations=10, lam=0.5, mu=0.0, bmin=dlo, bmax=dhi).cpu().numpy()
    assert np.array_equal(_bits(taubin), _bits(mr.smooth(v, t, lo, hi, 0.5, -0.53, 10)))
    assert np.array_equal(_bits(laplace), _bits(mr.smooth(v, t, lo, hi, 0.5, 0.0, 10)))
    print("radius (mean, std): before %s, taubin %s, laplace %s" % (mr.radii(v), mr.radii(taubin), mr.radii(laplace)))
    mr.check_noisy_sphere_figures(mr.noisy_sphere_figures(v, taubin, laplace))
