"""csrc/mesh_topo.hip against tests/mesh_topo_restatement.py (numpy, from include/pvd_hip_mesh_topo.h), BIT FOR BIT: the sixteen
totals, the per-triangle flags, the per-vertex shells, and of the clean-up the vertices (floats viewed as int32), the triangles and
both maps.  Every quantity of the definition is an integer that does not depend on any order, so there is no tolerance anywhere.

Sizes.  The scans work on workgroups of 256 items and, in one workgroup, on chunks of 8192 workgroup sums: V = 255, 256, 257 and
65 537 (257 workgroup sums), T around 256, 8192 and 16 384.  (More than one chunk needs more than 2^21 items, whose reference alone
takes longer than a test should: tests/test_hip_mesh.py runs the shared scan of csrc/block_scan.h at that size.)  A bucket of more
than 64 entries is walked by a wavefront whose lanes stride it by 64: a closed fan of k triangles around vertex 0 has a triangle
bucket of k entries and an edge bucket of 2 k, so k = 31 .. 65 puts 62, 64, 66, 126, 128 and 130 entries around one and two strides
of the edge bucket and k = 62 .. 130 does the same for the triangle bucket; one fan has 2^14 triangles."""
import functools

import numpy as np
import pytest
import torch

import mesh_simplify_restatement as sr
import mesh_topo_restatement as tr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FILTERS = ((0, False), (0, True))


def _dev(a, dtype):
    return torch.from_numpy(np.array(a, dtype)).to(DEV)  # a copy: the shared inputs are read-only


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


class _Built:
    """pvd_mesh_topo_build through the binding, sentinel-filled outputs with one guard row each; clean() may follow again and again."""

    def __init__(self, v, t, optional=True, ws=None):
        import pvd_hip
        self.V, self.T = len(v), len(t)
        self.v, self.t = _dev(v, np.float32).reshape(self.V, 3), _dev(t, np.int32).reshape(self.T, 3)
        self.ws = torch.empty(pvd_hip.mesh_topo_workspace_bytes(self.V, self.T), dtype=torch.uint8, device=DEV) if ws is None else ws
        totals = torch.full((17,), -7, dtype=torch.int64, device=DEV)
        flags = torch.full((self.T + 1,), 0xee, dtype=torch.uint8, device=DEV) if optional else None
        shell = torch.full((self.V + 1,), -7, dtype=torch.int32, device=DEV) if optional else None
        pvd_hip.mesh_topo_build(self.v, self.t, self.ws, totals[:16], None if flags is None else flags[:self.T],
                                None if shell is None else shell[:self.V])
        torch.cuda.synchronize()
        assert int(totals[16]) == -7
        self.totals = totals[:16].cpu().numpy()
        self.flags = self.shell = None
        if optional:
            assert int(flags[self.T]) == 0xee and int(shell[self.V]) == -7
            self.flags, self.shell = flags[:self.T].cpu().numpy(), shell[:self.V].cpu().numpy()

    def clean(self, least=0, largest=False):
        import pvd_hip
        counts = torch.full((3,), -7, dtype=torch.int64, device=DEV)
        pvd_hip.mesh_topo_clean_count(self.V, self.T, self.ws, least, largest, counts[:2])
        nv, nt, guard = (int(x) for x in counts.tolist())
        assert guard == -7 and 0 <= nv <= self.V and 0 <= nt <= self.T, (nv, nt, guard)
        out_v = torch.full((nv + 1, 3), 123.0, device=DEV)
        out_t = torch.full((nt + 1, 3), -7, dtype=torch.int32, device=DEV)
        vmap = torch.full((self.V + 1,), -7, dtype=torch.int32, device=DEV)
        tmap = torch.full((self.T + 1,), -7, dtype=torch.int32, device=DEV)
        pvd_hip.mesh_topo_clean_emit(self.v, self.t, self.ws, out_v[:nv], out_t[:nt], vmap[:self.V], tmap[:self.T])
        torch.cuda.synchronize()
        assert bool((out_v[nv] == 123.0).all()) and bool((out_t[nt] == -7).all()) and int(vmap[self.V]) == -7 and int(tmap[self.T]) == -7
        return dict(vertices=out_v[:nv].cpu().numpy(), triangles=out_t[:nt].cpu().numpy(), vertex_map=vmap[:self.V].cpu().numpy(),
                    triangle_map=tmap[:self.T].cpu().numpy())


def _same_clean(got, ref, label):
    for key in ("triangles", "vertex_map", "triangle_map"):
        assert got[key].dtype == ref[key].dtype and got[key].shape == ref[key].shape and np.array_equal(got[key], ref[key]), (label, key)
    assert got["vertices"].shape == ref["vertices"].shape and np.array_equal(_bits(got["vertices"]), _bits(ref["vertices"])), label


def _check(label, v, t, filters=FILTERS):
    ref = tr.report(v, t)
    b = _Built(v, t)
    d = tr.named(b.totals)
    print("%s: V=%d T=%d -> %s" % (label, len(v), len(t), d))
    assert np.array_equal(b.totals, ref["totals"]), (label, b.totals, ref["totals"])
    assert b.flags.dtype == np.uint8 and np.array_equal(b.flags, ref["flags"]), label
    assert b.shell.dtype == np.int32 and np.array_equal(b.shell, ref["vertex_shell"]), label
    for least, largest in filters:
        _same_clean(b.clean(least, largest), tr.clean(v, t, least, largest), (label, least, largest))
    return d, b, ref


def test_optional_outputs_and_the_guards():
    v, t, _ = tr.group_cases(0)
    with_them, without = _Built(v, t, optional=True), _Built(v, t, optional=False)
    assert np.array_equal(with_them.totals, without.totals) and np.array_equal(with_them.totals, tr.report(v, t)["totals"])
    _same_clean(without.clean(), tr.clean(v, t), "no optional outputs")


@pytest.mark.parametrize("V", [255, 256, 257, 65537])
def test_scan_boundaries_in_the_vertices(V):
    """A strip mesh over all V vertices, its last triangles doubled and mirrored so that the clean-up has something to drop."""
    v, t = tr.strip(V - 2, "shuffled", seed=V)
    t = np.concatenate([t, t[-3:], t[-7:-5, ::-1]]).astype(np.int32)
    d, _, _ = _check("V at a boundary", v, t, filters=((0, False),))
    assert d["referenced"] == V and d["duplicate"] == 3 and d["cancelled"] == 4


@pytest.mark.parametrize("T", [255, 256, 257, 8191, 8192, 8193, 16385])
def test_scan_boundaries_in_the_triangles(T):
    v, t, _ = sr.soup(1000, T, seed=T)
    t[T // 2:T // 2 + 40] = t[10:50]  # duplicates
    t[T // 2 + 40:T // 2 + 60] = t[60:80, ::-1]  # cancelled pairs
    _check("T at a boundary", v, t, filters=((0, False),))


@pytest.mark.parametrize("k", [31, 32, 33, 62, 63, 64, 65, 66, 126, 128, 130])
def test_bucket_lengths_around_the_wavefront_threshold(k):
    v, t = tr.fan(k, seed=k)
    d, _, _ = _check("fan of %d" % k, v, t, filters=((0, False),))
    assert d["survivors"] == k and d["edges"] == 2 * k and d["boundary"] == k
    # a second fan on the same hub, mirrored in part: duplicates, cancelled pairs and inconsistent edges inside the buckets
    extra = np.concatenate([t, t[: k // 3], t[k // 2:k // 2 + 5, ::-1], t[-2:][:, [1, 2, 0]]]).astype(np.int32)
    _check("fan of %d, dirty" % k, v, extra, filters=((0, False),))


def test_one_bucket_of_2_to_the_14_entries():
    """2^14 triangles under vertex 0 (an edge bucket of 2^15): duplicates and cancelled pairs planted inside, the representative --
    the lowest index of its group -- at the first, a middle and the last slot of the triangle array."""
    k = 1 << 14
    v, t = tr.fan(k, seed=14)
    d, _, _ = _check("big fan", v, t, filters=((0, False),))
    assert d["survivors"] == k and d["edges"] == 2 * k and d["shells"] == 1
    t2 = t.copy()
    t2[k - 1] = t[0][[1, 2, 0]]  # the group of triangle 0: its duplicate in the last slot, rotated
    t2[k // 2] = t[5][::-1]  # triangle 5 and its mirror image cancel
    t2[k // 2 + 1] = t[k - 2]  # the representative of this group sits in the middle, its duplicate near the end
    t2 = np.concatenate([t2, t[100:140][:, ::-1], t[100:140][:, [2, 0, 1]], t[100:120]]).astype(np.int32)  # (p, m) = (2, 1) and (3, 1)
    d, b, ref = _check("big fan, dirty", v, t2, filters=((0, False), (0, True)))
    assert b.flags[0] & 7 == 0 and b.flags[k - 1] == tr.DUPLICATE and b.flags[5] == b.flags[k // 2] == tr.CANCELLED
    assert b.flags[k // 2 + 1] & 7 == 0 and b.flags[k - 2] == tr.DUPLICATE


def test_every_group_and_every_edge_class_inside_a_larger_mesh():
    sv, st, _, _ = sr.sphere_mesh(12)
    gv, gt, expected = tr.group_cases(1)
    ev, et, _ = tr.edge_cases()
    v = np.concatenate([sv, gv, ev])
    t = np.concatenate([st, gt + len(sv), et + len(sv) + len(gv)]).astype(np.int32)
    order = np.random.default_rng(3).permutation(len(t))
    t = t[order]
    d, b, _ = _check("groups and edges", v, t, filters=((0, False), (0, True), (2, False), (5, False)))
    where = np.empty(len(t), np.int64)
    where[order] = np.arange(len(t))  # old row -> new row
    for p, m, members, winner in expected:
        rows = where[len(st) + np.array(members)]
        alive = rows[(b.flags[rows] & 7) == 0]
        if p == m:
            assert len(alive) == 0 and bool((b.flags[rows] == tr.CANCELLED).all()), (p, m)
        else:  # the lowest index of the majority orientation, in the shuffled order
            majority = [int(r) for r, i in zip(rows, members) if _even(gt[i]) == (p > m)]
            assert alive.tolist() == [min(majority)], (p, m)
            assert bool((b.flags[np.setdiff1d(rows, alive)] == tr.DUPLICATE).all()), (p, m)
    assert d["shells"] == 1 + 6 + len(tr.EDGE_CLASSES) and d["largest_size"] == len(st)


def _even(row):
    a, b, c = (int(x) for x in row)
    s = tuple(sorted((a, b, c)))
    return (a, b, c) in (s, (s[1], s[2], s[0]), (s[2], s[0], s[1]))


@pytest.mark.parametrize("order", ["ascending", "descending", "shuffled"])
def test_a_long_strip(order):
    v, t = tr.strip(4096, order, seed=4)
    d, b, _ = _check("strip", v, t, filters=((0, False),))
    assert d["shells"] == 1 and d["largest_size"] == 4096 and d["largest_label"] == 0 and d["inconsistent"] == 0 and bool((b.shell == 0).all())


def test_three_hundred_tetrahedra():
    v, t = tr.tetrahedra(300, seed=1)
    d, _, _ = _check("tetrahedra", v, t, filters=((0, False), (4, True), (5, False)))
    assert d["shells"] == 300 and d["closed"] and d["manifold"] and d["euler"] == 600 and d["largest_size"] == 4


@functools.lru_cache(maxsize=None)
def _numpy_mesh(kind, name):
    v, t = (tr.extracted if kind == "extracted" else tr.clustered)(name)
    for a in (v, t):
        a.setflags(write=False)
    return v, t


@pytest.mark.parametrize("name,euler,shells", [("sphere", 2, 1), ("torus", 0, 1), ("two_spheres", 4, 2)])
def test_extracted_meshes(name, euler, shells):
    """extract_mesh on the device (its bits are pinned to tests/mesh_restatement.py by tests/test_hip_mesh.py), then the report."""
    import mesh_restatement as mr
    from pvd.mesh import extract_mesh, mesh_topology
    field = {"sphere": lambda: mr.sphere_field(12), "torus": lambda: mr.torus_field(16), "two_spheres": lambda: mr.two_spheres_field(16)}[name]()
    dv, dt = extract_mesh(_dev(field, np.float32), 0.0, [-1.0] * 3, [1.0] * 3)
    v, t = _numpy_mesh("extracted", name)
    assert np.array_equal(dt.cpu().numpy(), t) and np.array_equal(_bits(dv.cpu().numpy()), _bits(v))
    d, _, _ = _check(name, v, t, filters=((0, False), (0, True), (len(t) // shells + 1, False)))
    assert d["closed"] and d["manifold"] and d["euler"] == euler and d["shells"] == shells
    top = mesh_topology(dv, dt)
    assert top == d


@pytest.mark.parametrize("name,G,R", [("sphere", 3, 12), ("torus", 9, 24), ("two_spheres", 5, 24)])
def test_clustered_meshes(name, G, R):
    """simplify_mesh on the device (pinned to tests/mesh_simplify_restatement.py by tests/test_hip_mesh_simplify.py), then the report
    and the clean-up: the figures of the CPU test."""
    import mesh_restatement as mr
    from pvd.mesh import clean_mesh, simplify_mesh
    field = {"sphere": mr.sphere_field, "torus": mr.torus_field, "two_spheres": mr.two_spheres_field}[name](R)
    lo, hi = np.full(3, -1.0, np.float32), np.full(3, 1.0, np.float32)
    fv, ft = mr.extract(field, 0.0, lo, hi)
    small = simplify_mesh(_dev(fv, np.float32), _dev(ft, np.int32), G, bmin=lo, bmax=hi)
    v, t = _numpy_mesh("clustered", name)
    assert np.array_equal(small["triangles"].cpu().numpy(), t) and np.array_equal(_bits(small["vertices"].cpu().numpy()), _bits(v))
    d, _, _ = _check("clustered " + name, v, t)
    want = {"sphere": dict(survivors=24, cancelled=12, duplicate=0, non_manifold=0, euler=2),
            "torus": dict(survivors=272, cancelled=0, duplicate=16, non_manifold=4, euler=0),
            "two_spheres": dict(survivors=36, cancelled=8, duplicate=0, non_manifold=0, euler=4)}[name]
    assert d["closed"] and {k: d[k] for k in want} == want
    done = clean_mesh(small["vertices"], small["triangles"])
    assert done["before"] == d and done["after"]["closed"] and done["after"]["euler"] == want["euler"]
    assert done["after"]["duplicate"] == done["after"]["cancelled"] == done["after"]["invalid"] == 0
    assert done["after"]["manifold"] == (name != "torus")  # the torus keeps its four non-manifold edges: nothing is split


def test_a_dirty_soup():
    v, t, _ = sr.soup(400, 900, seed=3, dirty=True)
    d, b, _ = _check("soup", v, t, filters=((0, False), (0, True), (3, False)))
    assert d["invalid"] == 38 and d["invalid"] + d["duplicate"] + d["cancelled"] + d["survivors"] == 900
    t2 = np.concatenate([t, t[100:140], t[100:120, ::-1], t[200:230][:, [1, 2, 0]], t[300:320][:, [0, 2, 1]]]).astype(np.int32)
    d, b, _ = _check("dirtier soup", v, t2, filters=((0, False), (0, True)))
    assert d["duplicate"] > 0 and d["cancelled"] > 0 and d["invalid"] + d["duplicate"] + d["cancelled"] + d["survivors"] == len(t2)
    v3, t3, _ = sr.soup(3000, 600, seed=8, dirty=True)  # sparse: 160 shells, the largest of 174 triangles
    d, _, _ = _check("sparse soup", v3, t3, filters=((0, False), (0, True), (2, False), (3, True), (174, False), (175, False)))
    assert d["shells"] == 160 and d["largest_size"] == 174


def test_repeatability():
    """A second build on the same workspace, a fresh build, and three filters after one build: identical bits."""
    v, t, _ = sr.soup(3000, 600, seed=8, dirty=True)  # 160 shells
    t = np.concatenate([t, t[100:140], t[100:120, ::-1]]).astype(np.int32)
    first = _Built(v, t)
    filters = ((0, False), (2, False), (0, True))
    cleaned = [first.clean(*f) for f in filters]
    again = _Built(v, t, ws=first.ws)  # the workspace as the cleans left it
    fresh = _Built(v, t)
    for other in (again, fresh):
        assert np.array_equal(other.totals, first.totals) and np.array_equal(other.flags, first.flags) and np.array_equal(other.shell, first.shell)
    for f, c in zip(filters, cleaned):
        _same_clean(c, tr.clean(v, t, *f), f)
        _same_clean(again.clean(*f), c, f)
        _same_clean(fresh.clean(*f), c, f)
    _same_clean(first.clean(*filters[0]), cleaned[0], "the first filter after the others")


def test_clean_is_idempotent_on_the_device():
    from pvd.mesh import clean_mesh
    v, t, _ = sr.soup(400, 900, seed=3, dirty=True)
    t = np.concatenate([t, t[100:140], t[100:120, ::-1]]).astype(np.int32)
    one = clean_mesh(_dev(v, np.float32), _dev(t, np.int32))
    two = clean_mesh(one["vertices"], one["triangles"])
    assert torch.equal(two["vertices"].view(torch.int32), one["vertices"].view(torch.int32)) and torch.equal(two["triangles"], one["triangles"])
    nv, nt = one["vertices"].shape[0], one["triangles"].shape[0]
    assert two["vertex_map"].tolist() == list(range(nv)) and two["triangle_map"].tolist() == list(range(nt))
    assert one["after"] == two["before"] == two["after"]
    b, a = one["before"], one["after"]
    assert a["invalid"] == a["duplicate"] == a["cancelled"] == 0 and a["valid"] == b["survivors"]
    for key in tr.NAMES[4:13]:
        assert a[key] == b[key], key
    assert a["largest_label"] == int(one["vertex_map"][b["largest_label"]])


def test_mesh_topology_and_clean_mesh_the_public_path():
    from pvd.mesh import clean_mesh, mesh_topology
    v, t, _ = sr.soup(400, 900, seed=3, dirty=True)
    t = np.concatenate([t, t[100:140], t[100:120, ::-1]]).astype(np.int32)
    dv, dt = _dev(v, np.float32), _dev(t, np.int32)
    ref = tr.report(v, t)
    top = mesh_topology(dv, dt, return_flags=True)
    assert {k: top[k] for k in tr.named(ref["totals"])} == tr.named(ref["totals"])
    assert np.array_equal(top["tri_flags"].cpu().numpy(), ref["flags"]) and np.array_equal(top["vertex_shell"].cpu().numpy(), ref["vertex_shell"])
    assert sorted(mesh_topology(dv, dt)) == sorted(tr.named(ref["totals"]))
    rng = np.random.default_rng(2)
    nrm, col = rng.normal(size=(len(v), 3)).astype(np.float32), rng.uniform(size=(len(v), 3)).astype(np.float32)
    for least, largest in ((0, False), (3, False), (0, True)):
        want = tr.clean(v, t, least, largest)
        got = clean_mesh(dv, dt, normals=_dev(nrm, np.float32), colors=_dev(col, np.float32), min_shell_triangles=least, largest_shell_only=largest)
        _same_clean({k: got[k].cpu().numpy() for k in ("vertices", "triangles", "vertex_map", "triangle_map")}, want, (least, largest))
        kept = want["vertex_map"] >= 0
        assert np.array_equal(_bits(got["normals"].cpu().numpy()), _bits(nrm[kept])) and np.array_equal(_bits(got["colors"].cpu().numpy()), _bits(col[kept]))
        assert got["before"] == tr.named(ref["totals"])
        assert got["after"] == tr.named(tr.report(want["vertices"], want["triangles"])["totals"])
    bare = clean_mesh(dv, dt)
    assert bare["normals"] is None and bare["colors"] is None


def test_extract_surface_with_and_without_clean():
    from pvd.mesh import extract_surface
    from test_hip_mesh_normals import _AnalyticSphere
    R = 24
    model = _AnalyticSphere()
    plain = extract_surface(model, resolution=R)
    off = extract_surface(model, resolution=R, clean=False)
    assert sorted(off) == sorted(plain) == ["colors", "counts", "field", "normals", "threshold", "triangles", "vertices"]
    for key in ("vertices", "triangles", "normals", "colors", "field"):
        assert torch.equal(off[key], plain[key]), key
    m = extract_surface(model, resolution=R, clean=True)
    assert sorted(m) == sorted(list(plain) + ["topology", "triangle_map", "vertex_map"])
    top = m["topology"]
    assert top["before"] == top["after"] and top["after"]["closed"] and top["after"]["manifold"] and top["after"]["euler"] == 2
    for key in ("vertices", "triangles", "normals", "colors"):  # a closed manifold mesh goes through unchanged
        assert torch.equal(m[key], plain[key]), key
    assert m["vertex_map"].tolist() == list(range(plain["vertices"].shape[0]))
    both = extract_surface(model, resolution=R, simplify=4, clean=True)
    only = extract_surface(model, resolution=R, simplify=4)
    lo, hi = model.aabb_infer[:3].cpu().numpy(), model.aabb_infer[3:].cpu().numpy()
    small = sr.simplify(plain["vertices"].cpu().numpy(), plain["triangles"].cpu().numpy(), lo, hi, 4)
    want = tr.clean(small["vertices"], small["triangles"])
    assert np.array_equal(_bits(both["vertices"].cpu().numpy()), _bits(want["vertices"]))
    assert np.array_equal(both["triangles"].cpu().numpy(), want["triangles"])
    assert both["full_counts"] == only["full_counts"] and both["topology"]["before"] == tr.named(tr.report(small["vertices"], small["triangles"])["totals"])
    assert both["topology"]["after"]["closed"] and both["topology"]["after"]["duplicate"] == both["topology"]["after"]["cancelled"] == 0
    composed = np.where(small["vertex_map"] >= 0, want["vertex_map"][np.maximum(small["vertex_map"], 0)], -1)
    assert np.array_equal(both["vertex_map"].cpu().numpy(), composed)
    assert both["normals"].shape == both["vertices"].shape and both["colors"].shape == both["vertices"].shape
    kept = torch.from_numpy(want["vertex_map"] >= 0).to(DEV)
    assert torch.equal(both["normals"], only["normals"][kept]) and torch.equal(both["colors"], only["colors"][kept])


def test_empty_inputs():
    from pvd.mesh import clean_mesh, mesh_topology
    none_v, none_t = np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)
    v, t, _ = sr.soup(50, 20, seed=1, dirty=False)
    for label, vv, tt, invalid in (("nothing", none_v, none_t, 0), ("V = 0", none_v, t, 20), ("T = 0", v, none_t, 0),
                                   ("all triangles invalid", v, np.full((20, 3), 50, np.int32), 20),
                                   ("all triangles repeat an index", v, np.stack([t[:, 0], t[:, 0], t[:, 2]], axis=1), 20)):
        d, b, _ = _check(label, vv, tt, filters=((0, False), (0, True), (1, False)))
        want = np.zeros(16, np.int64)
        want[1], want[13] = invalid, -1
        assert np.array_equal(b.totals, want), label
        done = clean_mesh(_dev(vv, np.float32).reshape(-1, 3), _dev(tt, np.int32).reshape(-1, 3))
        assert done["vertices"].shape == (0, 3) and done["triangles"].shape == (0, 3) and done["after"]["survivors"] == 0
        assert mesh_topology(_dev(vv, np.float32).reshape(-1, 3), _dev(tt, np.int32).reshape(-1, 3))["largest_label"] == -1
