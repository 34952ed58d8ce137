"""tests/mesh_topo_restatement.py pinned before the kernels are compared with it: hand-built cases with the figures of
include/pvd_hip_mesh_topo.h worked out by hand, the extracted and clustered meshes with the figures measured when the rule was
chosen, and a second, naive dict-and-loop implementation of the same header (below) on every input.  No GPU."""
import collections

import numpy as np
import pytest

import mesh_simplify_restatement as sr
import mesh_topo_restatement as tr


# ------------------------------------------------------------------ the header once more, triangle by triangle
def naive(v, t, min_shell_triangles=0, largest_only=False, keep_first=False):
    """dict(totals, flags, vertex_shell, vertices, triangles, vertex_map, triangle_map).  keep_first: the rule the header does NOT
    have -- the first member of every group survives whatever the orientations."""
    v = np.asarray(v, np.float32).reshape(-1, 3)
    t = [tuple(int(x) for x in row) for row in np.asarray(t, np.int32).reshape(-1, 3)]
    V, T = len(v), len(t)
    flags = [0] * T
    groups = collections.OrderedDict()
    for i, (a, b, c) in enumerate(t):
        if not all(0 <= x < V for x in (a, b, c)) or len({a, b, c}) < 3 or not all(np.isfinite(v[x]).all() for x in (a, b, c)):
            flags[i] = tr.INVALID
            continue
        s = tuple(sorted((a, b, c)))
        even = (a, b, c) in (s, (s[1], s[2], s[0]), (s[2], s[0], s[1]))
        groups.setdefault(s, []).append((i, even))
    survivors = []
    for members in groups.values():
        evens, odds = [i for i, e in members if e], [i for i, e in members if not e]
        if keep_first:
            win = members[0][0]
        elif len(evens) == len(odds):
            win = None
        else:
            win = evens[0] if len(evens) > len(odds) else odds[0]
        for i, _ in members:
            if win is None:
                flags[i] = tr.CANCELLED
            elif i != win:
                flags[i] = tr.DUPLICATE
        if win is not None:
            survivors.append(win)
    survivors.sort()
    edges = {}
    for i in survivors:
        for k in range(3):
            u, w = t[i][k], t[i][(k + 1) % 3]
            e = edges.setdefault((min(u, w), max(u, w)), [0, 0])
            e[0 if u < w else 1] += 1
    cls = {}
    for key, (f, b) in edges.items():
        n = f + b
        cls[key] = (tr.BOUNDARY if n == 1 else 0) | (tr.INCONSISTENT if n == 2 and f != 1 else 0) | (tr.NON_MANIFOLD if n >= 3 else 0)
    for i in survivors:
        for k in range(3):
            u, w = t[i][k], t[i][(k + 1) % 3]
            flags[i] |= cls[(min(u, w), max(u, w))]
    parent = list(range(V))

    def root(x):
        while parent[x] != x:
            x = parent[x]
        return x
    for i in survivors:
        for x in t[i][1:]:
            ra, rb = root(t[i][0]), root(x)
            parent[max(ra, rb)] = min(ra, rb)
    used = sorted({x for i in survivors for x in t[i]})
    shell = [-1] * V
    for x in used:
        shell[x] = root(x)
    sizes = collections.Counter(shell[t[i][0]] for i in survivors)
    best = min(sizes, key=lambda lab: (-sizes[lab], lab)) if sizes else -1
    totals = [0] * 16
    totals[0] = sum(1 for f in flags if not f & tr.INVALID)
    totals[1:5] = [sum(1 for f in flags if f & bit) for bit in (tr.INVALID, tr.DUPLICATE, tr.CANCELLED)] + [len(survivors)]
    totals[5:7] = [len(used), len(edges)]
    totals[7:10] = [sum(1 for c in cls.values() if c & bit) for bit in (tr.BOUNDARY, tr.INCONSISTENT, tr.NON_MANIFOLD)]
    totals[10] = sum(1 for f, b in edges.values() if f != b)
    totals[11:14] = [len(sizes), sizes[best] if sizes else 0, best]
    kept = [i for i in survivors if sizes[shell[t[i][0]]] >= min_shell_triangles and (not largest_only or shell[t[i][0]] == best)]
    kept_v = sorted({x for i in kept for x in t[i]})
    vmap, tmap = [-1] * V, [-1] * T
    for n, x in enumerate(kept_v):
        vmap[x] = n
    for n, i in enumerate(kept):
        tmap[i] = n
    return dict(totals=np.array(totals, np.int64), flags=np.array(flags, np.uint8), vertex_shell=np.array(shell, np.int32),
                vertices=v[kept_v].reshape(-1, 3), triangles=np.array([[vmap[x] for x in t[i]] for i in kept], np.int32).reshape(-1, 3),
                vertex_map=np.array(vmap, np.int32), triangle_map=np.array(tmap, np.int32))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def both(v, t, min_shell_triangles=0, largest_only=False):
    """The restatement's report and clean, checked against the naive implementation; -> (named totals, report, clean)."""
    rep, cl = tr.report(v, t), tr.clean(v, t, min_shell_triangles, largest_only)
    ref = naive(v, t, min_shell_triangles, largest_only)
    for key in ("totals", "flags", "vertex_shell"):
        assert rep[key].dtype == ref[key].dtype and np.array_equal(rep[key], ref[key]), key
    for key in ("triangles", "vertex_map", "triangle_map"):
        assert cl[key].dtype == ref[key].dtype and cl[key].shape == ref[key].shape and np.array_equal(cl[key], ref[key]), key
    assert np.array_equal(_bits(cl["vertices"]), _bits(ref["vertices"]))
    tot = rep["totals"]
    assert tot[0] + tot[1] == len(t) and tot[2] + tot[3] + tot[4] == tot[0] and tot[14] == tot[15] == 0
    return tr.named(tot), rep, cl


def _expect(d, **figures):
    zero = dict(invalid=0, duplicate=0, cancelled=0, boundary=0, inconsistent=0, non_manifold=0, unbalanced=0)
    zero.update(figures)
    for k, x in zero.items():
        assert d[k] == x, (k, d[k], x)


# ------------------------------------------------------------------ hand-built cases
def test_a_closed_tetrahedron():
    d, rep, cl = both(tr.points(4), tr.TET)
    _expect(d, survivors=4, edges=6, referenced=4, euler=2, shells=1, largest_size=4, largest_label=0, valid=4)
    assert d["closed"] and d["manifold"] and not rep["flags"].any() and np.array_equal(rep["vertex_shell"], [0, 0, 0, 0])
    assert np.array_equal(cl["triangles"], tr.TET) and np.array_equal(cl["vertex_map"], np.arange(4))


def test_a_tetrahedron_minus_one_face():
    d, rep, _ = both(tr.points(4), tr.TET[:3])
    _expect(d, survivors=3, edges=6, referenced=4, euler=1, boundary=3, unbalanced=3, shells=1, largest_size=3, largest_label=0, valid=3)
    assert not d["closed"] and not d["manifold"] and np.array_equal(rep["flags"], [tr.BOUNDARY] * 3)


def test_two_tetrahedra_glued_on_a_face_kept_twice():
    """The face (1, 2, 3) of the first and its mirror image of the second: once in each orientation, a collapsed sheet."""
    second = np.array([(1, 3, 2), (1, 2, 4), (2, 3, 4), (1, 4, 3)], np.int32)  # apex 4, outward with the shared face (1, 3, 2)
    t = np.concatenate([tr.TET, second])
    d, rep, cl = both(tr.points(5), t)
    _expect(d, valid=8, cancelled=2, survivors=6, edges=9, referenced=5, euler=2, shells=1, largest_size=6, largest_label=0)
    assert d["closed"] and not d["manifold"]  # not manifold as given: it holds cancelled triangles
    assert np.array_equal(np.nonzero(rep["flags"] == tr.CANCELLED)[0], [2, 4])
    again = tr.named(tr.report(cl["vertices"], cl["triangles"])["totals"])
    assert again["manifold"] and again["closed"] and again["euler"] == 2 and again["survivors"] == 6


def test_three_triangles_on_one_edge():
    d, rep, _ = both(tr.points(5), np.array([(0, 1, 2), (0, 1, 3), (0, 1, 4)], np.int32))
    _expect(d, valid=3, survivors=3, edges=7, referenced=5, euler=1, non_manifold=1, boundary=6, unbalanced=7, shells=1, largest_size=3,
            largest_label=0)
    assert np.array_equal(rep["flags"], [tr.NON_MANIFOLD | tr.BOUNDARY] * 3)


def test_a_triangle_pair_with_a_flipped_neighbour():
    """(0, 1, 2) and (1, 2, 3) both traverse 1 -> 2; (0, 1, 2) and (1, 0, 4) are wound consistently."""
    d, rep, _ = both(tr.points(5), np.array([(0, 1, 2), (1, 2, 3), (1, 0, 4)], np.int32))
    _expect(d, valid=3, survivors=3, edges=7, referenced=5, euler=1, inconsistent=1, boundary=5, unbalanced=6, shells=1, largest_size=3,
            largest_label=0)
    assert np.array_equal(rep["flags"], [tr.INCONSISTENT | tr.BOUNDARY, tr.INCONSISTENT | tr.BOUNDARY, tr.BOUNDARY])


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_every_group(seed):
    v, t, expected = tr.group_cases(seed)
    d, rep, cl = both(v, t)
    assert [(p, m) for p, m, _, _ in expected] == list(tr.GROUPS)
    for p, m, members, winner in expected:
        assert len(members) == p + m
        for i in members:
            want = tr.CANCELLED if winner < 0 else (tr.BOUNDARY if i == winner else tr.DUPLICATE)  # a lone survivor: three boundary edges
            assert rep["flags"][i] == want, (p, m, i)
            assert (cl["triangle_map"][i] >= 0) == (i == winner)
    # six groups have a survivor -- all but (1, 1) and (2, 2) --, each a lone triangle on vertices of its own
    _expect(d, valid=len(t), survivors=6, duplicate=1 + 2 + 2 + 2 + 3, cancelled=2 + 4, edges=18, boundary=18, unbalanced=18, referenced=18,
            euler=6, shells=6, largest_size=1, largest_label=0)


def test_every_edge_class():
    v, t, classes = tr.edge_cases()
    d, rep, _ = both(v, t)
    n = [f + b for f, b in classes]
    _expect(d, valid=len(t), survivors=len(t), edges=len(classes) + 2 * len(t), boundary=n.count(1) + 2 * len(t),
            inconsistent=sum(1 for f, b in classes if f + b == 2 and f != 1), non_manifold=sum(1 for x in n if x >= 3),
            unbalanced=sum(1 for f, b in classes if f != b) + 2 * len(t), referenced=len(v), euler=len(v) - len(classes) - len(t),
            shells=len(classes), largest_size=4, largest_label=len(v) - 6)  # the last class, (2, 2): two vertices and four apexes
    row = 0
    for f, b in classes:
        want = tr.BOUNDARY | (tr.INCONSISTENT if f + b == 2 and f != 1 else 0) | (tr.NON_MANIFOLD if f + b >= 3 else 0)
        assert np.all(rep["flags"][row:row + f + b] == want), (f, b)
        row += f + b


# ------------------------------------------------------------------ the meshes of the issue
@pytest.mark.parametrize("name,V,T,E,euler,shells", [("sphere", 614, 1224, 1836, 2, 1), ("torus", 1368, 2736, 4104, 0, 1),
                                                       ("two_spheres", 536, 1064, 1596, 4, 2)])
def test_extracted_meshes_are_closed_manifolds(name, V, T, E, euler, shells):
    v, t = tr.extracted(name)
    assert (len(v), len(t)) == (V, T)
    d, rep, cl = both(v, t)
    _expect(d, valid=T, survivors=T, referenced=V, edges=E, euler=euler, shells=shells, largest_size=T // shells, largest_label=0)
    assert d["closed"] and d["manifold"] and not rep["flags"].any()
    assert np.array_equal(cl["triangles"], t) and np.array_equal(_bits(cl["vertices"]), _bits(v))


def test_clustered_meshes():
    v, t = tr.clustered("sphere")
    d, _, _ = both(v, t)
    _expect(d, valid=36, cancelled=12, survivors=24, euler=2, referenced=14, edges=36, shells=1, largest_size=24, largest_label=0)
    assert len(t) == 36 and d["closed"]
    first = tr.named(naive(v, t, keep_first=True)["totals"])  # the rule that was not chosen leaves open flaps
    assert first["survivors"] == 30 and first["boundary"] == 12 and first["non_manifold"] == 6 and not first["closed"]
    v, t = tr.clustered("torus")
    d, _, _ = both(v, t)
    assert len(t) == 288
    _expect(d, valid=288, duplicate=16, survivors=272, non_manifold=4, referenced=132, edges=404, euler=0, shells=1, largest_size=272,
            largest_label=0)
    v, t = tr.clustered("two_spheres")
    d, _, _ = both(v, t)
    assert len(t) == 44 and d["closed"]
    _expect(d, valid=44, cancelled=8, survivors=36, referenced=22, edges=54, euler=4, shells=2, largest_size=18, largest_label=0)


def test_a_dirty_soup():
    v, t, _ = sr.soup(400, 900, seed=3, dirty=True)
    d, rep, cl = both(v, t)
    f = rep["flags"]
    assert d["invalid"] == 38 and int((f == tr.INVALID).sum()) == 38
    assert d["invalid"] + d["duplicate"] + d["cancelled"] + d["survivors"] == len(t) == 900
    assert not (f[f & 7 != 0] & 56).any()  # only survivors carry edge bits
    assert f[[0, 1, 2, 4, 6, 8]].tolist() == [tr.INVALID] * 6
    # a dirtier one: planted duplicates, mirror images and their rotations
    t2 = np.concatenate([t, t[100:140], t[100:120, ::-1], t[200:230][:, [1, 2, 0]], t[300:320][:, [0, 2, 1]]]).astype(np.int32)
    d2, _, _ = both(v, t2)
    assert d2["duplicate"] > 0 and d2["cancelled"] > 0


# ------------------------------------------------------------------ clean
@pytest.mark.parametrize("maker", ["soup", "groups", "clustered torus", "edges"])
def test_clean_is_idempotent_and_keeps_the_totals(maker):
    if maker == "soup":
        v, t, _ = sr.soup(400, 900, seed=3, dirty=True)
        t = np.concatenate([t, t[100:140], t[100:120, ::-1]]).astype(np.int32)
    elif maker == "groups":
        v, t, _ = tr.group_cases(0)
    elif maker == "edges":
        v, t, _ = tr.edge_cases()
    else:
        v, t = tr.clustered("torus")
    d, rep, cl = both(v, t)
    d2, _, cl2 = both(cl["vertices"], cl["triangles"])
    assert np.array_equal(_bits(cl2["vertices"]), _bits(cl["vertices"])) and np.array_equal(cl2["triangles"], cl["triangles"])
    assert np.array_equal(cl2["vertex_map"], np.arange(len(cl["vertices"]))) and np.array_equal(cl2["triangle_map"], np.arange(len(cl["triangles"])))
    assert d2["invalid"] == d2["duplicate"] == d2["cancelled"] == 0 and d2["valid"] == d["survivors"]
    for key in tr.NAMES[4:13]:
        assert d2[key] == d[key], key
    assert d2["largest_label"] == (cl["vertex_map"][d["largest_label"]] if d["largest_label"] >= 0 else -1)


def _two_shells(small=4):
    """A strip of `small` triangles on the low indices and one of 6 on the high ones."""
    va, ta = tr.strip(small)
    vb, tb = tr.strip(6, "descending")
    return np.concatenate([va, vb + np.float32(5)]), np.concatenate([ta, tb + len(va)]).astype(np.int32)


def test_the_shell_filter():
    v, t = _two_shells(4)
    d, _, _ = both(v, t)
    assert d["shells"] == 2 and d["largest_size"] == 6 and d["largest_label"] == 6
    for least, kept in ((0, 10), (3, 10), (4, 10), (5, 6), (6, 6), (7, 0)):
        _, _, cl = both(v, t, min_shell_triangles=least)
        assert len(cl["triangles"]) == kept, least
        assert len(cl["vertices"]) == {10: 14, 6: 8, 0: 0}[kept]
    _, _, cl = both(v, t, largest_only=True)
    assert np.array_equal(cl["triangle_map"], [-1] * 4 + list(range(6))) and np.array_equal(cl["vertex_map"], [-1] * 6 + list(range(8)))
    _, _, cl = both(v, t, min_shell_triangles=7, largest_only=True)
    assert len(cl["triangles"]) == 0 and len(cl["vertices"]) == 0
    # a tie goes to the smaller label
    v, t = _two_shells(6)
    d, _, cl = both(v, t, largest_only=True)
    assert d["largest_size"] == 6 and d["largest_label"] == 0
    assert np.array_equal(cl["triangle_map"], list(range(6)) + [-1] * 6)


def test_a_vertex_permutation():
    v, t, _ = sr.soup(300, 700, seed=5, dirty=True)
    t = np.concatenate([t, t[100:130], t[100:120, ::-1]]).astype(np.int32)
    _, rep, cl = both(v, t)
    perm = np.random.default_rng(7).permutation(len(v))  # old index -> new index
    pv = np.empty_like(v)
    pv[perm] = v
    inside = ((t >= 0) & (t < len(v))).all(axis=1)
    pt = t.copy()
    pt[inside] = perm[t[inside]]
    pt[~inside] = np.where((t[~inside] >= 0) & (t[~inside] < len(v)), 0, t[~inside])  # still out of range where it was
    _, prep, pcl = both(pv, pt)
    assert np.array_equal(prep["totals"][:13], rep["totals"][:13]) and np.array_equal(prep["flags"], rep["flags"])
    assert np.array_equal(pcl["triangle_map"], cl["triangle_map"])
    assert np.array_equal(pcl["vertex_map"][perm] >= 0, cl["vertex_map"] >= 0)
    # the same partition into shells: vertices share a label after the permutation iff they did before
    a, b = rep["vertex_shell"], prep["vertex_shell"][perm]
    assert np.array_equal(a >= 0, b >= 0)
    pairs = set(zip(a[a >= 0].tolist(), b[a >= 0].tolist()))
    assert len(pairs) == len({x for x, _ in pairs}) == len({y for _, y in pairs})
    for lab in {y for _, y in pairs}:  # and every label is the smallest new index of its shell
        assert lab == perm[a == dict((y, x) for x, y in pairs)[lab]].min()
    # the cleaned vertices are the same points, in the new order
    assert np.array_equal(_bits(pcl["vertices"][pcl["vertex_map"][perm][cl["vertex_map"] >= 0]]), _bits(cl["vertices"]))


def test_empty_inputs():
    none_v, none_t = np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)
    v, t, _ = sr.soup(50, 20, seed=1, dirty=False)
    for vv, tt, invalid in ((none_v, none_t, 0), (none_v, t, 20), (v, none_t, 0), (v, np.full((20, 3), 50, np.int32), 20)):
        d, rep, cl = both(vv, tt)
        want = np.zeros(16, np.int64)
        want[1], want[13] = invalid, -1
        assert np.array_equal(rep["totals"], want)
        assert np.all(rep["vertex_shell"] == -1) and np.all(rep["flags"] == tr.INVALID)
        assert cl["vertices"].shape == (0, 3) and cl["triangles"].shape == (0, 3)
        assert np.all(cl["vertex_map"] == -1) and np.all(cl["triangle_map"] == -1)
