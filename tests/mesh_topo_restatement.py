"""The mesh topology report and clean-up, restated in vectorised numpy from the definition in include/pvd_hip_mesh_topo.h (not from
the kernels: no buckets, no union-find; groups and edges through np.unique, shells by propagating the smallest index): what
csrc/mesh_topo.hip is compared with, bit for bit, in tests/test_hip_mesh_topo.py, and what tests/test_mesh_topo_restatement.py
pins first against hand-built cases and a naive dict-and-loop implementation.  The input makers the test files share are at the end.
"""
import numpy as np

NAMES = ("valid", "invalid", "duplicate", "cancelled", "survivors", "referenced", "edges", "boundary", "inconsistent", "non_manifold",
         "unbalanced", "shells", "largest_size", "largest_label")
INVALID, DUPLICATE, CANCELLED, BOUNDARY, INCONSISTENT, NON_MANIFOLD = 1, 2, 4, 8, 16, 32


def _ids(*columns):
    """A dense id per distinct row of the columns (int64, values below 2^31): np.unique on packed 62-bit keys, column by column."""
    g = np.unique(columns[0], return_inverse=True)[1].reshape(-1)
    for c in columns[1:]:
        g = np.unique(g.astype(np.int64) * (1 << 31) + c, return_inverse=True)[1].reshape(-1)
    return g


def _status(vertices, triangles):
    """(tri [T,3] int64, valid, survivor, duplicate, cancelled -- [T] bool each)."""
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    tri = np.asarray(triangles, np.int32).reshape(-1, 3).astype(np.int64)
    V, T = len(v), len(tri)
    finite = np.isfinite(v).all(axis=1)
    valid = ((tri >= 0) & (tri < V)).all(axis=1)
    valid &= (tri[:, 0] != tri[:, 1]) & (tri[:, 1] != tri[:, 2]) & (tri[:, 0] != tri[:, 2])
    valid[valid] = finite[tri[valid]].all(axis=1)
    idx = np.nonzero(valid)[0]
    survivor, cancelled = np.zeros(T, bool), np.zeros(T, bool)
    if len(idx):
        t = tri[idx]
        k = np.argmin(t, axis=1)
        r = np.arange(len(t))
        x, y = t[r, (k + 1) % 3], t[r, (k + 2) % 3]  # a rotation keeps the parity
        even = x < y
        key = np.stack([t[r, k], np.minimum(x, y), np.maximum(x, y)], axis=1)
        g = _ids(key[:, 0], key[:, 1], key[:, 2])
        G = int(g.max()) + 1
        p, m = np.bincount(g[even], minlength=G), np.bincount(g[~even], minlength=G)
        first_even, first_odd = np.full(G, T, np.int64), np.full(G, T, np.int64)
        np.minimum.at(first_even, g[even], idx[even])
        np.minimum.at(first_odd, g[~even], idx[~even])
        winner = np.where(p > m, first_even, np.where(m > p, first_odd, -1))
        survivor[idx] = winner[g] == idx
        cancelled[idx] = (p == m)[g]
    return tri, valid, survivor, valid & ~survivor & ~cancelled, cancelled


def _shells(V, s):
    """label [V] int64 of the survivors s [F,3]: the smallest vertex index of the shell, -1 for a vertex no survivor uses."""
    lab = np.arange(V, dtype=np.int64)  # always: lab[x] <= x, a vertex of x's shell, and lab[lab[x]] == lab[x] between the rounds
    while len(s):
        low = lab[s].min(axis=1)
        new = lab.copy()
        for k in range(3):
            np.minimum.at(new, lab[s[:, k]], low)  # the label of every corner takes the triangle's smallest label
        while True:  # pointer jumping until every label is its own label
            jumped = new[new]
            if np.array_equal(jumped, new):
                break
            new = jumped
        if np.array_equal(new, lab):  # the corners of every triangle agree, and a label that is its own is the shell's smallest
            break
        lab = new
    ref = np.zeros(V, bool)
    ref[s.reshape(-1)] = True
    return np.where(ref, lab, -1)


def report(vertices, triangles):
    """dict(totals [16] int64, flags [T] uint8, vertex_shell [V] int32) of the header."""
    V = len(np.asarray(vertices, np.float32).reshape(-1, 3))
    tri, valid, survivor, duplicate, cancelled = _status(vertices, triangles)
    T = len(tri)
    flags = np.zeros(T, np.uint8)
    flags[~valid] |= INVALID
    flags[duplicate] |= DUPLICATE
    flags[cancelled] |= CANCELLED
    sidx = np.nonzero(survivor)[0]
    s = tri[sidx]
    F = len(s)
    totals = np.zeros(16, np.int64)
    totals[:5] = (valid.sum(), (~valid).sum(), duplicate.sum(), cancelled.sum(), F)
    totals[13] = -1
    shell = _shells(V, s)
    if F:
        u, w = np.concatenate([s[:, 0], s[:, 1], s[:, 2]]), np.concatenate([s[:, 1], s[:, 2], s[:, 0]])  # corner k -> k + 1
        fwd = u < w
        e = _ids(np.minimum(u, w), np.maximum(u, w))
        E = int(e.max()) + 1
        n_fwd, n_bwd = np.bincount(e[fwd], minlength=E), np.bincount(e[~fwd], minlength=E)
        n = n_fwd + n_bwd
        boundary, inconsistent, non_manifold = n == 1, (n == 2) & (n_fwd != 1), n >= 3
        totals[5:11] = ((shell >= 0).sum(), E, boundary.sum(), inconsistent.sum(), non_manifold.sum(), (n_fwd != n_bwd).sum())
        for cls, bit in ((boundary, BOUNDARY), (inconsistent, INCONSISTENT), (non_manifold, NON_MANIFOLD)):
            flags[sidx[cls[e].reshape(3, F).any(axis=0)]] |= bit
        labels, sizes = np.unique(shell[s[:, 0]], return_counts=True)  # sorted by label: argmax takes the smallest label of a tie
        best = int(np.argmax(sizes))
        totals[11:14] = (len(labels), sizes[best], labels[best])
    return dict(totals=totals, flags=flags, vertex_shell=shell.astype(np.int32))


def clean(vertices, triangles, min_shell_triangles=0, largest_only=False):
    """dict(vertices [V',3] f32 -- the input bits --, triangles [T',3] int32, vertex_map [V] int32, triangle_map [T] int32)."""
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    tri, _, survivor, _, _ = _status(v, triangles)
    V, T = len(v), len(tri)
    shell = _shells(V, tri[survivor])
    keep_t = survivor.copy()
    if survivor.any():
        of = shell[tri[survivor][:, 0]]
        labels, sizes = np.unique(of, return_counts=True)
        size_of = np.zeros(V, np.int64)
        size_of[labels] = sizes
        ok = size_of[of] >= int(min_shell_triangles)
        if largest_only:
            ok &= of == labels[int(np.argmax(sizes))]
        keep_t[survivor] = ok
    keep_v = np.zeros(V, bool)
    keep_v[tri[keep_t].reshape(-1)] = True
    vmap = np.where(keep_v, np.cumsum(keep_v) - 1, -1).astype(np.int32)
    tmap = np.where(keep_t, np.cumsum(keep_t) - 1, -1).astype(np.int32)
    return dict(vertices=v[keep_v].copy(), triangles=vmap[tri[keep_t]].astype(np.int32).reshape(-1, 3), vertex_map=vmap, triangle_map=tmap)


def named(totals):
    """The totals as the dict pvd.mesh.mesh_topology returns: the names, euler, closed, manifold."""
    d = {k: int(x) for k, x in zip(NAMES, totals)}
    d["euler"] = d["referenced"] - d["edges"] + d["survivors"]
    d["closed"] = d["unbalanced"] == 0
    d["manifold"] = not (d["boundary"] or d["inconsistent"] or d["non_manifold"] or d["duplicate"] or d["cancelled"])
    return d


# ------------------------------------------------------------------ inputs the CPU and the GPU tests share
TET = np.array([(0, 2, 1), (0, 1, 3), (1, 2, 3), (0, 3, 2)], np.int32)  # closed and consistently wound
ROTATIONS = ((0, 1, 2), (1, 2, 0), (2, 0, 1))
GROUPS = ((1, 0), (2, 0), (0, 3), (1, 1), (2, 1), (1, 2), (2, 2), (3, 1))  # (p, m)
EDGE_CLASSES = ((1, 0), (0, 1), (1, 1), (2, 0), (0, 2), (2, 1), (1, 2), (3, 0), (2, 2))  # (n_fwd, n_bwd)


def points(n, seed=0):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (n, 3)).astype(np.float32)


def group_cases(seed=0):
    """(vertices, triangles, expected): one group per (p, m) of GROUPS on three vertices of its own, the members' corner orders
    cycling through the three rotations, even and odd interleaved and shuffled; expected[i] = (p, m, indices of the group, the
    survivor's index or -1)."""
    rng = np.random.default_rng(seed)
    rows, owner = [], []
    for gi, (p, m) in enumerate(GROUPS):
        a, b, c = 3 * gi, 3 * gi + 1, 3 * gi + 2
        for j in range(p):
            rows.append([(a, b, c)[i] for i in ROTATIONS[j % 3]])
            owner.append((gi, True))
        for j in range(m):
            rows.append([(a, c, b)[i] for i in ROTATIONS[(j + 1) % 3]])
            owner.append((gi, False))
    order = rng.permutation(len(rows))
    tri = np.array(rows, np.int32)[order]
    owner = [owner[i] for i in order]
    expected = []
    for gi, (p, m) in enumerate(GROUPS):
        members = [i for i, (g, _) in enumerate(owner) if g == gi]
        evens, odds = [i for i in members if owner[i][1]], [i for i in members if not owner[i][1]]
        expected.append((p, m, members, min(evens) if p > m else (min(odds) if m > p else -1)))
    return points(3 * len(GROUPS), seed), tri, expected


def edge_cases():
    """(vertices, triangles, classes): for every (n_fwd, n_bwd) of EDGE_CLASSES an edge {a < b} of its own with that many triangles
    (a, b, apex) and (b, a, apex), every apex a vertex of its own -- all other edges are boundary edges."""
    rows, nv = [], 0
    for nf, nb in EDGE_CLASSES:
        a, b = nv, nv + 1
        nv += 2
        for j in range(nf + nb):
            rows.append((a, b, nv) if j < nf else (b, a, nv))
            nv += 1
    return points(nv, 1), np.array(rows, np.int32), EDGE_CLASSES


def strip(n, order="ascending", seed=0):
    """A strip of n triangles in a row over n + 2 vertices, consistently wound; the vertex indices ascending along the strip,
    descending, or shuffled."""
    V = n + 2
    k = np.arange(n)
    tri = np.where((k % 2 == 0)[:, None], np.stack([k, k + 1, k + 2], axis=1), np.stack([k + 1, k, k + 2], axis=1))
    pos = np.stack([(np.arange(V) // 2).astype(np.float32), (np.arange(V) % 2).astype(np.float32), np.zeros(V, np.float32)], axis=1)
    perm = {"ascending": np.arange(V), "descending": np.arange(V)[::-1], "shuffled": np.random.default_rng(seed).permutation(V)}[order]
    v = np.empty_like(pos)
    v[perm] = pos
    return v, perm[tri].astype(np.int32)


def tetrahedra(n, seed=0):
    """n disjoint closed tetrahedra, their vertex indices shuffled over the whole mesh."""
    perm = np.random.default_rng(seed).permutation(4 * n)
    tri = (TET[None, :, :] + 4 * np.arange(n)[:, None, None]).reshape(-1, 3)
    return points(4 * n, seed), perm[tri].astype(np.int32)


def fan(k, seed=0):
    """A closed fan of k triangles (0, 1 + i, 1 + (i + 1) % k) around vertex 0: a triangle bucket of k entries and an edge bucket of
    2 k entries under vertex 0."""
    i = np.arange(k)
    return points(k + 1, seed), np.stack([np.zeros(k, np.int64), 1 + i, 1 + (i + 1) % k], axis=1).astype(np.int32)


def extracted(name):
    """(vertices, triangles) of tests/mesh_restatement.py's level sets in the box [-1, 1]^3."""
    import mesh_restatement as mr
    field = {"sphere": lambda: mr.sphere_field(12), "torus": lambda: mr.torus_field(16), "two_spheres": lambda: mr.two_spheres_field(16)}[name]()
    return mr.extract(field, 0.0, np.full(3, -1.0, np.float32), np.full(3, 1.0, np.float32))


def clustered(name):
    """(vertices, triangles) of tests/mesh_simplify_restatement.py's clustering: sphere R=12 at G=3, torus R=24 at G=9, two
    spheres R=24 at G=5."""
    import mesh_restatement as mr
    import mesh_simplify_restatement as sr
    field, G = {"sphere": (lambda: mr.sphere_field(12), 3), "torus": (lambda: mr.torus_field(24), 9),
                "two_spheres": (lambda: mr.two_spheres_field(24), 5)}[name]
    lo, hi = np.full(3, -1.0, np.float32), np.full(3, 1.0, np.float32)
    v, t = mr.extract(field(), 0.0, lo, hi)
    small = sr.simplify(v, t, lo, hi, G)
    return small["vertices"], small["triangles"]
