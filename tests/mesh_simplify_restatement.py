"""Uniform-grid vertex clustering, restated in plain numpy from the definition in include/pvd_hip_mesh_simplify.h (not from the
kernels: the cells are grouped with np.unique, nothing is scanned): what csrc/mesh_simplify.hip is compared with, bit for bit, in
tests/test_hip_mesh_simplify.py, and what tests/test_mesh_simplify_restatement.py pins first.  int64 sums, float64 finalisation.
"""
import os
import re

import numpy as np

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pvd_hip_mesh_simplify.h")
ONE = 1 << 30


def header_bound_terms():
    """The two constants of PVD_MESH_SIMPLIFY_BOUND, read from the header: e / G + quant * e + round * max(|lo|, |hi|)."""
    src = re.sub(r"\\\n", " ", open(HEADER).read())
    m = re.search(r"#define PVD_MESH_SIMPLIFY_BOUND\(e, G, lo, hi\)\s+\(\(e\) / \(double\)\(G\) \+ (0x1p-\d+) \* \(e\) \+\s+(0x1p-\d+) \* \(", src)
    assert m, "PVD_MESH_SIMPLIFY_BOUND is not where the tests read it"
    return float.fromhex(m.group(1)), float.fromhex(m.group(2))


def bound(bmin, bmax, G):
    """The header's displacement bound per axis, float64 [3] (0 on a flat axis, where nothing is promised)."""
    lo, hi = np.asarray(bmin, np.float32).astype(np.float64), np.asarray(bmax, np.float32).astype(np.float64)
    quant, rnd = header_bound_terms()
    with np.errstate(invalid="ignore"):
        e = hi - lo
        ok = (e > 0) & np.isfinite(e)
        return np.where(ok, e / G + quant * e + rnd * np.maximum(np.abs(lo), np.abs(hi)), 0.0)


def quantise(vertices, bmin, bmax):
    """(valid [V] bool, q [V,3] int64 -- 0 for rows that are not valid --, e [3] float64, flat [3] bool)."""
    v = np.asarray(vertices, np.float32).reshape(-1, 3).astype(np.float64)
    lo, hi = np.asarray(bmin, np.float32).astype(np.float64), np.asarray(bmax, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        e = hi - lo
        flat = ~((e > 0) & np.isfinite(e))
    valid = np.isfinite(v).all(axis=1)
    q = np.zeros(v.shape, np.int64)
    for a in range(3):
        if not flat[a]:
            f = np.clip((v[valid, a] - lo[a]) / e[a], 0.0, 1.0)
            q[valid, a] = np.rint(f * float(ONE)).astype(np.int64)  # rint: ties to even
    return valid, q, e, flat


def cells(q, G):
    k = np.minimum(G - 1, (q * G) >> 30)
    return (k[:, 0] * G + k[:, 1]) * G + k[:, 2]


def quantise_attrs(attrs):
    a = np.asarray(attrs, np.float32).astype(np.float64)
    fin = np.isfinite(a)
    return np.where(fin, np.rint(np.clip(np.where(fin, a, 0.0), -1.0, 1.0) * float(ONE)), 0.0).astype(np.int64)


def simplify(vertices, triangles, bmin, bmax, G, attrs=None):
    """dict(vertices [V',3] f32, attrs [V',K] f32 | None, triangles [T',3] int32, vertex_map [V] int32, survives [T] bool,
    n [V'] int64, S [V',3] int64, A [V',K] int64 | None)."""
    vertices = np.asarray(vertices, np.float32).reshape(-1, 3)
    tri = np.asarray(triangles, np.int32).reshape(-1, 3).astype(np.int64)
    V, G = vertices.shape[0], int(G)
    lo = np.asarray(bmin, np.float32).astype(np.float64)
    valid, q, e, flat = quantise(vertices, bmin, bmax)
    cell = np.where(valid, cells(q, G), -1)

    inside = ((tri >= 0) & (tri < V)).all(axis=1)
    safe = np.where(inside[:, None], tri, 0)
    tc = cell[safe] if V else np.full(tri.shape, -1, np.int64)
    ok = inside & (tc >= 0).all(axis=1)
    survives = ok & (tc[:, 0] != tc[:, 1]) & (tc[:, 1] != tc[:, 2]) & (tc[:, 0] != tc[:, 2])

    kept = np.unique(tc[survives])  # ascending linear index
    at = np.minimum(np.searchsorted(kept, cell), max(len(kept) - 1, 0))
    vertex_map = (np.where(kept[at] == cell, at, -1) if len(kept) else np.full(V, -1)).astype(np.int32).reshape(V)
    member = vertex_map >= 0
    Vn = len(kept)
    n = np.zeros(Vn, np.int64)
    S = np.zeros((Vn, 3), np.int64)
    np.add.at(n, vertex_map[member], 1)
    np.add.at(S, vertex_map[member], q[member])
    A = None
    if attrs is not None:
        qa = quantise_attrs(np.asarray(attrs, np.float32).reshape(V, -1))
        A = np.zeros((Vn, qa.shape[1]), np.int64)
        np.add.at(A, vertex_map[member], qa[member])

    nd = n.astype(np.float64)
    out = np.empty((Vn, 3), np.float32)
    for a in range(3):
        if flat[a]:
            out[:, a] = np.asarray(bmin, np.float32)[a]
        else:
            out[:, a] = (lo[a] + (S[:, a].astype(np.float64) / nd) * (e[a] * 2.0 ** -30)).astype(np.float32)
    out_attrs = None if A is None else ((A.astype(np.float64) / nd[:, None]) * 2.0 ** -30).astype(np.float32)
    out_tri = vertex_map[safe[survives]].astype(np.int32).reshape(-1, 3)
    return dict(vertices=out, attrs=out_attrs, triangles=out_tri, vertex_map=vertex_map, survives=survives, n=n, S=S, A=A)


# ------------------------------------------------------------------ inputs the CPU and the GPU tests share
def sphere_mesh(R=12, radius=0.6):
    """(vertices f32, triangles int32, lo, hi) of tests/mesh_restatement.py's sphere in the box [-1, 1]^3."""
    import mesh_restatement as mr
    lo, hi = np.full(3, -1.0, np.float32), np.full(3, 1.0, np.float32)
    v, t = mr.extract(mr.sphere_field(R, radius), 0.0, lo, hi)
    return v, t, lo, hi


def sphere_attrs(vertices, K):
    """K = 3: unit normals (radial); K = 6: normals and a colour in [0, 1]."""
    v = np.asarray(vertices, np.float64)
    nrm = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
    if K == 0:
        return None
    if K == 3:
        return nrm
    assert K == 6
    return np.concatenate([nrm, (0.5 + 0.5 * np.sin(3.0 * v)).astype(np.float32)], axis=1)


def finite_box(vertices):
    """pvd.mesh._finite_box in numpy: the bounding box of the finite rows, the unit box where there is none."""
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    ok = np.isfinite(v).all(axis=1)
    if not ok.any():
        return np.zeros(3, np.float32), np.ones(3, np.float32)
    return v[ok].min(axis=0), v[ok].max(axis=0)


def soup(V=1000, T=3000, seed=0, dirty=True, K=0):
    """A random triangle soup in roughly [-1.2, 1.2]^3; dirty: indices -1 and V, NaN / +-inf vertices, and (K > 0) attributes that
    are not finite or outside [-1, 1]."""
    rng = np.random.default_rng(seed)
    v = rng.uniform(-1.2, 1.2, (V, 3)).astype(np.float32)
    t = rng.integers(0, max(V, 1), (T, 3)).astype(np.int32)
    a = rng.uniform(-1.0, 1.0, (V, K)).astype(np.float32) if K else None
    if dirty and V >= 16 and T >= 16:
        v[3, 0], v[5, 1], v[7, 2], v[9] = np.nan, np.inf, -np.inf, np.nan
        t[0, 0], t[1, 1], t[2, 2], t[4] = -1, V, -5, (V, V + 1, 2 ** 31 - 1)
        t[6], t[8] = (3, 10, 11), (12, 12, 13)
        if K:
            a[0, 0], a[1, K - 1], a[2, 0], a[11, 0], a[12, K - 1], a[13, 0] = np.nan, np.inf, -np.inf, 3.5, -2.0, 1.0
    return v, t, a
