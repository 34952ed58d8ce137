"""Taubin's lambda|mu smoothing, restated in plain numpy from the definition in include/pvd_hip_mesh_smooth.h (not from the kernels:
no rows are stored, the sums go through np.add.at over the corners of the valid triangles): what csrc/mesh_smooth.hip is compared
with, bit for bit, in tests/test_hip_mesh_smooth.py, and what tests/test_mesh_smooth_restatement.py pins first.  int64 sums, float64
passes.  The input makers the two test files share are at the end.
"""
import os
import re

import numpy as np

import mesh_simplify_restatement as sr

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pvd_hip_mesh_smooth.h")
ONE = 1 << 30
OTHERS = ((1, 2), (2, 0), (0, 1))  # corner k of a triangle contributes these two to the row of its vertex


def header_bound_terms():
    """The two constants of PVD_MESH_SMOOTH_BOUND, read from the header: quant * e + round * max(|lo|, |hi|)."""
    src = re.sub(r"\\\n", " ", open(HEADER).read())
    m = re.search(r"#define PVD_MESH_SMOOTH_BOUND\(e, lo, hi\)\s+\((0x1p-\d+) \* \(e\) \+ (0x1p-\d+) \* \(", src)
    assert m, "PVD_MESH_SMOOTH_BOUND is not where the tests read it"
    return float.fromhex(m.group(1)), float.fromhex(m.group(2))


def bound(bmin, bmax):
    """The header's round-trip bound per axis, float64 [3] (0 on a flat axis, where nothing is promised)."""
    lo, hi = np.asarray(bmin, np.float32).astype(np.float64), np.asarray(bmax, np.float32).astype(np.float64)
    quant, rnd = header_bound_terms()
    with np.errstate(invalid="ignore"):
        e = hi - lo
        ok = (e > 0) & np.isfinite(e)
        return np.where(ok, quant * e + rnd * np.maximum(np.abs(lo), np.abs(hi)), 0.0)


def rows(vertices, triangles, bmin, bmax):
    """(valid [V] bool, q [V,3] int64, e, flat, tri [T',3] int64 -- the valid triangles --, n [V] int64 -- the row sizes)."""
    vertices = np.asarray(vertices, np.float32).reshape(-1, 3)
    tri = np.asarray(triangles, np.int32).reshape(-1, 3).astype(np.int64)
    V = vertices.shape[0]
    valid, q, e, flat = sr.quantise(vertices, bmin, bmax)  # the q_a of include/pvd_hip_mesh_simplify.h
    inside = ((tri >= 0) & (tri < V)).all(axis=1)
    tri = tri[inside]
    ok = valid[tri].all(axis=1) if len(tri) else np.zeros(0, bool)
    ok &= (tri[:, 0] != tri[:, 1]) & (tri[:, 1] != tri[:, 2]) & (tri[:, 0] != tri[:, 2])
    tri = tri[ok]
    n = np.zeros(V, np.int64)
    np.add.at(n, tri.reshape(-1), 2)
    return valid, q, e, flat, tri, n


def one_pass(q, tri, n, movable, w):
    """q' [V,3] int64 of one pass with weight w."""
    S = np.zeros(q.shape, np.int64)
    for k, (a, b) in enumerate(OTHERS):
        np.add.at(S, tri[:, k], q[tri[:, a]])
        np.add.at(S, tri[:, k], q[tri[:, b]])
    out = q.copy()
    m = movable
    mean = S[m].astype(np.float64) / n[m].astype(np.float64)[:, None]
    step = np.rint(np.float64(w) * (mean - q[m].astype(np.float64))).astype(np.int64)  # rint: ties to even
    out[m] = np.clip(q[m] + step, 0, ONE)
    return out


def smooth(vertices, triangles, bmin, bmax, lam, mu, iterations, pinned=None, return_state=False):
    """out_vertices [V,3] f32 (return_state: also dict(q, n, movable, totals))."""
    vertices = np.asarray(vertices, np.float32).reshape(-1, 3)
    V = vertices.shape[0]
    valid, q, e, flat, tri, n = rows(vertices, triangles, bmin, bmax)
    pin = np.zeros(V, bool) if pinned is None else (np.asarray(pinned).reshape(V) != 0)
    movable = valid & ~pin & (n > 0)
    for _ in range(int(iterations)):
        q = one_pass(q, tri, n, movable, lam)
        q = one_pass(q, tri, n, movable, mu)
    out = vertices.copy()  # the input bits, NaN payloads included
    if int(iterations) > 0:
        lo = np.asarray(bmin, np.float32).astype(np.float64)
        for a in range(3):
            if flat[a]:
                out[movable, a] = np.asarray(bmin, np.float32)[a]
            else:
                out[movable, a] = (lo[a] + q[movable, a].astype(np.float64) * (e[a] * 2.0 ** -30)).astype(np.float32)
    if return_state:
        return out, dict(q=q, n=n, movable=movable, totals=(int(n.sum()), int(n.max()) if V else 0))
    return out


# ------------------------------------------------------------------ inputs the CPU and the GPU tests share
def noisy_sphere(seed=0, amplitude=0.03):
    """(vertices f32, triangles int32, lo, hi): sphere_mesh(12) with every vertex set to the mean radius plus a uniform radial offset
    in +-amplitude."""
    v, t, lo, hi = sr.sphere_mesh(12)
    v = v.astype(np.float64)
    r = np.linalg.norm(v, axis=1)
    rng = np.random.default_rng(seed)
    new_r = r.mean() + rng.uniform(-amplitude, amplitude, len(v))
    return (v / r[:, None] * new_r[:, None]).astype(np.float32), t, lo, hi


def radii(vertices):
    """(mean, std) of the vertex radii, float64."""
    r = np.linalg.norm(np.asarray(vertices, np.float64), axis=1)
    return float(r.mean()), float(r.std())


def noisy_sphere_figures(before, taubin, laplace):
    """(std after / std before, relative change of the mean radius, share of the mean radius ten plain passes lose)."""
    (m0, s0), (m1, s1), (m2, _) = radii(before), radii(taubin), radii(laplace)
    return s1 / s0, abs(m1 - m0) / m0, (m0 - m2) / m0


def check_noisy_sphere_figures(figures):
    """The conditions of the issue: Taubin at least halves the radius std and keeps the mean radius within 0.5 %; ten plain
    Laplacian passes lose more than 5 % of it."""
    ratio, drift, shrink = figures
    print("noisy sphere: std after / before %.4f, mean radius change %.5f, plain Laplacian loses %.4f of the mean radius" % figures)
    assert ratio <= 0.5 and drift < 0.005 and shrink > 0.05, figures


def fan(k, seed=0, closed=False):
    """A hub (vertex 0) with k triangles around it: a row of 2 k entries.  Open: k + 1 rim vertices; closed: k, the last triangle
    returns to the first rim vertex.  The rim is a noisy circle, the hub sits off its plane."""
    rng = np.random.default_rng(seed)
    rim = k if closed else k + 1
    ang = np.linspace(0.0, 2.0 * np.pi, rim, endpoint=False)
    v = np.zeros((rim + 1, 3), np.float32)
    v[0] = (0.1, -0.2, 0.7)
    v[1:, 0], v[1:, 1] = np.cos(ang), np.sin(ang)
    v[1:] += rng.uniform(-0.05, 0.05, (rim, 3)).astype(np.float32)
    t = np.stack([np.zeros(k, np.int64), 1 + np.arange(k), 1 + (np.arange(k) + 1) % rim], axis=1).astype(np.int32)
    return v, t
