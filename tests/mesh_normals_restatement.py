"""Vertex normals of the marching-tetrahedra mesh, restated in plain numpy from the description in include/pvd_hip_mesh_attr.h (not
from the kernel): what pvd_mesh_normals (csrc/mesh.hip) is compared with in tests/test_hip_mesh_normals.py, and what
tests/test_mesh_normals_restatement.py pins first.  Built on mesh_restatement.topology (vertex order: owner, slot) and SLOTS.

Per lattice point q and axis a, with c = q's index along a:  d_a = (u[q+e_a] - u[q-e_a]) * 0.5 inside, u[q+e_a] - u[q] at c == 0,
u[q] - u[q-e_a] at c == R-1;  g_a = d_a * inv_h_a,  inv_h_a = (R-1) / (bmax_a - bmin_a).  Per vertex on the edge A -> B at
t = (thresh - u_A) / (u_B - u_A):  G_a = g_a(A) + t * (g_a(B) - g_a(A)),  len = sqrt(G_x^2 + G_y^2 + G_z^2) summed left to right,
n = -G / len, and n = 0 where len is 0 or not finite.  Every operation is one numpy operation of `dtype`, so rounded on its own.
"""
import numpy as np

import mesh_restatement as mr


def lattice_gradient(u, inv_h, dtype):
    """g [R,R,R,3] in `dtype`: the world gradient at every lattice point."""
    u = np.asarray(u, np.float32).astype(dtype)
    R = u.shape[0]
    g = np.empty(u.shape + (3,), dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        for a in range(3):
            v = np.moveaxis(u, a, 0)
            d = np.empty_like(v)
            d[0] = v[1] - v[0]
            d[R - 1] = v[R - 1] - v[R - 2]
            if R > 2:
                d[1:R - 1] = (v[2:] - v[:R - 2]) * dtype(0.5)
            g[..., a] = np.moveaxis(d, 0, a) * inv_h[a]
    return g


def normals(u, thresh, bmin, bmax, dtype=np.float32):
    """(n [V,3], S [V,3], length [V]) in `dtype` arithmetic on the SAME float32 inputs: the normal of every vertex in the order of
    mesh_restatement.topology, S_a = |g_a(A)| + |g_a(B)| (the magnitudes the interpolation along the edge is made of: what its
    rounding errors scale with), and len."""
    u = np.asarray(u, np.float32)
    R = u.shape[0]
    owners, slots, _ = mr.topology(u, thresh)
    lo, hi = np.asarray(bmin, np.float32).astype(dtype), np.asarray(bmax, np.float32).astype(dtype)
    inv_h = dtype(R - 1) / (hi - lo)
    g = lattice_gradient(u, inv_h, dtype).reshape(-1, 3)
    d = np.asarray(mr.SLOTS, np.int64)[slots].reshape(-1, 3)
    p = np.stack([owners // (R * R), (owners // R) % R, owners % R], axis=1)
    other = ((p[:, 0] + d[:, 0]) * R + p[:, 1] + d[:, 1]) * R + p[:, 2] + d[:, 2]
    flat = u.reshape(-1)
    ua, ub, th = flat[owners].astype(dtype), flat[other].astype(dtype), dtype(np.float32(thresh))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        t = (th - ua) / (ub - ua)
        ga, gb = g[owners], g[other]
        G = ga + t[:, None] * (gb - ga)
        length = np.sqrt(G[:, 0] * G[:, 0] + G[:, 1] * G[:, 1] + G[:, 2] * G[:, 2])
        ok = np.isfinite(length) & (length > 0)
        n = np.where(ok[:, None], -G / length[:, None], dtype(0))
        S = np.abs(ga) + np.abs(gb)
    assert n.dtype == dtype and S.dtype == dtype and length.dtype == dtype
    return n, S, length


def smooth_field(R, seed):
    """A sum of four products of sines with seeded frequencies, phases and weights (the smooth field of tests/test_hip_mesh.py)."""
    rng = np.random.RandomState(seed)
    X, Y, Z = mr.grid(R)
    u = np.zeros_like(X)
    for _ in range(4):
        f, ph = rng.uniform(0.5, 3.0, 3), rng.uniform(0, 2 * np.pi, 3)
        u += rng.uniform(0.3, 1.0) * np.sin(f[0] * X + ph[0]) * np.sin(f[1] * Y + ph[1]) * np.sin(f[2] * Z + ph[2])
    return u.astype(np.float32)


def field(kind, R, thresh):
    """The fields tests/test_hip_mesh.py meshes, rebuilt: the surface is the level set `thresh`."""
    thresh = np.float32(thresh)
    if kind == "sphere":
        u = mr.sphere_field(R)
    elif kind == "torus":
        u = mr.torus_field(R)
    elif kind == "two_spheres":
        u = mr.two_spheres_field(R)
    elif kind == "smooth":
        u = smooth_field(R, 7)
    elif kind == "plane":  # u == thresh on the whole layer i = (R - 1) // 2; the gradient is (0.5 * inv_h_x, 0, 0) everywhere
        i = np.arange(R, dtype=np.float32)[:, None, None]
        return np.broadcast_to((i - (R - 1) // 2) * np.float32(0.5) + thresh, (R, R, R)).astype(np.float32).copy()
    elif kind == "nan":
        u = smooth_field(R, 11)
        u[np.random.RandomState(R).uniform(size=u.shape) < 0.02] = np.nan
    elif kind == "far_spheres":  # two small spheres, one cut by the face x = 1: vertices owned by points of the last layer
        u = mr.two_spheres_field(R, 0.12, (-0.8, -0.75, -0.7), (1.0, 0.75, 0.7))
    else:
        raise KeyError(kind)
    return (u + thresh).astype(np.float32)


def bound(S, length, eps=2.0 ** -24):
    """[V,3]: the error a float32 evaluation of the chain may have against the exact one, per vertex and axis (derivation:
    tests/test_hip_mesh_normals.py).  S and length are the float64 restatement's."""
    S, length = np.asarray(S, np.float64), np.asarray(length, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        s2 = np.sqrt((S * S).sum(axis=1))
        return eps * ((14.0 * S + 14.0 * s2[:, None]) / length[:, None] + 4.0) * 1.001
