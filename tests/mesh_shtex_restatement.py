"""csrc/pvd_hip_mesh_shtex.h restated in numpy, float32, operation for operation: the basis, the mirrored query direction of the bake,
the projection with its batch split, and the sample (the addressing is mesh_tex_restatement's).  numpy rounds every float32 operation on
its own, which is what the header asks of the kernels.  Pinned by tests/test_mesh_shtex_restatement.py; tests/test_hip_mesh_shtex.py
compares the kernels with it bit for bit.  Also here: the same real spherical harmonics in float64 from their definition (Legendre
polynomials), the reference the basis is pinned against, and a host bake built from the pieces."""
import math

import numpy as np

import mesh_tex_restatement as mt

F32 = np.float32
MAX_L = 4


def _f(a):
    return np.asarray(a, F32)


def basis(dirs, L):
    """[N, L*L] float32 of dirs [N,3]: the header's sixteen polynomials, as given (nothing is normalised)."""
    assert 1 <= int(L) <= MAX_L
    d = _f(dirs).reshape(-1, 3)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    with np.errstate(all="ignore"):
        Y = [np.full(len(d), F32(0.282094806), F32)]
        if L > 1:
            Y += [F32(-0.488602519) * y, F32(0.488602519) * z, F32(-0.488602519) * x]
        if L > 2:
            xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
            Y += [F32(1.09254849) * xy, F32(-1.09254849) * yz, F32(0.946174681) * zz - F32(0.31539157), F32(-1.09254849) * xz,
                  F32(0.546274245) * (xx - yy)]
        if L > 3:
            Y += [F32(-0.590043604) * (y * (F32(3.0) * xx - yy)), F32(2.89061141) * (xy * z),
                  (F32(0.457045794) - F32(2.28522897) * zz) * y, (F32(1.86588168) * zz - F32(1.11952901)) * z,
                  (F32(0.457045794) - F32(2.28522897) * zz) * x, F32(1.44530571) * (z * (xx - yy)),
                  F32(-0.590043604) * (x * (xx - F32(3.0) * yy))]
    out = np.stack(Y, 1)
    assert out.dtype == F32 and out.shape[1] == L * L
    return out


def basis64_terms(dirs, L):
    """(Y [N,K] float64, largest [N,K] float64): the real spherical harmonics of the float32 directions as given, from their definition
    in float64 -- Y_lm = N_lm Q_l^|m|(z) {Re, Im}(x + i y)^|m| with Q_l^m the m-th derivative of the Legendre polynomial P_l, the
    Condon-Shortley sign (-1)^m and N_lm = sqrt((2l + 1) / (4 pi) (l - |m|)! / (l + |m|)!) (times sqrt 2 for m != 0) -- and the largest
    absolute monomial of each expanded polynomial."""
    from numpy.polynomial import legendre, polynomial
    d = np.asarray(dirs, np.float64).reshape(-1, 3)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    Y = np.zeros((len(d), L * L))
    big = np.zeros((len(d), L * L))
    for l in range(L):
        P = legendre.leg2poly([0.0] * l + [1.0])  # P_l in powers of z
        for m in range(-l, l + 1):
            a = abs(m)
            Q = polynomial.polyder(P, a) if a else P
            N = math.sqrt((2 * l + 1) / (4.0 * math.pi) * math.factorial(l - a) / math.factorial(l + a)) * (math.sqrt(2.0) if a else 1.0)
            N *= (-1.0) ** a
            zs = [N * q * z ** e for e, q in enumerate(Q) if q != 0.0]  # the monomials in z
            # the monomials of Re / Im (x + i y)^a: binom(a, b) x^(a-b) (i y)^b
            ws = []
            for b in range(a + 1):
                if (b % 2 == 0) == (m >= 0):  # even powers of i y are real, odd ones imaginary
                    sign = (-1.0) ** (b // 2)
                    ws.append(sign * math.comb(a, b) * x ** (a - b) * y ** b)
            k = l * l + l + m
            for zt in zs:
                for wt in ws:
                    Y[:, k] += zt * wt
                    big[:, k] = np.maximum(big[:, k], np.abs(zt * wt))
    return Y, big


def mirrored(n, U):
    """d [J,M,3] float32: the header's query directions of the normals n [M,3] and the fitting directions U [J,3]."""
    n, U = _f(n).reshape(-1, 3), _f(U).reshape(-1, 3)
    nx, ny, nz = n[:, 0], n[:, 1], n[:, 2]
    out = np.empty((len(U), len(n), 3), F32)
    with np.errstate(all="ignore"):
        q = (nx * nx + ny * ny) + nz * nz
        for j, (ux, uy, uz) in enumerate(U):
            s = (ux * nx + uy * ny) + uz * nz
            flip = (s > 0) & np.isfinite(q) & (q > 0)
            r = (F32(2.0) * s) / q
            for c, (u, nc) in enumerate(((ux, nx), (uy, ny), (uz, nz))):
                out[j, :, c] = np.where(flip, u - r * nc, u)
    return out


def project(rgb, P, coef=None):
    """coef [M,K,3] float32 after the directions of rgb [J,M,3] with the columns P [K,J]; coef=None starts from +0."""
    rgb, P = _f(rgb), _f(P)
    J, M = rgb.shape[:2]
    K = P.shape[0]
    assert P.shape == (K, J)
    acc = np.zeros((M, K, 3), F32) if coef is None else _f(coef).copy()
    with np.errstate(all="ignore"):
        for j in range(J):
            acc = acc + P[None, :, j, None] * rgb[j][:, None, :]
    assert acc.dtype == F32
    return acc


def project_batched(rgb, P, batch):
    """project over the D directions, `batch` at a time, storing and reloading the accumulators."""
    coef = None
    for j0 in range(0, rgb.shape[0], batch):
        coef = project(rgb[j0:j0 + batch], np.ascontiguousarray(P[:, j0:j0 + batch]), coef)
    return coef


def clamp01(c):
    with np.errstate(all="ignore"):
        return np.fmin(np.fmax(_f(c), F32(0)), F32(1))


def sample(texture, T, S, L, tri, bary, dirs, bg):
    """color [N,3] float32: the header's sample of texture [Ht,Wt,K,3] float32."""
    tex = _f(texture)
    _, _, Wt, Ht = mt.layout(T, S)
    K = L * L
    assert tex.shape == (Ht, Wt, K, 3)
    tri = np.asarray(tri, np.int64).reshape(-1)
    xs, ys, _, (tx, ty) = mt.touched(T, S, tri, bary)
    out = np.empty((len(tri), 3), F32)
    out[:] = _f(bg).reshape(3)
    hit = xs[:, 0] >= 0
    xs, ys, tx, ty = xs[hit], ys[hit], tx[hit][:, None], ty[hit][:, None]
    Y = basis(_f(dirs).reshape(-1, 3)[hit], L)
    c = []
    with np.errstate(all="ignore"):
        for e in range(4):
            t = tex[ys[:, e], xs[:, e]]  # [n,K,3]
            acc = t[:, 0] * Y[:, 0, None]
            for k in range(1, K):
                acc = acc + t[:, k] * Y[:, k, None]
            c.append(acc)
        sx, sy = F32(1) - tx, F32(1) - ty
        out[hit] = clamp01((c[0] * sx + c[1] * tx) * sy + (c[2] * sx + c[3] * tx) * ty)
    return out


def fit_matrix(dirs, L):
    """P [K,D] float32: the pseudo-inverse of the float32 basis at dirs [D,3], taken in float64 and rounded once."""
    return np.linalg.pinv(basis(dirs, L).astype(np.float64)).astype(F32)


def bake(source, vertices, triangles, S, L, dirs, normals=None, batch=8):
    """texture [Ht,Wt,K,3] float32 of the callable source(x [M,3], d [M,3]) -> [M,3] on the host: mesh_tex_restatement's points, the
    mirrored directions, the projection in batches; unowned and invalid texels get zeros and never reach the source."""
    T = len(np.asarray(triangles).reshape(-1, 3))
    _, _, Wt, Ht = mt.layout(T, S)
    x, n = mt.points(vertices, triangles, S, normals=normals)
    good = np.isfinite(x).all(1) & np.isfinite(n).all(1)
    U, P = _f(dirs).reshape(-1, 3), fit_matrix(dirs, L)
    d = mirrored(n[good], U)
    rgb = np.stack([_f(source(x[good], d[j])) for j in range(len(U))])
    coef = np.zeros((len(x), L * L, 3), F32)
    coef[good] = project_batched(rgb, P, batch)
    return coef.reshape(Ht, Wt, L * L, 3)


# ------------------------------------------------------------------------------------------------ the planar recovery case
# Two triangles in the plane z = 0 with the normal +z, and a source in the span at L = 3 that is even across the plane (no odd power of dz):
# the mirrored bake must recover it, and a lookup must return it for every direction that sees the plane (dz < 0).
PLANE_V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]], F32)
PLANE_T = np.array([[0, 1, 2], [1, 3, 2]], np.int32)
PLANE_A = np.array([0.30, 0.45, 0.20])
PLANE_B = np.array([0.25, 0.10, 0.30])
PLANE_C = np.array([0.15, -0.10, 0.05])


def plane_colour(d):
    """[M,3] float64 of directions d [M,3]: a + b dz^2 + c dx per channel (inside [0, 1] for unit d)."""
    d = np.asarray(d, np.float64)
    return PLANE_A[None, :] + PLANE_B[None, :] * (d[:, 2] ** 2)[:, None] + PLANE_C[None, :] * d[:, 0][:, None]


def fit_bound(P, rgb, D):
    """[K,3] float64: (D + 2) 2^-24 sum_j |P_kj| |rgb_jc| -- how far a float32 projection of the float32 rgb [D,3] with the float32
    P [K,D] can lie from the float64 fit: D roundings of the running sum (the product's folded into P's and rgb's own two)."""
    return (D + 2) * 2.0 ** -24 * (np.abs(np.asarray(P, np.float64)) @ np.abs(np.asarray(rgb, np.float64)))


def sample_bound(bound, coef, Y):
    """[N,3] float64: fit_bound carried through the K-term dot of the sample for the basis rows Y [N,K] and one texel's coef [K,3]:
    sum_k bound_kc |Y_k|, plus (K + 12) 2^-24 sum_k |coef_kc Y_k| for the basis' own 8 ulps, the K roundings of the dot and the four of
    the bilinear mix of equal texels."""
    Y, coef = np.abs(np.asarray(Y, np.float64)), np.abs(np.asarray(coef, np.float64))
    return Y @ np.asarray(bound, np.float64) + (Y.shape[1] + 12) * 2.0 ** -24 * (Y @ coef)


def look_at(eye, target):
    """[4,4] float32 cam2world of a camera at eye whose +z axis (the viewing direction of pvd.scene.get_rays) points at target."""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    fwd = (target - eye) / np.linalg.norm(target - eye)
    right = np.cross([0.0, 1.0, 0.0] if abs(fwd[1]) < 0.9 else [1.0, 0.0, 0.0], fwd)
    right /= np.linalg.norm(right)
    up = np.cross(fwd, right)
    pose = np.eye(4)
    pose[:3, 0], pose[:3, 1], pose[:3, 2], pose[:3, 3] = right, up, fwd, eye
    return pose.astype(F32)
