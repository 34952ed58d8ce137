"""include/pvd_hip_mesh_tex.h restated in numpy, float32, operation for operation: the layout, the owner of every texel, the corner
coordinates, the point and normal of every texel (pvd_mesh_tex_points) and the bilinear lookup (pvd_mesh_tex_sample).  numpy rounds every
float32 operation on its own, which is what the header asks of the kernels; np.fmax / np.fmin carry the header's NaN rule.  Pinned by
tests/test_mesh_tex_restatement.py; tests/test_hip_mesh_tex.py compares the kernels with it bit for bit."""
import numpy as np

import mesh_dist_restatement as md

F32 = np.float32
MIN_S, MAX_S, MAX_SIDE = 4, 64, 16384
NAN = np.array(0x7fc00000, np.uint32).view(F32)[()]


def layout(T, S):
    """(C, rows, Wt, Ht); ValueError where the header says PVD_ERR_UNSUPPORTED."""
    T, S = int(T), int(S)
    if not MIN_S <= S <= MAX_S:
        raise ValueError("S")
    cells = (T + 1) // 2
    C = 1
    while C * C < cells:
        C += 1
    rows = max(1, -(-cells // C))
    if C * S > MAX_SIDE or rows * S > MAX_SIDE:
        raise ValueError("side")
    return C, rows, C * S, rows * S


def owners(T, S):
    """(f, p, q) [Ht,Wt] int64: the triangle index 2k or 2k + 1 of every texel -- also where f >= T, which nothing owns -- and its
    (p, q)."""
    C, rows, Wt, Ht = layout(T, S)
    y, x = np.meshgrid(np.arange(Ht, dtype=np.int64), np.arange(Wt, dtype=np.int64), indexing="ij")
    k = (y // S) * C + (x // S)
    i, j = x % S, y % S
    lower = i + j <= S - 1
    return np.where(lower, 2 * k, 2 * k + 1), np.where(lower, i, S - 1 - i), np.where(lower, j, S - 1 - j)


def corner_texels(T, S):
    """[T,3,2] int64: the integer texel (x, y) whose centre is the corner a, b, c of every triangle."""
    C = layout(T, S)[0]
    m = S - 3
    f = np.arange(int(T), dtype=np.int64)
    k = f // 2
    cx, cy = k % C, k // C
    odd = (f % 2) == 1
    ax, ay = cx * S + np.where(odd, S - 1, 0), cy * S + np.where(odd, S - 1, 0)
    sgn = np.where(odd, -1, 1)
    return np.stack([np.stack([ax, ay], 1), np.stack([ax + sgn * m, ay], 1), np.stack([ax, ay + sgn * m], 1)], 1)


def corner_coordinates(T, S):
    """[T,3,2] float64: the corners in continuous texel units (texel centres at integer + 0.5)."""
    return corner_texels(T, S).astype(np.float64) + 0.5


def uv(T, S):
    """[T,3,2] float64 in the OBJ convention: (X / Wt, 1 - Y / Ht)."""
    _, _, Wt, Ht = layout(T, S)
    c = corner_coordinates(T, S)
    return np.stack([c[..., 0] / Wt, 1.0 - c[..., 1] / Ht], -1)


def valid(vertices, triangles, normals=None):
    """bool [T]: the rule of pvd_hip_mesh_dist.h and, with normals, the three normals finite as well."""
    v, t = np.asarray(vertices, F32).reshape(-1, 3), np.asarray(triangles, np.int64).reshape(-1, 3)
    ok = md.valid_triangles(v, t)
    if normals is not None and len(t):
        n = np.asarray(normals, F32).reshape(-1, 3)
        inr = np.all((t >= 0) & (t < len(v)), axis=1)
        ok = ok & inr & np.all(np.isfinite(n[np.where(inr[:, None], t, 0)]), axis=(1, 2))
    return ok


def _mix(wa, wb, wc, a, b, c):
    return ((wa * a).astype(F32) + (wb * b).astype(F32)).astype(F32) + (wc * c).astype(F32)


def weights(p, q, S):
    """(alpha, beta, gamma) float32 of the texels (p, q)."""
    m = F32(S - 3)
    beta, gamma = np.asarray(p).astype(F32) / m, np.asarray(q).astype(F32) / m
    return (F32(1) - beta) - gamma, beta, gamma


def points(vertices, triangles, S, normals=None, row0=0, row1=None):
    """(x, n) [(row1 - row0) * Wt, 3] float32 of the image rows row0 .. row1 - 1."""
    v, t = np.asarray(vertices, F32).reshape(-1, 3), np.asarray(triangles, np.int64).reshape(-1, 3)
    T = len(t)
    _, _, Wt, Ht = layout(T, S)
    row1 = Ht if row1 is None else row1
    assert 0 <= row0 <= row1 <= Ht
    f, p, q = (a[row0:row1].reshape(-1) for a in owners(T, S))
    x = np.full((len(f), 3), NAN, F32)
    n = np.full((len(f), 3), NAN, F32)
    if T == 0 or len(f) == 0:
        return x, n
    ok = np.zeros(len(f), bool)
    ok[f < T] = valid(v, t, normals)[f[f < T]]
    f, p, q = f[ok], p[ok], q[ok]
    al, be, ga = (w[:, None] for w in weights(p, q, S))
    with np.errstate(all="ignore"):
        A, B, Cc = v[t[f, 0]], v[t[f, 1]], v[t[f, 2]]
        x[ok] = _mix(al, be, ga, A, B, Cc)
        if normals is not None:
            nn = np.asarray(normals, F32).reshape(-1, 3)
            n[ok] = _mix(al, be, ga, nn[t[f, 0]], nn[t[f, 1]], nn[t[f, 2]])
        else:
            u, w = B - A, Cc - A
            n[ok] = np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2],
                              u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], 1)
    return x, n


def _texel(w, S):
    """(i0 int64, t float32) of one weight."""
    m = F32(S - 3)
    with np.errstate(all="ignore"):
        fu = np.fmin(np.fmax(np.asarray(w, F32) * m, F32(0)), m)
    i0 = np.minimum(np.floor(fu).astype(np.int64), S - 3)
    return i0, fu - i0.astype(F32)


def touched(T, S, tri, bary):
    """(xs, ys, wts) [N,4] int64, int64, float32: the four texels c00, c10, c01, c11 the sample of every row reads, as image coordinates,
    and their bilinear weights; rows whose tri is outside 0 .. T - 1 get -1 and 0."""
    C = layout(T, S)[0]
    tri = np.asarray(tri, np.int64).reshape(-1)
    bary = np.asarray(bary, F32).reshape(-1, 2)
    i0, tx = _texel(bary[:, 0], S)
    j0, ty = _texel(bary[:, 1], S)
    hit = (tri >= 0) & (tri < T)
    k = np.where(hit, tri, 0) // 2
    odd = (tri % 2) == 1
    cx, cy = k % C, k // C
    P = np.stack([i0, i0 + 1, i0, i0 + 1], 1)
    Q = np.stack([j0, j0, j0 + 1, j0 + 1], 1)
    xs = cx[:, None] * S + np.where(odd[:, None], S - 1 - P, P)
    ys = cy[:, None] * S + np.where(odd[:, None], S - 1 - Q, Q)
    sx, sy = F32(1) - tx, F32(1) - ty
    wts = np.stack([sx * sy, tx * sy, sx * ty, tx * ty], 1)
    return np.where(hit[:, None], xs, -1), np.where(hit[:, None], ys, -1), np.where(hit[:, None], wts, F32(0)), (tx, ty)


def sample(texture, T, S, tri, bary, bg):
    """color [N,3] float32: the header's sample of texture [Ht,Wt,3] float32."""
    tex = np.asarray(texture, F32)
    _, _, Wt, Ht = layout(T, S)
    assert tex.shape == (Ht, Wt, 3)
    tri = np.asarray(tri, np.int64).reshape(-1)
    xs, ys, _, (tx, ty) = touched(T, S, tri, bary)
    out = np.empty((len(tri), 3), F32)
    out[:] = np.asarray(bg, F32).reshape(3)
    hit = xs[:, 0] >= 0
    xs, ys, tx, ty = xs[hit], ys[hit], tx[hit][:, None], ty[hit][:, None]
    c00, c10, c01, c11 = (tex[ys[:, e], xs[:, e]] for e in range(4))
    sx, sy = F32(1) - tx, F32(1) - ty
    with np.errstate(all="ignore"):
        out[hit] = (c00 * sx + c10 * tx) * sy + (c01 * sx + c11 * tx) * ty
    return out


# ------------------------------------------------------------------------------------------------ the end-to-end job
# What a texture is for: a colour field finer than the triangles.  The sphere fixture at R = 17 (triangles of about 0.125 across) carries
# the analytic colour 0.5 + 0.5 sin(K x) per axis: K = 20 is a wavelength of 0.31, about 2.5 triangles -- vertex colours cannot follow
# it, 13 texels per triangle edge (S = 16) can.  One 64 x 64 view, the camera looking along +z from outside the box.
JOB_K, JOB_S, JOB_HW, JOB_R = 20.0, 16, 64, 17
JOB_INTRINSICS = (90.0, 90.0, 32.0, 32.0)
JOB_POSE = np.array([[1, 0, 0, 0.3], [0, 1, 0, 0.3], [0, 0, 1, -0.875], [0, 0, 0, 1]], F32)  # cam2world: 2 in front of the sphere, off axis


def job_colour(x):
    """[M,3] float64 of points [M,3]."""
    return 0.5 + 0.5 * np.sin(JOB_K * np.asarray(x, np.float64))


def job_rays():
    """(origins, dirs) [HW * HW, 3] float32 as pvd.scene.get_rays makes them for JOB_POSE (torch on the host: the same float32 ops)."""
    import torch
    from pvd.scene import get_rays
    r = get_rays(torch.from_numpy(JOB_POSE)[None], JOB_INTRINSICS, JOB_HW, JOB_HW, -1)
    return r["rays_o"].reshape(-1, 3).numpy().copy(), r["rays_d"].reshape(-1, 3).numpy().copy()


def job_errors(vertices, triangles, t, tri, bary, textured, vertex_coloured, origins, dirs):
    """(mse_textured, mse_vertex_coloured, hits): both renders [N,3] against the analytic colour at the hit points o + t d (float64), over
    the pixels that hit."""
    hit = np.asarray(tri).reshape(-1) >= 0
    point = np.asarray(origins, np.float64)[hit] + np.asarray(t, np.float64).reshape(-1)[hit, None] * np.asarray(dirs, np.float64)[hit]
    truth = job_colour(point)
    e_tex = ((np.asarray(textured, np.float64).reshape(-1, 3)[hit] - truth) ** 2).mean()
    e_vc = ((np.asarray(vertex_coloured, np.float64).reshape(-1, 3)[hit] - truth) ** 2).mean()
    return float(e_tex), float(e_vc), int(hit.sum())


def job_on_the_host():
    """The whole job in numpy: (mse_textured, mse_vertex_coloured, hits) with mesh_ray_restatement's hits, this file's points and sample,
    and the barycentric mean of the vertex colours as render_mesh takes it."""
    import mesh_ray_restatement as rr
    v, tr_ = md.fixture("sphere", JOB_R)
    T = len(tr_)
    o, d = job_rays()
    t, tri, bary = rr.first_hit(o, d, v, tr_)
    _, _, Wt, Ht = layout(T, JOB_S)
    x, _ = points(v, tr_, JOB_S)
    tex = np.where(np.isnan(x), 0.0, np.clip(job_colour(np.nan_to_num(x)), 0.0, 1.0)).astype(F32).reshape(Ht, Wt, 3)
    textured = sample(tex, T, JOB_S, tri, bary, (1.0, 1.0, 1.0))
    col = job_colour(v).astype(F32)
    idx = tr_[np.maximum(tri, 0)]
    w = np.stack([F32(1) - bary[:, 0] - bary[:, 1], bary[:, 0], bary[:, 1]], 1)
    vertex_coloured = (w[:, :, None] * col[idx]).sum(1)
    return job_errors(v, tr_, t, tri, bary, textured, vertex_coloured, o, d)
