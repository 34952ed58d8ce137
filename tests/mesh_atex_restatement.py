"""csrc/pvd_hip_mesh_atex.h restated in numpy, float32, operation for operation: the class of a triangle, its rank, slot / order / totals,
the layout, the point and normal of every texel, the corner coordinates and the bilinear lookup.  The arithmetic inside a cell is
mesh_tex_restatement's (weights, _mix, valid, _texel): the header says it is the uniform atlas's with S = S_c and the rank for f.  Pinned by
tests/test_mesh_atex_restatement.py; tests/test_hip_mesh_atex.py compares the kernels with it bit for bit."""
import numpy as np

import mesh_tex_restatement as tr

F32 = np.float32
CELLS = (4, 8, 16, 32, 64)
STEPS = tuple(s - 3 for s in CELLS)  # m_c
MAX_SIDE, MAX_T = 16384, 2 ** 28 - 1
TOTALS = ("count_0", "count_1", "count_2", "count_3", "count_4", "capped")
NAN = tr.NAN


def _len2(a, b):
    u = (b - a).astype(F32)
    return ((u[:, 0] * u[:, 0]).astype(F32) + (u[:, 1] * u[:, 1]).astype(F32)).astype(F32) + (u[:, 2] * u[:, 2]).astype(F32)


def classes(vertices, triangles, density, max_class=4):
    """(c uint32 [T], capped bool [T], q float32 [T]): the header's class of every triangle; q is 0 for an invalid one."""
    v, t = np.asarray(vertices, F32).reshape(-1, 3), np.asarray(triangles, np.int64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        rho2 = F32(density) * F32(density)
    if not (F32(density) > 0 and np.isfinite(rho2) and rho2 > 0):
        raise ValueError("density")
    if not 0 <= int(max_class) <= 4:
        raise ValueError("max_class")
    ok = tr.valid(v, t)
    ts = np.where(ok[:, None], t, 0)
    q = np.zeros(len(t), F32)
    if len(t) and len(v):
        with np.errstate(all="ignore"):
            A, B, C = v[ts[:, 0]], v[ts[:, 1]], v[ts[:, 2]]
            L2 = np.fmax(np.fmax(_len2(A, B), _len2(A, C)), _len2(B, C))
            q = np.where(ok, (L2 * rho2).astype(F32), F32(0)).astype(F32)
    c0 = sum((q > F32(m * m)).astype(np.uint32) for m in STEPS[:4]) if len(t) else np.zeros(0, np.uint32)
    c0 = np.asarray(c0, np.uint32)
    capped = ok & ((c0 > max_class) | (q > F32(3721)))
    return np.minimum(c0, np.uint32(max_class)).astype(np.uint32), capped, q


def build(vertices, triangles, density, max_class=4):
    """(slot uint32 [T], order uint32 [T], totals uint32 [6]): a stable counting sort by class."""
    c, capped, _ = classes(vertices, triangles, density, max_class)
    T = len(c)
    counts = np.bincount(c, minlength=5).astype(np.uint32)
    order = np.argsort(c, kind="stable").astype(np.uint32)
    base = np.concatenate([[0], np.cumsum(counts)[:4]]).astype(np.int64)
    rank = np.empty(T, np.uint32)
    rank[order] = (np.arange(T, dtype=np.int64) - base[c[order]]).astype(np.uint32)
    slot = (c << np.uint32(28)) | rank
    return slot.astype(np.uint32), order, np.concatenate([counts, [capped.sum()]]).astype(np.uint32)


def layout(counts):
    """dict(Wt, Ht, y0, rows, C, count, base); ValueError where the header says PVD_ERR_UNSUPPORTED."""
    counts = [int(c) for c in counts]
    assert len(counts) == 5
    if sum(counts) > MAX_T:
        raise ValueError("T")
    cells = [(n + 1) // 2 for n in counts]
    area = sum(k * s * s for k, s in zip(cells, CELLS))
    Wt = 64
    while Wt * Wt < area:
        Wt += 64
        if Wt > MAX_SIDE:
            raise ValueError("side")
    C = [Wt // s for s in CELLS]
    rows = [-(-k // cc) for k, cc in zip(cells, C)]
    y0, y = [], 0
    for r, s in zip(rows, CELLS):
        y0.append(y)
        y += r * s
    if y > MAX_SIDE:
        raise ValueError("side")
    base = [sum(counts[:i]) for i in range(5)]
    return dict(Wt=Wt, Ht=y if y else 4, y0=y0, rows=rows, C=C, count=counts, base=base, area=area)


def layout_words(counts):
    """The 17 words pvd_mesh_atex_layout writes."""
    lay = layout(counts)
    return [lay["Wt"], lay["Ht"]] + lay["y0"] + lay["rows"] + lay["C"]


def owners(counts, order):
    """(f, p, q, S) [Ht,Wt] int64: the owner of every texel (-1 where nothing owns it), its (p, q) and its cell edge."""
    lay = layout(counts)
    Wt, Ht = lay["Wt"], lay["Ht"]
    order = np.asarray(order, np.int64)
    f = np.full((Ht, Wt), -1, np.int64)
    p, q, Sc = np.zeros((Ht, Wt), np.int64), np.zeros((Ht, Wt), np.int64), np.full((Ht, Wt), 4, np.int64)
    x = np.arange(Wt, dtype=np.int64)[None, :]
    for c, S in enumerate(CELLS):
        h = lay["rows"][c] * S
        if not h:
            continue
        yy = np.arange(h, dtype=np.int64)[:, None]
        k = (yy // S) * lay["C"][c] + x // S
        i, j = x % S, yy % S
        lower = i + j <= S - 1
        rank = np.where(lower, 2 * k, 2 * k + 1)
        own = rank < lay["count"][c]
        band = slice(lay["y0"][c], lay["y0"][c] + h)
        f[band] = np.where(own, order[np.where(own, lay["base"][c] + rank, 0)] if len(order) else -1, -1)
        p[band], q[band], Sc[band] = np.where(lower, i, S - 1 - i), np.where(lower, j, S - 1 - j), S
    return f, p, q, Sc


def points(vertices, triangles, counts, order, normals=None, row0=0, row1=None):
    """(x, n) [(row1 - row0) * Wt, 3] float32 of the image rows row0 .. row1 - 1."""
    v, t = np.asarray(vertices, F32).reshape(-1, 3), np.asarray(triangles, np.int64).reshape(-1, 3)
    lay = layout(counts)
    row1 = lay["Ht"] if row1 is None else row1
    assert 0 <= row0 <= row1 <= lay["Ht"] and sum(lay["count"]) == len(t)
    f, p, q, S = (a[row0:row1].reshape(-1) for a in owners(counts, order))
    x = np.full((len(f), 3), NAN, F32)
    n = np.full((len(f), 3), NAN, F32)
    if len(t) == 0 or len(f) == 0:
        return x, n
    ok = np.zeros(len(f), bool)
    ok[f >= 0] = tr.valid(v, t, normals)[f[f >= 0]]
    f, p, q, S = f[ok], p[ok], q[ok], S[ok]
    m = (S - 3).astype(F32)
    beta, gamma = p.astype(F32) / m, q.astype(F32) / m
    al, be, ga = (((F32(1) - beta) - gamma)[:, None], beta[:, None], gamma[:, None])
    with np.errstate(all="ignore"):
        A, B, Cc = v[t[f, 0]], v[t[f, 1]], v[t[f, 2]]
        x[ok] = tr._mix(al, be, ga, A, B, Cc)
        if normals is not None:
            nn = np.asarray(normals, F32).reshape(-1, 3)
            n[ok] = tr._mix(al, be, ga, nn[t[f, 0]], nn[t[f, 1]], nn[t[f, 2]])
        else:
            u, w = B - A, Cc - A
            n[ok] = np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2],
                              u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], 1)
    return x, n


def _slot_fields(counts, slot):
    lay = layout(counts)
    slot = np.asarray(slot, np.int64) & 0xffffffff
    c, rank = slot >> 28, slot & 0x0fffffff
    good = (c < 5)
    cs = np.where(good, c, 0)
    good &= rank < np.asarray(lay["count"], np.int64)[cs]
    return lay, cs, rank, good, np.asarray(CELLS, np.int64)[cs], np.asarray(lay["C"], np.int64)[cs], np.asarray(lay["y0"], np.int64)[cs]


def corner_texels(counts, slot):
    """[T,3,2] int64: the integer texel (x, y) whose centre is the corner a, b, c of every triangle."""
    _, _, rank, good, S, C, y0 = _slot_fields(counts, slot)
    assert good.all()
    k, odd = rank // 2, (rank % 2) == 1
    ax, ay = (k % C) * S + np.where(odd, S - 1, 0), y0 + (k // C) * S + np.where(odd, S - 1, 0)
    step = np.where(odd, -1, 1) * (S - 3)
    return np.stack([np.stack([ax, ay], 1), np.stack([ax + step, ay], 1), np.stack([ax, ay + step], 1)], 1)


def uv(counts, slot):
    """[T,3,2] float64 in the OBJ convention: (X / Wt, 1 - Y / Ht)."""
    lay = layout(counts)
    c = corner_texels(counts, slot).astype(np.float64) + 0.5
    return np.stack([c[..., 0] / lay["Wt"], 1.0 - c[..., 1] / lay["Ht"]], -1)


def touched(T, counts, slot, tri, bary):
    """(xs, ys [N,4] int64, (tx, ty) float32): the four texels c00, c10, c01, c11 every row reads (-1 where it reads nothing)."""
    tri = np.asarray(tri, np.int64).reshape(-1)
    bary = np.asarray(bary, F32).reshape(-1, 2)
    hit = (tri >= 0) & (tri < T)
    _, _, rank, good, S, C, y0 = _slot_fields(counts, np.asarray(slot)[np.where(hit, tri, 0)] if T else np.zeros(len(tri), np.int64))
    hit &= good
    m = (S - 3).astype(F32)

    def texel(w):
        with np.errstate(all="ignore"):
            fu = np.fmin(np.fmax(w * m, F32(0)), m)
        i0 = np.minimum(np.floor(fu).astype(np.int64), S - 3)
        return i0, fu - i0.astype(F32)
    i0, tx = texel(bary[:, 0])
    j0, ty = texel(bary[:, 1])
    k, odd = rank // 2, (rank % 2) == 1
    cx, cy = k % C, k // C
    P = np.stack([i0, i0 + 1, i0, i0 + 1], 1)
    Q = np.stack([j0, j0, j0 + 1, j0 + 1], 1)
    xs = (cx * S)[:, None] + np.where(odd[:, None], S[:, None] - 1 - P, P)
    ys = (y0 + cy * S)[:, None] + np.where(odd[:, None], S[:, None] - 1 - Q, Q)
    return np.where(hit[:, None], xs, -1), np.where(hit[:, None], ys, -1), (tx, ty)


def sample(texture, T, counts, slot, tri, bary, bg):
    """color [N,3] float32: the header's sample of texture [Ht,Wt,3] float32."""
    tex = np.asarray(texture, F32)
    lay = layout(counts)
    assert tex.shape == (lay["Ht"], lay["Wt"], 3) and sum(lay["count"]) == T
    tri = np.asarray(tri, np.int64).reshape(-1)
    xs, ys, (tx, ty) = touched(T, counts, slot, tri, bary)
    out = np.empty((len(tri), 3), F32)
    out[:] = np.asarray(bg, F32).reshape(3)
    hit = xs[:, 0] >= 0
    xs, ys, tx, ty = xs[hit], ys[hit], tx[hit][:, None], ty[hit][:, None]
    c00, c10, c01, c11 = (tex[ys[:, e], xs[:, e]] for e in range(4))
    sx, sy = F32(1) - tx, F32(1) - ty
    with np.errstate(all="ignore"):
        out[hit] = (c00 * sx + c10 * tx) * sy + (c01 * sx + c11 * tx) * ty
    return out


# ------------------------------------------------------------------------------------------------ the graded fixture
# Right isosceles triangles with legs 2, 1, 1/2, ..., 1/64 inside the box [-1, 1]^3, REPEAT of each, interleaved (LEG_ORDER) so that the
# classes alternate along f.  At density 20 the longest edge (the hypotenuse, leg * sqrt 2) gives q = 800 leg^2 = 3200, 800, 200, 50,
# 12.5, 3.1, 0.78, 0.2: classes 4, 3, 3, 2, 1, 1, 0, 0 (m = 61, 29, 29, 13, 5, 5, 1, 1) and nothing capped.
LEGS = tuple(2.0 / 2 ** i for i in range(8))
LEG_ORDER = (0, 7, 1, 6, 2, 5, 3, 4)
FIXTURE_DENSITY, LEG_CLASSES, REPEAT = 20.0, (4, 3, 3, 2, 1, 1, 0, 0), 3
WAVE_K = np.array([6.4, 4.8, 0.0])  # |k| = 8, in the plane of the triangles: the colour field of the accuracy test


def fixture_leg(f):
    """The index into LEGS of triangle f of the graded fixture."""
    return LEG_ORDER[f % 8]


def graded_fixture():
    """(vertices [V,3] float32, triangles [T,3] int64): T = 8 * REPEAT, triangle f has the leg LEGS[fixture_leg(f)]; no vertex is shared
    and no two triangles overlap.  Round r lies in the plane z = -0.75 + 0.75 r: the leg-2 triangle fills the half x + y <= 0 of the
    square, the others sit along the diagonal of the other half with their right angle at (1 - leg, 1 - leg); odd rounds swap B and Cc.
    Every coordinate is a dyadic number: exact in float32."""
    verts, tris = [], []
    for r in range(REPEAT):
        z = -0.75 + 0.75 * r
        for i in LEG_ORDER:
            leg = LEGS[i]
            a = np.array([-1.0, -1.0, z]) if i == 0 else np.array([1.0 - leg, 1.0 - leg, z])
            b, c = a + [leg, 0, 0], a + [0, leg, 0]
            if r % 2:
                b, c = c, b
            tris.append([len(verts), len(verts) + 1, len(verts) + 2])
            verts += [a, b, c]
    return np.asarray(verts, F32), np.asarray(tris, np.int64)


def wave_colour(x):
    """[M,3] float64 of points [M,3]: 0.5 + 0.5 sin(k . x + phase) with |k| = 8, one phase per channel."""
    s = np.asarray(x, np.float64) @ WAVE_K
    return 0.5 + 0.5 * np.sin(s[:, None] + np.array([0.0, 1.0, 2.0])[None, :])


def random_lookups(T, per_triangle, seed):
    """(tri int32 [T * per_triangle], bary float32 [N,2]) uniformly inside every triangle."""
    rng = np.random.RandomState(seed)
    tri = np.repeat(np.arange(T, dtype=np.int32), per_triangle)
    u = rng.rand(len(tri), 2)
    flip = u.sum(1) > 1
    u[flip] = 1.0 - u[flip]
    return tri, u.astype(F32)


def lookup_points(vertices, triangles, tri, bary):
    """[N,3] float64: the surface point of every lookup, in float64 from the float32 inputs."""
    v, t = np.asarray(vertices, np.float64), np.asarray(triangles, np.int64)
    b = np.asarray(bary, np.float64)
    A, B, C = v[t[tri, 0]], v[t[tri, 1]], v[t[tri, 2]]
    return A + b[:, :1] * (B - A) + b[:, 1:] * (C - A)
