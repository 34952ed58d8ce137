"""A float64 restatement of the VM plane x line lookup, forward and backward, with a derived per-element error bound, the input
generators that steer the kernel's register-window walk through every branch, and the bookkeeping that proves they do (test helper,
like head_ref64.py).  Nothing here imports the kernel's binding or reads kernel code.

FORMULATION.  NeRFNetwork.get_sigma_feat / get_color_feat (pvd/network.py): for factor set i (mat_ids = (0,1),(0,2),(1,2), vec_ids =
2,1,0) plane_i[r] = bilinear(mat_i[r], (x[m0], x[m1])), line_i[r] = linear(vec_i[r], x[vec_id]) (grid_sample, align_corners=True, zero
padding), sigma_feat = sum_i sum_r<16 plane * line, color_prod[i*48 + r] = plane * line.

COORDINATES are float32, by the documented rule (what grid_sample itself does, and include/pvd_hip.h states):
    x_n = (2 (x - lo)) / (hi - lo) - 1;  pos = ((x_n + 1) / 2) (size - 1);  i0 = floor(pos);  w1 = pos - i0;  w0 = (i0 + 1) - pos
Everything after that is float64 with no intermediate rounding: tap values, plane and line values, products, the sigma sum and every
table gradient (vectorised index_add_, no loop over samples).

BOUND.  With every output y come
    y_abs  the same multilinear expression with every factor (table value, weight, incoming gradient) replaced by its magnitude;
    y_w    the sum, over the interpolation weights occurring in the expression, of y_abs's terms that hold that weight with the
           weight replaced by 1: sum_w |d y / d w| in magnitudes, the sensitivity to the float32 position;
    n      the number of sample contributions summed into the element (table gradients; 1 for forward outputs)
and the bound is derived, not fitted:
    |kernel - ref| <= EPS32 ((K + n) y_abs + 2 (S - 1) y_w),   K = 16, S = the largest table size of the case, EPS32 = 2^-23.
K: one contribution passes at most about 8 roundings (weight product, four tap products and three adds of the plane value, two and
one of the line value, the product, the gradient's two products and the add into the window), the sigma feature about 7 more in
the lanes' shuffle tree; doubled.  n: a sum of n terms in any order is off by at most (n - 1) eps times the sum of magnitudes.
2 (S - 1): pos <= S - 1 is the result of two rounded operations on x_n, so a float32 implementation that associates them otherwise
moves a weight by up to 2 (S - 1) eps.  f16 products add 2^-11 |ref| + 2^-25 (the final rounding, normal and subnormal range);
f16 incoming gradients are widened exactly.  An element with bound 0 (nothing contributes) must be exactly 0.

GENERATORS (all from committed seeds).  scripted_case(): rays that walk in TEXEL space by steps from {-1,0,+1}^3 plus occasional
multi-texel jumps, fractional part in [0.1, 0.9] so float32 and float64 agree on i0 -- interior only, across each of the six faces
and back by single-texel steps (i0 = -2, -1, 0 and size-2, size-1, size), and far outside (up to +-50 extents).  lattice_case():
x = +-1, texel centres and one ulp either side of each face on 2^k + 1 tables, where everything is dyadic.  hot_case(),
uniform_case(), tile_case() (cyclic repetition with the ray order reversed in every other repetition).

BOOKKEEPING.  move_classes() / coverage() classify, from the reference's own i0 sequence and an assumed chunk length, how each
sample moves each plane window (same, +x, -x, +y, -y, jump) and line window (same, +1, -1, jump), whether the old and the new
footprint are both interior, and whether the sample opens its chunk.  reachable() says which combinations a table of given sizes
admits at all (an axis of size 1 has the single position i0 = 0; an interior slide needs two interior positions, size >= 3)."""
import collections
import functools

import numpy as np
import torch

MAT_IDS = ((0, 1), (0, 2), (1, 2))
VEC_IDS = (2, 1, 0)
RS, RC = 16, 48
EPS32 = float(np.finfo(np.float32).eps)
K_ROUNDINGS = 16
UNIT_AABB = (-1.0, -1.0, -1.0, 1.0, 1.0, 1.0)
ASYM_AABB = (-0.5, -1.0, -2.0, 1.5, 1.0, 0.0)
CHUNKS = (16, 32, 64)
PLANE_CLASSES = ("same", "+x", "-x", "+y", "-y", "jump")
LINE_CLASSES = ("same", "+1", "-1", "jump")
TABLE_NAMES = ["sigma_mat%d" % i for i in range(3)] + ["sigma_vec%d" % i for i in range(3)] + \
              ["color_mat%d" % i for i in range(3)] + ["color_vec%d" % i for i in range(3)]

Out = collections.namedtuple("Out", "y y_abs y_w n")      # float64 tensors (n: float64 tensor or 1.0)
Coords = collections.namedtuple("Coords", "i0 w0 w1")     # [M,3] int64 / float64 tensors


# ---------------------------------------------------------------------------------------------- coordinates
def normalise32(xyz, aabb):
    """x_n in float32 by the documented rule."""
    x = np.ascontiguousarray(np.asarray(xyz, dtype=np.float32)).reshape(-1, 3)
    a = np.asarray(aabb, dtype=np.float32)
    lo, ext = a[:3], a[3:] - a[:3]
    xn = (np.float32(2.0) * (x - lo)) / ext - np.float32(1.0)
    assert xn.dtype == np.float32
    return xn


def coords_from_xn(xn, res, dtype=np.float32):
    """pos / i0 / weights from normalised coordinates, evaluated in `dtype` (float32: the documented rule; float64: what float64
    grid_sample does with the same x_n)."""
    xn = np.asarray(xn).astype(dtype)
    size = np.asarray(res, dtype=dtype)
    one, two = dtype(1.0), dtype(2.0)
    pos = ((xn + one) / two) * (size - one)
    fl = np.floor(pos)
    w1 = pos - fl
    w0 = (fl + one) - pos
    assert pos.dtype == dtype and w0.dtype == dtype
    return Coords(torch.from_numpy(fl.astype(np.int64)), torch.from_numpy(w0.astype(np.float64)), torch.from_numpy(w1.astype(np.float64)))


def coords(xyz, aabb, res):
    return coords_from_xn(normalise32(xyz, aabb), res, np.float32)


def take(C, rows):
    return Coords(C.i0[rows], C.w0[rows], C.w1[rows])


# ---------------------------------------------------------------------------------------------- tables
def make_tables(res, seed, scale=1.0):
    """Twelve float32 factors in the reference's logical shapes ([1,R,H,W] planes, [1,R,L,1] lines), randn."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for R in (RS, RC):
        out += [torch.randn(1, R, res[m1], res[m0], generator=g) * scale for m0, m1 in MAT_IDS]
        out += [torch.randn(1, R, res[v], 1, generator=g) * scale for v in VEC_IDS]
    return out


def _flat(t):
    """[1,R,H,W] -> [H*W, R] float64"""
    return t.detach().to("cpu", torch.float64).permute(0, 2, 3, 1).reshape(-1, t.shape[1]).contiguous()


def _plane_taps(C, i, res):
    """the four taps of plane i: (flat texel index, valid, weight, d weight: the weight with each of its two factors set to 1)"""
    ax, ay = MAT_IDS[i]
    W, H = int(res[ax]), int(res[ay])
    wx, wy = (C.w0[:, ax], C.w1[:, ax]), (C.w0[:, ay], C.w1[:, ay])
    taps = []
    for dy in (0, 1):
        for dx in (0, 1):
            x, y = C.i0[:, ax] + dx, C.i0[:, ay] + dy
            valid = (x >= 0) & (x < W) & (y >= 0) & (y < H)
            idx = y.clamp(0, H - 1) * W + x.clamp(0, W - 1)
            v = valid.to(torch.float64)
            taps.append((idx, valid, v * wx[dx] * wy[dy], v * (wx[dx] + wy[dy])))
    return taps


def _line_taps(C, i, res):
    al = VEC_IDS[i]
    L = int(res[al])
    w = (C.w0[:, al], C.w1[:, al])
    taps = []
    for d in (0, 1):
        l = C.i0[:, al] + d
        valid = (l >= 0) & (l < L)
        v = valid.to(torch.float64)
        taps.append((l.clamp(0, L - 1), valid, v * w[d], v))
    return taps


def _values(T, taps):
    """(value, magnitude form, weight sensitivity) of one interpolated factor, [M,R]"""
    A = T.abs()
    val = sum(w[:, None] * T[idx] for idx, _, w, _ in taps)
    mag = sum(w[:, None] * A[idx] for idx, _, w, _ in taps)
    sens = sum(dw[:, None] * A[idx] for idx, _, _, dw in taps)
    return val, mag, sens


def _set_values(C, tables, res, k, i):
    P = _values(_flat(tables[6 * k + i]), _plane_taps(C, i, res))
    L = _values(_flat(tables[6 * k + 3 + i]), _line_taps(C, i, res))
    return P, L


# ---------------------------------------------------------------------------------------------- forward / backward
def forward(C, tables, res):
    """-> {"sigma_feat": Out [M], "color_prod": Out [M,144]}"""
    M = C.i0.shape[0]
    sig = [torch.zeros(M, dtype=torch.float64) for _ in range(3)]
    prod = [torch.zeros(M, 3 * RC, dtype=torch.float64) for _ in range(3)]
    for k in (0, 1):
        for i in range(3):
            (P, Pa, Pw), (L, La, Lw) = _set_values(C, tables, res, k, i)
            trip = (P * L, Pa * La, Pw * La + Pa * Lw)
            for q in range(3):
                if k == 0:
                    sig[q] += trip[q].sum(1)
                else:
                    prod[q][:, i * RC:(i + 1) * RC] = trip[q]
    return {"sigma_feat": Out(sig[0], sig[1], sig[2], 1.0), "color_prod": Out(prod[0], prod[1], prod[2], 1.0)}


def _scatter(size, R, taps, terms):
    """sum over taps of index_add(idx, term(tap)) for each of the three term functions, plus the contribution count"""
    outs = [torch.zeros(size, R, dtype=torch.float64) for _ in terms]
    n = torch.zeros(size, dtype=torch.float64)
    for idx, valid, w, dw in taps:
        sel = valid.nonzero().squeeze(1)
        if sel.numel() == 0:
            continue
        for o, f in zip(outs, terms):
            o.index_add_(0, idx[sel], f(w, dw)[sel])
        n += torch.bincount(idx[sel], minlength=size).to(torch.float64)
    return outs, n


def backward(C, tables, res, g_sigma, g_prod):
    """-> list of 12 Out in the tables' order and logical shapes ([1,R,H,W] / [1,R,L,1]; n is [1,1,H,W] / [1,1,L,1])"""
    gs = g_sigma.detach().to("cpu", torch.float64)
    gp = g_prod.detach().to("cpu", torch.float64)
    grads = [None] * 12
    for k, R in ((0, RS), (1, RC)):
        for i in range(3):
            ax, ay = MAT_IDS[i]
            W, H, Ln = int(res[ax]), int(res[ay]), int(res[VEC_IDS[i]])
            (P, Pa, Pw), (L, La, Lw) = _set_values(C, tables, res, k, i)
            g = gs[:, None].expand(-1, RS) if k == 0 else gp[:, i * RC:(i + 1) * RC]
            ga = g.abs()
            (y, ya, yw), n = _scatter(H * W, R, _plane_taps(C, i, res),
                                      (lambda w, dw: w[:, None] * (g * L), lambda w, dw: w[:, None] * (ga * La),
                                       lambda w, dw: dw[:, None] * (ga * La) + w[:, None] * (ga * Lw)))
            sh = lambda t, a, b: t.reshape(a, b, -1).permute(2, 0, 1).unsqueeze(0).contiguous()
            grads[6 * k + i] = Out(sh(y, H, W), sh(ya, H, W), sh(yw, H, W), n.reshape(1, 1, H, W))
            (y, ya, yw), n = _scatter(Ln, R, _line_taps(C, i, res),
                                      (lambda w, dw: w[:, None] * (g * P), lambda w, dw: w[:, None] * (ga * Pa),
                                       lambda w, dw: dw[:, None] * (ga * Pa) + w[:, None] * (ga * Pw)))
            grads[6 * k + 3 + i] = Out(sh(y, Ln, 1), sh(ya, Ln, 1), sh(yw, Ln, 1), n.reshape(1, 1, Ln, 1))
    return grads


# ---------------------------------------------------------------------------------------------- bound and comparison
def bound(o, S, f16=False):
    b = EPS32 * ((K_ROUNDINGS + o.n) * o.y_abs + 2.0 * (S - 1) * o.y_w)
    if f16:
        b = b + 2.0 ** -11 * o.y.abs() + 2.0 ** -25
    return b


def ratio(got, o, S, f16=False, extra=None):
    """max(err / bound) of one tensor; an element whose bound is 0 has to be met exactly (else inf).  extra: added to the bound."""
    err = (got.detach().to("cpu", torch.float64).reshape(o.y.shape) - o.y).abs()
    b = bound(o, S, f16)
    if extra is not None:
        b = b + extra
    r = torch.where(b > 0, err / b.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    r = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), r)
    return float(r.max()) if r.numel() else 0.0


def report(label, names, gots, outs, S, f16=False, extras=None):
    """One line per case: max(err / bound) per output tensor.  Returns (line, worst ratio)."""
    rs = [ratio(g, o, S, f16 and nm == "color_prod", None if extras is None else extras[j]) for j, (nm, g, o) in enumerate(zip(names, gots, outs))]
    line = "%s | " % label + " ".join("%s=%.3g" % (nm, r) for nm, r in zip(names, rs))
    return line, (max(rs) if rs else 0.0)


# ---------------------------------------------------------------------------------------------- bookkeeping
def move_classes(i0, res, chunk):
    """From an i0 sequence [M,3] and a chunk length: per sample and factor set the plane / line move class, whether the previous and
    the current footprint are both interior, and whether the sample is the first of its chunk (it opens the windows: no move)."""
    i0 = np.asarray(i0, dtype=np.int64)
    M = i0.shape[0]
    size = np.asarray(res, dtype=np.int64)
    inside = (i0 >= 0) & (i0 + 1 < size)
    prev, prev_inside = np.roll(i0, 1, 0), np.roll(inside, 1, 0)
    d = i0 - prev
    first = (np.arange(M) % chunk) == 0
    pc, pi = np.zeros((M, 3), np.int64), np.zeros((M, 3), bool)
    lc, li = np.zeros((M, 3), np.int64), np.zeros((M, 3), bool)
    for i in range(3):
        ax, ay, al = MAT_IDS[i][0], MAT_IDS[i][1], VEC_IDS[i]
        dx, dy, dl = d[:, ax], d[:, ay], d[:, al]
        pc[:, i] = np.select([(dx == 0) & (dy == 0), (dy == 0) & (dx == 1), (dy == 0) & (dx == -1), (dx == 0) & (dy == 1), (dx == 0) & (dy == -1)],
                             [0, 1, 2, 3, 4], 5)
        pi[:, i] = inside[:, ax] & inside[:, ay] & prev_inside[:, ax] & prev_inside[:, ay]
        lc[:, i] = np.select([dl == 0, dl == 1, dl == -1], [0, 1, 2], 3)
        li[:, i] = inside[:, al] & prev_inside[:, al]
    return {"plane": pc, "plane_interior": pi, "line": lc, "line_interior": li, "first": first}


def coverage(i0, res, chunk):
    """counts[factor set, move class, interior] for planes [3,6,2] and lines [3,4,2], first-of-chunk samples left out"""
    mc = move_classes(i0, res, chunk)
    keep = ~mc["first"]
    cp, cl = np.zeros((3, 6, 2), np.int64), np.zeros((3, 4, 2), np.int64)
    for i in range(3):
        np.add.at(cp[i], (mc["plane"][keep, i], mc["plane_interior"][keep, i].astype(np.int64)), 1)
        np.add.at(cl[i], (mc["line"][keep, i], mc["line_interior"][keep, i].astype(np.int64)), 1)
    return cp, cl


def reachable(res):
    """Which (factor set, class, interior) combinations tables of these sizes admit.  An axis of size s has s - 1 interior positions
    (i0 in [0, s-2]); size 1 has the single position i0 = 0 (pos = 0 for every finite x), not interior, never moving."""
    ni = [max(int(s) - 1, 0) for s in res]
    mv = [int(s) >= 2 for s in res]  # the axis can move at all
    rp, rl = np.zeros((3, 6, 2), bool), np.zeros((3, 4, 2), bool)
    for i in range(3):
        ax, ay, al = MAT_IDS[i][0], MAT_IDS[i][1], VEC_IDS[i]
        rp[i, 0] = (True, ni[ax] >= 1 and ni[ay] >= 1)
        rp[i, 1] = rp[i, 2] = (mv[ax], ni[ax] >= 2 and ni[ay] >= 1)
        rp[i, 3] = rp[i, 4] = (mv[ay], ni[ay] >= 2 and ni[ax] >= 1)
        rp[i, 5] = (mv[ax] or mv[ay], (ni[ax] >= 2 and ni[ay] >= 2) or (ni[ax] >= 3 and ni[ay] >= 1) or (ni[ay] >= 3 and ni[ax] >= 1))
        rl[i, 0] = (True, ni[al] >= 1)
        rl[i, 1] = rl[i, 2] = (mv[al], ni[al] >= 2)
        rl[i, 3] = (mv[al], ni[al] >= 3)
    return rp, rl


def assert_coverage(i0, res, least=8):
    """every reachable (factor set, move class, interior / not) combination at least `least` times under every chunk length"""
    rp, rl = reachable(res)
    for chunk in CHUNKS:
        cp, cl = coverage(i0, res, chunk)
        for i in range(3):
            for c in range(6):
                for z in range(2):
                    assert not rp[i, c, z] or cp[i, c, z] >= least, ("plane", i, PLANE_CLASSES[c], "interior" if z else "border", chunk, int(cp[i, c, z]))
            for c in range(4):
                for z in range(2):
                    assert not rl[i, c, z] or cl[i, c, z] >= least, ("line", i, LINE_CLASSES[c], "interior" if z else "border", chunk, int(cl[i, c, z]))


def describe(i0, res, chunk, m):
    """bookkeeping of sample m, for a failure message"""
    mc = move_classes(i0, res, chunk)
    return "sample %d chunk %d phase %d i0 %s: " % (m, chunk, m % chunk, tuple(int(v) for v in i0[m])) + ", ".join(
        "set%d plane %s%s line %s%s" % (i, PLANE_CLASSES[mc["plane"][m, i]], "(int)" if mc["plane_interior"][m, i] else "(brd)",
                                       LINE_CLASSES[mc["line"][m, i]], "(int)" if mc["line_interior"][m, i] else "(brd)") for i in range(3))


# ---------------------------------------------------------------------------------------------- generators
_STEPS = np.array([(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1)], dtype=np.int64)
_NZ = np.abs(_STEPS).sum(1)
_STEP_P = np.where(_NZ == 0, 0.16, np.where(_NZ == 1, 0.09, 0.015))
_STEP_P = _STEP_P / _STEP_P.sum()


def _inside_range(res):
    return np.zeros(3, np.int64), np.maximum(np.asarray(res, np.int64) - 2, 0)


def _step_inside(rng, pos, res, free=(True, True, True), p_jump=0.06):
    """one step of a walk that keeps the free axes at interior positions: a step from {-1,0,1}^3 (reflected at the range's ends) or,
    now and then, a jump of one or more axes to any interior position"""
    lo, hi = _inside_range(res)
    new = pos.copy()
    if rng.random() < p_jump:
        for a in range(3):
            if free[a] and rng.random() < 0.6:
                new[a] = rng.integers(lo[a], hi[a] + 1)
        return new
    st = _STEPS[rng.choice(27, p=_STEP_P)]
    for a in range(3):
        if not free[a]:
            continue
        t = pos[a] + st[a]
        if t < lo[a] or t > hi[a]:
            t = pos[a] - st[a]
        if t < lo[a] or t > hi[a]:
            t = pos[a]
        new[a] = t
    return new


def _ray_interior(rng, res, n):
    lo, hi = _inside_range(res)
    pos = rng.integers(lo, hi + 1)
    out = []
    for _ in range(n):
        out.append(pos)
        pos = _step_inside(rng, pos, res)
    return np.array(out)


def _ray_face(rng, res, axis, high):
    """axis `axis` leaves through one face and comes back by single-texel steps (i0 = 1, 0, -1, -2 or size-3 .. size) while the
    other two axes keep walking inside; every position is held for 1..3 samples"""
    s = int(res[axis])
    path = [s - 3, s - 2, s - 1, s, s, s - 1, s - 2, s - 3] if high else [1, 0, -1, -2, -2, -1, 0, 1]
    if rng.random() < 0.5:  # now and then the way out or back is one multi-texel jump
        path = path[:1] + path[3:] if rng.random() < 0.5 else path[:5] + path[7:]
    lo, hi = _inside_range(res)
    pos = rng.integers(lo, hi + 1)
    free = tuple(a != axis for a in range(3))
    out = []
    for p in path:
        pos = pos.copy()
        pos[axis] = p
        out.append(pos)  # the crossing step itself: usually only this axis moves
        for _ in range(int(rng.integers(0, 3))):
            pos = _step_inside(rng, pos, res, free, p_jump=0.03)
            out.append(pos)
        if rng.random() < 0.3:
            pos = _step_inside(rng, pos, res, free, p_jump=0.0)  # ... sometimes the others move with it
    return np.array(out)


def _ray_far(rng, res, n):
    """long stretches outside the box, up to +-50 extents, by single steps and jumps; short visits inside between them"""
    size = np.asarray(res, np.int64)
    lo, hi = _inside_range(res)
    pos = rng.integers(lo, hi + 1)
    out = []
    while len(out) < n:
        far = pos.copy()
        for a in range(3):
            if rng.random() < 0.7:
                reach = max(50 * (int(size[a]) - 1), 3)
                far[a] = int(rng.integers(int(size[a]), reach)) if rng.random() < 0.5 else -int(rng.integers(2, reach))
                if rng.random() < 0.3:
                    far[a] = int(size[a]) if far[a] > 0 else -2  # just outside
        pos = far
        for _ in range(int(rng.integers(6, 20))):
            out.append(pos)
            pos = pos + _STEPS[rng.choice(27, p=_STEP_P)]
        pos = rng.integers(lo, hi + 1)
        for _ in range(int(rng.integers(1, 4))):
            out.append(pos)
            pos = _step_inside(rng, pos, res, p_jump=0.0)
    return np.array(out[:n])


def texels_to_xyz(rng, texels, res, aabb):
    """integer texel positions -> float32 points with a fractional part in [0.1, 0.9] per axis (an axis of size 1 has no texel
    coordinate: any point of [-1.5, 1.5] normalised)"""
    size = np.asarray(res, np.float64)
    a = np.asarray(aabb, np.float64)
    lo, ext = a[:3], a[3:] - a[:3]
    pos = texels.astype(np.float64) + rng.uniform(0.1, 0.9, texels.shape)
    xn = np.where(size > 1, 2.0 * pos / np.maximum(size - 1, 1) - 1.0, rng.uniform(-1.5, 1.5, texels.shape))
    return (lo + (xn + 1.0) / 2.0 * ext).astype(np.float32)


def scripted_case(res, aabb, seed, variants=("interior", "face", "far")):
    """-> {"xyz" [M,3] f32, "rays" [(variant, start, stop)], "res", "aabb"}; ray lengths vary so chunk boundaries meet every phase"""
    rng = np.random.default_rng(seed)
    rays = []
    if "interior" in variants:
        rays += [("interior", _ray_interior(rng, res, int(rng.integers(90, 140)))) for _ in range(10)]
    if "face" in variants:
        for rep in range(9):
            for axis in range(3):
                for high in (False, True):
                    rays.append(("face%d%s" % (axis, "+" if high else "-"), _ray_face(rng, res, axis, high)))
    if "far" in variants:
        rays += [("far", _ray_far(rng, res, int(rng.integers(150, 220)))) for _ in range(3)]
    order = rng.permutation(len(rays))
    rays = [rays[j] for j in order]
    tex = np.concatenate([r for _, r in rays])
    xyz = texels_to_xyz(rng, tex, res, aabb)
    got = coords(xyz, aabb, res).i0.numpy()
    multi = np.asarray(res) > 1
    assert (got[:, multi] == tex[:, multi]).all(), "float32 coordinates left the scripted texel"
    spans, at = [], 0
    for name, r in rays:
        spans.append((name, at, at + len(r)))
        at += len(r)
    return {"xyz": xyz, "rays": spans, "res": tuple(res), "aabb": tuple(aabb)}


def tile_case(case, M):
    """the case repeated cyclically to M rows; every other repetition has the order of its whole rays reversed, so chunk boundaries
    fall at different phases of the walk"""
    xyz, spans = case["xyz"], case["rays"]
    fwd = xyz
    rev = np.concatenate([xyz[a:b] for _, a, b in reversed(spans)])
    parts, have, j = [], 0, 0
    while have < M:
        parts.append(fwd if j % 2 == 0 else rev)
        have += len(xyz)
        j += 1
    return np.ascontiguousarray(np.concatenate(parts)[:M])


def lattice_case(res, seed, M=1536):
    """exact points of the unit box on tables of size 2^k + 1: x = +-1, texel centres, one ulp inside and outside each face"""
    for s in res:
        assert s >= 3 and (s - 1) & (s - 2) == 0, "sizes 2^k + 1"
    rng = np.random.default_rng(seed)
    one = np.float32(1.0)
    cols, special = [], []
    for s in res:
        centres = (2.0 * np.arange(s) / (s - 1) - 1.0).astype(np.float32)  # includes -1 and +1
        edge = np.array([np.nextafter(one, np.float32(0)), np.nextafter(one, np.float32(2)),
                         np.nextafter(-one, np.float32(0)), np.nextafter(-one, np.float32(-2)), one, -one], dtype=np.float32)
        cand = np.concatenate([centres, edge, edge])
        col = np.concatenate([cand, cand[rng.integers(0, len(cand), M - len(cand))]])
        cols.append(rng.permutation(col))
        special.append(edge)
    return {"xyz": np.ascontiguousarray(np.stack(cols, 1)), "res": tuple(res), "aabb": UNIT_AABB, "special": special}


def hot_case(M, aabb, point=(0.31, -0.17, 0.55)):
    """all rows at one point, like the marcher's padding rows (given in normalised coordinates)"""
    a = np.asarray(aabb, np.float64)
    p = a[:3] + (np.asarray(point) + 1.0) / 2.0 * (a[3:] - a[:3])
    return np.ascontiguousarray(np.tile(p.astype(np.float32), (M, 1)))


def uniform_case(M, aabb, seed, spread=1.1):
    rng = np.random.default_rng(seed)
    a = np.asarray(aabb, np.float64)
    xn = rng.uniform(-spread, spread, (M, 3))
    return np.ascontiguousarray((a[:3] + (xn + 1.0) / 2.0 * (a[3:] - a[:3])).astype(np.float32))


def make_grads(M, seed, f16=False):
    """incoming gradients g_sigma [M] f32 and g_prod [M,144] (f32, or f16: what the reference then reads is the widened value)"""
    g = torch.Generator().manual_seed(seed)
    gs, gp = torch.randn(M, generator=g), torch.randn(M, 3 * RC, generator=g)
    return gs, (gp.half() if f16 else gp)


# ---------------------------------------------------------------------------------------------- the float32 grid_sample formulation
def grid_sample_formulation(xn, tables, dtype):
    """sigma_feat, color_prod of the twelve F.grid_sample calls (align_corners=True, zero padding) on normalised coordinates xn [M,3],
    in `dtype` on the CPU; tables: 12 logical tensors (used as given: pass leaves that require grad for autograd)"""
    import torch.nn.functional as F
    x = torch.as_tensor(np.asarray(xn)).to(dtype)
    outs = []
    for k in (0, 1):
        per = []
        for i, (m0, m1) in enumerate(MAT_IDS):
            pc = torch.stack([x[:, m0], x[:, m1]], -1).view(1, -1, 1, 2)
            lc = torch.stack([torch.zeros_like(x[:, 0]), x[:, VEC_IDS[i]]], -1).view(1, -1, 1, 2)
            mat, vec = tables[6 * k + i], tables[6 * k + 3 + i]
            pv = F.grid_sample(mat, pc, mode="bilinear", padding_mode="zeros", align_corners=True).view(mat.shape[1], -1)
            lv = F.grid_sample(vec, lc, mode="bilinear", padding_mode="zeros", align_corners=True).view(vec.shape[1], -1)
            per.append(pv * lv)
        outs.append(torch.cat(per, 0))
    return outs[0].sum(0), outs[1].T


# ---------------------------------------------------------------------------------------------- cached cases
class Case:
    """points + tables + the float64 reference of them, computed once and shared (never modified) by the tests that need it"""

    def __init__(self, label, xyz, res, aabb, table_seed, grad_seed, meta=None):
        self.label, self.xyz, self.res, self.aabb, self.meta = label, np.ascontiguousarray(xyz, dtype=np.float32), tuple(res), tuple(aabb), meta
        self.M, self.S = self.xyz.shape[0], max(res)
        self.tables = make_tables(res, table_seed)
        self.C = coords(self.xyz, aabb, res)
        self.grad_seed = grad_seed
        self._fwd, self._bwd = None, {}

    @property
    def fwd(self):
        if self._fwd is None:
            self._fwd = forward(self.C, self.tables, self.res)
        return self._fwd

    def grads(self, f16=False):
        return make_grads(self.M, self.grad_seed, f16)

    def bwd(self, f16=False):
        if f16 not in self._bwd:
            self._bwd[f16] = backward(self.C, self.tables, self.res, *self.grads(f16))
        return self._bwd[f16]


AABBS = {"unit": UNIT_AABB, "asym": ASYM_AABB}
WALK_SEED, LATTICE_SEED, TABLE_SEED, GRAD_SEED = 7, 11, 3, 5


@functools.lru_cache(maxsize=16)
def walk_case(res, aabb_name="unit"):
    c = scripted_case(res, AABBS[aabb_name], WALK_SEED)
    return Case("walk %s %s" % ("x".join(map(str, res)), aabb_name), c["xyz"], res, AABBS[aabb_name], TABLE_SEED, GRAD_SEED, meta=c)


@functools.lru_cache(maxsize=4)
def lattice(res=(9, 17, 33)):
    c = lattice_case(res, LATTICE_SEED)
    return Case("lattice %s unit" % "x".join(map(str, res)), c["xyz"], res, UNIT_AABB, TABLE_SEED, GRAD_SEED, meta=c)
