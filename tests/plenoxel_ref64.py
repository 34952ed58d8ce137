"""A float64 restatement of the Plenoxel lookup and its SH colour head, forward and backward, with a derived per-element error bound,
the input generators that steer the kernels' register-window walk through every branch, the bookkeeping that proves they do, and a
float32 restatement of the kernels' own operation order with switchable faults (test helper, like vm_ref64.py, whose coordinate
rule, walk generator and tiling are imported, not copied).  Nothing here imports the kernel's binding.

FORMULATION.  NeRFNetwork.forward, "tensors" branch (pvd/network.py) and pvd/activation.py: with x_n the normalised point,
    h[c]    = sum_t vol[tap_t, c] w_t      trilinear grid_sample of the [1,C,D,H,W] volume, align_corners=True, zero padding,
                                           tap t = bx | by << 1 | bz << 2 at voxel (x0 + bx, y0 + by, z0 + bz), w_t = wx wy wz
    sigma_l = clamp(h[0], clip_min, clip_max);   sigma = exp(sigma_l);   rgb[c] = sigmoid(sum_k h[1 + c K2 + k] SH_k(d)),  K2 = deg^2
and the volume gradient for any subset of g_feat, g_sigma, g_sigma_l, g_rgb (g_feat together with the head's included).  The
backward is teacher-forced, as the kernel is: it takes h0_raw and rgb as inputs, the mask is clip_min <= h0_raw <= clip_max and the
trunc_exp factor exp(clamp(clamp(h0_raw), -12, 12)), so both are decided exactly by the inputs and no sample is left out.

COORDINATES are float32 by the documented rule (vm_ref64.normalise32 / coords_from_xn; axis a of the point indexes W, H, D for
a = 0, 1, 2).  Everything after that is float64 with no intermediate rounding.  SH_k are the closed-form real polynomials of bands
l < deg <= 3 (r = 1 baked in, Condon-Shortley phase), index l l + l + m.

BOUND.  With every multilinear output y come y_abs (every factor replaced by its magnitude), y_w (sum over the interpolation weights
of |d y / d w| in magnitudes) and n (contributions summed into the element, a prefilled value counted as one), and
    |kernel - ref| <= EPS32 ((K + n) y_abs + 2 (S - 1) y_w) + extra,     EPS32 = 2^-23, S = the largest axis of the volume.
One rounding is at most EPS32 / 2 relative, so K EPS32 is twice the first-order sum of K roundings (the second order is far below
the other half).  K, counted from the kernels (csrc/plenoxel.hip, built with contraction off):
    K_FEAT = 11   the weight's two products, the tap product, the eight adds of h += a_t w_t
    K_HEAD = K_FEAT + 1 + L   the SH product and the L levels of the lanes' shuffle tree (off = 1, 2, 4, 8 < K2: L = 0, 2, 4)
    K_BWD  = 9    (1 - y), its product with y, with g_rgb, with SH_k, the add onto g_feat (the density lane needs three), then the
                  weight's two products, g w_t and the add into the window
n: a sum of n terms in any order (window, then atomics) is off by at most (n - 1) EPS32 / 2 times the sum of magnitudes.
2 (S - 1): as in vm_ref64 (pos <= S - 1 comes from two rounded operations on x_n).  An element with bound 0 must be exactly 0.
`extra` holds what is not a rounding of the multilinear form:
    SH     float32 evaluation of a polynomial: SH_ROUNDINGS = 4 roundings (constant, y b1, the fused a2 / b2, the product with q) of
           at most EPS32 / 2 each on the sum of the MAGNITUDES of the polynomial's terms, SH_mag_k: EPS32 SH_ROUNDINGS SH_mag_k / 2,
           taken as EPS32 SH_ROUNDINGS SH_mag_k like K
    expf   EXPF_ULPS float32 ulps of the value (an ulp is at most EPS32 |value|).  EXPF_ULPS = 2 x the maximum measured once on the
           MI355X against numpy's float64 exp of the same float32 arguments (tests/test_hip_plenoxel_fp64.py measures it again on
           every run and fails if the constant is not twice its figure; profiles/plenoxel_fp64_pin.txt keeps both numbers)
sigma and rgb propagate h's bound b through exp and sigmoid by their derivatives, taken at the worst point of [a - b, a + b]:
    sigma: exp(sigma_l) (expm1(b) + EXPF_ULPS EPS32)
    rgb  : s'(max(|a| - b, 0)) b + EPS32 s (EXPF_ULPS (1 - s) + 2)     (s = 1 / (1 + t), t = expf(-a): d s / s = -(1 - s) d t / t; the
           add and the divide are 2 more)
In the chained test the backward reads the kernel's own h0_raw and rgb; their bounds enter `extra` through d exp = exp expm1(b) and
|d (1 - y) y| <= b.  Nothing in the bound is fitted to the kernel's output.

GENERATORS (committed seeds).  walk_case(dims, box): vm_ref64.scripted_case in voxel space (steps from {-1,0,+1}^3 plus multi-voxel
jumps, fractional part in [0.1, 0.9], each face crossed out and back by single voxels, far outside up to +-50 extents) plus short
single-axis shuttles outside and across the volume's faces, unit and asymmetric aabb.  lattice_case(dims): x = +-1, voxel centres and
one ulp either side of each face on 2^k + 1 volumes with dyadic values; channel 0 takes clip_min, clip_max and their float32
neighbours, so h0 equals each clip value exactly at some centres and lies one ulp outside at others.  corner_case(dims): samples whose
taps include the last voxel of the volume (the largest offset) and the first.

BOOKKEEPING.  move_classes() / coverage() / reachable() / assert_coverage(): from the reference's own i0 sequence and an assumed chunk
length every sample is open, same, +x, -x, +y, -y, +z, -z or jump (two axes by one voxel is a jump), crossed with the position of its
footprint (what the forward loads) and of the footprint it leaves (what the backward flushes): inside, partly outside, wholly outside.
An axis of size 1 has the single position 0, with its second tap outside.

Model32: the kernels' order in float32 -- the half-wave streams, px_move's four paths, px_close, the 24-bit and the 64-bit offset,
the lanes' shuffle tree, the head -- with switchable faults, for tests/test_plenoxel_ref64.py."""
import collections
import functools

import numpy as np
import torch

import vm_ref64 as v

EPS32 = v.EPS32
K_FEAT, K_BWD = 11, 9
SH_ROUNDINGS = 4
EXPF_ULPS = 1.53  # 2 x the measured maximum of device expf, 0.761 float32 ulp (module docstring)
CHUNKS = v.CHUNKS
AABBS = v.AABBS
CLASSES = ("open", "same", "+x", "-x", "+y", "-y", "+z", "-z", "jump")
POSITIONS = ("inside", "partly", "outside")
WALK_SEED, LATTICE_SEED, CORNER_SEED, VOLUME_SEED, GRAD_SEED, DIR_SEED = 7, 11, 19, 3, 5, 23

Val = collections.namedtuple("Val", "y b")              # float64 value and bound, same shape
Grad = collections.namedtuple("Grad", "idx y b n parts")  # voxel indices [T] (sorted), value / bound [T,C], count [T], additive parts


def channels(degree):
    return 3 * degree * degree + 1


def tree_levels(degree):
    return int(np.ceil(np.log2(degree * degree))) if degree > 1 else 0


def k_head(degree):
    return K_FEAT + 1 + tree_levels(degree)


def res_of(dims):
    """(D, H, W) -> the sizes the point's axes x, y, z index: (W, H, D)"""
    return (int(dims[2]), int(dims[1]), int(dims[0]))


def coords(xyz, aabb, dims):
    return v.coords(xyz, aabb, res_of(dims))


# ---------------------------------------------------------------------------------------------- SH, closed form
def sh_basis(dirs, degree):
    """-> (SH [M,K2], SH_mag [M,K2]) float64: the real SH polynomials of bands l < degree and the sum of their terms' magnitudes"""
    d = np.asarray(dirs, dtype=np.float64).reshape(-1, 3)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    one = np.ones_like(x)
    c0, c1, c2a, c2b, c2c, c2d = 0.28209479177387814, 0.4886025119029199, 1.0925484305920792, 0.9461746957575601, 0.31539156525252005, \
        0.5462742152960396
    Y, A = [c0 * one], [c0 * one]
    if degree > 1:
        Y += [-c1 * y, c1 * z, -c1 * x]
        A += [c1 * np.abs(y), c1 * np.abs(z), c1 * np.abs(x)]
    if degree > 2:
        Y += [c2a * x * y, -c2a * y * z, c2b * z * z - c2c, -c2a * x * z, c2d * (x * x - y * y)]
        A += [c2a * np.abs(x * y), c2a * np.abs(y * z), c2b * z * z + c2c, c2a * np.abs(x * z), c2d * (x * x + y * y)]
    assert 1 <= degree <= 3
    return np.stack(Y, 1), np.stack(A, 1)


# ---------------------------------------------------------------------------------------------- volumes
def make_volume(dims, degree, seed=VOLUME_SEED, scale0=1.0, scale=0.5):
    """float32 rows [D*H*W, C] (the channels-last storage order), channel 0 (log-density) scaled on its own"""
    g = torch.Generator().manual_seed(seed)
    vol = torch.randn(int(np.prod(dims)), channels(degree), generator=g) * scale
    vol[:, 0] *= scale0 / scale
    return vol


def logical(rows, dims):
    """rows [V,C] -> the parameter's logical shape [1,C,D,H,W] (contiguous)"""
    D, H, W = dims
    return rows.reshape(D, H, W, -1).permute(3, 0, 1, 2).unsqueeze(0).contiguous()


class DenseVol:
    def __init__(self, rows):
        self.rows = rows.detach().to("cpu", torch.float64)

    def __call__(self, idx):
        return self.rows[idx]


class SparseVol:
    """the rows of some voxels only (the large volumes): unknown voxels read as 0 and must carry weight 0"""

    def __init__(self, idx, rows):
        self.idx, order = torch.sort(idx)
        self.rows = rows.detach().to("cpu", torch.float64)[order]

    def __call__(self, idx):
        pos = torch.searchsorted(self.idx, idx).clamp_max(self.idx.numel() - 1)
        hit = self.idx[pos] == idx
        return self.rows[pos] * hit[:, None].to(torch.float64)


def taps(C, dims):
    """the eight taps: (voxel index (0 where outside), valid, weight, the weight with each of its three factors set to 1 in turn)"""
    D, H, W = (int(s) for s in dims)
    size = (W, H, D)
    out = []
    for t in range(8):
        bit = (t & 1, (t >> 1) & 1, t >> 2)
        p = [C.i0[:, a] + bit[a] for a in range(3)]
        valid = (p[0] >= 0) & (p[0] < W) & (p[1] >= 0) & (p[1] < H) & (p[2] >= 0) & (p[2] < D)
        w = [C.w1[:, a] if bit[a] else C.w0[:, a] for a in range(3)]
        vf = valid.to(torch.float64)
        idx = torch.where(valid, (p[2] * H + p[1]) * W + p[0], torch.zeros_like(p[0]))
        out.append((idx, valid, vf * w[0] * w[1] * w[2], vf * (w[1] * w[2] + w[0] * w[2] + w[0] * w[1])))
    return out


def touched(C, dims):
    """sorted voxel indices some tap of some sample reads"""
    return torch.unique(torch.cat([idx[valid] for idx, valid, _, _ in taps(C, dims)]))


# ---------------------------------------------------------------------------------------------- forward
def _vm_bound(K, n, y_abs, y_w, S):
    return EPS32 * ((K + n) * y_abs + 2.0 * (S - 1) * y_w)


def forward(C, dims, vol, degree, dirs=None, clip=(0.0, 0.0)):
    """-> {"feat": Val [M,C]} and, with dirs, {"h0_raw", "sigma_l", "sigma" [M], "rgb" [M,3], "pre" (the colours' pre-activation)}"""
    S = max(dims)
    tp = taps(C, dims)
    rows = [vol(idx) for idx, _, _, _ in tp]
    h = sum(w[:, None] * r for (_, _, w, _), r in zip(tp, rows))
    h_abs = sum(w[:, None] * r.abs() for (_, _, w, _), r in zip(tp, rows))
    h_w = sum(dw[:, None] * r.abs() for (_, _, _, dw), r in zip(tp, rows))
    out = {"feat": Val(h, _vm_bound(K_FEAT, 1.0, h_abs, h_w, S))}
    if dirs is None:
        return out
    K2 = degree * degree
    Y, Ym = (torch.from_numpy(a) for a in sh_basis(dirs, degree))
    cmin, cmax = float(np.float32(clip[0])), float(np.float32(clip[1]))
    b0 = out["feat"].b[:, 0]
    sl = h[:, 0].clamp(cmin, cmax)
    out["h0_raw"] = Val(h[:, 0], b0)
    out["sigma_l"] = Val(sl, b0)
    out["sigma"] = Val(torch.exp(sl), torch.exp(sl) * (torch.expm1(b0) + EXPF_ULPS * EPS32))
    M = h.shape[0]
    hc, hca, hcw = (t[:, 1:].reshape(M, 3, K2) for t in (h, h_abs, h_w))
    a = (hc * Y[:, None, :]).sum(-1)
    a_abs = (hca * Y.abs()[:, None, :]).sum(-1)
    a_w = (hcw * Y.abs()[:, None, :]).sum(-1)
    ba = _vm_bound(k_head(degree), 1.0, a_abs, a_w, S) + EPS32 * SH_ROUNDINGS * (hca * Ym[:, None, :]).sum(-1)
    assert float(a.abs().max()) < 80.0
    s = torch.sigmoid(a)
    near = torch.sigmoid((a.abs() - ba).clamp_min(0.0))
    out["pre"] = Val(a, ba)
    out["rgb"] = Val(s, near * (1.0 - near) * ba + EPS32 * s * (EXPF_ULPS * (1.0 - s) + 2.0))
    return out


# ---------------------------------------------------------------------------------------------- backward
def sample_gradient(degree, clip, dirs=None, h0_raw=None, rgb=None, g_feat=None, g_sigma=None, g_sigma_l=None, g_rgb=None, M=None,
                    b_h0=None, b_rgb=None):
    """d loss / d h per sample and channel: (g, g_abs, g_extra) float64 [M,C].  Without dirs only g_feat counts (the kernel's rule).
    b_h0 / b_rgb: bounds of h0_raw / rgb where they are a kernel's outputs, not exact inputs (the chained test)."""
    f64 = lambda t: None if t is None else torch.as_tensor(t).detach().to("cpu", torch.float64)
    h0_raw, rgb, g_feat, g_sigma, g_sigma_l, g_rgb = (f64(t) for t in (h0_raw, rgb, g_feat, g_sigma, g_sigma_l, g_rgb))
    Cn, K2 = channels(degree), degree * degree
    M = M if M is not None else next(t.shape[0] for t in (g_feat, h0_raw) if t is not None)
    g = torch.zeros(M, Cn, dtype=torch.float64) if g_feat is None else g_feat.clone()
    ga, ge = g.abs(), torch.zeros(M, Cn, dtype=torch.float64)
    if dirs is None:
        return g, ga, ge
    cmin, cmax = float(np.float32(clip[0])), float(np.float32(clip[1]))
    if g_sigma is not None or g_sigma_l is not None:
        mask = ((h0_raw >= cmin) & (h0_raw <= cmax)).to(torch.float64)
        if g_sigma_l is not None:
            g[:, 0] += mask * g_sigma_l
            ga[:, 0] += mask * g_sigma_l.abs()
        if g_sigma is not None:
            E = torch.exp(h0_raw.clamp(cmin, cmax).clamp(-12.0, 12.0))
            g[:, 0] += mask * g_sigma * E
            ga[:, 0] += mask * g_sigma.abs() * E
            ge[:, 0] += mask * g_sigma.abs() * E * (EXPF_ULPS * EPS32 + (0.0 if b_h0 is None else torch.expm1(b_h0)))
    if g_rgb is not None:
        Y, Ym = (torch.from_numpy(a) for a in sh_basis(dirs, degree))
        s = g_rgb * (1.0 - rgb) * rgb                                       # [M,3]
        sa = g_rgb.abs() * (1.0 - rgb).abs() * rgb.abs()
        g[:, 1:] += (s[:, :, None] * Y[:, None, :]).reshape(M, 3 * K2)
        ga[:, 1:] += (sa[:, :, None] * Y.abs()[:, None, :]).reshape(M, 3 * K2)
        ge[:, 1:] += EPS32 * SH_ROUNDINGS * (sa[:, :, None] * Ym[:, None, :]).reshape(M, 3 * K2)
        if b_rgb is not None:
            ge[:, 1:] += ((g_rgb.abs() * b_rgb)[:, :, None] * Y.abs()[:, None, :]).reshape(M, 3 * K2)
    return g, ga, ge


def scatter(C, dims, g, ga, ge, idx=None):
    """the additive parts of the volume gradient on the voxels `idx` (default: the touched ones): (idx, y, y_abs, y_w, extra, n)"""
    tp = taps(C, dims)
    if idx is None:
        idx = touched(C, dims)
    T, Cn = idx.numel(), g.shape[1]
    y, ya, yw, ex = (torch.zeros(T, Cn, dtype=torch.float64) for _ in range(4))
    n = torch.zeros(T, dtype=torch.float64)
    for vox, valid, w, dw in tp:
        sel = valid.nonzero().squeeze(1)
        if sel.numel() == 0:
            continue
        pos = torch.searchsorted(idx, vox[sel])
        assert bool((idx[pos.clamp_max(T - 1)] == vox[sel]).all())
        ws, dws = w[sel, None], dw[sel, None]
        y.index_add_(0, pos, ws * g[sel])
        ya.index_add_(0, pos, ws * ga[sel])
        yw.index_add_(0, pos, dws * ga[sel])
        ex.index_add_(0, pos, ws * ge[sel])
        n += torch.bincount(pos, minlength=T).to(torch.float64)
    return (idx, y, ya, yw, ex, n)


def add_parts(a, b):
    assert torch.equal(a[0], b[0])
    return (a[0],) + tuple(p + q for p, q in zip(a[1:], b[1:]))


def grad_of(parts, dims, prefill=None):
    """Grad of summed parts; prefill [T,C]: the values the buffer held (one more contribution each, of magnitude |prefill|)"""
    idx, y, ya, yw, ex, n = parts
    nn = n[:, None]
    if prefill is not None:
        p = prefill.detach().to("cpu", torch.float64)
        y, ya, nn = y + p, ya + p.abs(), nn + 1.0
    return Grad(idx, y, _vm_bound(K_BWD, nn, ya, yw, max(dims)) + ex, n, parts)


def backward(C, dims, degree, clip, idx=None, prefill=None, **inputs):
    g, ga, ge = sample_gradient(degree, clip, M=C.i0.shape[0], **inputs)
    return grad_of(scatter(C, dims, g, ga, ge, idx), dims, prefill)


# ---------------------------------------------------------------------------------------------- comparison
def ratio(got, val):
    """max(err / bound); an element whose bound is 0 has to be met exactly (else inf); NaN is inf"""
    y, b = val.y, val.b
    err = (torch.as_tensor(got).detach().to("cpu", torch.float64).reshape(y.shape) - y).abs()
    r = torch.where(b > 0, err / b.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    r = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), r)
    return float(r.max()) if r.numel() else 0.0


def report(label, names, gots, vals):
    rs = [ratio(g, o) for g, o in zip(gots, vals)]
    return "[plenoxel fp64] %-58s max err/bound: " % label + " ".join("%s=%.3g" % (nm, r) for nm, r in zip(names, rs)), (max(rs) if rs else 0.0)


# ---------------------------------------------------------------------------------------------- bookkeeping
def footprint_position(i0, dims):
    """0 inside (all eight taps in the volume), 1 partly outside, 2 wholly outside, per sample"""
    i0 = np.asarray(i0, np.int64)
    size = np.asarray(res_of(dims), np.int64)
    full = ((i0 >= 0) & (i0 + 1 < size)).all(1)
    none = ((i0 + 1 < 0) | (i0 >= size)).any(1)
    return np.where(full, 0, np.where(none, 2, 1))


def move_classes(i0, dims, chunk):
    """per sample: move class (index into CLASSES), position of its footprint and of the one it leaves (-1 for `open`)"""
    i0 = np.asarray(i0, np.int64)
    M = i0.shape[0]
    d = i0 - np.roll(i0, 1, 0)
    moved = (d != 0).sum(1)
    cls = np.full(M, 8, np.int64)
    cls[moved == 0] = 1
    for a in range(3):
        one = (moved == 1) & (np.abs(d[:, a]) == 1)
        cls[one & (d[:, a] == 1)] = 2 + 2 * a
        cls[one & (d[:, a] == -1)] = 3 + 2 * a
    first = (np.arange(M) % chunk) == 0
    cls[first] = 0
    pos = footprint_position(i0, dims)
    left = np.where(first, -1, np.roll(pos, 1))
    return {"class": cls, "position": pos, "left": left}


def coverage(i0, dims, chunk):
    """(counts[class, position of the footprint], counts[class, position of the footprint left]) [9,3] each"""
    mc = move_classes(i0, dims, chunk)
    a, b = np.zeros((9, 3), np.int64), np.zeros((9, 3), np.int64)
    np.add.at(a, (mc["class"], mc["position"]), 1)
    keep = mc["left"] >= 0
    np.add.at(b, (mc["class"][keep], mc["left"][keep]), 1)
    return a, b


def reachable(dims):
    """[9,3]: which (class, position) a volume admits.  An axis of size s >= 2 has both taps in for i0 in [0, s-2], one for -1 and
    s-1, none beyond; an axis of size 1 stays at i0 = 0 with its second tap outside.  So: inside needs every size >= 2, wholly
    outside some size >= 2, partly outside is always there; +-a needs size_a >= 2, a jump some size >= 2."""
    size = res_of(dims)
    mv = [s >= 2 for s in size]
    pos = np.array([all(mv), True, any(mv)])
    r = np.zeros((9, 3), bool)
    r[0] = r[1] = pos
    for a in range(3):
        r[2 + 2 * a] = r[3 + 2 * a] = pos & mv[a]
    r[8] = pos & any(mv)
    return r


def assert_coverage(i0, dims, least=8):
    """every reachable (class, position) at least `least` times under every chunk length, for the footprint entered and the one left"""
    r = reachable(dims)
    for chunk in CHUNKS:
        a, b = coverage(i0, dims, chunk)
        for c in range(9):
            for p in range(3):
                assert not r[c, p] or a[c, p] >= least, ("entered", CLASSES[c], POSITIONS[p], chunk, int(a[c, p]))
                assert not r[c, p] or c == 0 or b[c, p] >= least, ("left", CLASSES[c], POSITIONS[p], chunk, int(b[c, p]))


def describe(i0, dims, chunk, m):
    mc = move_classes(i0, dims, chunk)
    return "sample %d chunk %d phase %d i0 %s: %s, footprint %s" % (m, chunk, m % chunk, tuple(int(x) for x in i0[m]), CLASSES[mc["class"][m]],
                                                                  POSITIONS[mc["position"][m]])


# ---------------------------------------------------------------------------------------------- generators
def _shuttles(rng, res):
    """single-axis walks that vm_ref64's rays seldom take in three dimensions: along each axis, by single voxels, with the other two
    axes held -- inside, half out and wholly out -- every position held for one or two samples"""
    size = np.asarray(res, np.int64)
    out = []
    for a in range(3):
        if size[a] < 2:
            continue
        for other in ("in", "half", "out"):
            for rep in range(4):
                base = np.array([rng.integers(0, max(s - 1, 1)) for s in size])
                if other != "in":
                    cand = [b for b in range(3) if b != a and size[b] >= 2] or [a]
                    b = cand[rep % len(cand)]
                    if b != a:
                        base[b] = {"half": (-1, size[b] - 1), "out": (-3, size[b] + 1)}[other][rep // 2 % 2]
                up = list(range(-3, size[a] + 2)) if size[a] <= 12 else list(range(-3, 5)) + list(range(size[a] - 5, size[a] + 2))
                path = up + up[::-1]  # (on a long axis: one multi-voxel jump between the two faces)
                for p in path:
                    pos = base.copy()
                    pos[a] = p
                    out += [pos] * int(rng.integers(1, 3))
    return np.array(out)


def scripted_case(dims, aabb, seed):
    """-> {"xyz", "rays", "res", "aabb"} like vm_ref64.scripted_case, with the shuttles appended as one more ray"""
    res = res_of(dims)
    c = v.scripted_case(res, aabb, seed)
    rng = np.random.default_rng(seed + 1000)
    tex = _shuttles(rng, res)
    xyz = v.texels_to_xyz(rng, tex, res, aabb)
    got = v.coords(xyz, aabb, res).i0.numpy()
    multi = np.asarray(res) > 1
    assert (got[:, multi] == tex[:, multi]).all()
    M0 = c["xyz"].shape[0]
    c["xyz"] = np.ascontiguousarray(np.concatenate([c["xyz"], xyz]))
    c["rays"] = c["rays"] + [("shuttle", M0, M0 + len(xyz))]
    return c


def make_dirs(M, seed=DIR_SEED):
    """unit directions, a few of them along the axes and not quite unit (the polynomials have r = 1 baked in)"""
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((M, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    special = np.array([[1, 0, 0], [0, -1, 0], [0, 0, 1], [0.6, 0.0, -0.8], [0.3, -0.2, 0.5]])
    d[:min(M, len(special))] = special[:M]
    return np.ascontiguousarray(d.astype(np.float32))


def make_grads(M, degree, seed=GRAD_SEED):
    g = torch.Generator().manual_seed(seed)
    return {"g_feat": torch.randn(M, channels(degree), generator=g), "g_sigma": torch.randn(M, generator=g) * 0.01,
            "g_sigma_l": torch.randn(M, generator=g), "g_rgb": torch.randn(M, 3, generator=g)}


def tile_case(case, M):
    return v.tile_case(case.meta, M)


def lattice_points(dims, seed=LATTICE_SEED):
    return v.lattice_case(res_of(dims), seed)


def lattice_volume(dims, degree, clip, seed=LATTICE_SEED):
    """dyadic rows; channel 0 draws from the clip values, their float32 neighbours and a few values well inside and outside"""
    rng = np.random.default_rng(seed + 1)
    V, Cn = int(np.prod(dims)), channels(degree)
    rows = (rng.integers(-16, 17, (V, Cn)) / 8.0).astype(np.float32)
    lo, hi = np.float32(clip[0]), np.float32(clip[1])
    inf = np.float32(np.inf)
    special = np.array([lo, np.nextafter(lo, -inf), np.nextafter(lo, inf), hi, np.nextafter(hi, inf), np.nextafter(hi, -inf),
                        lo - 2, hi + 1.5, 0.25, -1.5, 3.0], np.float32)
    rows[:, 0] = special[rng.integers(0, len(special), V)]
    return torch.from_numpy(rows), special[:6]


def corner_points(dims, aabb, seed=CORNER_SEED, reps=6):
    """samples around the last and the first voxel: on every axis i0 from {size-2, size-1} (the last voxel is tap 7 ... tap 0) or
    {-1, 0}, all combinations, the two ends alternating (each change is a full reload / flush across the whole offset range)"""
    res = res_of(dims)
    size = np.asarray(res, np.int64)
    rng = np.random.default_rng(seed)
    tex = []
    for rep in range(reps):
        for m in range(8):
            bits = np.array([m & 1, (m >> 1) & 1, m >> 2])
            tex.append(size - 2 + bits)
            tex.append(-bits)
    tex = np.array(tex)
    xyz = v.texels_to_xyz(rng, tex, res, aabb)
    got = v.coords(xyz, aabb, res).i0.numpy()
    multi = size > 1
    assert (got[:, multi] == tex[:, multi]).all()
    return xyz


# ---------------------------------------------------------------------------------------------- cached cases
class Case:
    """points + directions + volume + gradients and the float64 reference of them, computed once and shared (never modified)"""

    def __init__(self, label, xyz, dims, aabb, degree, clip, rows, meta=None):
        """rows: float32 [V,C], or for a volume too large for a dense reference a function idx -> float32 [n,C]; the gradient is
        then kept on the touched voxels only (self.idx)"""
        self.label, self.dims, self.aabb, self.degree, self.clip, self.meta = label, tuple(dims), tuple(aabb), degree, tuple(clip), meta
        self.xyz = np.ascontiguousarray(xyz, dtype=np.float32)
        self.M, self.C = self.xyz.shape[0], coords(self.xyz, aabb, dims)
        self.dirs = make_dirs(self.M)
        if callable(rows):
            self.idx = touched(self.C, dims)
            self.rows, self.rows32 = None, rows
            self.vol = SparseVol(self.idx, torch.from_numpy(np.asarray(rows(self.idx.numpy()), np.float32)))
        else:
            self.idx = torch.arange(int(np.prod(dims)))
            self.rows, self.vol = rows, DenseVol(rows)
        self.grads = make_grads(self.M, degree)
        self._fwd, self._bwd = None, {}

    @property
    def fwd(self):
        if self._fwd is None:
            self._fwd = forward(self.C, self.dims, self.vol, self.degree, self.dirs, self.clip)
        return self._fwd

    def rows32(self, idx):
        return self.rows.numpy()[np.asarray(idx)]

    def forced(self):
        """the backward's float32 inputs: the reference's h0 and rgb, rounded"""
        return self.fwd["h0_raw"].y.float(), self.fwd["rgb"].y.float()

    def bwd(self, names, prefill=None):
        """Grad on every voxel for the gradient inputs `names` (a tuple out of g_feat, g_sigma, g_sigma_l, g_rgb); head inputs => dirs"""
        key = tuple(sorted(names))
        if key not in self._bwd:
            head = any(nm != "g_feat" for nm in key)
            h0, rgb = self.forced()
            kw = {nm: self.grads[nm] for nm in key}
            if head:
                kw.update(dirs=self.dirs, h0_raw=h0, rgb=rgb)
            g, ga, ge = sample_gradient(self.degree, self.clip, M=self.M, **kw)
            self._bwd[key] = scatter(self.C, self.dims, g, ga, ge, self.idx)
        return grad_of(self._bwd[key], self.dims, prefill)


CLIPS = {"narrow": ((-2.0, 7.0), 6.0), "wide": ((-15.0, 15.0), 12.0)}  # clip range, scale of channel 0


@functools.lru_cache(maxsize=32)
def walk_case(dims, box="unit", degree=3, clip="narrow"):
    c = scripted_case(dims, AABBS[box], WALK_SEED)
    rng, s0 = CLIPS[clip]
    return Case("walk %s deg%d %s %s" % ("x".join(map(str, dims)), degree, box, clip), c["xyz"], dims, AABBS[box], degree, rng,
                make_volume(dims, degree, scale0=s0), meta=c)


@functools.lru_cache(maxsize=4)
def lattice(dims=(9, 17, 33), degree=3):
    c = lattice_points(dims)
    rng = CLIPS["narrow"][0]
    rows, special = lattice_volume(dims, degree, rng)
    c["special_h0"] = special
    return Case("lattice %s deg%d unit" % ("x".join(map(str, dims)), degree), c["xyz"], dims, v.UNIT_AABB, degree, rng, rows, meta=c)


lattice_case = lattice


def corner_case(dims, box="unit", degree=1, rows=None, walk=256):
    """corner_points plus the first `walk` samples of the walk on the same volume; rows: as for Case (default: hashed_rows)"""
    xyz = np.concatenate([corner_points(dims, AABBS[box]), scripted_case(dims, AABBS[box], WALK_SEED)["xyz"][:walk]])
    Cn = channels(degree)
    return Case("corner %s deg%d %s" % ("x".join(map(str, dims)), degree, box), xyz, dims, AABBS[box], degree, CLIPS["narrow"][0],
                rows if rows is not None else (lambda idx: hashed_rows(idx, Cn) * np.float32(4.0)))


# ---------------------------------------------------------------------------------------------- the kernels' order in float32
f32 = np.float32
FAULTS = ("lost_flush_chunk", "lost_flush_M", "rename+x", "rename-x", "rename+y", "rename-y", "rename+z", "rename-z", "leave_at_new",
          "clamp_tap", "mask_lt", "no_exp_clamp", "tree_drops_last", "wrong_colour", "gfeat_ignored", "offset_mod24")


def px_chunk(M):
    chunk = 16
    while chunk < 64 and M // chunk > 2 * 256 * 16:
        chunk <<= 1
    return chunk


def is_small(dims, Cn):
    vox = int(np.prod([int(s) for s in dims]))
    return vox < (1 << 24) and vox * Cn < (1 << 32)


def sh32(dirs, degree):
    """the kernel's float32 evaluation (sh_basis.inc): a2 = fma(x, x, -(y y)), b2 = fma(x, y, y x), constants rounded to float32"""
    d = np.asarray(dirs, f32).reshape(-1, 3)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    fma = lambda a, b, c: (a.astype(np.float64) * b.astype(np.float64) + np.asarray(c, np.float64)).astype(f32)
    out = [np.full(x.shape, f32(0.28209479177387814))]
    if degree > 1:
        q = f32(-0.48860251190292)
        out += [q * y, f32(0.4886025119029199) * z, q * x]
    if degree > 2:
        z2 = z * z
        a2, b2 = fma(x, x, -(y * y)), fma(x, y, y * x)
        q1, q2 = f32(-1.0925484305920792) * z, f32(0.5462742152960396)
        out += [q2 * b2, q1 * y, fma(np.full(x.shape, f32(0.9461746957575601)), z2, f32(-0.31539156525252005)), q1 * x, q2 * a2]
    return np.stack(out, 1).astype(f32)


def hashed_rows(idx, Cn, seed=VOLUME_SEED):
    """float32 volume rows as a function of the voxel index: a volume of any size without a dense buffer"""
    i = np.asarray(idx, np.uint64)[:, None] * np.uint64(Cn) + np.arange(Cn, dtype=np.uint64)[None, :]
    h = (i + np.uint64(seed)) * np.uint64(0x9E3779B97F4A7C15)
    h ^= h >> np.uint64(29)
    h *= np.uint64(0xBF58476D1CE4E5B9)
    h ^= h >> np.uint64(32)
    return ((h >> np.uint64(40)).astype(np.float64) / float(1 << 23) - 1.0).astype(f32)  # dyadic in [-1, 1)


class Model32:
    """k_plenoxel_fwd / k_plenoxel_bwd restated sample by sample in float32 (numpy), all channels of a half-wave at once.
    vol_rows(idx array) -> float32 [n, C].  The gradient is kept sparse: {voxel index: float32 [C]} (prefill: a function of idx)."""

    def __init__(self, xyz, aabb, dims, degree, clip, vol_rows=None, dirs=None, chunk=None, fault=None, fault_stream=None):
        assert fault is None or fault in FAULTS
        self.dims, self.degree, self.fault, self.fault_stream = tuple(int(s) for s in dims), degree, fault, fault_stream
        self.Cn, self.K2 = channels(degree), degree * degree
        self.M = xyz.shape[0]
        self.chunk = chunk or px_chunk(self.M)
        self.vol_rows = vol_rows
        self.cmin, self.cmax = f32(clip[0]), f32(clip[1])
        xn = v.normalise32(xyz, aabb)
        size = np.asarray(res_of(dims), f32)
        pos = ((xn + f32(1)) / f32(2)) * (size - f32(1))
        fl = np.floor(pos)
        self.i0 = fl.astype(np.int64)
        w1, w0 = pos - fl, (fl + f32(1)) - pos
        self.w = np.stack([((w1[:, 0] if t & 1 else w0[:, 0]) * (w1[:, 1] if t & 2 else w0[:, 1])) * (w1[:, 2] if t & 4 else w0[:, 2])
                           for t in range(8)], 1).astype(f32)
        self.sh = None if dirs is None else sh32(dirs, degree)
        self.small = is_small(dims, self.Cn)
        self.grad = {}

    # -- px_inside / px_offset / px_touch
    def _inside(self, p):
        D, H, W = self.dims
        return 0 <= p[0] < W and 0 <= p[1] < H and 0 <= p[2] < D

    def _cells(self, p):
        """(voxel index per channel, channel index per channel): where the lanes' accesses of voxel p land"""
        D, H, W = self.dims
        ch = np.arange(self.Cn, dtype=np.int64)
        off = ((p[2] * H + p[1]) * W + p[0]) * self.Cn + ch
        if self.fault == "offset_mod24":
            off = off % (1 << 24)
        return off // self.Cn, off % self.Cn

    def _load(self, p):
        if not self._inside(p):
            if self.fault != "clamp_tap":
                return np.zeros(self.Cn, f32)
            D, H, W = self.dims
            p = (min(max(p[0], 0), W - 1), min(max(p[1], 0), H - 1), min(max(p[2], 0), D - 1))
        vox, ch = self._cells(p)
        if (vox == vox[0]).all() and (ch == np.arange(self.Cn)).all():
            return self.vol_rows(vox[:1])[0]
        return self.vol_rows(vox)[np.arange(self.Cn), ch]

    def _flush(self, p, a):
        if not self._inside(p):
            if self.fault != "clamp_tap":
                return
            D, H, W = self.dims
            p = (min(max(p[0], 0), W - 1), min(max(p[1], 0), H - 1), min(max(p[2], 0), D - 1))
        vox, ch = self._cells(p)
        for vx, c, val in zip(vox.tolist(), ch.tolist(), a):
            row = self.grad.get(vx)
            if row is None:
                row = self.grad[vx] = self.prefill(vx).copy()
            row[c] = f32(row[c] + val)

    @staticmethod
    def _corner(c, t):
        return (c[0] + (t & 1), c[1] + ((t >> 1) & 1), c[2] + (t >> 2))

    def _move(self, win, n, fwd):
        """px_move: win = {"c": cell or None, "a": float32 [8, C]}"""
        a = win["a"]
        if win["c"] is None:
            win["c"] = n
            for t in range(8):
                a[t] = self._load(self._corner(n, t)) if fwd else 0
            return
        c = win["c"]
        d = (n[0] - c[0], n[1] - c[1], n[2] - c[2])
        if d == (0, 0, 0):
            return
        moved = sum(x != 0 for x in d)
        slid = False
        if moved == 1:
            for ax in range(3):
                if d[ax] in (1, -1):
                    slid = True
                    bit = 1 << ax
                    plus = d[ax] == 1
                    if self.fault == "rename%s%s" % ("+" if plus else "-", "xyz"[ax]):
                        plus = not plus
                    for t in range(8):
                        leaving = (not (t & bit)) if plus else bool(t & bit)
                        if not leaving:
                            continue
                        stay = t ^ bit
                        if not fwd:
                            self._flush(self._corner(n if self.fault == "leave_at_new" else c, t), a[t])
                        a[t] = a[stay]
                        a[stay] = self._load(self._corner(n, stay)) if fwd else 0
        if not slid:
            for t in range(8):
                if fwd:
                    a[t] = self._load(self._corner(n, t))
                else:
                    self._flush(self._corner(c, t), a[t])
                    a[t] = 0
        win["c"] = n

    def _streams(self):
        return [(s0, min(self.M, s0 + self.chunk)) for s0 in range(0, self.M, self.chunk)]

    def forward(self, want_feat=True):
        M, Cn, K2 = self.M, self.Cn, self.K2
        feat = np.zeros((M, Cn), f32)
        h0, sl, sg, rgb = np.zeros(M, f32), np.zeros(M, f32), np.zeros(M, f32), np.zeros((M, 3), f32)
        for s0, s1 in self._streams():
            win = {"c": None, "a": np.zeros((8, Cn), f32)}
            for m in range(s0, s1):
                self._move(win, tuple(int(x) for x in self.i0[m]), True)
                h = np.zeros(Cn, f32)
                for t in range(8):
                    h = h + win["a"][t] * self.w[m, t]
                feat[m] = h
                if self.sh is None:
                    continue
                part = (h[1:].reshape(3, K2) * self.sh[m][None, :]).astype(f32)
                off = 1
                while off < K2:
                    nxt = part.copy()
                    for k in range(K2 - off):
                        if self.fault == "tree_drops_last" and k + off == K2 - 1:
                            continue
                        nxt[:, k] = part[:, k] + part[:, k + off]
                    part, off = nxt, off << 1
                cl = min(self.cmax, max(self.cmin, h[0]))
                h0[m], sl[m], sg[m] = h[0], cl, np.exp(f32(cl))
                rgb[m] = f32(1) / (f32(1) + np.exp(-part[:, 0]))
        return {"feat": feat, "h0_raw": h0, "sigma_l": sl, "sigma": sg, "rgb": rgb}

    def backward(self, h0_raw=None, rgb=None, g_feat=None, g_sigma=None, g_sigma_l=None, g_rgb=None, prefill=None):
        """-> {voxel: float32 [C]} of every voxel some flush reached (prefill(voxel) -> float32 [C]: what the buffer held)"""
        Cn, K2 = self.Cn, self.K2
        zero = np.zeros(Cn, f32)
        self.prefill = prefill or (lambda vx: zero)
        self.grad = {}
        n32 = lambda t: None if t is None else np.asarray(t, f32)
        h0_raw, rgb, g_feat, g_sigma, g_sigma_l, g_rgb = (n32(t) for t in (h0_raw, rgb, g_feat, g_sigma, g_sigma_l, g_rgb))
        streams = self._streams()
        for j, (s0, s1) in enumerate(streams):
            win = {"c": None, "a": np.zeros((8, Cn), f32)}
            for m in range(s0, s1):
                g = g_feat[m].copy() if g_feat is not None and not (self.fault == "gfeat_ignored" and self.sh is not None) else np.zeros(Cn, f32)
                if self.sh is not None:
                    raw = h0_raw[m]
                    gh = g_sigma_l[m] if g_sigma_l is not None else f32(0)
                    if g_sigma is not None:
                        x = min(self.cmax, max(self.cmin, raw))
                        if self.fault != "no_exp_clamp":
                            x = min(f32(12), max(f32(-12), x))
                        gh = f32(gh + g_sigma[m] * np.exp(f32(x)))
                    ok = (raw > self.cmin and raw < self.cmax) if self.fault == "mask_lt" else (raw >= self.cmin and raw <= self.cmax)
                    g[0] = g[0] + (gh if ok else f32(0))
                    if g_rgb is not None:
                        y = rgb[m] if self.fault != "wrong_colour" else np.roll(rgb[m], -1)
                        s = (g_rgb[m] * ((f32(1) - y) * y)).astype(f32)
                        g[1:] = g[1:] + (s[:, None] * self.sh[m][None, :]).reshape(-1)
                self._move(win, tuple(int(x) for x in self.i0[m]), False)
                win["a"] += g[None, :] * self.w[m][:, None]
            lost = (self.fault == "lost_flush_M" and j == len(streams) - 1) or (self.fault == "lost_flush_chunk" and j == self.fault_stream)
            if win["c"] is not None and not lost:
                for t in range(8):
                    self._flush(self._corner(win["c"], t), win["a"][t])
        return self.grad


def grad_rows(sparse, idx, Cn):
    """{voxel: row} -> float32 [len(idx), C] (0 where no flush arrived) and the voxels that are not in idx"""
    out = np.zeros((len(idx), Cn), f32)
    where = {int(vx): j for j, vx in enumerate(np.asarray(idx).tolist())}
    stray = []
    for vx, row in sparse.items():
        if vx in where:
            out[where[vx]] = row
        elif np.any(row != 0):
            stray.append(vx)
    return out, stray
