"""float64 restatement of the hash-grid encoder's table gradient (the scatter-add of csrc/gridencoder.hip), numpy only.

What decides WHERE a contribution goes is restated exactly; everything else is float64:

  position   p = float32(fma(x, scale, 0.5 or 0)): the float64 product of two float32 values is exact, adding the offset is exact in
             float64 for all but astronomically rare inputs (checked: `positions` asserts that the float64 neighbours of the sum
             round to the same float32, so one rounding to float32 is what it computes); scale = float32(exp2f(l S) H - 1) in
             np.float32 arithmetic, exp2f as the correctly rounded float64 exp2 (tests/test_grid_ref64.py ties it to the host value
             of make_scales through the oracle's grid_level_params);
  cell/frac  cell = floor(p), frac = p - cell (exact in float32);
  bounds     dead iff x < 0 or x > 1 in any dimension, after x01 = float32(float32(x + add) / div) when an affine map is given;
  index      LevelIndex of csrc/grid_lookup.h in uint32 arithmetic: stride[d] = 0 once the running product passed the table size
             (the running product WRAPS at 2^32, as the uint32 of the kernels and of the reference does: with S = 1, H = 16 the
             levels 12 and 13 come out dense for that reason), hashed iff gridtype == 0 and s > size, `&` for power-of-two sizes
             and `%` otherwise, dense indices wrapped by `%` when they pass the size;
  weights    products of frac / 1 - frac in float64 (1 - frac is exact there);
  gradient   the f16 / f32 input value widened exactly.

Per table element: ref = sum w g, s_abs = sum |w g|, k = number of contributions, vmax = largest single |w g|.

THE BOUND (`bound`).  u = 2^-11 for f16 tables, 2^-24 for f32.  Every kernel path forms each contribution in float32: 1 - frac, the
D - 1 products of the weight and w * g are at most D + 1 <= 4 roundings of 2^-24 relative each; a run-merging kernel then sums a run
in float32 registers, which is recursive summation with the SMALLER unit 2^-24 and is covered by the gamma term below, which is
written for the coarser unit u per addition.  Then the plain kernel rounds each contribution, and a merging kernel each run sum, to
the table type (one rounding u per term), and at most k atomics add them in some order, each rounding to the table type.  Recursive
summation of k terms in any order and any grouping, each term carrying one more rounding, obeys (Higham, Accuracy and Stability,
section 4.2)

    |got - ref| <= gamma(k + 1, u) s_abs + 8 * 2^-24 s_abs + k a,        gamma(n, u) = n u / (1 - n u),

where 8 * 2^-24 s_abs bounds the float32 formation of the contributions (4 roundings, doubled for the second-order terms and the
interaction with gamma) and `a` is the absolute underflow term of one rounding to the table type: 2^-25 for f16 (half the smallest
subnormal 2^-24: gradual underflow, as half_of_product and the oracle have it; f16 additions of f16 values are exact in the subnormal
range) and 0 for f32 (2^-150 is nothing at these magnitudes).  An output buffer that already holds p adds one term: |p| joins s_abs
and k grows by one.  n u < 1/4 is asserted.  Nothing in here is fitted to a measured ratio.

EXACT CASES (`exact_case`).  S = 1 makes the scales 16 * 2^l - 1, so a position m/4 has p = 4 m 2^l - m/4 + 1/2: frac is 1/2, 1/4, 0
or 3/4 on EVERY level, the weights are multiples of 4^-D and with g = +-1, +-2 every contribution is a multiple of q = 4^-D.  As long
as an element's s_abs stays <= 2048 q (f16) or 2^24 q (f32), every partial sum of any subset in any order is an integer below 2^11
(2^24) times q, hence exactly representable, and the GPU result must equal ref bit for bit: the merging logic is checked without any
tolerance.  Both conditions are asserted from the reference itself.

SCRIPTED RUNS (`script`).  One sample sequence that contains, on the one-lane-per-sample mapping (waves of 64 samples, workgroups of
256: k_grid_bwd_coarse, k_grid_bwd) and on the two-lanes-per-sample mapping (lanes of equal parity form the scan, i.e. waves of 32
samples, workgroups of 128: k_grid_bwd_lps2), the run shapes listed in `FEATURES`; `coverage` finds them again from the reference's
own keys.  Two x-corners of one sample can never share a row: hashed, x and x + 1 differ in bit 0 before the mask (prime 1, sizes
are multiples of 8); dense or tiled, they differ by stride 1 modulo a size of at least 8.  `coverage` checks that this stays so.
"""
import numpy as np

PRIMES = (1, 2654435761, 805459861)
M32 = 0xFFFFFFFF
U16, U32 = 2.0 ** -11, 2.0 ** -24


# ------------------------------------------------------------------------------------------------ geometry
def level_scales(L, S, H):
    """float32(exp2f(l S) H - 1), as make_scales (csrc/grid_lookup.h) computes it on the host"""
    l = np.arange(L, dtype=np.float32)
    e = np.exp2((l * np.float32(S)).astype(np.float64)).astype(np.float32)  # exp2f of the float32 product, correctly rounded
    return (e * np.float32(H) - np.float32(1.0)).astype(np.float32)


def level_offsets(D, L, per_level_scale, H, log2_hashmap_size, align=False):
    """gridencoder.grid.level_offsets restated (that module imports torch)"""
    offs, o = [], 0
    for i in range(L):
        res = int(np.ceil(H * per_level_scale ** i))
        side = res if align else res + 1
        n = min(2 ** log2_hashmap_size, side ** D)
        offs.append(o)
        o += int(np.ceil(n / 8) * 8)
    offs.append(o)
    return np.array(offs, np.int32)


def positions(x, scale, align):
    """p = float32(fma(x, scale, align ? 0 : 0.5)) -> (cell uint32 as int64, frac float64)"""
    prod = x.astype(np.float64) * np.float64(scale)  # exact: 24 x 24 bits
    s = prod + (0.0 if align else 0.5)
    p = s.astype(np.float32)
    lo, hi = np.nextafter(s, -np.inf).astype(np.float32), np.nextafter(s, np.inf).astype(np.float32)
    inexact = (s - (0.0 if align else 0.5)) != prod
    assert not np.any(inexact & ((lo != p) | (hi != p))), "a position sits on a float32 rounding tie that float64 cannot decide"
    cell = np.floor(p)
    frac = (p - cell).astype(np.float64)  # exact in float32
    return cell.astype(np.int64), frac


def level_index(pg, size, resolution, gridtype, align):
    """LevelIndex<D>::init + operator() of grid_lookup.h in uint32 arithmetic; pg [..., D] int64 -> rows int64"""
    D = pg.shape[-1]
    size = int(size)
    s, stride = 1, []
    for d in range(D):
        if s <= size:
            stride.append(s)
            s = (s * (resolution if align else resolution + 1)) & M32
        else:
            stride.append(0)
    hashed = gridtype == 0 and s > size
    pg = pg.astype(np.uint64)
    idx = np.zeros(pg.shape[:-1], np.uint64)
    if hashed:
        for d in range(D):
            idx ^= (pg[..., d] * np.uint64(PRIMES[d])) & np.uint64(M32)
        idx = idx & np.uint64(size - 1) if size & (size - 1) == 0 else idx % np.uint64(size)
    else:
        for d in range(D):
            idx = (idx + pg[..., d] * np.uint64(stride[d])) & np.uint64(M32)
        idx = np.where(idx >= size, idx % np.uint64(size), idx)
    return idx.astype(np.int64), hashed


class Geometry:
    """rows [L, B, 2^D] (level-local, -1 for dead samples) and weights [L, B, 2^D] float64 of every corner of every sample"""

    def __init__(self, x, offsets, S, H, D, gridtype, align, affine=None):
        x = np.ascontiguousarray(x, np.float32)
        assert x.shape[1] == D
        if affine is not None:
            x = ((x + np.float32(affine[0])) / np.float32(affine[1])).astype(np.float32)
        self.x01, self.D, self.L, self.B = x, D, len(offsets) - 1, x.shape[0]
        self.offsets = np.asarray(offsets, np.int64)
        self.live = ~((x < 0) | (x > 1)).any(1)
        self.scales = level_scales(self.L, S, H)
        nc = 1 << D
        self.rows = np.full((self.L, self.B, nc), -1, np.int64)
        self.w = np.zeros((self.L, self.B, nc), np.float64)
        self.hashed = []
        xl = x[self.live]
        for l in range(self.L):
            scale = self.scales[l]
            res = int(np.ceil(np.float64(scale))) + 1
            cell, frac = positions(xl, scale, align)
            size = self.offsets[l + 1] - self.offsets[l]
            for idx in range(nc):
                bits = np.array([(idx >> d) & 1 for d in range(D)])
                w = np.prod(np.where(bits[None, :] == 1, frac, 1.0 - frac), axis=1)
                r, hashed = level_index(cell + bits[None, :], size, res, gridtype, align)
                self.rows[l, self.live, idx] = r
                self.w[l, self.live, idx] = w
            self.hashed.append(hashed)


class Ref:
    """the reference of one case.  Kept on the touched elements only (idx: their flat positions row * C + c, ascending; t_ref, t_s_abs,
    t_k, t_vmax: their values); ref, s_abs, k and vmax are the same per table element, [rows, C], zero where nothing lands"""

    def _dense(self, t, dtype=np.float64):
        out = np.zeros(self.n_rows * self.C, dtype)
        out[self.idx] = t
        return out.reshape(self.n_rows, self.C)

    ref = property(lambda self: self._dense(self.t_ref))
    s_abs = property(lambda self: self._dense(self.t_s_abs))
    k = property(lambda self: self._dense(self.t_k, np.int64))
    vmax = property(lambda self: self._dense(self.t_vmax))


def backward(grad, x, offsets, S, H, D, C, gridtype, align, table_dtype, affine=None, geometry=None):
    """float64 table gradient of grad [L, B, C] (values of table_dtype) at positions x [B, D]: Ref, with the flat contribution list
    (elem, val, level, b, corner) behind it"""
    geo = geometry if geometry is not None else Geometry(x, offsets, S, H, D, gridtype, align, affine)
    L, B, nc = geo.rows.shape
    g = np.asarray(grad)
    assert g.dtype == np.dtype(table_dtype) and g.shape == (L, B, C)
    g = g.astype(np.float64)  # exact widening
    lv, bb, cc = np.nonzero(geo.rows >= 0)
    rows = geo.rows[lv, bb, cc] + geo.offsets[lv]
    val = geo.w[lv, bb, cc][:, None] * g[lv, bb, :]  # [N, C]
    elem = rows[:, None] * C + np.arange(C)[None, :]
    r = Ref()
    r.geo, r.C, r.n_rows, r.dtype = geo, C, int(geo.offsets[-1]), np.dtype(table_dtype)
    r.elem, r.val = elem.ravel(), val.ravel()
    r.level, r.b, r.corner = (np.repeat(a, C) for a in (lv, bb, cc))
    r.idx, r.slot = np.unique(r.elem, return_inverse=True)
    r.t_ref, r.t_s_abs, r.t_k, r.t_vmax = accumulate(r.slot, r.val, len(r.idx))
    return r


def accumulate(slot, val, n):
    ref = np.bincount(slot, weights=val, minlength=n)
    s_abs = np.bincount(slot, weights=np.abs(val), minlength=n)
    k = np.bincount(slot, minlength=n)
    vmax = np.zeros(n)
    np.maximum.at(vmax, slot, np.abs(val))
    return ref, s_abs, k, vmax


def _touched(r, a):
    return None if a is None else np.asarray(a).reshape(-1)[r.idx]


def bound(r, prefill=None, a=None):
    """the per-element bound of the module docstring on the touched elements (r.idx); prefill: what the output buffer held before, [rows, C]"""
    f16 = r.dtype == np.float16
    u = U16 if f16 else U32
    if a is None:
        a = 2.0 ** -25 if f16 else 0.0
    k, s_abs = r.t_k.astype(np.float64), r.t_s_abs
    if prefill is not None:
        k = k + 1
        s_abs = s_abs + np.abs(_touched(r, prefill).astype(np.float64))
    n = k + 1
    assert n.max() * u < 0.25, "k too large for the bound: n u = %g" % (n.max() * u)
    return (n * u / (1 - n * u)) * s_abs + 8 * U32 * s_abs + k * a


def sensitive_fraction(r, prefill=None):
    """share of the touched elements in which ONE dropped contribution (the largest) would break the bound; f32: among the elements
    whose largest contribution is not negligible (vmax > 2^-20 s_abs)"""
    bd = bound(r, prefill)
    sel = np.ones(len(r.idx), bool)
    if r.dtype == np.float32:
        s_abs = r.t_s_abs if prefill is None else r.t_s_abs + np.abs(_touched(r, prefill).astype(np.float64))  # |prefill| joins s_abs
        sel = r.t_vmax > 2.0 ** -20 * s_abs
    assert sel.any()
    return float((r.t_vmax[sel] > 2 * bd[sel]).mean()), int(sel.sum())


def assert_sensitive(case):
    frac, n = sensitive_fraction(case.ref, case.prefill)
    need = 0.9 if case.ref.dtype == np.float16 else 1.0
    assert frac >= need, "%s: only %.3f of %d touched elements would show a dropped contribution" % (case.name, frac, n)
    return frac


def subnormal_rate(r):
    """share of the non-zero contributions below the smallest normal f16"""
    v = np.abs(r.val)
    return float(((v > 0) & (v < 2.0 ** -14)).sum() / max(1, (v > 0).sum()))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def ratio(got, r, prefill=None, a=None, touched_only=False):
    """(max(err / bound), flat element) of a whole table `got` [rows, C] (or, touched_only, of values on r.idx); an element with bound 0
    must be equal, and an element that nothing lands in must keep its bits (zero or the prefill): else the ratio is inf"""
    bd = bound(r, prefill, a)
    want = r.t_ref if prefill is None else r.t_ref + _touched(r, prefill).astype(np.float64)
    if touched_only:
        got_t = np.asarray(got, np.float64)
    else:
        flat = np.asarray(got).reshape(-1)
        assert flat.size == r.n_rows * r.C
        got_t = flat[r.idx].astype(np.float64)
        rest = np.ones(flat.size, bool)
        rest[r.idx] = False
        base = np.zeros(flat.size, flat.dtype) if prefill is None else np.asarray(prefill, flat.dtype).reshape(-1)
        changed = _bits(flat)[rest] != _bits(base)[rest]
        if changed.any():
            return float("inf"), int(np.nonzero(rest)[0][np.argmax(changed)])
    err = np.abs(got_t - want)
    q = np.where(bd > 0, err / np.where(bd > 0, bd, 1.0), np.where(err > 0, np.inf, 0.0))
    m = int(np.argmax(q))
    return float(q[m]), int(r.idx[m])


def bit_equal(got, r):
    """exact cases: the whole table equals the reference rounded (exactly) to the table type, bit for bit"""
    return np.array_equal(_bits(np.asarray(got)), _bits(r.ref.astype(r.dtype)))


def describe(r, flat_elem, got=None):
    """level, row, channel, k and the lane slots of the contributions of one element, for a failure message"""
    row, c = divmod(int(flat_elem), r.C)
    level = int(np.searchsorted(r.geo.offsets, row, side="right") - 1)
    sel = np.nonzero(r.elem == row * r.C + c)[0]
    slots = ["b%d/c%d(lane %d|%d)=%.6g" % (r.b[i], r.corner[i], r.b[i] % 64, (2 * r.b[i] + (r.corner[i] & 1)) % 64, r.val[i]) for i in sel[:24]]
    s = "level %d (%s) row %d (local %d) channel %d k %d" % (level, "hashed" if r.geo.hashed[level] else "dense", row, row - r.geo.offsets[level], c, len(sel))
    if len(sel):
        t = int(r.slot[sel[0]])
        s += " ref %.9g s_abs %.6g" % (r.t_ref[t], r.t_s_abs[t])
    if got is not None:
        s += " got %.9g" % float(np.asarray(got).reshape(-1)[row * r.C + c])
    return s + "; contributions sample/corner(lane one-lane|two-lane)=value: " + ", ".join(slots) + (" ..." if len(sel) > 24 else "")


# ------------------------------------------------------------------------------------------------ run shapes
FEATURES_ONE_LANE = {"len1", "len2", "len3", "len31", "len32", "len33", "whole_wave", "cross_wave", "cross_group", "end_last", "end_before_last",
                     "start0", "start1", "aba", "dead_in_run", "dead_between_runs", "dead2", "dead_wave"}
# among 32 lanes of equal parity a run of 33 exists only as a run that continues into the next wave
FEATURES_TWO_LANE = FEATURES_ONE_LANE - {"len33"}


def coverage(geo, W, G):
    """the run shapes that occur, on some level and corner, when W consecutive samples form one scan (64: one lane per sample; 32:
    two lanes per sample, scan among lanes of equal parity) and G samples one workgroup"""
    rows = geo.rows
    L, B, nc = rows.shape
    assert not np.any((rows >= 0) & (rows == rows[:, :, np.arange(nc) ^ 1])), "two x-corners of one sample share a row"
    pad = (-B) % W
    k = np.concatenate([rows, np.full((L, pad, nc), -1, np.int64)], axis=1).transpose(0, 2, 1).reshape(L * nc, -1, W)
    nw = k.shape[1]
    feats = set()
    head = np.ones(k.shape, bool)
    head[..., 1:] = k[..., 1:] != k[..., :-1]
    flat, hflat = k.ravel(), head.ravel()
    starts = np.nonzero(hflat)[0]
    lens = np.diff(np.append(starts, flat.size))
    livek = flat[starts] >= 0
    sl, ll = starts[livek] % W, lens[livek]
    for n in (1, 2, 3, 31, 32, 33):
        if np.any(ll == n):
            feats.add("len%d" % n)
    if np.any(ll == W):
        feats.add("whole_wave")
    if np.any((sl == 0) & (ll < W)):
        feats.add("start0")
    if np.any(sl == 1):
        feats.add("start1")
    if np.any((sl + ll - 1 == W - 1) & (ll < W)):
        feats.add("end_last")
    if np.any(sl + ll - 1 == W - 2):
        feats.add("end_before_last")
    if nw > 1:
        cont = (k[:, :-1, W - 1] == k[:, 1:, 0]) & (k[:, 1:, 0] >= 0)
        if cont.any():
            feats.add("cross_wave")
        gb = ((np.arange(1, nw) * W) % G) == 0
        if cont[:, gb].any():
            feats.add("cross_group")
    a, b, c = k[..., :-2], k[..., 1:-1], k[..., 2:]
    if np.any((a == c) & (a >= 0) & (b >= 0) & (b != a)):
        feats.add("aba")
    if np.any((a == c) & (a >= 0) & (b < 0)):
        feats.add("dead_in_run")
    if np.any((a != c) & (a >= 0) & (c >= 0) & (b < 0)):
        feats.add("dead_between_runs")
    some_live = (k >= 0).any(-1)
    if np.any((k[..., :-1] < 0) & (k[..., 1:] < 0) & some_live[..., None]):
        feats.add("dead2")
    full = (np.arange(nw) + 1) * W <= B
    if np.any(~some_live[:, full]):
        feats.add("dead_wave")
    return feats


# ------------------------------------------------------------------------------------------------ cases
class Case:
    prefill = None
    affine = None
    a = None
    exact = False

    def __init__(self, name, x, g, offsets, S, H, D, C, gridtype, align, dtype, **kw):
        self.name, self.x, self.g, self.offsets = name, np.ascontiguousarray(x, np.float32), g, np.asarray(offsets, np.int32)
        self.S, self.H, self.D, self.C, self.gridtype, self.align, self.dtype = float(S), H, D, C, gridtype, align, np.dtype(dtype)
        self.L, self.B = len(offsets) - 1, self.x.shape[0]
        for k, v in kw.items():
            setattr(self, k, v)
        self.ref = backward(g, self.x, self.offsets, self.S, H, D, C, gridtype, align, dtype, self.affine)

    def prefix(self, B):
        """the first B samples as a case of their own"""
        return Case("%s[:%d]" % (self.name, B), self.x[:B], np.ascontiguousarray(self.g[:, :B]), self.offsets, self.S, self.H, self.D, self.C,
                    self.gridtype, self.align, self.dtype, exact=self.exact, q=getattr(self, "q", None))


PRODUCT_PLS = float(np.exp2(np.log2(2048 / 16) / 13))  # the product's per-level scale: 16 .. 2048 over 14 levels


def script():
    """the scripted sample sequence as (role, count): role >= 0 a heavy position (long runs), -1 dead, -2 - j the j-th light position
    (short runs).  Index arithmetic in the comments is for waves of 64 | 32 samples."""
    seq, n = [], [0]
    light = [0]

    def put(role, count=1):
        seq.append((role, count))
        n[0] += count

    def singles_to(idx):  # distinct neighbours, never equal to a heavy role
        while n[0] < idx:
            put(-2 - light[0])
            light[0] += 1

    put(0, 1)              # [0]: run of 1 starting at slot 0
    put(1, 2)              # [1, 3): run of 2 starting at slot 1
    put(2, 3)              # [3, 6): run of 3
    put(-2 - 1000), put(-2 - 1001), put(-2 - 1000)  # [6, 9): A B A
    put(1), put(-1), put(1)  # [9, 12): a dead sample inside an otherwise equal run
    put(2), put(-1), put(0)  # [12, 15): a dead sample between two different runs
    put(-1, 2)             # [15, 17): two adjacent dead samples
    singles_to(33)
    put(3, 31)             # [33, 64): run of 31 from slot 33 | 1 to the last slot
    put(4, 32)             # [64, 96): run of 32 from slot 0 | a whole wave
    put(5, 33)             # [96, 129): 32 + 1 across a wave boundary | across the workgroup boundary at 128
    singles_to(130)
    put(0, 33)             # [130, 163): run of 33 inside one wave of 64
    singles_to(192)
    put(6, 70)             # [192, 262): a whole wave of 64 and on across the workgroup boundary at 256
    singles_to(320)
    put(-1, 64)            # [320, 384): a wave (two waves) entirely dead
    singles_to(441)
    put(7, 6)              # [441, 447): ends one slot before the last (62 | 30)
    singles_to(461)        # [447]: a run of 1 in the last slot; ragged tail
    return seq


def _script_positions(D, rng, exact, align=False):
    """x [B, D] for script(): exact -> lattice points m/4 (heavy: the corners of the unit box, frac 1/2 in every dimension, light: the other
    lattice points); else heavy = centres of level-0 cells with a jitter that stays inside the cell, light = uniform random"""
    nh = 1 << D
    if exact:
        heavy = np.stack(np.meshgrid(*[np.array([0.0, 1.0])] * D, indexing="ij"), -1).reshape(-1, D)
        lightp = _light_lattice(D)
        lightp = lightp[rng.permutation(len(lightp))]
    else:
        cells = rng.permutation(13 ** D)[:nh]
        heavy = (np.stack(np.unravel_index(cells, (13,) * D), -1) + (2.5 if align else 2.0)) / 15.0  # p = 15 x + 0.5 (align_corners: 15 x) = cell + 2.5: mid-cell
    xs = []
    for role, count in script():
        if role == -1:
            pos = np.full((count, D), 0.5)
            pos[:, rng.randint(D)] = rng.choice([-0.25, 1.25])
        elif role >= 0:
            pos = np.repeat(heavy[role % nh][None], count, 0)
            if not exact:
                pos = pos + rng.uniform(-0.012, 0.012, pos.shape)
        elif exact:
            pos = np.repeat(lightp[(-2 - role) % len(lightp)][None], count, 0)
        else:
            pos = np.repeat(np.random.RandomState(7000 + (-2 - role)).uniform(0.02, 0.98, (1, D)), count, 0)
        xs.append(pos)
    return np.concatenate(xs).astype(np.float32)


def scripted_x(D, seed, exact, tail=480, align=False):
    """script() (461 samples) and a tail of short runs (1 to 3 equal positions) behind it, so that the launch has several workgroups"""
    rng = np.random.RandomState(seed)
    a = _script_positions(D, rng, exact, align)
    lat = _light_lattice(D)
    xs, n = [a], 0
    while n < tail:
        c = min(int(rng.randint(1, 4)), tail - n)
        pos = lat[rng.randint(len(lat))] if exact else rng.uniform(0.0, 1.0, D)
        xs.append(np.repeat(pos[None], c, 0))
        n += c
    return np.concatenate(xs).astype(np.float32)


def _light_lattice(D):
    """lattice points m/4 that are no corner of the box and have at most one coordinate 1/2 (frac 0, weight 1): no weight above 9/16"""
    lat = np.stack(np.meshgrid(*[np.arange(5)] * D, indexing="ij"), -1).reshape(-1, D)
    keep = ~np.all((lat == 0) | (lat == 4), axis=1) & ((lat == 2).sum(1) <= 1)
    return lat[keep] / 4.0


def _grads(rng, L, B, C, dtype, exact, scale=1.0):
    if exact:
        return rng.choice([-2.0, -1.0, 1.0, 2.0], (L, B, C), p=[0.1, 0.4, 0.4, 0.1]).astype(dtype)
    # of order 1 and bounded away from 0, so that contributions below the smallest normal f16 stay rare (subnormal_rate)
    return (rng.choice([-1.0, 1.0], (L, B, C)) * rng.uniform(0.5, 2.0, (L, B, C)) * scale).astype(dtype)


def exact_case(D=3, C=2, dtype=np.float16, log2_hashmap_size=19, gridtype=0, align=False, L=None, H=16, seed=0, name=None):
    """the scripted runs on inputs for which float arithmetic is exact in any order and grouping (module docstring); align_corners
    moves frac to multiples of 1/4 of another phase (p = m scale / 4), the quantum stays 4^-D.  f32 tables: L = 14.  f16 tables: L = 12,
    because with S = 1 the levels 12 and 13 (resolutions 65537 and 131073) come out dense through the uint32 wrap of the stride product
    and then fold some twenty lattice positions into one row, which the 2048 q of f16 cannot hold; the f32 cases keep those levels."""
    if L is None:
        L = 14 if np.dtype(dtype) == np.float32 else 12
    x = scripted_x(D, seed, True)
    rng = np.random.RandomState(seed + 1)
    offs = level_offsets(D, L, 2.0, H, log2_hashmap_size, align)
    g = _grads(rng, L, x.shape[0], C, dtype, True)
    case = Case(name or "scripted-exact D%d C%d %s T%d g%d a%d" % (D, C, np.dtype(dtype).name, log2_hashmap_size, gridtype, align), x, g, offs,
                1.0, H, D, C, gridtype, align, dtype, exact=True, q=4.0 ** -D)
    assert_exact(case)
    return case


def assert_exact(case):
    r, q = case.ref, case.q
    m = r.val / q
    assert np.array_equal(m, np.rint(m)), "%s: a contribution is not a multiple of the quantum" % case.name
    limit = 2048 if r.dtype == np.float16 else 2 ** 24
    assert r.t_s_abs.max() <= limit * q, "%s: s_abs %g q passes %d q" % (case.name, r.t_s_abs.max() / q, limit)
    assert np.array_equal(r.t_ref.astype(r.dtype).astype(np.float64), r.t_ref)


def scripted_case(D=3, C=2, dtype=np.float16, log2_hashmap_size=19, gridtype=0, align=False, L=14, H=16, seed=0, affine=None, name=None):
    """the scripted runs with random values: jittered positions (runs hold on the coarse levels and break up on the fine ones)"""
    x = scripted_x(D, seed, False, align=align)
    rng = np.random.RandomState(seed + 2)
    offs = level_offsets(D, L, PRODUCT_PLS, H, log2_hashmap_size, align)
    if affine is not None:
        x = _unmap(x, affine)
    g = _grads(rng, L, x.shape[0], C, dtype, False)
    return Case(name or "scripted D%d C%d %s T%d g%d a%d" % (D, C, np.dtype(dtype).name, log2_hashmap_size, gridtype, align), x, g, offs,
                np.log2(PRODUCT_PLS), H, D, C, gridtype, align, dtype, affine=affine)


def _unmap(x01, affine):
    """positions whose affine image is (about) x01: the reference maps them again in float32, exactly as locate does"""
    return (x01.astype(np.float64) * affine[1] - affine[0]).astype(np.float32)


def coherent_case(D=3, C=2, dtype=np.float16, log2_hashmap_size=19, gridtype=0, align=False, L=14, H=16, seed=0, B=3000, n_rays=60, affine=None,
                  name=None):
    """samples marching along rays at 1.7e-3 steps, some leaving [0, 1]"""
    rng = np.random.RandomState(seed + 3)
    o = rng.uniform(0.1, 0.9, (n_rays, 1, D))
    d = rng.standard_normal((n_rays, 1, D))
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    o[: n_rays // 4] = np.where(d[: n_rays // 4] > 0, 0.97, 0.03)  # a quarter of the rays start near a face and walk out
    steps = np.arange(B // n_rays + 1)[None, :, None] * 1.7e-3
    x = (o + d * steps).reshape(-1, D)[:B].astype(np.float32)
    if affine is not None:
        x = _unmap(x, affine)
    offs = level_offsets(D, L, PRODUCT_PLS, H, log2_hashmap_size, align)
    g = _grads(rng, L, B, C, dtype, False)
    return Case(name or "coherent D%d C%d %s T%d g%d a%d" % (D, C, np.dtype(dtype).name, log2_hashmap_size, gridtype, align), x, g, offs,
                np.log2(PRODUCT_PLS), H, D, C, gridtype, align, dtype, affine=affine)


def random_case(D=3, C=2, dtype=np.float16, log2_hashmap_size=19, gridtype=0, align=False, L=14, H=16, seed=0, B=3001, affine=None, prefill=False,
                name=None):
    """uniform random positions, the box's corners and faces, a few out-of-range ones; prefill: the output buffer holds values already"""
    rng = np.random.RandomState(seed + 4)
    x = rng.uniform(0, 1, (B, D)).astype(np.float32)
    x[:4] = [[0.0] * D, [1.0] * D, [0.5] * D, [1.0] + [0.0] * (D - 1)]
    x[4:B:97, rng.randint(D)] = -0.01
    x[5:B:89, rng.randint(D)] = 1.0001
    if affine is not None:
        x = _unmap(x, affine)
    offs = level_offsets(D, L, PRODUCT_PLS, H, log2_hashmap_size, align)
    g = _grads(rng, L, B, C, dtype, False)
    kw = {}
    case = lambda: Case(name or "%s D%d C%d %s T%d g%d a%d" % ("prefilled" if prefill else "random", D, C, np.dtype(dtype).name, log2_hashmap_size, gridtype,
                                                      align), x, g, offs, np.log2(PRODUCT_PLS), H, D, C, gridtype, align, dtype, affine=affine, **kw)
    if not prefill:
        return case()
    # f32: an element whose only contribution is about 1e-6 of its prefill lies between the filter of the sensitivity condition (2^-20)
    # and twice the bound; about one element in 4e5 does.  Take the first prefill, in a fixed order of seeds, that has none.
    for k in range(16):
        kw["prefill"] = np.random.RandomState(seed + 40 + k).standard_normal((int(offs[-1]), C)).astype(dtype)
        c = case()
        if sensitive_fraction(c.ref, c.prefill)[0] >= (0.9 if c.dtype == np.float16 else 1.0):
            return c
    raise AssertionError("no prefill satisfies the sensitivity condition")


def subnormal_case(log2_hashmap_size=12, seed=0, B=600):
    """f16, D 3, C 2: gradients of order 2^-13, so that most contributions and many sums lie below the smallest normal 2^-14"""
    rng = np.random.RandomState(seed + 5)
    x = rng.uniform(0, 1, (B, 3)).astype(np.float32)
    x[::3] = x[1::3][: len(x[::3])]  # repeated positions: runs of equal rows, merged sums
    offs = level_offsets(3, 14, PRODUCT_PLS, 16, log2_hashmap_size)
    g = (rng.standard_normal((14, B, 2)) * 2.0 ** -13).astype(np.float16)
    return Case("subnormal D3 C2 float16 T%d" % log2_hashmap_size, x, g, offs, np.log2(PRODUCT_PLS), 16, 3, 2, 0, False, np.float16)


# ------------------------------------------------------------------------------------------------ the cases of the GPU test
AFFINE = (2.0, 4.0)  # GridEncoder.forward's (x + bound) / (2 bound) at bound 2
OTHER = [(dt, D, C) for dt in ("float32", "float16") for D, C in ((3, 1), (3, 4), (3, 8), (2, 1), (2, 2), (2, 8))] + [("float32", 3, 2)]
SIZES = (1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257)

CASES = {
    # f16, D 3, C 2: the three kernels of the training shape (paths 1 to 4)
    "exact": lambda: exact_case(),
    "scripted": lambda: scripted_case(),
    "scripted-T11": lambda: scripted_case(log2_hashmap_size=11),
    "coherent": lambda: coherent_case(),
    "random": lambda: random_case(),
    "random-T10": lambda: random_case(log2_hashmap_size=10),
    "prefilled": lambda: random_case(log2_hashmap_size=12, prefill=True),
    "random-tiled": lambda: random_case(log2_hashmap_size=12, gridtype=1, B=2001),
    "random-align": lambda: random_case(log2_hashmap_size=12, align=True, B=2001),
    "scripted-tiled-align": lambda: scripted_case(log2_hashmap_size=12, gridtype=1, align=True),
    # path 5
    "affine-scripted": lambda: scripted_case(log2_hashmap_size=12, affine=AFFINE, name="affine scripted T12"),
    "affine-coherent": lambda: coherent_case(affine=AFFINE, name="affine coherent T19"),
    "affine-random": lambda: random_case(log2_hashmap_size=12, affine=AFFINE, name="affine random T12"),
    "affine-prefilled": lambda: random_case(log2_hashmap_size=12, affine=AFFINE, prefill=True, name="affine prefilled T12"),
    # bit-exact tiled / align_corners (f32: the quantum budget of f16 does not hold the rows that tiling folds together)
    "exact-f32-tiled": lambda: exact_case(dtype=np.float32, log2_hashmap_size=12, gridtype=1),
    "exact-f32-align": lambda: exact_case(dtype=np.float32, log2_hashmap_size=12, align=True),
    # S = 1 with 2^19 rows: the stride products of levels 12 and 13 wrap at 2^32 and the levels come out dense
    "exact-f32-wrap": lambda: exact_case(dtype=np.float32, log2_hashmap_size=19, name="scripted-exact D3 C2 float32 T19 (levels 12, 13 wrap)"),
    "subnormal": lambda: subnormal_case(),
}
MAIN = ["exact", "scripted", "scripted-T11", "coherent", "random", "random-T10", "prefilled", "random-tiled", "random-align", "scripted-tiled-align"]
AFFINE_CASES = ["affine-scripted", "affine-coherent", "affine-random", "affine-prefilled"]


def other_names(dt, D, C):
    return ["%s-%s-D%dC%d" % (kind, dt, D, C) for kind in ("exact", "scripted", "coherent", "random", "prefilled")]


for _dt, _D, _C in OTHER:
    _kw = dict(D=_D, C=_C, dtype=np.dtype(_dt).type)
    _n = other_names(_dt, _D, _C)
    # f16 exact: 2^19 rows (smaller hash tables fold lattice positions together beyond 2048 q); everything else 2^12
    CASES[_n[0]] = lambda kw=_kw: exact_case(log2_hashmap_size=19 if kw["dtype"] == np.float16 else 12, **kw)
    CASES[_n[1]] = lambda kw=_kw: scripted_case(log2_hashmap_size=12, **kw)
    CASES[_n[2]] = lambda kw=_kw: coherent_case(log2_hashmap_size=12, B=2000, n_rays=40, **kw)
    CASES[_n[3]] = lambda kw=_kw: random_case(log2_hashmap_size=12, B=2001, **kw)
    CASES[_n[4]] = lambda kw=_kw: random_case(log2_hashmap_size=12, B=2001, prefill=True, **kw)
for _B in SIZES:
    CASES["exact[:%d]" % _B] = lambda B=_B: case("exact").prefix(B)

TOLERANCE_CASES = [n for n in CASES if not n.startswith("exact") and n != "subnormal"]
_cache = {}


def case(name):
    if name not in _cache:
        _cache[name] = CASES[name]()
    return _cache[name]


# ------------------------------------------------------------------------------------------------ mutations of the checker's own arrays
def mutate(r, kind, j=0):
    """what a faulty scatter would have summed on the touched elements, in float64, from the reference's own contribution list:
       drop   : one contribution of one run of >= 3 equal rows (one-lane mapping) is lost;
       double : the contribution of the last lane of such a run is added twice;
       merge  : two runs separated by one dead sample are merged: the second run's sum lands in the first run's row;
       skip   : samples [256 j, 256 j + 256) of the finest level are never scattered."""
    geo, C = r.geo, r.C
    slot, val = r.slot.copy(), r.val.copy()
    if kind == "skip":
        gone = (r.level == geo.L - 1) & (r.b >= 256 * j) & (r.b < 256 * j + 256)
        assert gone.any() and np.any(val[gone] != 0)
        return accumulate(slot[~gone], val[~gone], len(r.idx))[0]
    rows = geo.rows[0, :, 0]  # level 0, corner 0
    if kind in ("drop", "double"):
        b = next(i for i in range(2, geo.B) if rows[i] >= 0 and rows[i] == rows[i - 1] == rows[i - 2] and (i + 1 == geo.B or rows[i + 1] != rows[i]))
        b = b - 1 if kind == "drop" else b
        sel = np.nonzero((r.level == 0) & (r.b == b) & (r.corner == 0))[0]
        assert len(sel) == C and np.all(val[sel] != 0)
        val[sel] *= 0.0 if kind == "drop" else 2.0
    elif kind == "merge":
        b = next(i for i in range(1, geo.B - 1) if rows[i] < 0 and rows[i - 1] >= 0 and rows[i + 1] >= 0 and rows[i - 1] != rows[i + 1])
        sel = np.nonzero((r.level == 0) & (r.b == b + 1) & (r.corner == 0))[0]
        assert len(sel) == C and np.all(val[sel] != 0)
        slot[sel] = np.searchsorted(r.idx, (geo.offsets[0] + rows[b - 1]) * C + np.arange(C))
    else:
        raise ValueError(kind)
    return accumulate(slot, val, len(r.idx))[0]


def caught(case, got_t):
    """would the check of this case fail on the touched-element values `got_t`?"""
    if case.exact:
        return not np.array_equal(got_t, case.ref.t_ref)
    return ratio(got_t, case.ref, touched_only=True)[0] > 1.0


def report(label, got, case, a=None):
    """(line, worst ratio, flat element) of one whole-table result against the case's reference"""
    worst, at = ratio(got, case.ref, prefill=case.prefill, a=a if a is not None else case.a)
    return "%-34s %-44s max(err/bound) %.4f  (k max %d, %d elements)" % (label, case.name, worst, case.ref.t_k.max(), len(case.ref.idx)), worst, at
