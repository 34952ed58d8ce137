"""Float64 reference of ONE call of the flat AdamW kernels (csrc/optimizer.hip: k_adamw, its tail, k_adamw_lazy_flush, the L1 sums),
teacher-forced: it takes the fp32 state the kernel is about to read and returns the state after the call.  numpy only.

step64    decoupled AdamW as torch defines it, float64 throughout, no kernel-order rounding:
              G  = (g + widened g16) / scale + coef * sign(p)      (the half gradient carries the GradScaler's scale like g does)
              p1 = p (1 - lr wd);  m' = m + (1 - b1)(G - m);  v' = b2 v + (1 - b2) G^2;  t = step + 1
              p' = p1 - (lr / (1 - b1^t)) m' / (sqrt(v') / sqrt(1 - b2^t) + eps)
          lr is the fp32 value handed in, or the documented closed form of the schedule: eta + (base - eta)(1 + cos(pi tick / T)) / 2
          (cosine) or base * factor^min(tick / T, 1) (exponential).
bound     what the kernel may differ by, per element and output, from u = 2^-24 and nothing fitted.  With x the exact value and e_x
          the error carried so far, every rounding to fp32 costs  r(x, e) = u (|x| + e) + FLOOR  (FLOOR = 2^-150: half the spacing of
          the fp32 subnormals, where a result can be subnormal), and every fp64 expression costs  E64 * sum |terms|  (E64 = 8 * 2^-53:
          at most eight fp64 operations, each within 2^-53 of its operands' size, and the double rounding fp64 -> fp32).  In the
          kernel's order:
              A = g + (float)h            e_A = r(A)                                 (g16 only)
              B = (float)(A / scale)      e_B = e_A / scale + r(B, e_A / scale)       (grad_scale only)
              C = B + coef sign(p)        e_C = e_B + r(C, e_B)                       (inside an L1 range only)
              p1 = (float)(p - lr wd p)   e_1 = |p| wd e_lr + r(p1, .) + E64 |p|
              m' = (float)(m + (1-b1)(C - m))          e_m = (1-b1) e_C + r(m', .) + E64 (|m| + |C|)
              v' = (float)(b2 v + (1-b2) C C)          e_v = (1-b2)(2 |C| e_C + e_C^2) + r(v', .) + E64 (v + C^2)
              s = sqrtf(v')                            e_s = sqrt(v' + e_v) - sqrt(max(v' - e_v, 0)) + r(s, .)
              d = (float)(s / sqrt(bc2) + eps)         e_d = (e_s + s rel2) / sqrt(bc2) + r(d, .) + E64 d
              ss = (float)(lr / bc1)                   e_ss = (e_lr + lr rel1) / bc1 + r(ss, .)
              x = ss * m'                              e_x = e_ss |m'| + ss e_m + e_ss e_m + r(x, .)
              y = x / d                                e_y = (e_x + |y| e_d) / (d - e_d) + r(y, .)
              p' = p1 - y                              e_p = e_1 + e_y + r(p', e_1 + e_y)
          sqrtf and the fp32 division are correctly rounded (the build does not relax them), products are not contracted.
          rel1 / rel2 are the device library's share: LIB_ULPS fp64 ulps on pow(), amplified by the cancellation in 1 - b^t
          (b^t / (1 - b^t), halved under the square root); e_lr is 0 for a rate handed in, and under a schedule
          u lr + LIB_ULPS 2^-53 (|base - eta| or lr) + E64 (...).  LIB_ULPS: the ROCm device-library documentation installed with
          the toolchain states no figure, so it is measured on the MI355X (test_device_pow_cos_allowance, profiles/adamw_fp64_pin.txt:
          pow <= 1 ulp, cos <= 1 ulp against numpy over every scripted t / tick) and doubled.
model32   numpy restatement of the KERNEL's order, the fp64 expression and one rounding per line as k_adamw reads.  On the CPU it shows
          that the bound is neither too tight (it stays inside) nor too loose (single faults injected into it leave it); on the GPU it
          only records how many elements differ from it, since device pow / cos / sqrtf need not match the host's bit for bit.
exact     parts without a library call, asserted bit for bit: decay_exact (cold groups), flush_exact (the lazy log's replay; +-0 stay
          zero, and -0 - f (-0) = +0 as IEEE subtraction and torch's fused `param -= lr wd param` give), the skipped step, tail_ref (every scalar the tail writes; the published rate under a schedule may be 1 fp32
          ulp off, device cos / pow feed it).
l1_*      the L1 sums with gamma_k sum |terms|, k counted from the kernels' reduction depth (see l1_next64 / l1_ranges64).

Scripted cases: case("small") ~20 k elements with everything below, case("stride") the smallest sizes at which each loop runs twice
with a ragged end, case("tiny") n = 4, case("grid<G>") a dense buffer of exactly G workgroups.  assert_coverage fails if a case stops
containing what it promises; validate() checks every list / bitmap / table a test is about to upload."""
import functools

import numpy as np

f32, f64 = np.float32, np.float64
U = 2.0 ** -24
FLOOR = 2.0 ** -150
E64 = 8 * 2.0 ** -53
LIB_ULPS = 2  # 2 x the measured 1 ulp of device pow / cos (module docstring)
BETA1, BETA2, EPS, WD = 0.9, 0.99, 1e-15, 0.01
BLOCK, MAX_BLOCKS, REPLAY_BLOCKS, L1_BLOCKS, MAX_SEGMENTS = 256, 4096, 512, 1024, 16
SCALE = 64.0
STEPS = (0, 1, 9, 999)
PAD = 160  # sentinel elements behind every buffer the GPU tests hand to a kernel
REGIMES = ("normal", "zero", "tiny", "large", "cold")
POISON = 0xFFFFFFFF


# ---------------------------------------------------------------------------------------------- cases
class Case:
    pass


class Form:
    """one call: which extras are on, and the scalars it starts from"""
    _defaults = dict(n=None, step=0.0, found_inf=0.0, scaled=False, amp=None, scale=SCALE, tracker=0, sched=None, l1=False, l1_next=False,
                     g16=False, cold=None, warm=None, nograd_from=0, replay=False, snapshot=False, zero_after=False, arrivals=False,
                     compact=False, tail_clear=None, lazy_count=0, lazy_capacity=16, lr=None)

    def __init__(self, **kw):
        bad = set(kw) - set(self._defaults)
        assert not bad, bad
        self.__dict__.update(self._defaults)
        self.__dict__.update(kw)

    def but(self, **kw):
        d = {k: getattr(self, k) for k in self._defaults}
        d.update(kw)
        return Form(**d)


def _segments(n):
    """16 segments: one empty, one of 4 elements, every end a multiple of 4"""
    if n < 4 * 64:
        return np.array([0] * 15 + [n], np.uint64)  # fifteen empty segments in front of the only one
    unit = n // 14 // 4 * 4
    sizes = [unit, unit, 0, 4] + [unit] * 11
    ends = np.cumsum(sizes)
    return np.concatenate([ends, [n]]).astype(np.uint64)


def _build(label, n4, seed, cold_frac, exact_warm=None):
    rs = np.random.RandomState(seed)
    c = Case()
    c.label, c.n4, c.n = label, n4, 4 * n4
    n = c.n
    c.seg_ends = _segments(n)
    c.n_seg = 16
    c.base_lr = (1e-2 * 0.8 ** np.arange(16)).astype(f32)
    c.lr = (c.base_lr * f32(0.75)).astype(f32)
    if n >= 20000:
        q = n // 5 // 4 * 4
        c.l1 = [(q, q + 800, 1e-3), (q + 800, q + 800, 5e-4), (q + 800, q + 2000, 2e-3)]
        c.g16_begin, c.g16_end = 2 * q + 4, 2 * q + 4004  # (not a multiple of its own length: a wrong index base shows)
    else:
        c.l1 = [(0, n, 1e-3)]
        c.g16_begin, c.g16_end = 0, 0
    c.coef = np.zeros(n, f32)
    for b, e, co in c.l1:
        c.coef[b:e] = f32(co)
    starts = np.unique(np.concatenate([[0], c.seg_ends[:-1].astype(np.int64)])) // 4  # first group of every segment
    starts = starts[starts < n4]
    protect = np.zeros(n4, bool)
    protect[starts] = True
    for b, e, _ in c.l1:
        protect[b // 4:e // 4] = True
    protect[c.g16_begin // 4:c.g16_end // 4] = True
    cold = (rs.rand(n4) < cold_frac) & ~protect
    if exact_warm is not None:  # exactly that many warm groups
        extra = int((~cold).sum()) - exact_warm
        assert extra >= 0
        free = np.flatnonzero(~cold & ~protect)
        cold[free[rs.permutation(free.size)[:extra]]] = True
    c.cold4 = cold
    regime = rs.randint(0, 4, n4).astype(np.int8)
    regime[starts] = 0
    regime[cold] = 4
    c.regime = regime
    el = np.repeat(regime, 4)
    sign = np.where(rs.rand(n) < 0.5, -1.0, 1.0)
    g = rs.randn(n) * SCALE
    g[el == 1] = 0.0
    g[el == 2] = sign[el == 2] * 10.0 ** rs.uniform(-16.0, np.log10(6.4e-12), int((el == 2).sum()))
    g[el == 3] = sign[el == 3] * 10.0 ** rs.uniform(10.0, 18.0, int((el == 3).sum()))
    m = rs.randn(n) * 0.1
    v = rs.rand(n) * 0.01
    m[el == 2] = 0.0
    v[el == 2] = 0.0
    half = rs.rand(n) < 0.5
    m[(el == 3) & half] = 0.0
    v[(el == 3) & half] = 0.0
    for a in (g, m, v):
        a[el == 4] = 0.0
    p = rs.randn(n)
    for b, e, _ in c.l1:  # +0, -0 and both signs inside every L1 range
        if e - b >= 8:
            p[b:b + 8] = [0.0, -0.0, 0.5, -0.5, -0.0, 0.0, -2.0, 2.0]
    ce = np.flatnonzero(el == 4)
    if ce.size >= 8:
        p[ce[:4]] = 0.0
        p[ce[4:8]] = -0.0
    c.p, c.g, c.m, c.v = p.astype(f32), g.astype(f32), m.astype(f32), v.astype(f32)
    c.g16 = (rs.randn(c.g16_end - c.g16_begin) * 8.0).astype(np.float16)
    c.warm = np.flatnonzero(~cold).astype(np.int32)
    # the list [B | A] of the one-launch two-part form: A = warm groups with a structurally zero gradient, outside the half range
    is_a = (regime == 1) & (np.arange(n4) >= n4 * 3 // 4)
    c.warm_b = np.flatnonzero(~cold & ~is_a).astype(np.int32)
    c.warm_a = np.flatnonzero(is_a).astype(np.int32)
    c.gc = (rs.randn(4 * c.warm.size) * SCALE).astype(f32)  # the exchanged compact gradient: entry j of the warm list
    return c


STRIDE_DENSE = MAX_BLOCKS * BLOCK + 37       # groups of the dense walk and of the warm-list walk
STRIDE_REPLAY = 2 * REPLAY_BLOCKS * BLOCK + 37  # list entries of the replay form
GRIDS = (1, 2, 63, 64, 65, 127, 4096)
CASE_NAMES = ("small", "stride", "tiny")


@functools.lru_cache(maxsize=None)
def case(name):
    if name == "small":
        return _build(name, 5001, 1, 0.3)  # n = 20004 = 156 * 128 + 36
    if name == "stride":  # 2 x STRIDE_DENSE groups, exactly STRIDE_DENSE of them warm; the dense walk takes the first STRIDE_DENSE
        return _build(name, 2 * STRIDE_DENSE, 2, 0.5, exact_warm=STRIDE_DENSE)
    if name == "tiny":
        return _build(name, 1, 3, 0.0)
    if name.startswith("grid"):
        return _build(name, int(name[4:]) * BLOCK - 19, 4, 0.0)
    raise KeyError(name)


def pack_bits(cold4):
    words = (cold4.size + 31) // 32
    b = np.zeros(words * 32, np.uint64)
    b[:cold4.size] = cold4
    return (b.reshape(words, 32) << np.arange(32, dtype=np.uint64)).sum(1).astype(np.uint32).view(np.int32)


def n_of(c, f):
    return c.n if f.n is None else f.n


def walk(c, f):
    """the groups the call visits, in the order of the walk: (group index [J], gradient structurally zero [J])"""
    if f.warm is not None:
        grp = np.asarray(f.warm, np.int64)
        ng = np.arange(grp.size) >= f.nograd_from if f.nograd_from else np.zeros(grp.size, bool)
        return grp, ng
    grp = np.arange(n_of(c, f) // 4, dtype=np.int64)
    return grp, np.zeros(grp.size, bool)


def grid_of(c, f):
    n_walk = walk(c, f)[0].size
    return max(1, min(REPLAY_BLOCKS if f.replay else MAX_BLOCKS, -(-n_walk // BLOCK)))


def validate(c, f):
    """everything a test uploads for this call, checked against the buffers' sizes: no index can leave them"""
    n = n_of(c, f)
    assert n % 4 == 0 and 0 < n <= c.n
    ends = c.seg_ends.astype(np.int64)
    assert ends.size == c.n_seg <= MAX_SEGMENTS and (ends % 4 == 0).all() and (np.diff(ends) >= 0).all() and ends[-1] >= n
    assert c.lr.size == c.base_lr.size == c.n_seg
    for b, e, _ in c.l1:
        assert b % 4 == 0 and e % 4 == 0 and 0 <= b <= e <= n
    assert len(c.l1) <= MAX_SEGMENTS
    if f.g16:
        assert c.g16_begin % 4 == 0 and c.g16_end % 4 == 0 and c.g16_begin <= c.g16_end <= n and c.g16.size == c.g16_end - c.g16_begin
    assert c.cold4.size * 4 >= n and pack_bits(c.cold4).size * 128 >= n
    if f.warm is not None:
        w = np.asarray(f.warm, np.int64)
        assert f.cold == "lazy", "a warm list needs the deferred decay"
        assert w.size >= 1 and w.min() >= 0 and w.max() < n // 4, "warm index outside the buffers"
        assert np.unique(w).size == w.size and not c.cold4[w].any(), "warm list repeats a group or names a cold one"
        cut = f.nograd_from if f.nograd_from else w.size
        assert 0 <= f.nograd_from < max(w.size, 1)
        assert (np.diff(w[:cut]) > 0).all() and (np.diff(w[cut:]) > 0).all(), "each run of the list ascends"
        if f.compact:
            assert c.gc.size >= 4 * w.size and not f.nograd_from and not f.g16 and not f.replay
    else:
        assert not f.compact and not f.replay and not f.nograd_from
    if f.cold == "lazy":
        assert f.lazy_capacity >= 1
    if f.tail_clear is not None:
        assert f.tail_clear[0] >= 1 and f.tail_clear[1] >= 1 and not f.replay
    if f.replay:
        assert not f.snapshot and not f.g16 and not f.arrivals
    assert grid_of(c, f) <= MAX_BLOCKS  # l1_next holds 4096 partials
    return True


def assert_coverage(c):
    n, el = c.n, np.repeat(c.regime, 4)
    assert n % 4 == 0 and n % 128 != 0
    if c.label == "tiny":
        assert n == 4 and c.n_seg == 16 and c.seg_ends[-1] == 4
        return
    ends = c.seg_ends.astype(np.int64)
    sizes = np.diff(np.concatenate([[0], ends]))
    assert c.n_seg == 16 and (sizes == 0).any() and (sizes == 4).any(), "16 segments, one empty, one of 4 elements"
    assert np.unique(c.lr).size == 16 and np.unique(c.base_lr).size == 16, "a wrong segment must change the rate"
    firsts = np.unique(ends[:-1]) // 4
    assert (c.regime[firsts] == 0).all(), "the first group of every segment takes a normal, warm update"
    if not c.label.startswith("grid"):
        assert len(c.l1) == 3 and any(b == e for b, e, _ in c.l1), "three L1 ranges, one empty"
        assert all(c.l1[i][1] == c.l1[i + 1][0] for i in range(2)), "adjacent ranges"
        assert c.g16_begin > 0 and c.g16_end > c.g16_begin
    for b, e, _ in c.l1:
        if e > b:
            q = c.p[b:e]
            assert ((q == 0) & ~np.signbit(q)).any() and ((q == 0) & np.signbit(q)).any() and (q > 0).any() and (q < 0).any()
            assert not c.cold4[b // 4:e // 4].any()
    for r in range(4):
        assert (c.regime == r).sum() >= 8, REGIMES[r]
    assert (c.g[el == 1] == 0).all() and (c.m[el == 1] != 0).all() and (c.v[el == 1] != 0).all(), "zero gradients with live moments"
    big = np.abs(c.g[el == 3].astype(f64))
    assert big.max() > 1e17 and big.max() <= 1e18 and np.isfinite(f32(0.01) * c.g[el == 3] * c.g[el == 3]).all()
    for scaled in (False, True):  # sqrt(v') / sqrt(bc2) on both sides of eps, whichever step the test takes
        gt = np.abs(c.g[el == 2].astype(f64)) / (SCALE if scaled else 1.0)
        assert gt.min() >= 1e-18 and gt.max() <= 1e-11
        for step in STEPS:
            d = np.sqrt((1 - BETA2) * gt * gt) / np.sqrt(1 - BETA2 ** (step + 1.0))
            assert (d < EPS / 2).sum() >= 4 and (d > 2 * EPS).sum() >= 4, "tiny gradients straddle eps"
    if not c.label.startswith("grid"):
        frac = c.cold4.mean()
        assert 0.2 < frac < 0.6 and (c.g[el == 4] == 0).all() and (c.m[el == 4] == 0).all() and (c.v[el == 4] == 0).all()
        cp = c.p[el == 4]
        assert ((cp == 0) & np.signbit(cp)).any() and ((cp == 0) & ~np.signbit(cp)).any(), "cold +0 and -0"
        assert c.warm_a.size >= 8 and c.warm_b.size >= 8 and (c.g[np.repeat(c.warm_a, 4) * 4] == 0).all()
    if c.label == "stride":
        assert c.warm.size == STRIDE_DENSE and STRIDE_DENSE > MAX_BLOCKS * BLOCK and STRIDE_REPLAY > 2 * REPLAY_BLOCKS * BLOCK
        assert c.n4 >= STRIDE_DENSE and STRIDE_DENSE % BLOCK == 37 and STRIDE_REPLAY % BLOCK == 37
    if c.label.startswith("grid"):
        assert grid_of(c, Form()) == int(c.label[4:])


# ---------------------------------------------------------------------------------------------- the schedule and the segments
def lr_in(c, f):
    """the fp32 rates the call is handed (the record's, for the deferred part)"""
    return c.lr if f.lr is None else np.asarray(f.lr, f32)


def lr64(c, f, tick=None):
    if f.sched is None:
        return lr_in(c, f).astype(f64)
    kind, T, param, t0 = f.sched
    tick = f64(f32(t0 if tick is None else tick))
    T, param, base = f64(f32(T)), f64(f32(param)), c.base_lr.astype(f64)
    if kind == 1:
        return param + (base - param) * (1.0 + np.cos(np.pi * tick / T)) * 0.5
    return base * param ** min(tick / T, 1.0)


def lr_err(c, f):
    if f.sched is None:
        return np.zeros(c.n_seg)
    kind, T, param, _ = f.sched
    lr, base = np.abs(lr64(c, f)), c.base_lr.astype(f64)
    span = np.abs(base - f64(f32(param))) if kind == 1 else lr
    return U * lr + FLOOR + (LIB_ULPS * 2.0 ** -53 + E64) * (span + lr + abs(param))


def seg_of(c, e):
    return np.minimum(np.searchsorted(c.seg_ends.astype(np.int64), e, side="right"), c.n_seg - 1)


def _elements(grp):
    return (grp[:, None] * 4 + np.arange(4)).reshape(-1)


def _split(c, f):
    """(groups updated in full, their no-grad flags, their list positions, cold groups decayed now)"""
    grp, ng = walk(c, f)
    pos = np.arange(grp.size)
    if f.cold and f.warm is None:
        is_cold = c.cold4[grp]
        decay = grp[is_cold] if f.cold == "eager" else grp[:0]
        return grp[~is_cold], ng[~is_cold], pos[~is_cold], decay
    return grp, ng, pos, grp[:0]


def _scalars(f, replayed=None):
    """(found_inf, step, scale) the update uses: the live ones, or the record's"""
    return (f.found_inf, f.step, f.scale) if replayed is None else (replayed[0], replayed[1], replayed[2])


# ---------------------------------------------------------------------------------------------- float64 reference and its bound
def step64(c, f, g=None, want_bound=True):
    """-> dict p, m, v (float64 [c.n], the state after the call), bp, bm, bv (the bound, 0 where the result is exact or untouched),
    kind int8 [c.n] (0 untouched, 1 updated, 2 decayed: exact, see decay_exact)."""
    g = c.g if g is None else g
    P, M, V = c.p.astype(f64), c.m.astype(f64), c.v.astype(f64)
    out = dict(p=P, m=M, v=V, bp=np.zeros(c.n), bm=np.zeros(c.n), bv=np.zeros(c.n), kind=np.zeros(c.n, np.int8))
    if f.found_inf:
        return out
    lr_all, lre_all = lr64(c, f), lr_err(c, f)
    grp, ng, pos, decay = _split(c, f)
    if decay.size:
        e = _elements(decay)
        P[e] = P[e] - lr_all[seg_of(c, e)] * WD * P[e]
        out["kind"][e] = 2
    e = _elements(grp)
    nge = np.repeat(ng, 4)
    src = c.gc[_elements(pos)] if f.compact else g[e]
    A = np.where(nge, 0.0, src.astype(f64))
    eA = np.zeros(e.size)
    if f.g16:
        inr = (e >= c.g16_begin) & (e < c.g16_end)
        A[inr] += c.g16[e[inr] - c.g16_begin].astype(f64)
        eA[inr] = U * np.abs(A[inr]) + FLOOR
    if f.scaled:
        A = A / f.scale
        eA = eA / f.scale
        eA = eA + U * (np.abs(A) + eA) + FLOOR
    p, m, v = P[e], M[e], V[e]
    if f.l1:
        co = c.coef[e].astype(f64)
        A = A + co * np.sign(p)
        eA = np.where(co != 0, eA + U * (np.abs(A) + eA) + FLOOR, eA)
    k = seg_of(c, e)
    lr, lre = lr_all[k], lre_all[k]
    t = f64(f32(f.step)) + 1.0
    bc1, bc2 = 1.0 - BETA1 ** t, 1.0 - BETA2 ** t
    p1 = p * (1.0 - lr * WD)
    m1 = m + (1.0 - BETA1) * (A - m)
    v1 = BETA2 * v + (1.0 - BETA2) * A * A
    s = np.sqrt(v1)
    d = s / np.sqrt(bc2) + EPS
    ss = lr / bc1
    y = ss * m1 / d
    p2 = p1 - y
    P[e], M[e], V[e] = p2, m1, v1
    out["kind"][e] = 1
    if not want_bound:
        return out
    rnd = lambda x, err: U * (np.abs(x) + err) + FLOOR
    e1 = np.abs(p) * WD * lre
    e1 = e1 + rnd(p1, e1) + E64 * np.abs(p)
    em = (1.0 - BETA1) * eA
    em = em + rnd(m1, em) + E64 * (np.abs(m) + np.abs(A))
    ev = (1.0 - BETA2) * (2.0 * np.abs(A) * eA + eA * eA)
    ev = ev + rnd(v1, ev) + E64 * (v + A * A)
    es = np.sqrt(v1 + ev) - np.sqrt(np.maximum(v1 - ev, 0.0))
    es = es + rnd(s, es)
    rel1 = LIB_ULPS * 2.0 ** -53 * BETA1 ** t / bc1 + 2.0 ** -52
    rel2 = 0.5 * LIB_ULPS * 2.0 ** -53 * BETA2 ** t / bc2 + 2.0 ** -51
    ed = (es + s * rel2) / np.sqrt(bc2)
    ed = ed + rnd(d, ed) + E64 * d
    ess = (lre + lr * rel1) / bc1
    ess = ess + rnd(ss, ess)
    x = ss * m1
    ex = ess * np.abs(m1) + ss * em + ess * em
    ex = ex + rnd(x, ex)
    ey = (ex + np.abs(y) * ed) / (d - ed)
    ey = ey + rnd(y, ey)
    ep = e1 + ey
    ep = ep + rnd(p2, ep)
    out["bp"][e], out["bm"][e], out["bv"][e] = ep, em, ev
    return out


def bound(c, f, g=None):
    r = step64(c, f, g)
    return r["bp"], r["bm"], r["bv"]


# ---------------------------------------------------------------------------------------------- exact parts
def decay_exact(p32, lr32, seg, wd=WD):
    """the cold groups' decay: (float)(p - (lr wd) p), fp64 expression, one rounding"""
    lrk = lr32.astype(f64)[seg]
    p = p32.astype(f64)
    return (p - lrk * wd * p).astype(f32)


def flush_exact(c, p32, log, count, n=None, wd=WD):
    """pvd_adamw_lazy_flush: every cold group takes the logged steps one after the other -> (p, status, count after)"""
    p = p32.copy()
    if count == POISON:
        return p, -1, 0
    n = c.n if n is None else n
    e = _elements(np.flatnonzero(c.cold4[:n // 4]))
    k = seg_of(c, e)
    q = p[e]
    for s in range(count):
        fac = log[s].astype(f64)[k] * wd
        q = (q.astype(f64) - fac * q.astype(f64)).astype(f32)
    p[e] = q
    return p, int(count), 0


def _tail(c, f, lr_pub, fault=None):
    """what the tail leaves: every scalar, bit for bit (lr_pub: the fp32 rates the step used)"""
    inf = f.found_inf != 0
    amp = f.amp is not None
    r = dict(step=f32(f.step), tick=None, lr=lr_pub.astype(f32), scale=f32(f.scale), tracker=int(f.tracker), found_inf=f32(f.found_inf),
             lazy_count=int(f.lazy_count), log_row=None, snapshot=None, clear=f.tail_clear is not None)
    if f.sched is not None:
        r["tick"] = f32(f.sched[3])
    if f.replay:  # the deferred part records and advances nothing
        r["clear"] = False
        return r
    if f.snapshot:
        r["snapshot"] = np.concatenate([[1.0 if inf else 0.0, f.step, f.scale if amp else 1.0, 0.0], lr_pub]).astype(f32)
    if not inf or fault == "step_on_skip":
        r["step"] = f32(f32(f.step) + f32(1))
    if f.sched is not None and not (inf and fault == "tick_frozen_on_skip"):
        r["tick"] = f32(f32(f.sched[3]) + f32(1))
    if f.cold == "lazy" and not inf:
        if f.lazy_count < f.lazy_capacity:
            r["log_row"], r["lazy_count"] = (int(f.lazy_count), lr_pub.astype(f32)), int(f.lazy_count) + 1
        else:
            r["lazy_count"] = POISON
    if amp:
        growth, backoff, interval = f.amp
        if inf:
            r["scale"], r["tracker"] = f32(f64(f32(f.scale)) * backoff), 0
        else:
            ok = f.tracker + 1
            if ok == interval:
                with np.errstate(over="ignore"):
                    ns = f32(f64(f32(f.scale)) * growth)
                if not np.isinf(ns):
                    r["scale"] = ns
                r["tracker"] = ok if fault == "tracker_no_reset" else 0
            else:
                r["tracker"] = ok
        r["found_inf"] = f32(0)
    return r


def tail_ref(c, f):
    return _tail(c, f, lr64(c, f).astype(f32))


# ---------------------------------------------------------------------------------------------- the kernel's order, in numpy
FAULTS = ("t_is_step", "bc2_no_sqrt", "eps_inside", "wd_after", "wd_in_grad", "betas_swapped", "unscale_mul", "sign0_plus", "sign_after",
          "seg_gt", "g16_index", "nograd_reads", "step_on_skip", "tick_frozen_on_skip", "tracker_no_reset")


def model32(c, f, fault=None, g=None):
    """-> dict p, m, v (fp32 [c.n]) and tail (as tail_ref) after one call, evaluated as k_adamw reads"""
    g = c.g if g is None else g
    P, M, V = c.p.copy(), c.m.copy(), c.v.copy()
    lr32 = lr64(c, f).astype(f32)
    out = dict(p=P, m=M, v=V, tail=_tail(c, f, lr32, fault))
    if f.found_inf:
        return out
    ends = c.seg_ends.astype(np.int64)

    def seg(e):  # k = 0; while (k + 1 < count && e >= end[k]) k++
        cond = (e[:, None] > ends[None, :-1]) if fault == "seg_gt" else (e[:, None] >= ends[None, :-1])
        return np.logical_and.accumulate(cond, axis=1).sum(1)

    grp, ng, pos, decay = _split(c, f)
    if decay.size:
        e = _elements(decay)
        P[e] = decay_exact(P[e], lr32, seg(e))
    e = _elements(grp)
    nge = np.repeat(ng, 4)
    src = c.gc[_elements(pos)] if f.compact else g[e]
    G = src.astype(f32) if fault == "nograd_reads" else np.where(nge, f32(0), src).astype(f32)
    if f.g16:
        inr = (e >= c.g16_begin) & (e < c.g16_end)
        idx = e[inr] % c.g16.size if fault == "g16_index" else e[inr] - c.g16_begin
        G[inr] = G[inr] + c.g16[idx].astype(f32)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        if f.scaled:
            sc = f64(f32(f.scale))
            G = (G.astype(f64) * sc if fault == "unscale_mul" else G.astype(f64) / sc).astype(f32)
        p, m, v = P[e], M[e], V[e]
        k = seg(e)
        lrk = lr32.astype(f64)[k]
        t = f64(f32(f.step)) + (0.0 if fault == "t_is_step" else 1.0)
        bc1 = 1.0 - BETA1 ** t
        bc2s = 1.0 - BETA2 ** t if fault == "bc2_no_sqrt" else np.sqrt(1.0 - BETA2 ** t)
        b1, b2 = (BETA2, BETA1) if fault == "betas_swapped" else (BETA1, BETA2)

        def update(grad):
            if fault == "wd_in_grad":
                grad = (grad + f32(WD) * p).astype(f32)
                param = p
            elif fault == "wd_after":
                param = p
            else:
                param = (p.astype(f64) - lrk * WD * p.astype(f64)).astype(f32)
            ea = (m.astype(f64) + (1.0 - b1) * (grad.astype(f64) - m.astype(f64))).astype(f32)
            es = (b2 * v.astype(f64) + (1.0 - b2) * grad.astype(f64) * grad.astype(f64)).astype(f32)
            if fault == "eps_inside":
                denom = np.sqrt(es.astype(f64) / (bc2s * bc2s) + EPS).astype(f32)
            else:
                denom = (np.sqrt(es).astype(f64) / bc2s + EPS).astype(f32)
            step_size = (lrk / bc1).astype(f32)
            param = (param - (step_size * ea).astype(f32) / denom).astype(f32)
            if fault == "wd_after":
                param = (param.astype(f64) - lrk * WD * param.astype(f64)).astype(f32)
            return param, ea, es

        grad = G
        if f.l1:
            co = c.coef[e]
            sgn = np.sign(update(G)[0]) if fault == "sign_after" else np.sign(p)
            if fault == "sign0_plus":
                sgn = np.where(p == 0, f32(1), sgn)
            grad = np.where(co != 0, (G + co * sgn.astype(f32)).astype(f32), G)
        P[e], M[e], V[e] = update(grad)
    return out


# ---------------------------------------------------------------------------------------------- the L1 sums
def _gamma(k):
    return k * U / (1.0 - k * U)


def l1_next64(c, f, p_after):
    """l1_next[b] = scale-free partial of workgroup b: sum of coef |p'| over the groups it walked -> (sums [grid], bounds [grid]).
    Depth: per group 4 products and 4 adds per thread and loop pass, 6 shuffle levels, 4 waves, the final scale."""
    grp, ng, pos, _ = _split(c, f)
    grid = grid_of(c, f)
    e = _elements(grp)
    terms = c.coef[e].astype(f64) * np.abs(p_after[e].astype(f64))
    blk = np.repeat((pos // BLOCK) % grid, 4)
    sums = np.bincount(blk, weights=terms, minlength=grid)
    passes = -(-walk(c, f)[0].size // (grid * BLOCK))
    k = 8 * passes + 6 + 4 + 1
    return sums, _gamma(k) * sums + FLOOR


def l1_ranges64(p32, ranges):
    """pvd_l1_ranges -> (sum, bound).  Depth: 4 adds per group and pass, a product and an add per range, 6 shuffle levels, 4 waves;
    then the final pass: 1024 / 256 adds per thread, 6 levels, 4 waves."""
    total, passes = 0.0, 1
    for b, e, co in ranges:
        total += float(f64(f32(co))) * np.abs(p32[b:e].astype(f64)).sum()
        passes = max(passes, -(-((e - b) // 4) // (L1_BLOCKS * BLOCK)))
    k = 4 * passes + 2 * len(ranges) + 10 + (L1_BLOCKS // BLOCK + 10)
    return total, _gamma(k) * total + FLOOR


# ---------------------------------------------------------------------------------------------- reporting
def report(label, c, f, got, ref):
    """one line: the worst err / bound over p, m, v with element, regime and segment -> (line, worst ratio)"""
    parts, worst = [], 0.0
    touched = ref["kind"] == 1
    for name, b in (("p", "bp"), ("m", "bm"), ("v", "bv")):
        err = np.abs(got[name].astype(f64) - ref[name])
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio = np.where(touched, err / ref[b], 0.0)
        ratio = np.where(np.isnan(ratio), np.inf, ratio)
        i = int(np.argmax(ratio))
        worst = max(worst, float(ratio[i]))
        parts.append("%s %.3f @%d %s seg %d" % (name, ratio[i], i, REGIMES[c.regime[i // 4]], seg_of(c, np.array([i]))[0]))
    return "[adamw fp64] %-44s max err/bound: %s" % (label, " | ".join(parts)), worst


def ulp_diff(a, b):
    """(count of elements whose bits differ, largest distance in fp32 ulps)"""
    def key(x):
        i = x.view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    d = np.abs(key(np.ascontiguousarray(a, f32)) - key(np.ascontiguousarray(b, f32)))
    return int((d != 0).sum()), int(d.max()) if d.size else 0
