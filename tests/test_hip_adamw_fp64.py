"""The flat AdamW kernels of csrc/optimizer.hip (k_adamw in every form, its tail, k_adamw_lazy_flush, the L1 sums, the finite checks,
the gather-zero-check of the ray-DP exchange) against tests/adamw_ref64.py: one teacher-forced call per test step, p / m / v element
by element under the bound derived there, everything without a library call bit for bit.  Everything goes through pvd_hip directly.

Every buffer a kernel receives has PAD sentinel elements behind it that must come back untouched; m and v of cold groups and g of
entries the call must not read hold NaN.  The scripted cases (adamw_ref64.case, checked by assert_coverage / validate before anything
is uploaded) hold four gradient regimes (normal x 64, zero with live moments, tiny so that sqrt(v') straddles eps, large up to 1e18),
+-0 parameters inside L1 ranges, 16 segments with an empty one and one of 4 elements, steps 0 / 1 / 9 / 999, n no multiple of 128;
"stride" is the only place where the second pass of the grid-stride loop and its prefetch are checked element by element.

Every test prints its worst err / bound with element, regime and segment, and how far the kernel is from the float32 restatement
(pytest -s); profiles/adamw_fp64_pin.txt keeps the lines of one run on the MI355X.  Those numbers are a record; the threshold is the
bound.  Out of scope: FlatAdamW / FlatGradScaler host logic, the multi-rank exchange, gradients that overflow v.  No hipGraph is
recorded here."""
import copy

import numpy as np
import pytest
import torch

import adamw_ref64 as R
from test_adamw_ref64 import forms, poisoned_g

pytestmark = pytest.mark.gpu

SENT = -1.2345e11
f32, f64 = np.float32, np.float64
L1_SCALE = 0.5


def _say(capsys, line):
    with capsys.disabled():
        print("\n" + line, end="")


def _pad_host(a, pad=R.PAD):
    a = np.ascontiguousarray(a)
    with np.errstate(over="ignore"):
        tail = np.full((pad,) + a.shape[1:], SENT if a.dtype.kind == "f" else 0x5A5A5A5A, a.dtype)
    return np.concatenate([a, tail])


def _pad(a, pad=R.PAD):
    return torch.from_numpy(_pad_host(a, pad)).cuda()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.int16, 4: np.int32}[a.dtype.itemsize])


def _same(t, host, what):
    """the device tensor still holds these bits, padding included"""
    got = t.cpu().numpy()
    k = host.shape[0]
    assert np.array_equal(_bits(got[:k]), _bits(host)), what + " was written"
    ref = _pad_host(np.zeros((0,) + host.shape[1:], host.dtype), pad=got.shape[0] - k)
    assert np.array_equal(_bits(got[k:]), _bits(ref)), "the padding behind " + what + " was written"


def _run(c, f, capsys=None, label=None):
    """one call of pvd_hip.adamw_step in the form f on the state of case c, everything checked -> what the device left"""
    import pvd_hip
    R.validate(c, f)
    n, skip = R.n_of(c, f), f.found_inf != 0
    cold_el = np.repeat(c.cold4, 4)
    g0 = poisoned_g(c, f)
    m0, v0 = c.m.copy(), c.v.copy()
    if f.cold:
        m0[cold_el], v0[cold_el] = np.nan, np.nan
    p, g, m, v = _pad(c.p), _pad(g0), _pad(m0), _pad(v0)
    lr_live = R.lr_in(c, f) * f32(3) if (f.sched is not None or f.replay) else R.lr_in(c, f)  # a schedule / a record must not read it
    step_live = f.step + 5.0 if f.replay else f.step
    flag_live = 1.0 - f.found_inf if f.replay else f.found_inf
    lr, base = _pad(lr_live), _pad(c.base_lr)
    step, flag, scale = _pad(np.array([step_live], f32)), _pad(np.array([flag_live], f32)), _pad(np.array([f.scale * (4 if f.replay else 1)], f32))
    tick = _pad(np.array([f.sched[3] if f.sched else 0.0], f32))
    tracker = _pad(np.array([f.tracker], np.int32))
    kw, keep = {}, []
    if f.sched is not None:
        kw["schedule"] = (f.sched[0], f.sched[1], f.sched[2], base[:16], tick[:1])
    if f.l1:
        kw["l1_ranges"] = c.l1
    if f.amp is not None:
        kw["amp_update"] = (scale[:1], tracker[:1]) + tuple(f.amp)
    if f.g16:
        g16 = _pad(c.g16)
        kw["half_grad"] = (c.g16_begin, c.g16_end, g16[:c.g16.size])
        keep.append((g16, c.g16, "g16"))
    l1n = _pad(np.full(R.MAX_BLOCKS, SENT, f32))
    if f.l1_next:
        kw["l1_next"] = (l1n[:R.MAX_BLOCKS], L1_SCALE)
    if f.cold:
        words = R.pack_bits(c.cold4)
        bits = _pad(words)
        kw["cold_bits"] = bits[:words.size]
        keep.append((bits, words, "the cold bitmap"))
    log0 = np.full((f.lazy_capacity, 16), SENT, f32)
    log, count = _pad(log0, pad=2), _pad(np.array([f.lazy_count], np.uint32).view(np.int32))
    if f.cold == "lazy":
        lazy = [log[:f.lazy_capacity], count[:1]]
        if f.warm is not None:
            wl = np.asarray(f.warm, np.int32)
            warm = _pad(wl)
            lazy += [warm[:wl.size], int(f.nograd_from)]
            keep.append((warm, wl, "the warm list"))
        kw["lazy"] = tuple(lazy)
    snap0 = np.full(20, SENT, f32)
    if f.replay:
        snap0 = np.concatenate([[f.found_inf, f.step, f.scale, 0.0], R.lr_in(c, f)]).astype(f32)
    snap = _pad(snap0)
    if f.snapshot:
        kw["snapshot"] = snap[:20]
    if f.replay:
        kw["replay"] = snap[:20]
    arrivals = _pad(np.zeros(65 * 32, np.int32))
    if f.arrivals:
        kw["arrivals"] = arrivals[:65 * 32]
    if f.compact:
        nw = len(f.warm)
        gc, pc = _pad(c.gc[:4 * nw]), _pad(np.full(4 * nw, SENT, f32))
        kw["compact_grad"], kw["compact_param_out"] = gc[:4 * nw], pc[:4 * nw]
        keep.append((gc, c.gc[:4 * nw], "the compact gradient"))
    if f.tail_clear is not None:
        stride, cnt = f.tail_clear
        tc = _pad(np.full(stride * cnt, SENT, f32))
        kw["tail_clear"] = (tc[:stride * cnt], stride, cnt)
    grad_scale = (snap[2:3] if f.replay else scale[:1]) if f.scaled else None
    pvd_hip.adamw_step(p[:n], g[:n], m[:n], v[:n], [int(e) for e in c.seg_ends], lr[:16], R.BETA1, R.BETA2, R.EPS, R.WD, step[:1], grad_scale,
                       None if f.replay else flag[:1], zero_after=f.zero_after, **kw)
    torch.cuda.synchronize()
    got = {k: t.cpu().numpy() for k, t in (("p", p), ("m", m), ("v", v), ("g", g))}
    for t, host, what in keep + [(base, c.base_lr, "base_lr")]:
        _same(t, host, what)
    # ---- the scalars, bit for bit
    ref_t = R.tail_ref(c, f)
    lr_got = lr.cpu().numpy()
    if f.replay:  # the deferred part touches no live scalar and not the record
        _same(lr, lr_live, "lr"), _same(step, np.array([step_live], f32), "step"), _same(flag, np.array([flag_live], f32), "found_inf")
        _same(scale, np.array([f.scale * 4], f32), "scale"), _same(snap, snap0, "the record")
        lr_used = R.lr_in(c, f)
    else:
        lr_used = lr_got[:16]
        if f.sched is not None:
            worst_lr = R.ulp_diff(lr_used, ref_t["lr"])[1]
            assert worst_lr <= 1, "published rate %d ulps from the closed form" % worst_lr
        else:
            assert np.array_equal(_bits(lr_used), _bits(ref_t["lr"]))
        _same(lr, lr_used, "lr")
        _same(step, np.array([ref_t["step"]], f32), "step")
        _same(flag, np.array([ref_t["found_inf"]], f32), "found_inf")
        _same(scale, np.array([ref_t["scale"]], f32), "scale")
    _same(tracker, np.array([ref_t["tracker"]], np.int32), "the growth tracker")
    _same(tick, np.array([ref_t["tick"] if f.sched else 0.0], f32), "the scheduler tick")
    _same(count, np.array([ref_t["lazy_count"]], np.uint32).view(np.int32), "lazy_count")
    log_ref = log0.copy()
    if ref_t["log_row"] is not None:
        log_ref[ref_t["log_row"][0]] = lr_used  # the rates as published
    _same(log, log_ref, "the lazy log")
    if f.snapshot:
        want = ref_t["snapshot"].copy()
        want[4:] = lr_used
        _same(snap, want, "the record")
    elif not f.replay:
        _same(snap, snap0, "the record")
    _same(arrivals, np.zeros(65 * 32, np.int32), "arrivals (counters back at zero)")
    if f.tail_clear is not None:
        want = np.full(stride * cnt, SENT, f32)
        if ref_t["clear"]:
            want[::stride] = 0.0
        _same(tc, want, "tail_clear")
    # ---- the gradient: zeroed exactly where zero_after says, untouched elsewhere
    g_ref = g0.copy()
    grp, ng = R.walk(c, f)
    if f.zero_after:
        z = grp[~ng]
        if f.cold and f.warm is None:
            z = z[~c.cold4[z]]
        g_ref[R._elements(z)] = 0.0
    _same(g, g_ref, "g")
    # ---- p, m, v
    ref = R.step64(c, f, g0)
    state0 = dict(p=c.p, m=m0, v=v0)
    for k in "pmv":
        same = ref["kind"] == 0
        assert np.array_equal(_bits(got[k][:c.n][same]), _bits(state0[k][same])), k + ": an element the call does not own was written"
        _same({"p": p, "m": m, "v": v}[k][c.n:], np.zeros(0, f32), k)
    dec = ref["kind"] == 2
    if dec.any():
        want = R.decay_exact(c.p[dec], lr_used, R.seg_of(c, np.flatnonzero(dec)))
        assert np.array_equal(_bits(got["p"][:c.n][dec]), _bits(want)), "cold decay is not (float)(p - lr wd p)"
        assert np.isnan(got["m"][:c.n][dec]).all() and np.isnan(got["v"][:c.n][dec]).all()
    view = {k: got[k][:c.n] for k in "pmv"}
    line, worst = R.report("hip %s %s" % (c.label, label), c, f, view, ref)
    if not skip and c.n <= 1 << 22:  # the record: distance from the float32 restatement (not asserted: device pow / cos / sqrtf)
        mod = R.model32(c, f, g=g0)
        upd = ref["kind"] == 1
        line += " || vs model32: " + ", ".join("%s %d differ, max %d ulp" % ((k,) + R.ulp_diff(view[k][upd], mod[k][upd])) for k in "pmv")
    if capsys is not None:
        _say(capsys, line)
    assert worst <= 1.0, line
    # ---- side outputs
    l1_got = l1n.cpu().numpy()
    grid = R.grid_of(c, f)
    if f.l1_next and not skip:
        sums, bnd = R.l1_next64(c, f, view["p"])
        err = np.abs(l1_got[:grid].astype(f64) - L1_SCALE * sums)
        assert (err <= L1_SCALE * bnd).all(), "l1_next: err / bound %.3f" % (err / (L1_SCALE * bnd)).max()
        assert sums.sum() > 0
        _same(l1n[grid:], np.zeros(0, f32), "l1_next past the grid")
    else:
        _same(l1n, np.full(R.MAX_BLOCKS, SENT, f32), "l1_next (a skipped step keeps the old partials)")
    if f.compact:
        _same(pc, view["p"][R._elements(grp)], "compact_param_out != the updated parameters")
    got.update(lr=lr_used, step=step.cpu().numpy()[0], scale=scale.cpu().numpy()[0], tracker=int(tracker.cpu().numpy()[0]), flag=flag.cpu().numpy()[0],
               count=int(count.cpu().numpy().view(np.uint32)[0]), log=log.cpu().numpy()[:f.lazy_capacity], snap=snap.cpu().numpy()[:20],
               tick=tick.cpu().numpy()[0], view=view, worst=worst)
    return got


def _after(c, got):
    """the case with the device's p / m / v as its state (cold moments back to their zeros): the next teacher-forced call"""
    c2 = copy.copy(c)
    cold_el = np.repeat(c.cold4, 4)
    c2.p, c2.m, c2.v = got["view"]["p"].copy(), np.where(cold_el, f32(0), got["view"]["m"]), np.where(cold_el, f32(0), got["view"]["v"])
    return c2


# ---------------------------------------------------------------------------------------------- the library allowance
def test_device_pow_cos_allowance(capsys):
    """LIB_ULPS of adamw_ref64: the device's fp64 pow / cos against numpy over every scripted t and tick, in fp64 ulps (x 2 = margin)"""
    ts = np.array([s + 1.0 for s in R.STEPS] + [2.0, 40.0, 56.0])
    ticks = np.array([0.0, 3.0, 7.0, 39.0, 40.0, 41.0, 55.0])
    rows = [("pow(0.9, t)", np.full(ts.size, R.BETA1), ts), ("pow(0.99, t)", np.full(ts.size, R.BETA2), ts),
            ("pow(0.1, min(tick / T, 1))", np.full(ticks.size, f64(f32(0.1))), np.minimum(ticks / 40.0, 1.0))]
    worst = 0.0
    for name, a, b in rows:
        dev = torch.pow(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()).cpu().numpy()
        ulps = np.abs(dev - a ** b) / np.spacing(a ** b)
        _say(capsys, "[adamw fp64] device %-28s max %.1f fp64 ulp from numpy" % (name, ulps.max()))
        worst = max(worst, ulps.max())
    x = np.pi * ticks / 40.0
    dev = torch.cos(torch.from_numpy(x).cuda()).cpu().numpy()
    ulps = np.abs(dev - np.cos(x)) / np.maximum(np.spacing(np.abs(np.cos(x))), 2.0 ** -53)
    _say(capsys, "[adamw fp64] device %-28s max %.1f fp64 ulp from numpy" % ("cos(pi tick / T)", ulps.max()))
    worst = max(worst, ulps.max())
    assert 2 * worst <= R.LIB_ULPS, "adamw_ref64.LIB_ULPS must be twice the measured %.1f" % worst


# ---------------------------------------------------------------------------------------------- one call per path
SMALL = sorted(forms(R.case("small")))
EXTRA = {
    "zero_after": lambda c: R.Form(step=1.0, scaled=True, l1=True, zero_after=True),
    "zero_after cold": lambda c: R.Form(step=1.0, scaled=True, l1=True, cold="eager", zero_after=True),
    "zero_after warm nograd": lambda c: R.Form(step=9.0, scaled=True, l1=True, cold="lazy", warm=np.concatenate([c.warm_b, c.warm_a]),
                                               nograd_from=int(c.warm_b.size), zero_after=True, l1_next=True),
    "arrivals amp sched": lambda c: R.Form(step=9.0, scaled=True, l1=True, amp=(2.0, 0.5, 2000), sched=(2, 40.0, 0.1, 9.0), arrivals=True,
                                           zero_after=True, cold="lazy", warm=c.warm, lazy_count=1, l1_next=True),
    "compact arrivals": lambda c: R.Form(step=1.0, scaled=True, l1=True, amp=(2.0, 0.5, 2000), cold="lazy", warm=c.warm, compact=True,
                                         tail_clear=(7, 4), arrivals=True, zero_after=True, l1_next=True),
}


def _form(c, label):
    return EXTRA[label](c) if label in EXTRA else forms(c)[label]


@pytest.mark.parametrize("label", SMALL + sorted(EXTRA))
def test_one_step_on_small(label, capsys):
    c = R.case("small")
    R.assert_coverage(c)
    _run(c, _form(c, label), capsys, label)


@pytest.mark.parametrize("label", SMALL + sorted(EXTRA))
def test_a_skipped_step_on_small(label, capsys):
    """found_inf = 1 through each form: nothing but the documented side effects (_run checks every one): p / m / v untouched, pc <- p,
    g zeroed only under zero_after, l1_next keeps its partials, backoff, the scheduler tick advances, the log does not grow."""
    c = R.case("small")
    f = _form(c, label).but(found_inf=1.0)
    got = _run(c, f, None, label + " skipped")
    assert got["step"] == f32(f.step) and got["count"] == f.lazy_count
    if f.amp is not None:
        assert got["scale"] == f32(f.scale * 0.5) and got["flag"] == 0
    if f.sched is not None:
        assert got["tick"] == f32(f.sched[3] + 1)


def test_snapshot_then_replay_uses_the_record(capsys):
    """The two-part update: part B (list warm_b, tail, record) and then part A (list warm_a) from the record, while the live found_inf,
    step, scale and rates hold other values (_run sets them so): only the record can give the right answer."""
    c = R.case("small")
    fb = R.Form(step=9.0, scaled=True, l1=True, amp=(2.0, 0.5, 2000), sched=(1, 40.0, 5e-5, 9.0), cold="lazy", warm=c.warm_b, snapshot=True)
    b = _run(c, fb, capsys, "snapshot (part B)")
    assert b["snap"][0] == 0 and b["snap"][1] == f32(9) and b["snap"][2] == f32(R.SCALE) and b["snap"][3] == 0
    c2 = _after(c, b)
    fa = R.Form(step=float(b["snap"][1]), found_inf=float(b["snap"][0]), scale=float(b["snap"][2]), lr=b["snap"][4:20].copy(), scaled=True, l1=True,
                cold="lazy", warm=c.warm_a, replay=True, lazy_count=1)
    a = _run(c2, fa, capsys, "replay (part A)")
    assert (a["view"]["m"][R._elements(c.warm_a.astype(np.int64))] != c.m[R._elements(c.warm_a.astype(np.int64))]).any()
    # a recorded skip: part A does nothing either, whatever the live flag says
    _run(c2, fa.but(found_inf=1.0), None, "replay of a skipped step")


def test_growth_after_three_clean_steps_and_the_isinf_guard(capsys):
    c = R.case("tiny")
    scale, tracker, seen = R.SCALE, 0, []
    for k in range(4):
        got = _run(c, R.Form(step=float(k), scaled=True, amp=(2.0, 0.5, 3), scale=scale, tracker=tracker), None, "growth %d" % k)
        scale, tracker = float(got["scale"]), got["tracker"]
        seen.append((scale, tracker))
    assert seen == [(64.0, 1), (64.0, 2), (128.0, 0), (128.0, 1)]
    big = float(f32(3e38))  # scale * 2 overflows: the scale stays, the tracker starts again
    got = _run(c, R.Form(step=4.0, scaled=True, amp=(2.0, 0.5, 3), scale=big, tracker=2), None, "isinf guard")
    assert got["scale"] == f32(big) and got["tracker"] == 0 and got["step"] == f32(5)
    got = _run(c, R.Form(step=4.0, scaled=True, amp=(2.0, 0.5, 3), scale=big, tracker=2, arrivals=True), None, "isinf guard, in-kernel tail")
    assert got["scale"] == f32(big) and got["tracker"] == 0


def test_lazy_log_overflow_poisons_and_the_flush_refuses(capsys):
    import pvd_hip
    c = R.case("small")
    cap, count, log = 3, 0, None
    for k in range(cap + 1):
        f = R.Form(step=float(k), scaled=True, cold="lazy", warm=c.warm, lazy_capacity=cap, lazy_count=count)
        got = _run(c, f, None, "log %d" % k)
        count = got["count"]
    assert count == R.POISON
    # the flush on the device's own log: capacity steps replayed bit for bit, then the poisoned count -> p untouched, status -1
    words = R.pack_bits(c.cold4)
    rows = np.stack([c.lr, c.base_lr, (c.lr * f32(0.5)).astype(f32)])
    for cnt in (cap, 0, R.POISON):
        p, bits, logt = _pad(c.p), _pad(words), _pad(rows, pad=2)
        ct, status = _pad(np.array([cnt], np.uint32).view(np.int32)), _pad(np.array([77], np.int32))
        pvd_hip.adamw_lazy_flush(p[:c.n], [int(e) for e in c.seg_ends], bits[:words.size], logt[:cap], ct[:1], R.WD, status[:1])
        want, st, left = R.flush_exact(c, c.p, rows, cnt)
        _same(p, want, "p after the flush (cnt %d)" % cnt)
        _same(status, np.array([st], np.int32), "status"), _same(ct, np.array([left], np.int32), "lazy_count"), _same(logt, rows, "the log")
    assert st == -1


@pytest.mark.parametrize("G", R.GRIDS)
def test_in_kernel_tail_runs_exactly_once_at_every_grid_size(G, capsys):
    c = R.case("grid%d" % G)
    R.assert_coverage(c)
    f = R.Form(step=1.0, scaled=True, l1=True, l1_next=True, amp=(2.0, 0.5, 2000), sched=(1, 40.0, 5e-5, 1.0), arrivals=True)
    assert R.grid_of(c, f) == G
    got = _run(c, f, capsys, "arrivals, %d workgroups" % G)
    assert got["step"] == f32(2) and got["tick"] == f32(2) and got["tracker"] == 1  # (the counters are checked by _run)
    got = _run(c, f.but(found_inf=1.0), None, "arrivals skipped")  # every workgroup returns early and still announces itself
    assert got["step"] == f32(1) and got["tick"] == f32(2) and got["scale"] == f32(32)


@pytest.mark.parametrize("label", ["dense", "warm", "replay"])
def test_second_loop_pass_on_stride(label, capsys):
    c = R.case("stride")
    R.assert_coverage(c)
    f = forms(c)[label]
    grid = R.grid_of(c, f)
    assert R.walk(c, f)[0].size > grid * R.BLOCK and R.walk(c, f)[0].size % R.BLOCK == 37
    _run(c, f, capsys, label)


def test_check_finite_sees_the_second_pass():
    import pvd_hip
    c = R.case("stride")
    n = 4 * R.STRIDE_DENSE
    g = _pad(c.g[:n])
    flag = _pad(np.zeros(1, f32))
    pvd_hip.check_finite(g[:n], flag[:1])
    _same(flag, np.zeros(1, f32), "found_inf on a finite buffer")
    for group, bad in ((0, np.inf), (R.MAX_BLOCKS * R.BLOCK, -np.inf), (R.STRIDE_DENSE - 1, np.nan)):
        keep = float(g[4 * group + 3])
        g[4 * group + 3] = float(bad)
        flag[:1].zero_()
        pvd_hip.check_finite(g[:n], flag[:1])
        _same(flag, np.ones(1, f32), "found_inf (group %d)" % group)
        g[4 * group + 3] = keep
    g[n] = float("inf")  # just behind the buffer: not looked at
    flag[:1].zero_()
    pvd_hip.check_finite(g[:n], flag[:1])
    assert float(flag[0]) == 0.0


def test_tiny_every_scalar_form(capsys):
    c = R.case("tiny")
    R.assert_coverage(c)
    todo = dict(forms(c))
    todo["amp arrivals"] = R.Form(step=1.0, scaled=True, l1=True, l1_next=True, amp=(2.0, 0.5, 2000), sched=(2, 40.0, 0.1, 41.0), arrivals=True,
                                  zero_after=True, snapshot=True)
    todo["warm compact"] = R.Form(step=1.0, scaled=True, cold="lazy", warm=c.warm, compact=True, tail_clear=(1, 1))
    for label, f in todo.items():
        _run(c, f, capsys, label)
        _run(c, f.but(found_inf=1.0), None, label + " skipped")


# ---------------------------------------------------------------------------------------------- the sums
@pytest.mark.parametrize("name", ["small", "tiny", "stride"])
def test_l1_ranges_against_float64(name, capsys):
    import pvd_hip
    c = R.case(name)
    ranges = list(c.l1)
    if name == "stride":  # a range of more groups than 1024 workgroups hold in one pass, ragged
        ranges = [(8, 8 + 4 * (R.L1_BLOCKS * R.BLOCK + 37), 3e-3)] + ranges[:1]
    p = _pad(c.p)
    for with_out in (True, False):
        scratch, out = _pad(np.full(R.L1_BLOCKS, SENT, f32)), _pad(np.full(1, SENT, f32))
        pvd_hip.l1_ranges(p[:c.n], ranges, scratch[:R.L1_BLOCKS], out[:1] if with_out else None)
        want, bnd = R.l1_ranges64(c.p, ranges)
        part = scratch.cpu().numpy()
        got = float(out[0]) if with_out else float(part[:R.L1_BLOCKS].astype(f64).sum())
        _say(capsys, "[adamw fp64] l1_ranges %-6s out=%-5s err/bound %.3f" % (name, with_out, abs(got - want) / bnd))
        assert abs(got - want) <= bnd and want > 0
        assert (part[R.L1_BLOCKS:] == f32(SENT)).all() and (out.cpu().numpy()[1:] == f32(SENT)).all()
        if not with_out:
            _same(out, np.full(1, SENT, f32), "out")
    _same(p, c.p, "p")


# ---------------------------------------------------------------------------------------------- the exchange's gather
@pytest.mark.parametrize("bad_in", ["none", "first", "last"])
@pytest.mark.parametrize("n_slots", [1, 3, 64])
def test_segments_gather_zero_check_against_indexing(bad_in, n_slots):
    import pvd_hip
    rs = np.random.RandomState(7)
    lens = [0, 1, 3, 4, 1025, 1024, 8, 2052, 5] + [4] * 300  # aligned and unaligned, more segments than one workgroup's worth of lanes
    n_flat = 40000
    starts, dsts, pos, dpos = [], [], 12, 0
    for k, ln in enumerate(lens):
        pos += 4 * rs.randint(1, 4)
        if ln % 4 == 0 and k % 2 == 1:  # start, dst and len on the 4-element grid: the float4 path (2052: more than one pass of it)
            pos, dpos = (pos + 3) // 4 * 4, (dpos + 3) // 4 * 4
        elif k % 3 == 0:
            pos += 1
        starts.append(pos)
        dsts.append(dpos)
        pos, dpos = pos + ln, dpos + ln + (3 if k % 5 == 0 else 0)  # gaps in the compact buffer stay untouched
    assert pos <= n_flat
    segs = np.stack([starts, dsts, lens], 1).astype(np.int32)
    on_grid = (segs[:, 0] | segs[:, 1] | segs[:, 2]) & 3 == 0
    assert on_grid[[3, 5, 7]].all() and not on_grid[[1, 2, 4, 8]].any() and (~on_grid[9:] & (segs[9:, 2] == 4)).any()
    flat0 = rs.randn(n_flat).astype(f32)
    if bad_in == "first":
        flat0[segs[1, 0]] = np.inf  # (segment 0 is empty: the first segment that holds anything)
    if bad_in == "last":
        flat0[segs[-1, 0] + 3] = np.nan
    n_buf, stride = dpos + 8, 37
    flat, buf, st = _pad(flat0), _pad(np.full(n_buf, SENT, f32)), _pad(segs, pad=2)
    slots = _pad(np.full(64 * stride, SENT, f32))
    pvd_hip.segments_gather_zero_check(flat[:n_flat], st[:len(lens)], buf[:n_buf], slots[:64 * stride], stride, n_slots)
    want_flat, want_buf, want_slots = flat0.copy(), np.full(n_buf, SENT, f32), np.full(64 * stride, SENT, f32)
    for s, d, ln in segs:
        want_buf[d:d + ln] = flat0[s:s + ln]
        want_flat[s:s + ln] = 0.0
    if bad_in != "none":
        want_slots[:n_slots * stride:stride] = 1.0
    _same(flat, want_flat, "flat outside the ranges / not zeroed inside")
    _same(buf, want_buf, "the compact buffer")
    _same(slots, want_slots, "a flag word")
    _same(st, segs, "the segment table")
