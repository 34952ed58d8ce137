"""tests/adamw_ref64.py earns its place before it judges a kernel (CPU only): step64 agrees with torch.optim.AdamW on float64 CPU
tensors (the independent anchor); the float32 restatement of k_adamw's order stays inside the derived bound on every scripted case
and form (the bound is not too tight); fifteen single faults injected into that restatement each leave the bound or break an exact
part (the bound and the cases are not too loose); the scripted tables hold what they promise and validate() refuses bad lists.

Every bound test prints one max(err / bound) line per form (pytest -s); profiles/adamw_fp64_pin.txt keeps one run."""
import numpy as np
import pytest

import adamw_ref64 as R

f32, f64 = np.float32, np.float64


def _say(capsys, line):
    with capsys.disabled():
        print("\n" + line, end="")


def forms(c):
    """the forms the GPU tests run on a case, by label"""
    if c.label == "tiny":
        return {"dense": R.Form(step=1.0), "scaled+l1": R.Form(step=9.0, scaled=True, l1=True), "cosine": R.Form(sched=(1, 40.0, 5e-5, 7.0)),
                "exp": R.Form(step=999.0, sched=(2, 40.0, 0.1, 41.0))}
    if c.label.startswith("grid"):
        return {"dense": R.Form(step=1.0, scaled=True, l1=True, l1_next=True)}
    if c.label == "stride":
        return {"dense": R.Form(n=4 * R.STRIDE_DENSE, step=9.0, scaled=True, l1=True, l1_next=True),
                "warm": R.Form(step=1.0, scaled=True, l1=True, l1_next=True, cold="lazy", warm=c.warm),
                "replay": R.Form(step=1.0, scaled=True, l1=True, cold="lazy", warm=c.warm[:R.STRIDE_REPLAY], replay=True, l1_next=True)}
    both = np.concatenate([c.warm_b, c.warm_a])
    out = {"dense step %d" % s: R.Form(step=float(s)) for s in R.STEPS}
    for kind, name, param in ((1, "cosine", 5e-5), (2, "exp", 0.1)):
        for tick in (0.0, 39.0, 40.0, 41.0, 55.0):
            out["%s tick %d" % (name, tick)] = R.Form(step=tick, sched=(kind, 40.0, param, tick))
    out.update({
        "scaled": R.Form(step=1.0, scaled=True),
        "scaled+amp": R.Form(step=9.0, scaled=True, amp=(2.0, 0.5, 2000)),
        "l1": R.Form(step=1.0, l1=True, l1_next=True),
        "g16": R.Form(step=9.0, scaled=True, g16=True),
        "cold eager": R.Form(step=1.0, scaled=True, l1=True, l1_next=True, cold="eager"),
        "cold lazy": R.Form(step=999.0, scaled=True, l1=True, cold="lazy", lazy_count=3),
        "warm": R.Form(step=9.0, scaled=True, l1=True, l1_next=True, g16=True, cold="lazy", warm=c.warm),
        "warm nograd": R.Form(step=1.0, scaled=True, l1=True, cold="lazy", warm=both, nograd_from=int(c.warm_b.size)),
        "compact": R.Form(step=1.0, scaled=True, l1=True, cold="lazy", warm=c.warm, compact=True, tail_clear=(5, 3)),
        "all": R.Form(step=0.0, scaled=True, l1=True, g16=True, cold="eager", sched=(1, 40.0, 5e-5, 3.0), amp=(2.0, 0.5, 2000)),
    })
    return out


def poisoned_g(c, f):
    """the gradient the GPU tests upload: NaN wherever the call must not read it"""
    g = c.g.copy()
    if f.cold:
        g[np.repeat(c.cold4, 4)] = np.nan
    if f.nograd_from:
        g[R._elements(np.asarray(f.warm[f.nograd_from:], np.int64))] = np.nan
    if f.compact:
        g[:] = np.nan
    return g


# ---------------------------------------------------------------------------------------------- the anchor
def test_step64_matches_torch_adamw_in_float64():
    """Five steps of torch.optim.AdamW(foreach=False) on float64 CPU tensors: two parameter groups (two segments here), weight decay,
    the gradient pre-divided by the scale, the L1 term added by autograd of coef * |p|.sum().  Both sides evaluate the same real
    function in float64 with a different association (torch: p.mul_(1 - lr wd), addcdiv with step_size = lr / bc1 and
    denom = sqrt(v) / sqrt(bc2) + eps); each of the ~12 operations per step contributes at most 2^-53 relative to a term no larger than
    |p| + |update|, so after 5 steps the two differ by at most 5 * 12 * 2^-53 (|p| + lr / bc1 ...) -- asserted as 64 * 2^-53 (|p| + 1)
    for p, and 16 * 2^-53 relative for m and v (a lerp / an addcmul, 3-4 operations a step on same-sign accumulations)."""
    import torch
    rs = np.random.RandomState(0)
    n, cut = 64, 24
    c = R.Case()
    c.label, c.n, c.n4, c.n_seg = "anchor", n, n // 4, 2
    c.seg_ends = np.array([cut, n], np.uint64)
    c.lr = c.base_lr = np.array([1e-2, 3e-3], f32)
    c.l1, c.coef = [(8, 16, 1e-3)], np.zeros(n, f32)
    c.coef[8:16] = f32(1e-3)
    c.cold4, c.regime = np.zeros(n // 4, bool), np.zeros(n // 4, np.int8)
    p0 = rs.randn(n).astype(f32)
    p0[8], p0[9] = 0.0, -0.0
    tp = [torch.nn.Parameter(torch.from_numpy(p0[:cut].astype(f64))), torch.nn.Parameter(torch.from_numpy(p0[cut:].astype(f64)))]
    opt = torch.optim.AdamW([{"params": tp[:1], "lr": float(c.lr[0])}, {"params": tp[1:], "lr": float(c.lr[1])}], betas=(R.BETA1, R.BETA2),
                            eps=R.EPS, weight_decay=R.WD, foreach=False)
    P, M, V = p0.astype(f64), np.zeros(n), np.zeros(n)
    for step in range(5):
        g = (rs.randn(n) * R.SCALE).astype(f32)
        # teacher-forced in float64: the reference's own float64 state goes back in (as fp32-free arrays)
        c.p, c.m, c.v, c.g = P, M, V, g
        r = R.step64(c, R.Form(step=float(step), scaled=True, l1=True), want_bound=False)
        P, M, V = r["p"], r["m"], r["v"]
        full = torch.cat([t.reshape(-1) for t in tp])
        l1 = (float(f32(1e-3)) * full[8:16].abs()).sum()
        gl = torch.autograd.grad(l1, tp, allow_unused=True)
        gt = torch.from_numpy(g.astype(f64) / R.SCALE)
        for t, sl, extra in ((tp[0], slice(0, cut), gl[0]), (tp[1], slice(cut, n), gl[1])):
            t.grad = gt[sl].clone() + (extra if extra is not None else 0.0)
        opt.step()
    got = torch.cat([t.detach().reshape(-1) for t in tp]).numpy()
    st = [opt.state[t] for t in tp]
    m_t = torch.cat([s["exp_avg"] for s in st]).numpy()
    v_t = torch.cat([s["exp_avg_sq"] for s in st]).numpy()
    assert (np.abs(got - P) <= 64 * 2.0 ** -53 * (np.abs(P) + 1.0)).all(), np.abs(got - P).max()
    assert (np.abs(m_t - M) <= 16 * 2.0 ** -53 * np.abs(M) + 1e-300).all() and (np.abs(v_t - V) <= 16 * 2.0 ** -53 * np.abs(V) + 1e-300).all()
    assert np.abs(got - p0).max() > 1e-3  # (it did move)


# ---------------------------------------------------------------------------------------------- the bound is not too tight
@pytest.mark.parametrize("name", R.CASE_NAMES + ("grid2", "grid65"))
def test_model32_stays_inside_the_bound(name, capsys):
    c = R.case(name)
    R.assert_coverage(c)
    for label, f in forms(c).items():
        R.validate(c, f)
        g = poisoned_g(c, f)
        ref, mod = R.step64(c, f, g), R.model32(c, f, g=g)
        line, worst = R.report("model32 %s %s" % (name, label), c, f, mod, ref)
        _say(capsys, line)
        assert worst <= 1.0, line
        same = ref["kind"] == 0
        for k in "pmv":
            assert (mod[k][same].view(np.int32) == getattr(c, k)[same].view(np.int32)).all()
        assert _tails_equal(mod["tail"], R.tail_ref(c, f))
        # nothing non-finite may come out of the elements the call updates (large gradients up to 1e18 included)
        assert all(np.isfinite(ref[k][ref["kind"] == 1]).all() for k in "pmv")


def _tails_equal(a, b):
    for k in a:
        x, y = a[k], b[k]
        if k == "log_row":
            if (x is None) != (y is None) or (x is not None and (x[0] != y[0] or not np.array_equal(x[1].view(np.int32), y[1].view(np.int32)))):
                return False
        elif isinstance(x, np.ndarray):
            if not np.array_equal(x.view(np.int32), y.view(np.int32)):
                return False
        elif x is None or y is None:
            if x is not y:
                return False
        elif isinstance(x, (f32, float)):
            if f32(x).view(np.int32) != f32(y).view(np.int32):
                return False
        elif x != y:
            return False
    return True


# ---------------------------------------------------------------------------------------------- the bound is not too loose
def _skipped(f):
    return f.but(found_inf=1.0)


@pytest.mark.parametrize("fault", R.FAULTS)
def test_an_injected_fault_leaves_the_bound_or_breaks_an_exact_part(fault, capsys):
    caught = []
    for name in ("small", "tiny"):
        c = R.case(name)
        todo = dict(forms(c))
        todo.update({k + " skipped": _skipped(f) for k, f in list(todo.items()) if f.amp or f.sched})
        if name == "small":
            todo["growth"] = R.Form(step=1.0, scaled=True, amp=(2.0, 0.5, 3), tracker=2)
        for label, f in todo.items():
            g = poisoned_g(c, f)
            ref, mod = R.step64(c, f, g), R.model32(c, f, fault=fault, g=g)
            _, worst = R.report("", c, f, mod, ref)
            exact = _tails_equal(mod["tail"], R.tail_ref(c, f))
            if not (worst <= 1.0) or not exact:
                caught.append("%s %s (%s)" % (name, label, "bound x %.3g" % worst if not (worst <= 1.0) else "exact part"))
    _say(capsys, "[adamw fp64] fault %-20s caught by %d forms, first: %s" % (fault, len(caught), caught[0] if caught else "-"))
    assert caught, "no scripted case notices the fault %r: the cases are too weak" % fault


# ---------------------------------------------------------------------------------------------- exact parts, tables, lists
def test_exact_parts_on_the_cpu():
    c = R.case("small")
    cold_el = np.repeat(c.cold4, 4)
    # a flush of k logged steps == k eager decays, warm elements untouched, the poison replays nothing
    log = np.stack([c.lr, c.base_lr, c.lr]).astype(f32)
    p, status, count = R.flush_exact(c, c.p, log, 3)
    q = c.p.copy()
    k = R.seg_of(c, np.arange(c.n))
    for row in log:
        q[cold_el] = R.decay_exact(q[cold_el], row, k[cold_el])
    assert np.array_equal(p.view(np.int32), q.view(np.int32)) and status == 3 and count == 0
    z = cold_el & (c.p == 0)
    # zeros stay zeros; (-0) - f (-0) is +0 in IEEE arithmetic (torch's fused kernel, `param -= lr * wd * param`, gives the same), so
    # a -0 loses its sign bit at the first replayed step and keeps it through an empty log
    assert z.any() and np.signbit(c.p[z]).any() and (p[z] == 0).all() and not np.signbit(p[z]).any()
    p_none = R.flush_exact(c, c.p, log, 0)[0]
    assert np.array_equal(p_none.view(np.int32), c.p.view(np.int32))
    assert np.array_equal(p[~cold_el].view(np.int32), c.p[~cold_el].view(np.int32)) and (p[cold_el & (c.p != 0)] != c.p[cold_el & (c.p != 0)]).any()
    p, status, count = R.flush_exact(c, c.p, log, R.POISON)
    assert np.array_equal(p.view(np.int32), c.p.view(np.int32)) and status == -1 and count == 0
    # GradScaler: growth after `interval` clean steps, the isinf guard, backoff
    t = R.tail_ref(c, R.Form(scaled=True, amp=(2.0, 0.5, 3), tracker=2))
    assert t["scale"] == f32(128) and t["tracker"] == 0 and t["step"] == f32(1)
    t = R.tail_ref(c, R.Form(scaled=True, amp=(2.0, 0.5, 3), tracker=2, scale=float(f32(3e38))))
    assert t["scale"] == f32(3e38) and t["tracker"] == 0
    t = R.tail_ref(c, R.Form(scaled=True, amp=(2.0, 0.5, 3), tracker=2, found_inf=1.0, sched=(1, 40.0, 5e-5, 7.0), cold="lazy", lazy_count=2))
    assert t["scale"] == f32(32) and t["tracker"] == 0 and t["step"] == f32(0) and t["tick"] == f32(8) and t["lazy_count"] == 2 and t["found_inf"] == 0
    t = R.tail_ref(c, R.Form(cold="lazy", lazy_count=16, lazy_capacity=16))
    assert t["lazy_count"] == R.POISON and t["log_row"] is None
    # the sums
    s, b = R.l1_ranges64(c.p, c.l1)
    assert abs(s - sum(float(f32(co)) * np.abs(c.p[b0:e0].astype(f64)).sum() for b0, e0, co in c.l1)) <= 1e-12 and 0 < b < 1e-4 * s


def test_validate_refuses_lists_that_leave_the_buffers():
    c = R.case("small")
    ok = R.Form(cold="lazy", warm=c.warm)
    assert R.validate(c, ok)
    for bad in (np.append(c.warm, c.n4).astype(np.int32), c.warm[::-1].copy(), np.append(c.warm, c.warm[-1]).astype(np.int32),
                np.sort(np.append(c.warm, np.flatnonzero(c.cold4)[0])).astype(np.int32), np.array([-1], np.int32)):
        with pytest.raises(AssertionError):
            R.validate(c, ok.but(warm=bad))
    with pytest.raises(AssertionError):
        R.validate(c, R.Form(warm=c.warm))  # a list without the deferred decay
    with pytest.raises(AssertionError):
        R.validate(c, R.Form(n=c.n + 4))
    for name in R.CASE_NAMES + tuple("grid%d" % g for g in R.GRIDS):
        cc = R.case(name)
        R.assert_coverage(cc)
        for f in forms(cc).values():
            assert R.validate(cc, f)
        assert R.pack_bits(cc.cold4).size * 32 >= cc.n4
