"""tests/composite_ref64.py earns its place before it judges a kernel (CPU only): its backward is the gradient of its forward
(central finite differences in float64, every scripted ray); a float32 numpy restatement of the KERNEL's order (64-lane
Hillis-Steele scans, excl from lane - 1, carries from lane 63) and one of the reference's sequential order stay inside the derived
bound on every case (the bound is not too tight); ten single faults injected into the wave model each leave it (the bound and the
inputs are not too loose); the scripted tables hold what they promise.

Every bound test prints one max(err / bound) line (pytest -s); profiles/composite_fp64_pin.txt keeps one run."""
import functools

import numpy as np
import pytest

import composite_ref64 as R

f32 = np.float32
ONE, ZERO = f32(1), f32(0)
MUTANTS = ["T_carry", "t_carry", "excl0", "pre_T", "r_carry", "no_unblend", "no_g_bg", "delta1", "nonstrict", "inactive"]


def _say(capsys, line):
    with capsys.disabled():
        print("\n" + line, end="")


# ---------------------------------------------------------------------------------------------- float32 models
def _scan(v, op):
    v = v.copy()
    off = 1
    while off < 64:
        v[off:] = op(v[off:], v[:-off])
        off <<= 1
    return v


def _wave_sum(v):
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        v = v + v[lanes ^ off]
    return v[0]


def _chunk(sig, rgb, dl, base, mut):
    n_in = min(64, sig.shape[0] - base)
    alpha, d0, d1, c = np.zeros(64, f32), np.zeros(64, f32), np.zeros(64, f32), np.zeros((64, 3), f32)
    sl = slice(base, base + n_in)
    d0[:n_in], d1[:n_in], c[:n_in] = dl[sl, 0], dl[sl, 1], rgb[sl]
    alpha[:n_in] = ONE - np.exp(-sig[sl] * d0[:n_in])
    if "inactive" in mut:
        alpha[n_in:] = f32(0.5)
    return n_in, alpha, d0, d1, c


def wave_forward_ray(sig, rgb, dl, mut=()):
    acc = np.zeros((64, 5), f32)
    T_carry, t_carry = ONE, ZERO
    for base in range(0, sig.shape[0], 64):
        n_in, alpha, d0, d1, c = _chunk(sig, rgb, dl, base, mut)
        incl = _scan(ONE - alpha, np.multiply)
        excl = np.concatenate([[incl[63] if "excl0" in mut else ONE], incl[:-1]]).astype(f32)
        w = alpha * (T_carry * excl)
        t = t_carry + _scan(d1, np.add)
        acc[:, :3] += w[:, None] * c
        acc[:, 3] += w
        acc[:, 4] += w * t
        T_carry = ONE if "T_carry" in mut else T_carry * incl[63]
        t_carry = ZERO if "t_carry" in mut else t[63]
    return [_wave_sum(acc[:, k].copy()) for k in range(5)]  # r g b ws depth


def wave_backward_ray(sig, rgb, dl, g, gws, F, wsF, mut=()):
    L = sig.shape[0]
    gs, gr = np.zeros(L, f32), np.zeros((L, 3), f32)
    T_carry, carry = ONE, np.zeros(4, f32)
    for base in range(0, L, 64):
        n_in, alpha, d0, d1, c = _chunk(sig, rgb, dl, base, mut)
        if "delta1" in mut:
            d0 = d1
            alpha[:n_in] = ONE - np.exp(-sig[base:base + n_in] * d0[:n_in])
        incl = _scan(ONE - alpha, np.multiply)
        excl = np.concatenate([[incl[63] if "excl0" in mut else ONE], incl[:-1]]).astype(f32)
        Tpre = T_carry * excl
        w = alpha * Tpre
        T = T_carry * incl
        pre = [carry[k] + _scan(w * c[:, k], np.add) for k in range(3)] + [carry[3] + _scan(w, np.add)]
        Tg = Tpre if "pre_T" in mut else T
        val = d0 * (g[0] * (Tg * c[:, 0] - (F[0] - pre[0])) + g[1] * (Tg * c[:, 1] - (F[1] - pre[1]))
                    + g[2] * (Tg * c[:, 2] - (F[2] - pre[2])) + gws * (Tg - (wsF - pre[3])))
        gs[base:base + n_in] = val[:n_in]
        gr[base:base + n_in] = (w[:, None] * g[None, :])[:n_in]
        T_carry = ONE if "T_carry" in mut else T[63]
        carry = np.zeros(4, f32) if "r_carry" in mut else np.array([p[63] for p in pre], f32)
    return gs, gr


def seq_forward_ray(sig, rgb, dl, mut=()):
    T, t = ONE, ZERO
    out = [ZERO] * 5
    for j in range(sig.shape[0]):
        alpha = ONE - np.exp(-sig[j] * dl[j, 0])
        w = alpha * T
        t = t + dl[j, 1]
        out = [out[0] + w * rgb[j, 0], out[1] + w * rgb[j, 1], out[2] + w * rgb[j, 2], out[3] + w, out[4] + w * t]
        T = T * (ONE - alpha)
    return out


def seq_backward_ray(sig, rgb, dl, g, gws, F, wsF, mut=()):
    L = sig.shape[0]
    gs, gr = np.zeros(L, f32), np.zeros((L, 3), f32)
    T, r, ws = ONE, np.zeros(3, f32), ZERO
    for j in range(L):
        alpha = ONE - np.exp(-sig[j] * dl[j, 0])
        w = alpha * T
        r = r + w * rgb[j]
        ws = ws + w
        T = T * (ONE - alpha)
        gr[j] = g * w
        gs[j] = dl[j, 0] * (g[0] * (T * rgb[j, 0] - (F[0] - r[0])) + g[1] * (T * rgb[j, 1] - (F[1] - r[1]))
                            + g[2] * (T * rgb[j, 2] - (F[2] - r[2])) + gws * (T - (wsF - ws)))
    return gs, gr


ORDERS = {"wave": (wave_forward_ray, wave_backward_ray), "seq": (seq_forward_ray, seq_backward_ray)}


def _dropped(c, n, budget, mut):
    lim = R.logical_budget(c.M, budget)
    off, num = int(c.rays[n, 1]), int(c.rays[n, 2])
    return num == 0 or (off + num > lim if "nonstrict" in mut else off + num >= lim)


def _bg32(c, bg):
    return None if bg is None else (np.full((c.N, 3), bg, f32) if np.isscalar(bg) else np.asarray(bg, f32))


def model_forward(c, order, mut=(), budget=None, bg=None):
    """float32 model of the forward launch -> ws [N], depth [N], image [N, 3] by ray index"""
    fwd = ORDERS[order][0]
    bgr = _bg32(c, bg)
    ws, dep, img = np.zeros(c.N, f32), np.zeros(c.N, f32), np.zeros((c.N, 3), f32)
    with np.errstate(under="ignore", over="ignore"):
        for n in range(c.N):
            idx, off, num = (int(v) for v in c.rays[n])
            o = [ZERO] * 5
            if not _dropped(c, n, budget, mut):
                o = fwd(c.sigmas[off:off + num], c.rgbs[off:off + num], c.deltas[off:off + num], mut)
            r, d = np.array(o[:3], f32), f32(o[4])
            if bgr is not None:
                r = r + (ONE - o[3]) * bgr[idx]
                d = np.maximum(d - c.nears[idx], ZERO) / (c.fars[idx] - c.nears[idx] + f32(c.depth_eps))
            ws[idx], dep[idx], img[idx] = o[3], d, r
    return ws, dep, img


def model_backward(c, order, ws_in, img_in, gws, gimg, mut=(), budget=None, bg=None):
    bwd = ORDERS[order][1]
    bgr = _bg32(c, bg)
    Mp = c.sigmas.shape[0]
    gs, gr = np.zeros(Mp, f32), np.zeros((Mp, 3), f32)
    with np.errstate(under="ignore", over="ignore"):
        for n in range(c.N):
            idx, off, num = (int(v) for v in c.rays[n])
            if _dropped(c, n, budget, mut):
                continue
            g, gw, F, wsF = gimg[idx].astype(f32), (ZERO if gws is None else f32(gws[idx])), img_in[idx].astype(f32), f32(ws_in[idx])
            if bgr is not None:
                tt = ONE - wsF
                if "no_unblend" not in mut:
                    F = F - tt * bgr[idx]
                if "no_g_bg" not in mut:
                    gw = gw - (g[0] * bgr[idx, 0] + g[1] * bgr[idx, 1] + g[2] * bgr[idx, 2])
            sl = slice(off, off + num)
            gs[sl], gr[sl] = bwd(c.sigmas[sl], c.rgbs[sl], c.deltas[sl], g, gw, F, wsF, mut)
    return gs, gr


FORMS = {"plain": None, "bg_tensor": "tensor", "bg_one": 1.0, "bg_zero": 0.0}


def _bg(c, form):
    return c.bg if FORMS[form] == "tensor" else FORMS[form]


@functools.lru_cache(maxsize=None)
def _reference(name, form, feed):
    """float64 forward of a case and its backward on the float32 ws / image of `feed` ('ref64': the float64 forward rounded;
    'wave' / 'seq': that model's own forward outputs, as training feeds the kernel's)"""
    c = R.case(name)
    bg = _bg(c, form)
    fwd = R.forward(c, bg=bg, depth_eps=c.depth_eps)
    if feed == "ref64":
        ws_in, img_in = fwd["ws"].y.astype(f32), fwd["image"].y.astype(f32)
    else:
        ws_in, _, img_in = model_forward(c, feed, bg=bg)
    gs, gr, owned = R.backward(c, ws_in, img_in, c.gws, c.gimg, bg=bg)
    return fwd, ws_in, img_in, gs, gr


def _ratios(c, order, form, mut=(), feed="ref64"):
    """all five outputs of a model against the reference -> (line, worst)"""
    bg = _bg(c, form)
    fwd, ws_in, img_in, gs, gr = _reference(c.label, form, feed)
    ws, dep, img = model_forward(c, order, mut, bg=bg)
    mgs, mgr = model_backward(c, order, ws_in, img_in, c.gws, c.gimg, mut, bg=bg)
    return R.report("%s %s %s feed=%s%s" % (order, c.label, form, feed, (" mutant " + ",".join(mut)) if mut else ""), c,
                    [("ws", ws, fwd["ws"]), ("depth", dep, fwd["depth"]), ("image", img, fwd["image"]),
                     ("grad_sigmas", mgs, gs), ("grad_rgbs", mgr, gr)])


# ---------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("name", R.CASE_NAMES)
def test_scripted_tables_hold_what_they_promise(name):
    R.assert_coverage(R.case(name))


@pytest.mark.parametrize("form", ["plain", "bg_tensor"])
def test_backward_is_the_gradient_of_the_forward(form):
    """central differences of sum image g + sum ws gws (after the blend) in every sigma and colour of every ray of the full table
    (all six regimes at every length, the 1024-sample ray); h = 1e-3, agreement to 2e-8 of d0 (sum |g| + |gws|)"""
    c = R.case("fresh")
    bg = _bg(c, form)
    fwd = R.forward(c, bg=bg, depth_eps=c.depth_eps)
    gs, gr, owned = R.backward(c, fwd["ws"].y, fwd["image"].y, c.gws, c.gimg, bg=bg)
    h, worst = 1e-3, 0.0
    keep = R.kept(c)
    regimes = set()
    for n in range(c.N):
        idx, off, L = (int(v) for v in c.rays[n])
        if not keep[n]:
            continue
        regimes.add(c.rows[n])
        sl = slice(off, off + L)
        sig, rgb, dl = c.sigmas[sl].astype(np.float64), c.rgbs[sl].astype(np.float64), c.deltas[sl].astype(np.float64)
        P = 4 * L
        S, C = np.tile(sig, (2 * P, 1)), np.tile(rgb, (2 * P, 1, 1))
        for p in range(L):
            S[2 * p, p] += h
            S[2 * p + 1, p] -= h
            for k in range(3):
                q = L + 3 * p + k
                C[2 * q, p, k] += h
                C[2 * q + 1, p, k] -= h
        tr = R.trace(S, C, dl, records=False)
        g, gw = c.gimg[idx].astype(np.float64), float(c.gws[idx])
        img = tr["image"] if bg is None else tr["image"] + (1 - tr["ws"])[:, None] * R._bg_rows(bg, c.N)[idx][None, :]
        loss = img @ g + tr["ws"] * gw
        fd = (loss[0::2] - loss[1::2]) / (2 * h)
        scale = np.abs(g).sum() + abs(gw)
        e_s = np.abs(fd[:L] - gs.y[sl]) / (dl[:, 0] * scale)
        e_c = np.abs(fd[L:].reshape(L, 3) - gr.y[sl]) / scale
        worst = max(worst, e_s.max(), e_c.max())
        assert e_s.max() <= 2e-8 and e_c.max() <= 2e-8, (n, c.rows[n], e_s.max(), e_c.max())
    assert {r for r, _ in regimes} == set(R.REGIMES) and {L for _, L in regimes} >= set(R.LENGTHS[1:]) | {R.LONG}


def test_objective_gradients_are_the_gradient_of_the_loss():
    c = R.case("small")
    ob = R.objective_inputs(c, 5)
    fwd = R.forward(c, bg=c.bg, depth_eps=c.depth_eps)

    def loss(o, image):
        S = R.objective_sums(image, np.zeros_like(image), o)
        return R.objective_finish(S, o)[2].y[0]
    S = R.objective_sums(fwd["image"].y, fwd["image"].bound, ob)
    nrm, coef, _, relc = R.objective_finish(S, ob)
    g_img, _, g_fea, g_col = R.objective_grads(coef.y, relc, ob, fwd["image"].y)
    up, h = float(ob["upstream"][0]), 1e-6
    for key, want, pos in (("fea_s", g_fea.y, (2, 0)), ("fea_s", g_fea.y, (4, 7)), ("col_s", g_col.y, (1, 2))):
        hi, lo = {k: v.astype(np.float64) for k, v in ob.items()}, {k: v.astype(np.float64) for k, v in ob.items()}
        hi[key][pos] += h
        lo[key][pos] -= h
        assert abs(up * (loss(hi, fwd["image"].y) - loss(lo, fwd["image"].y)) / (2 * h) - want[pos]) <= 1e-8
    hi, lo = fwd["image"].y.copy(), fwd["image"].y.copy()
    hi[1, 2] += h
    lo[1, 2] -= h
    assert abs(up * (loss(ob, hi) - loss(ob, lo)) / (2 * h) - g_img[1, 2]) <= 1e-8
    z = R.objective_inputs(c, 5, zero_term="col")
    Sz = R.objective_sums(fwd["image"].y, fwd["image"].bound, z)
    assert Sz.y[3] == 0 and Sz.bound[3] == 0 and R.objective_finish(Sz, z)[1].y[3] == 0


@pytest.mark.parametrize("name,form", [(n, f) for n in R.CASE_NAMES for f in ("plain", "bg_tensor")] + [("perm", "bg_one"), ("perm", "bg_zero")])
@pytest.mark.parametrize("order", ["wave", "seq"])
def test_float32_restatements_stay_inside_the_bound(order, name, form, capsys):
    c = R.case(name)
    for feed in ("ref64", order):
        line, worst = _ratios(c, order, form, feed=feed)
        _say(capsys, "cpu-f32 " + line)
        assert worst <= 1.0, line


@pytest.mark.parametrize("budget", ["below", "above", "zero", "negative"])
def test_wave_model_under_device_budgets(budget, capsys):
    c = R.case("fresh")
    b = R.device_budgets(c)[budget]
    fwd = R.forward(c, budget=b, bg=c.bg, depth_eps=c.depth_eps)
    ws, dep, img = model_forward(c, "wave", budget=b, bg=c.bg)
    gs, gr, owned = R.backward(c, ws, img, c.gws, c.gimg, budget=b, bg=c.bg)
    mgs, mgr = model_backward(c, "wave", ws, img, c.gws, c.gimg, budget=b, bg=c.bg)
    line, worst = R.report("cpu-f32 wave fresh bg_tensor budget=%s" % budget, c,
                           [("ws", ws, fwd["ws"]), ("depth", dep, fwd["depth"]), ("image", img, fwd["image"]),
                            ("grad_sigmas", mgs, gs), ("grad_rgbs", mgr, gr)])
    _say(capsys, line)
    assert worst <= 1.0, line
    assert int(owned.sum()) == int(c.rays[R.kept(c, b), 2].sum())


@pytest.mark.parametrize("mutant", MUTANTS)
def test_single_faults_in_the_wave_model_leave_the_bound(mutant, capsys):
    c = R.case("perm")
    form = "bg_tensor" if mutant in ("no_unblend", "no_g_bg") else "plain"
    line, worst = _ratios(c, "wave", form, mut=(mutant,))
    _say(capsys, "cpu-f32 " + line)
    assert worst > 1.0, line
