"""The training compositing kernels (k_composite_fwd_wave / k_composite_bwd_wave of csrc/raymarching.hip: one wave per ray, 64-sample
chunks, scans and carries; plain, epilogue, group and objective forms) against the float64 restatement in
tests/composite_ref64.py, element by element, under the bound derived there.  Everything goes through pvd_hip directly.

The scripted tables (composite_ref64.cases, checked by assert_coverage here and on the CPU) hold rays of 0, 1, 2, 63, 64, 65, 127,
128, 129, 192, 193 and 1024 samples in six sigma regimes, a permuted index column, the drop edges offset + num == M - 1 / M / > M,
every device-budget case, per-ray and scalar backgrounds, grad_ws present and absent, and near / far that clamp some depths.
Outputs are pre-filled with NaN or a sentinel: dropped and empty rays give exact zeros (exactly the background with the epilogue),
their gradient slots and all padding stay untouched, `fresh` clears exactly the slots nobody owns.

Every test prints its worst err / bound with ray, sample and length class (pytest -s); profiles/composite_fp64_pin.txt keeps the
lines of one run on the MI355X next to the float32 restatements' on the CPU.  Those numbers are a record; the threshold is the bound.

Out of scope: the inference compositing (early termination makes an element-wise bound discontinuous), marching, the autograd
wrappers, negative / inf / nan sigma.  No hipGraph is recorded here."""
import functools

import numpy as np
import pytest
import torch

import composite_ref64 as R

pytestmark = pytest.mark.gpu

SENT = -1.2345e11  # sentinel of the gradient buffers the kernels must leave alone
NAN = float("nan")
f32 = np.float32


def _say(capsys, line):
    with capsys.disabled():
        print("\n" + line, end="")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def _dev(name):
    """the case's buffers on the device, uploaded once and never written"""
    c = R.case(name)
    return {k: _t(getattr(c, k)) for k in ("sigmas", "rgbs", "deltas", "rays", "nears", "fars", "bg", "gws", "gimg")}


def _bg_args(d, bg_kind):
    return (d["bg"], 0.0) if bg_kind == "tensor" else (None, float(bg_kind))


def _bg_ref(c, bg_kind):
    return None if bg_kind is None else (c.bg if bg_kind == "tensor" else float(bg_kind))


def _budget_dev(b):
    return None if b is None else torch.tensor([b], dtype=torch.int32, device="cuda")


def _forward(c, d, bg_kind=None, budget=None):
    """one forward launch into NaN-filled buffers with PAD rays of padding -> ws [N], depth [N], image [N, 3] (device)"""
    import pvd_hip
    N = c.N
    ws, dep, img = (torch.full(s, NAN, device="cuda") for s in ((N + R.PAD,), (N + R.PAD,), (N + R.PAD, 3)))
    if bg_kind is None:
        pvd_hip.composite_rays_train_forward(d["sigmas"], d["rgbs"], d["deltas"], d["rays"], c.M, N, ws, dep, img)
    else:
        bg, bgs = _bg_args(d, bg_kind)
        pvd_hip.composite_rays_train_bg_forward(d["sigmas"], d["rgbs"], d["deltas"], d["rays"], c.M, N, bg, bgs, d["nears"], d["fars"],
                                                c.depth_eps, ws, dep, img, budget_dev=_budget_dev(budget))
    assert torch.isnan(ws[N:]).all() and torch.isnan(dep[N:]).all() and torch.isnan(img[N:]).all(), "padding behind N rays was written"
    return ws[:N], dep[:N], img[:N]


def _check_forward(capsys, label, c, got, bg_kind=None, budget=None):
    ref = R.forward(c, budget=budget, bg=_bg_ref(c, bg_kind), depth_eps=c.depth_eps)
    ws, dep, img = (g.cpu().numpy() for g in got)
    line, worst = R.report("hip fwd " + label, c, [("ws", ws, ref["ws"]), ("depth", dep, ref["depth"]), ("image", img, ref["image"])])
    _say(capsys, line)
    assert worst <= 1.0, line
    gone = c.rays[~R.kept(c, budget), 0]  # dropped and empty rays, by index: exact zeros (the background with the epilogue)
    assert (ws[gone] == 0).all() and (dep[gone] == 0).all()
    assert (img[gone] == (0 if bg_kind is None else R._bg_rows(_bg_ref(c, bg_kind), c.N)[gone].astype(f32))).all()
    return ref


def _backward(c, d, ws_in, img_in, bg_kind=None, budget=None, gws=True, fill=SENT, fresh=False):
    import pvd_hip
    Mp = c.sigmas.shape[0]
    gs, gr = torch.full((Mp,), fill, device="cuda"), torch.full((Mp, 3), fill, device="cuda")
    gw = d["gws"] if gws else None
    if bg_kind is None:
        pvd_hip.composite_rays_train_backward(gw, d["gimg"], d["sigmas"], d["rgbs"], d["deltas"], d["rays"], ws_in, img_in, c.M, c.N, gs, gr)
    else:
        bg, bgs = _bg_args(d, bg_kind)
        pvd_hip.composite_rays_train_bg_backward(gw, d["gimg"], d["sigmas"], d["rgbs"], d["deltas"], d["rays"], ws_in, img_in, c.M, c.N,
                                                 bg, bgs, gs, gr, fresh=fresh, budget_dev=_budget_dev(budget))
    return gs, gr


def _same(a, fill):
    return np.isnan(a).all() if fill != fill else (a.view(np.int32) == np.array(fill, f32).view(np.int32)).all()


def _check_grads(capsys, label, c, got, ref, fill, fresh=False):
    """owned slots inside the bound; everything else untouched (fresh: exactly 0 below M, untouched behind M)"""
    ref_gs, ref_gr, owned = ref
    gs, gr = got[0].cpu().numpy(), got[1].cpu().numpy()
    line, worst = R.report("hip bwd " + label, c, [("grad_sigmas", np.where(owned, gs, 0), ref_gs),
                                                   ("grad_rgbs", np.where(owned[:, None], gr, 0), ref_gr)])
    _say(capsys, line)
    assert worst <= 1.0, line
    free = ~owned
    if fresh:
        below = np.arange(owned.shape[0]) < c.M
        assert (gs[free & below] == 0).all() and (gr[free & below] == 0).all(), "fresh must clear every slot nobody owns"
        free = free & ~below
    assert _same(gs[free], fill) and _same(gr[free], fill), "a slot no kept ray owns was written"
    return worst


def _ref_backward(c, ws_in, img_in, bg_kind=None, budget=None, gws=True, gimg=None, e_g=None):
    return R.backward(c, ws_in.cpu().numpy(), img_in.cpu().numpy(), c.gws if gws else None, c.gimg if gimg is None else gimg,
                      budget=budget, bg=_bg_ref(c, bg_kind), e_g=e_g)


# ---------------------------------------------------------------------------------------------- plain form
@pytest.mark.parametrize("name", R.CASE_NAMES)
def test_plain_forward_and_backward(name, capsys):
    c, d = R.case(name), _dev(name)
    R.assert_coverage(c)
    got = _forward(c, d)
    ref = _check_forward(capsys, "%s plain" % name, c, got)
    feeds = {"own": (got[0], got[2]), "ref64": (_t(ref["ws"].y.astype(f32)), _t(ref["image"].y.astype(f32)))}
    for feed, (ws_in, img_in) in feeds.items():
        ref_b = _ref_backward(c, ws_in, img_in)
        for fill in (SENT, NAN):
            grads = _backward(c, d, ws_in.contiguous(), img_in.contiguous(), fill=fill)
            _check_grads(capsys, "%s plain feed=%s fill=%s" % (name, feed, "nan" if fill != fill else "sentinel"), c, grads, ref_b, fill)


# ---------------------------------------------------------------------------------------------- epilogue form
@pytest.mark.parametrize("gws", [True, False], ids=["gws", "gws_none"])
@pytest.mark.parametrize("bg_kind", ["tensor", 1.0, 0.0], ids=["bg_tensor", "bg_one", "bg_zero"])
@pytest.mark.parametrize("name", ["perm", "small"])
def test_bg_forward_and_backward(name, bg_kind, gws, capsys):
    c, d = R.case(name), _dev(name)
    R.assert_coverage(c)
    label = "%s bg=%s %s" % (name, bg_kind, "gws" if gws else "gws=None")
    got = _forward(c, d, bg_kind)
    ref = _check_forward(capsys, label, c, got, bg_kind)
    feeds = {"own": (got[0], got[2]), "ref64": (_t(ref["ws"].y.astype(f32)), _t(ref["image"].y.astype(f32)))}
    for feed, (ws_in, img_in) in feeds.items():
        grads = _backward(c, d, ws_in.contiguous(), img_in.contiguous(), bg_kind, gws=gws)
        _check_grads(capsys, "%s feed=%s" % (label, feed), c, grads, _ref_backward(c, ws_in, img_in, bg_kind, gws=gws), SENT)


@pytest.mark.parametrize("budget", ["absent", "below", "above", "zero", "negative", "roomy"])
@pytest.mark.parametrize("name", ["fresh", "perm"])
def test_bg_device_budgets_and_fresh(name, budget, capsys):
    """every device-budget case; on the prefix-sum table also fresh=True on NaN-filled buffers against fresh=False on zero-filled
    ones (same bits).  'roomy': M beyond the last ray's end, no budget word: nothing is dropped, `fresh` clears the tail."""
    c0, d = R.case(name), _dev(name)
    R.assert_coverage(c0)
    c = R.with_M(c0, c0.total + 37) if budget == "roomy" else c0
    b = None if budget == "roomy" else R.device_budgets(c)[budget]
    label = "%s bg=tensor budget=%s" % (name, budget)
    got = _forward(c, d, "tensor", b)
    _check_forward(capsys, label, c, got, "tensor", b)
    ws_in, img_in = got[0].contiguous(), got[2].contiguous()
    ref = _ref_backward(c, ws_in, img_in, "tensor", b)
    if budget == "roomy":
        assert int(R.kept(c).sum()) == int((c.rays[:, 2] > 0).sum())
    if name == "perm":
        _check_grads(capsys, label, c, _backward(c, d, ws_in, img_in, "tensor", b), ref, SENT)
        return
    fresh = _backward(c, d, ws_in, img_in, "tensor", b, fill=NAN, fresh=True)
    _check_grads(capsys, label + " fresh", c, fresh, ref, NAN, fresh=True)
    zeroed = _backward(c, d, ws_in, img_in, "tensor", b, fill=0.0, fresh=False)
    for a, z in zip(fresh, zeroed):
        assert torch.equal(a[:c.M].view(torch.int32), z[:c.M].view(torch.int32)), "fresh=True differs from fresh=False on zeroed buffers"


# ---------------------------------------------------------------------------------------------- group launch
def test_bg_forward_group_of_three(capsys):
    import pvd_hip
    segs = [R.case("perm"), R.case("fresh"), R.empty_like(R.case("perm"))]
    M, N, G = segs[0].M, segs[0].N, 3
    assert segs[1].M == M and segs[1].N == N
    budgets = [M + 100, R.device_budgets(segs[1])["below"], 5]
    cat = lambda key, rows: _t(np.concatenate([getattr(s, key)[:rows] for s in segs]))
    sig, rgb, dl = cat("sigmas", M), cat("rgbs", M), cat("deltas", M)
    rays, bg, nears, fars = cat("rays", N), cat("bg", N), cat("nears", N), cat("fars", N)
    bud = torch.tensor(budgets, dtype=torch.int32, device="cuda")
    ws, dep, img = (torch.full(s, NAN, device="cuda") for s in ((G * N,), (G * N,), (G * N, 3)))
    pvd_hip.composite_rays_train_bg_forward_group(sig, rgb, dl, rays, M, N, G, bg, 0.0, nears, fars, segs[0].depth_eps, ws, dep, img,
                                                  budget_dev=bud)
    for j, s in enumerate(segs):
        sl, sm = slice(j * N, (j + 1) * N), slice(j * M, (j + 1) * M)
        got = (ws[sl], dep[sl], img[sl])
        _check_forward(capsys, "group segment %d (%s) budget=%d" % (j, s.label, budgets[j]), s, got, "tensor", budgets[j])
        one = [torch.full(s_, NAN, device="cuda") for s_ in ((N,), (N,), (N, 3))]
        pvd_hip.composite_rays_train_bg_forward(sig[sm], rgb[sm], dl[sm], rays[sl], M, N, bg[sl], 0.0, nears[sl], fars[sl],
                                                s.depth_eps, one[0], one[1], one[2], budget_dev=bud[j:j + 1])
        for a, b in zip(got, one):
            assert torch.equal(a.contiguous().view(torch.int32), b.view(torch.int32)), "slice differs from the single-segment launch"
    assert int(R.kept(segs[2], 5).sum()) == 0


# ---------------------------------------------------------------------------------------------- objective riding along
def _objective_run(capsys, name, rows, fixed=False, fresh=False, zero_term=None, gws=True):
    import pvd_hip
    c, d = R.case(name), _dev(name)
    N, M = c.N, c.M
    ob = R.objective_inputs(c, rows, zero_term)
    od = {k: _t(v) for k, v in ob.items()}
    tag = "%s rows=%d%s%s%s" % (name, rows, " fixed_parts" if fixed else "", " fresh" if fresh else "", " zero=%s" % zero_term if zero_term else "")
    blocks = pvd_hip.composite_objective_blocks(N, rows, fixed)
    S4 = torch.full((4 + 4 * blocks,), NAN, device="cuda")
    ws, dep, img = (torch.full(s, NAN, device="cuda") for s in ((N + R.PAD,), (N + R.PAD,), (N + R.PAD, 3)))
    pvd_hip.composite_objective_forward(d["sigmas"], d["rgbs"], d["deltas"], d["rays"], M, N, d["bg"], 0.0, d["nears"], d["fars"], c.depth_eps,
                                        ws, dep, img, od["img_t"], od["fea_s"], od["fea_t"], od["col_s"], od["col_t"], S4, fixed_parts=fixed)
    assert torch.isnan(ws[N:]).all() and torch.isnan(dep[N:]).all() and torch.isnan(img[N:]).all()
    got = (ws[:N], dep[:N], img[:N])
    fwd = _check_forward(capsys, "objective " + tag, c, got, "tensor")
    S = R.objective_sums(fwd["image"].y, fwd["image"].bound, ob)
    totals = S4[4:].cpu().double().numpy().reshape(-1, 4).sum(0)
    line, worst = R.report("hip objective sums " + tag, c, [("S4", totals, S)])
    _say(capsys, line)
    assert worst <= 1.0, line
    ws_in, img_in = got[0].contiguous(), got[2].contiguous()
    img_h = img_in.cpu().numpy()
    Mp = c.sigmas.shape[0]
    fill = NAN if fresh else SENT
    gw = d["gws"] if gws else None

    def launch(coef4, finish):
        gs, gr = torch.full((Mp,), fill, device="cuda"), torch.full((Mp, 3), fill, device="cuda")
        g_fea, g_col = torch.full((rows, 16), NAN, device="cuda"), torch.full((rows, 3), NAN, device="cuda")
        pvd_hip.composite_objective_backward(gw, d["sigmas"], d["rgbs"], d["deltas"], d["rays"], ws_in, img_in, M, N, d["bg"], 0.0, gs, gr,
                                             od["img_t"], od["fea_s"], od["fea_t"], od["col_s"], od["col_t"], coef4, od["upstream"], g_fea,
                                             g_col, fresh=fresh, finish=finish, fixed_parts=fixed)
        return gs, gr, g_fea.cpu().numpy(), g_col.cpu().numpy()

    def check(label, out, coef, relc):
        g_img, e_g, r_fea, r_col = R.objective_grads(coef, relc, ob, img_h)
        ref = _ref_backward(c, ws_in, img_in, "tensor", gws=gws, gimg=g_img, e_g=e_g)
        _check_grads(capsys, label, c, out[:2], ref, fill, fresh=fresh)
        line, worst = R.report("hip " + label, c, [("g_fea", out[2], r_fea), ("g_col", out[3], r_col)])
        _say(capsys, line)
        assert worst <= 1.0, line

    nrm, coef, loss, relc = R.objective_finish(S, ob)
    coef32 = coef.y.astype(f32)
    check("objective coef4 given " + tag, launch(_t(coef32), None), coef32.astype(np.float64), np.zeros(4))
    for with_extra in (True, False):
        nrm, coef, loss, relc = R.objective_finish(S, ob, with_extra)
        coef_o, loss_o, norms_o = (torch.full((k,), NAN, device="cuda") for k in (4, 1, 4))
        S4f = S4.clone()
        out = launch(coef_o, (od["rates"], od["extra"] if with_extra else None, S4f, loss_o, norms_o))
        label = "objective finish %s %s" % ("extra" if with_extra else "no extra", tag)
        line, worst = R.report("hip " + label, c, [("sums", S4f[:4].cpu().numpy(), S), ("norms", norms_o.cpu().numpy(), nrm),
                                                   ("coef", coef_o.cpu().numpy(), coef), ("loss", loss_o.cpu().numpy(), loss)])
        _say(capsys, line)
        assert worst <= 1.0, line
        if zero_term == "col":
            assert S.y[3] == 0 and float(coef_o[3]) == 0.0 and (out[3] == 0).all(), "a zero norm must give coefficient exactly 0"
        check(label, out, coef.y, relc)


@pytest.mark.parametrize("rows", [1, 300])
def test_objective_forward_and_backward(rows, capsys):
    """rows = 1 and a count that is no multiple of the 256-thread workgroup (300 rows = 1200 float4 loads)"""
    R.assert_coverage(R.case("perm"))
    _objective_run(capsys, "perm", rows, gws=(rows == 1))


def test_objective_zero_norm_term_gives_coefficient_zero(capsys):
    _objective_run(capsys, "perm", 37, zero_term="col")


def test_objective_fresh(capsys):
    _objective_run(capsys, "fresh", 37, fresh=True)


def test_objective_fixed_parts(capsys):
    _objective_run(capsys, "small", 300, fixed=True)


def test_objective_refuses_zero_rows():
    """the library requires rows > 0 (PVD_REQUIRE before any launch): the binding reports it, nothing runs"""
    import pvd_hip
    c, d = R.case("small"), _dev("small")
    N = c.N
    e16, e3 = torch.empty((0, 16), device="cuda"), torch.empty((0, 3), device="cuda")
    ws, dep, img = torch.zeros(N, device="cuda"), torch.zeros(N, device="cuda"), torch.zeros(N, 3, device="cuda")
    S4 = torch.zeros(4 + 4 * pvd_hip.composite_objective_blocks(N, 0), device="cuda")
    with pytest.raises(pvd_hip.PvdHipError):
        pvd_hip.composite_objective_forward(d["sigmas"], d["rgbs"], d["deltas"], d["rays"], c.M, N, d["bg"], 0.0, d["nears"], d["fars"],
                                            c.depth_eps, ws, dep, img, _t(np.zeros((N, 3), f32)), e16, e16, e3, e3, S4)
