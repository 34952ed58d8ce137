"""The fused MFMA head's backward (k_head_bwd, k_head_reduce_dw, the VM reduction riding on the table scatter) against the float64
restatement in tests/head_ref64.py, at the sizes where its launch logic branches, plus the forward's device-side row count.

Bar (accuracy): per output tensor, max and mean |kernel - fp64| <= 2 x the same statistic of layer-by-layer autocast autograd on the
same inputs (torch's own f16 formulation of the head, which the kernel restates), plus a floor of 1e-6 * max|fp64| (fp32 sums and
__expf where autocast's error vanishes).  A dropped, doubled or misplaced 16-row tile moves a weight gradient by up to 100 % of that
tile's share: at one hot tile (test_every_tile_lands_exactly_once) that is 100 %.

Sizes come from the library: one workgroup's partial is head_backward_workspace_floats(kind, 1); the waves of a launch are
4 x workspace(M) / workspace(1); PVD_HEAD_NT (tiles per trip) follows from the M at which the workspace stops growing; one round of
the persistent grid covers R = waves_max * 16 * NT rows.  No hipGraph is recorded here."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import head_ref64 as h64
from test_hip_head import _inputs, _model

pytestmark = pytest.mark.gpu

CLIPS = (-2.0, -2.0, 7.0)
KIND = {"vm": 1, "hash": 0}
WNAMES = {"vm": ["gWa1", "gWc1", "gWc2", "gWc3"], "hash": ["gWa1", "gWa2", "gWc1", "gWc2", "gWc3"]}
F16_MAX = 65504.0


def _ws(kind, M):
    import pvd_hip
    return pvd_hip.head_backward_workspace_floats(KIND[kind], M)


def _nwaves(kind, M):
    return 4 * _ws(kind, M) // _ws(kind, 1)


@functools.lru_cache(maxsize=None)
def _geometry(kind):
    """(waves at the cap, NT, R).  The waves reach the cap once the trips exceed waves_max - 4 (workgroups of 4 waves), i.e. from
    M* = 16 NT (waves_max - 4) + 1 on."""
    big = 1 << 26
    nmax = _nwaves(kind, big)
    lo, hi = 1, big
    while lo < hi:
        mid = (lo + hi) // 2
        if _nwaves(kind, mid) >= nmax:
            hi = mid
        else:
            lo = mid + 1
    NT = (lo - 1) // (16 * (nmax - 4))
    assert NT >= 1 and lo - 1 == 16 * NT * (nmax - 4), (lo, nmax)
    assert _nwaves(kind, 1) == 4 and _nwaves(kind, 16 * NT * 4 + 1) == 8
    return nmax, NT, nmax * 16 * NT


@functools.lru_cache(maxsize=None)
def _model_weights(kind):
    m = _model(kind, seed=31)
    if kind == "vm":
        W = (m.basis_mat.weight, None, m.color_net[0].weight, m.color_net[1].weight, m.color_net[2].weight)
    else:
        W = tuple(l.weight for l in (m.sigma_net[0], m.sigma_net[1], m.color_net[0], m.color_net[1], m.color_net[2]))
    return m, tuple(None if w is None else w.detach().contiguous() for w in W)


_CASES = {}


def _case(kind, M):
    """(x0 in the kernel's layout, sigma_raw, dirs, weights, x): the model's own lookup of _inputs(M)"""
    key = (kind, M)
    if key not in _CASES:
        if len(_CASES) > 4:
            _CASES.clear()
        m, W = _model_weights(kind)
        x, d = _inputs(M, seed=M % 1000 + 1)
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            if kind == "vm":
                sraw, x0 = m.ops.vm_encode(x, m._aabb(), *m.sigma_mat, *m.sigma_vec, *m.color_mat, *m.color_vec)
                sraw, x0 = sraw.float().contiguous(), x0.half().contiguous()
            else:
                h = m.encoder(x, bound=m.bound)
                x0, sraw = h.half().reshape(M, 14, 2).permute(1, 0, 2).contiguous(), None
        _CASES[key] = (x0, sraw, d.float().contiguous(), W, x)
    return _CASES[key]


def _grads(M, seed, dev="cuda"):
    g = torch.Generator(device=dev).manual_seed(seed)
    return (torch.randn(M, device=dev, generator=g) * 1e-3, torch.randn(M, 3, device=dev, generator=g),
            torch.randn(M, 16, device=dev, generator=g) * 0.1)


def _kernel(kind, x0, sraw, d, W, gs, gr, gf, g_rgb2=None, image=None, clips=CLIPS, pre=None, defer_x=None):
    """pvd_hip.head_backward -> dict of the kernel's gradients.  pre: starting values of the weight gradients (accumulation);
    defer_x: (model, positions) -- the VM reduction rides on pvd_hip.vm_backward's launch instead of its own."""
    import pvd_hip
    M = d.shape[0]
    gx = torch.empty_like(x0)
    gsraw = torch.empty(M, device=d.device) if kind == "vm" else None
    gW = [None if w is None else (torch.zeros_like(w) if pre is None else p.clone()) for w, p in zip(W, pre or W)]
    ws = torch.empty(_ws(kind, M), device=d.device)
    hd = {} if defer_x is not None else None
    pvd_hip.head_backward(KIND[kind], x0, sraw, d, M, *W, *clips, gs, gr, gf, gsraw, gx, *gW, ws, image=image, g_rgb2=g_rgb2,
                          defer_reduce=hd)
    if defer_x is not None:
        from vmencoder.vm import is_channels_last, to_channels_last_param
        m, x = defer_x
        tabs = [t.detach() if is_channels_last(t) else to_channels_last_param(t.detach())
                for t in (*m.sigma_mat, *m.sigma_vec, *m.color_mat, *m.color_vec)]
        res = [tabs[0].shape[3], tabs[0].shape[2], tabs[1].shape[2]]
        gt = [torch.empty_strided(t.shape, t.stride(), dtype=torch.float32, device=t.device).zero_() for t in tabs]
        assert hd.get("rider") is not None
        pvd_hip.vm_backward(x.float().contiguous(), m._aabb(), tabs, res, gsraw, gx, gt, head_dw=hd)
        assert "rider" not in hd
    out = {"g_x0": gx}
    if kind == "vm":
        out["g_sigma_raw"] = gsraw
    for n, t in zip(["gWa1", "gWa2", "gWc1", "gWc2", "gWc3"], gW):
        if t is not None:
            out[n] = t
    return out


def _autocast(kind, x0, sraw, d, W, gs, gr, gf, g_rgb2=None, clips=CLIPS):
    """the head as pvd/network.py runs it under autocast (F.linear in f16, clamp, trunc_exp, sigmoid), autograd backward"""
    from pvd.activation import make_trunc_exp
    smin, fmin, cmax = clips
    X = h64.x0_rows(kind, x0).clone().requires_grad_(True)
    Ws = [None if w is None else w.clone().requires_grad_(True) for w in W]
    Wa1, Wa2, Wc1, Wc2, Wc3 = Ws
    sr = sraw.clone().requires_grad_(True) if kind == "vm" else None
    with torch.autocast("cuda", dtype=torch.float16):
        if kind == "vm":
            cf = torch.clamp(F.linear(X, Wa1), fmin, cmax)
            sf = torch.clamp(sr, smin, cmax)
        else:
            h = F.linear(F.relu(F.linear(X, Wa1)), Wa2)
            sf = torch.clamp(h[:, 0], smin, cmax)
            cf = h[:, 1:]
        feat = torch.cat([sf.unsqueeze(-1), cf], dim=-1)
        sigma = make_trunc_exp("cuda")(sf)
        c = torch.cat([h64.sh4(d).float(), cf], dim=-1)
        rgb = torch.sigmoid(F.linear(F.relu(F.linear(F.relu(F.linear(c, Wc1)), Wc2)), Wc3))
    loss = (sigma.float() * gs).sum() + (rgb.float() * gr).sum() + (0 if gf is None else (feat.float() * gf).sum())
    if g_rgb2 is not None:
        loss = loss + (rgb.float() * g_rgb2).sum()
    loss.backward()
    out = {"g_x0": X.grad}
    if kind == "vm":
        out["g_sigma_raw"] = sr.grad
    for n, w in zip(["gWa1", "gWa2", "gWc1", "gWc2", "gWc3"], Ws):
        if w is not None:
            out[n] = w.grad
    return out


def _bar_stats(ref, ac, kind, names):
    """per tensor: (max, mean) of autocast's error and the floor"""
    st = {}
    for n in names:
        r = h64.x0_rows(kind, ref[n]) if n == "g_x0" else ref[n]
        e = (h64.x0_rows(kind, ac[n]).double() if n == "g_x0" else ac[n].double()) - r
        floor = 1e-6 * float(r.abs().max()) if r.numel() else 0.0
        st[n] = (float(e.abs().max()) if r.numel() else 0.0, float(e.abs().mean()) if r.numel() else 0.0, floor)
    return st


def _names(kind):
    return ["g_x0"] + (["g_sigma_raw"] if kind == "vm" else []) + WNAMES[kind]


def _assert_within(kind, got, ref, stats, what, scale=1.0, extra=None):
    for n, (amax, amean, floor) in stats.items():
        k = h64.x0_rows(kind, got[n]).double() if n == "g_x0" else got[n].double()
        r = h64.x0_rows(kind, ref[n]) if n == "g_x0" else ref[n]
        if extra is not None:
            k = k - extra[n].double()
        assert bool(torch.isfinite(k).all()), (what, n)
        if k.numel() == 0:
            continue
        e = (k - r * scale).abs()
        slack = 0.0 if extra is None else 2.0 ** -22 * float(extra[n].abs().max() + (r * scale).abs().max())  # the fp32 +=
        assert float(e.max()) <= scale * (2 * amax + floor) + slack, (what, n, "max", float(e.max()), scale * amax, scale * floor)
        assert float(e.mean()) <= scale * (2 * amean + floor) + slack, (what, n, "mean", float(e.mean()), scale * amean, scale * floor)


def _sizes():
    _, _, R = _geometry("vm")
    return [1, 15, 16, 17, 63, 65, 4099, R - 1, R, R + 1, 2 * R + 17, 92928, 300001]


@pytest.mark.parametrize("kind", ["vm", "hash"])
def test_geometry_from_the_library(kind):
    nmax, NT, R = _geometry(kind)
    assert nmax % 4 == 0 and nmax >= 4 and R == nmax * 16 * NT
    assert _nwaves(kind, R) == nmax and _nwaves(kind, 10 * R) == nmax


@pytest.mark.parametrize("kind", ["vm", "hash"])
def test_backward_against_float64_at_every_branch_of_the_launch(kind):
    """(a) g_x0, g_sigma_raw and every weight gradient, a non-zero upstream gradient on sigma, rgb and feat16, at M where the grid
    has idle waves (1..63), fewer than 16 workgroups, exactly one round (R), one round and a tile, several trips (2R+17, 92 928,
    300 001); plus g_feat16 = None and a second rgb gradient."""
    for M in _sizes():
        x0, sraw, d, W, _ = _case(kind, M)
        gs, gr, gf = _grads(M, seed=M % 977)
        variants = [("plain", gf, None)]
        if M in (4099, 2 * _geometry(kind)[2] + 17):
            variants += [("g_feat16=None", None, None), ("g_rgb2", gf, _grads(M, seed=5)[1])]
        for what, gfv, gr2 in variants:
            ref = h64.head_ref64(kind, x0, sraw, d, W, CLIPS, g_sigma=gs, g_rgb=gr, g_feat16=gfv, g_rgb2=gr2)
            ac = _autocast(kind, x0, sraw, d, W, gs, gr, gfv, g_rgb2=gr2)
            got = _kernel(kind, x0, sraw, d, W, gs, gr, gfv, g_rgb2=gr2)
            for n in WNAMES[kind] if M >= 4099 else ():
                assert float(ref[n].abs().max()) > 0, (M, what, n)
            _assert_within(kind, got, ref, _bar_stats(ref, ac, kind, _names(kind)), (M, what))


def _tiles(M, NT, R):
    ntiles = (M + 15) // 16
    ntrips = (ntiles + NT - 1) // NT
    t = {0, R // 16 - 1, R // 16, (ntrips - 1) * NT, ntiles - 1}
    if ntrips > 2 * (R // (16 * NT)):
        t.add(2 * (R // 16))  # the first tile of the third round
    if NT > 1:
        t.add(NT + 1)  # the second tile of a trip
    return sorted(x for x in t if x < ntiles)


@pytest.mark.parametrize("kind", ["vm", "hash"])
def test_every_tile_lands_exactly_once(kind):
    """(b) upstream gradients only on the rows of one tile: every g_x0 / g_sigma_raw row outside it is exactly 0, and the weight
    gradients are the fp64 gradients of those rows alone.  Tiles: 0, the last of the first round, the first of the second, the first
    of the third, the last trip's, the partial tail; at M = 2R + 17 and 92 928.  VM: also with the reduction riding on vm_backward."""
    _, NT, R = _geometry(kind)
    for M in (2 * R + 17, 92928):
        x0, sraw, d, W, x = _case(kind, M)
        gs, gr, gf = _grads(M, seed=11)
        for t in _tiles(M, NT, R):
            lo, hi = 16 * t, min(16 * t + 16, M)
            keep = torch.zeros(M, device=d.device)
            keep[lo:hi] = 1.0
            gsk, grk, gfk = gs * keep, gr * keep[:, None], gf * keep[:, None]
            rows = slice(lo, hi)
            x0r = x0[:, rows].contiguous() if kind == "hash" else x0[rows]
            srr = sraw[rows] if kind == "vm" else None
            ref = h64.head_ref64(kind, x0r, srr, d[rows], W, CLIPS, g_sigma=gs[rows], g_rgb=gr[rows], g_feat16=gf[rows])
            ac = _autocast(kind, x0r, srr, d[rows], W, gs[rows], gr[rows], gf[rows])
            stats = _bar_stats(ref, ac, kind, _names(kind))
            runs = [("own launch", None)] + ([("rider", (_model_weights("vm")[0], x))] if kind == "vm" else [])
            for what, dx in runs:
                got = _kernel(kind, x0, sraw, d, W, gsk, grk, gfk, defer_x=dx)
                gx = h64.x0_rows(kind, got["g_x0"])
                assert not gx[:lo].any() and not gx[hi:].any(), (M, t, what)
                if kind == "vm":
                    assert not got["g_sigma_raw"][:lo].any() and not got["g_sigma_raw"][hi:].any(), (M, t, what)
                tile = {n: (got[n][:, rows] if kind == "hash" else got[n][rows]) if n in ("g_x0", "g_sigma_raw") else got[n]
                        for n in _names(kind)}
                _assert_within(kind, tile, ref, stats, (M, t, what))


def test_reduction_riding_on_the_scatter_against_float64():
    """(c) the VM weight-gradient reduction in its own launch and riding on vm_backward, each against fp64, at one workgroup, fewer
    than 16 workgroups (empty reduction slices), one round and a tile, and the cap"""
    kind = "vm"
    _, _, R = _geometry(kind)
    for M in (1, 17, R + 1, 92928):
        x0, sraw, d, W, x = _case(kind, M)
        gs, gr, gf = _grads(M, seed=13)
        ref = h64.head_ref64(kind, x0, sraw, d, W, CLIPS, g_sigma=gs, g_rgb=gr, g_feat16=gf)
        stats = _bar_stats(ref, _autocast(kind, x0, sraw, d, W, gs, gr, gf), kind, _names(kind))
        own = _kernel(kind, x0, sraw, d, W, gs, gr, gf)
        ride = _kernel(kind, x0, sraw, d, W, gs, gr, gf, defer_x=(_model_weights(kind)[0], x))
        _assert_within(kind, own, ref, stats, (M, "own launch"))
        _assert_within(kind, ride, ref, stats, (M, "rider"))
        assert torch.equal(own["g_x0"], ride["g_x0"]) and torch.equal(own["g_sigma_raw"], ride["g_sigma_raw"])


@pytest.mark.parametrize("kind", ["vm", "hash"])
def test_weight_gradients_accumulate(kind):
    """(c) gW += the batch's gradient: starting from non-zero buffers, the increment is the fp64 gradient (plus the fp32 add)"""
    _, _, R = _geometry(kind)
    for M in (1, 2 * R + 17):
        x0, sraw, d, W, _ = _case(kind, M)
        gs, gr, gf = _grads(M, seed=17)
        ref = h64.head_ref64(kind, x0, sraw, d, W, CLIPS, g_sigma=gs, g_rgb=gr, g_feat16=gf)
        stats = _bar_stats(ref, _autocast(kind, x0, sraw, d, W, gs, gr, gf), kind, WNAMES[kind])
        g = torch.Generator(device="cuda").manual_seed(19)
        pre = [None if w is None else torch.randn(w.shape, device="cuda", generator=g) * float(ref[n].abs().max())
               for w, n in zip(W, ["gWa1", "gWa2", "gWc1", "gWc2", "gWc3"])]
        got = _kernel(kind, x0, sraw, d, W, gs, gr, gf, pre=pre)
        extra = {n: p for n, p in zip(["gWa1", "gWa2", "gWc1", "gWc2", "gWc3"], pre) if p is not None}
        _assert_within(kind, {n: got[n] for n in WNAMES[kind]}, ref, stats, (M, "+="), extra=extra)


@pytest.mark.parametrize("kind", ["vm", "hash"])
def test_staging_and_optional_gradients_give_the_same_bits(kind):
    """(c) packed image vs fp32 masters, g_rgb2 vs the host-side sum, g_feat16 = None vs zeros: g_x0 / g_sigma_raw bit for bit (the
    same values reach the same operations); the weight gradients (atomic order not fixed) each against fp64"""
    import pvd_hip
    _, _, R = _geometry(kind)
    for M in (4099, 2 * R + 17):
        x0, sraw, d, W, _ = _case(kind, M)
        gs, gr, gf = _grads(M, seed=23)
        gr2 = _grads(M, seed=29)[1]
        image = pvd_hip.head_pack_weights(KIND[kind], *W)
        base = _kernel(kind, x0, sraw, d, W, gs, gr, gf)
        pairs = [("image", base, _kernel(kind, x0, sraw, d, W, gs, gr, gf, image=image), (gr, None, gf)),
                 ("g_rgb2", _kernel(kind, x0, sraw, d, W, gs, gr + gr2, gf), _kernel(kind, x0, sraw, d, W, gs, gr, gf, g_rgb2=gr2),
                  (gr, gr2, gf)),
                 ("g_feat16", _kernel(kind, x0, sraw, d, W, gs, gr, torch.zeros_like(gf)), _kernel(kind, x0, sraw, d, W, gs, gr, None),
                  (gr, None, None))]
        for what, a, b, (g1, g2, g3) in pairs:
            assert torch.equal(a["g_x0"], b["g_x0"]), (M, what)
            if kind == "vm":
                assert torch.equal(a["g_sigma_raw"], b["g_sigma_raw"]), (M, what)
            ref = h64.head_ref64(kind, x0, sraw, d, W, CLIPS, g_sigma=gs, g_rgb=g1, g_rgb2=g2, g_feat16=g3)
            stats = _bar_stats(ref, _autocast(kind, x0, sraw, d, W, gs, g1, g3, g_rgb2=g2), kind, WNAMES[kind])
            for got in (a, b):
                _assert_within(kind, {n: got[n] for n in WNAMES[kind]}, ref, stats, (M, what))


@pytest.mark.parametrize("kind", ["vm", "hash"])
def test_nothing_is_written_past_the_outputs(kind):
    """(c) guard rows: g_x0 / g_sigma_raw as the leading rows of larger NaN-filled buffers, a workspace 4096 floats longer than
    head_backward_workspace_floats: everything past M rows / past the documented workspace keeps its sentinel"""
    import pvd_hip
    _, _, R = _geometry(kind)
    for M in (17, 2 * R + 17):
        x0, sraw, d, W, _ = _case(kind, M)
        gs, gr, gf = _grads(M, seed=37)
        nan = float("nan")
        if kind == "vm":
            gx_buf = torch.full((M + 64, 144), nan, device="cuda").half()
            gx = gx_buf[:M]
        else:
            gx_buf = torch.full((14 * M * 2 + 4096,), nan, device="cuda").half()
            gx = gx_buf[:14 * M * 2].view(14, M, 2)
        gs_buf = torch.full((M + 64,), nan, device="cuda")
        wsf = _ws(kind, M)
        ws_buf = torch.full((wsf + 4096,), nan, device="cuda")
        gW = [None if w is None else torch.zeros_like(w) for w in W]
        pvd_hip.head_backward(KIND[kind], x0, sraw, d, M, *W, *CLIPS, gs, gr, gf, gs_buf[:M] if kind == "vm" else None, gx, *gW, ws_buf)
        torch.cuda.synchronize()
        tail = gx_buf[M:] if kind == "vm" else gx_buf[14 * M * 2:]
        assert bool(torch.isnan(tail).all()), (M, "g_x0")
        assert bool(torch.isfinite(gx).all()), (M, "g_x0 rows")
        if kind == "vm":
            assert bool(torch.isnan(gs_buf[M:]).all()) and bool(torch.isfinite(gs_buf[:M]).all()), (M, "g_sigma_raw")
        assert bool(torch.isnan(ws_buf[wsf:]).all()), (M, "workspace")


def _boundary(kind, vals, clips, seed, sigma_scale):
    x0, sraw, d, W = h64.clamp_boundary_case(kind, vals, seed=seed, device="cuda")
    M = d.shape[0]
    gs, gr, gf = _grads(M, seed=seed + 1)
    gs = gs * sigma_scale
    ref = h64.head_ref64(kind, x0, sraw, d, W, clips, g_sigma=gs, g_rgb=gr, g_feat16=gf)
    got = _kernel(kind, x0, sraw, d, W, gs, gr, gf, clips=clips)
    return M, ref, got


@pytest.mark.parametrize("kind", ["vm", "hash"])
def test_clamp_masks_at_the_boundaries_on_the_device(kind):
    """(d) pre-activations exactly on sigma_clip_min / sigma_clip_max and one f16 ulp either side (h64.clamp_boundary_case): the
    kernel's masks are torch.clamp's inclusive ones -- g_sigma_raw (VM), d basis_mat[c, r] (VM colour features), d sigma_net.1[0, r]
    (hash h0) -- and, with clip_max = 20, a log-density of 13 / 14 takes trunc_exp's exp(12) (VM, with the plenoxel-edit floor of
    -100: -13 takes exp(-12))."""
    # sigma's upstream gradient x 1e3 where exp(log-density) <= exp(7): as large as the others; x 1 where it meets exp(12), so that
    # the hash head's h0 gradient (stored in f16) stays inside the f16 range
    cases = [(h64.f16_neighbours(-2.0) + h64.f16_neighbours(7.0) + [0.5], CLIPS, 1e3)]
    cases.append(([-13.0, -12.0, 11.8984375, 12.0, 13.0, 14.0, 24.0, 0.5], (-100.0 if kind == "vm" else -2.0, -2.0, 20.0), 1.0))
    for ci, (vals, clips, sigma_scale) in enumerate(cases):
        M, ref, got = _boundary(kind, vals, clips, seed=41 + ci, sigma_scale=sigma_scale)
        if kind == "vm":
            rs, ks = ref["g_sigma_raw"], got["g_sigma_raw"].double()
            assert torch.equal(ks != 0, rs != 0), (clips, (ks != 0).int().tolist(), (rs != 0).int().tolist())
            assert bool(((ks - rs).abs() <= 1e-5 * rs.abs() + 1e-6 * float(rs.abs().max())).all()), (clips, float((ks - rs).abs().max()))
            assert torch.equal(got["gWa1"][:, :M] != 0, ref["gWa1"][:, :M] != 0), clips
            # the colour features' masked gradients, after the colour head's f16 chain (the f16-level bar of tests/test_hip_head.py)
            kb, rb = got["gWa1"][:, :M].double(), ref["gWa1"][:, :M]
            assert float((kb - rb).abs().max()) <= 2e-2 * float(rb.abs().max()), (clips, float((kb - rb).abs().max()))
        else:
            k, r = got["gWa2"][0, :M].double(), ref["gWa2"][0, :M]
            assert torch.equal(k != 0, r != 0), (clips, (k != 0).int().tolist(), (r != 0).int().tolist())
            assert float((k - r).abs().max()) <= 2e-2 * float(r.abs().max()), (clips, float((k - r).abs().max()))
        assert (ref["g_sigma_raw"] if kind == "vm" else ref["gWa2"][0, :M]).eq(0).any()  # both sides of the masks are exercised


@pytest.mark.parametrize("kind", ["vm", "hash"])
def test_loss_scale_overflow_is_never_finite_and_wrong(kind):
    """(e) upstream gradients x 2^k for k = 0, 1, ... until the fp64 intermediates are 4x past the f16 range.  Power-of-two scaling
    is exact in the reference, so the bar at 2^k is 2^k x the bar of k = 0.  Every result either meets it or has a non-finite value
    in g_x0 / g_sigma_raw / a weight gradient (what the gradient scaler's inf check catches)."""
    M = 4099
    x0, sraw, d, W, _ = _case(kind, M)
    gs, gr, gf = _grads(M, seed=43)
    ref = h64.head_ref64(kind, x0, sraw, d, W, CLIPS, g_sigma=gs, g_rgb=gr, g_feat16=gf)
    stats = _bar_stats(ref, _autocast(kind, x0, sraw, d, W, gs, gr, gf), kind, _names(kind))
    kmax = math.ceil(math.log2(4 * F16_MAX / ref["inter_max"]))
    assert kmax > 4
    finite_runs = 0
    for k in range(kmax + 1):
        s = 2.0 ** k
        got = _kernel(kind, x0, sraw, d, W, gs * s, gr * s, gf * s)
        if all(bool(torch.isfinite(got[n]).all()) for n in _names(kind)):
            _assert_within(kind, got, ref, stats, (k, "2^k"), scale=s)
            finite_runs += 1
    assert finite_runs >= 1


@pytest.mark.parametrize("M", [4099, 140001])  # 140 001: past the forward's 768-workgroup cap and the fused launch's 1024
def test_forward_device_row_count(M):
    """(f) head_forward (both kinds) and hash_head_forward_fused with a device row count of 0, -5, 17, M-1, M, M+100: rows below
    min(M, count) are the run without a count bit for bit, the rest keep their sentinel"""
    import numpy as np
    import pvd_hip
    nan = float("nan")
    runs = []
    for kind in ("vm", "hash"):
        x0, sraw, d, W, x = _case(kind, M)
        runs.append((kind, lambda s, r, f, rd, x0=x0, sraw=sraw, d=d, W=W, kind=kind: pvd_hip.head_forward(
            KIND[kind], x0, sraw, d, M, *W, *CLIPS, s, r, f, rows_dev=rd)))
    m, W = _model_weights("hash")
    _, _, d, _, x = _case("hash", M)
    enc = m.encoder
    emb16 = enc.embeddings.detach().half()
    image = pvd_hip.head_pack_weights(0, *W)
    runs.append(("fused", lambda s, r, f, rd: pvd_hip.hash_head_forward_fused(
        x.float().contiguous(), float(m.bound), float(2 * m.bound), emb16, enc.offsets, float(np.log2(enc.per_level_scale)),
        enc.base_resolution, enc.gridtype_id, enc.align_corners, d, M, *W, CLIPS[0], CLIPS[2], s, r, f, image=image, rows_dev=rd)))
    for what, fn in runs:
        full = [torch.full((M,), nan, device="cuda"), torch.full((M, 3), nan, device="cuda"), torch.full((M, 16), nan, device="cuda")]
        fn(*full, None)
        assert all(bool(torch.isfinite(t).all()) for t in full), what
        for n in (0, -5, 17, M - 1, M, M + 100):
            rd = torch.tensor([n], dtype=torch.int32, device="cuda")
            out = [torch.full_like(t, nan) for t in full]
            fn(*out, rd)
            k = max(0, min(M, n))
            for a, b in zip(out, full):
                assert torch.equal(a[:k], b[:k]), (what, n)
                assert bool(torch.isnan(a[k:]).all()), (what, n)
