"""Pins of tests/head_ref64.py, the float64 restatement of the sigma / colour head that tests/test_hip_head_fp64.py holds the fused
kernel's backward against: its forward is the reference's own autocast run, its clamp and trunc_exp backwards are torch's / the
project's, and its gradients are the derivatives of its forward."""
import os

import numpy as np
import pytest
import torch

import head_ref64 as h64

HERE = os.path.dirname(os.path.abspath(__file__))


def _w(g, pre, names):
    return tuple(None if n is None else torch.from_numpy(g[pre + "sd__" + n]) for n in names)


@pytest.mark.parametrize("mt", ["hash", "vm"])
def test_forward_is_the_references_head_under_autocast(mt):
    """reference_head_amp.npz: the reference's NeRFNetwork.forward under autocast on recorded head inputs.  The reference rounds
    every layer output to f16 (11 significant bits), the helper none: the bars are the f16-level bars of tests/test_hip_head.py.
    A different concatenation order, SH order or set of clamped channels moves these by O(1)."""
    g = np.load(os.path.join(HERE, "golden", "reference_head_amp.npz"))
    pre = "amp_%s__" % mt
    x0 = torch.from_numpy(g[pre + "x0"])
    d = torch.from_numpy(g["d"])
    if mt == "hash":
        W = _w(g, pre, ["sigma_net.0.weight", "sigma_net.1.weight", "color_net.0.weight", "color_net.1.weight", "color_net.2.weight"])
        out = h64.head_ref64("hash", x0, None, d, W, grads=False)
    else:
        W = _w(g, pre, ["basis_mat.weight", None, "color_net.0.weight", "color_net.1.weight", "color_net.2.weight"])
        out = h64.head_ref64("vm", x0, torch.from_numpy(g[pre + "sigma_raw"]), d, W, grads=False)
    feat_r, rgb_r, sig_r = (torch.from_numpy(g[pre + k]).double() for k in ("feature_sigma_color", "color", "sigma"))
    fd = (out["feat16"] - feat_r).abs()
    assert bool((fd <= 4e-3 * (1 + feat_r.abs())).all()), float(fd.max())
    assert float((out["rgb"] - rgb_r).abs().max()) <= 2e-3 and float((out["rgb"] - rgb_r).abs().mean()) <= 2e-4
    rel = (out["sigma"] - sig_r).abs() / (sig_r.abs() + 1e-6)
    assert float(rel.max()) <= 8e-3 and float(rel.mean()) <= 1e-3
    # the fixture exercises both sides of the clamps and a non-trivial colour
    assert float(feat_r[:, 1:].max() - feat_r[:, 1:].min()) > 1.0 and (rgb_r > 0.02).any() and (rgb_r < 0.98).any()
    if mt == "vm":
        assert torch.equal(out["feat16"][:, 0], feat_r[:, 0])  # the fp32 sigma feature, clamped: exact


def test_sh_is_the_oracles():
    import oracle
    g = torch.Generator().manual_seed(0)
    d = torch.randn(257, 3, generator=g)
    d = d / d.norm(dim=-1, keepdim=True)
    d[:3] = 0.0  # the marcher's padding rows
    ref, _ = oracle.sh_encode_forward(d.numpy(), 4)
    assert np.abs(h64.sh4(d).numpy() - ref).max() <= 2e-6


def test_trunc_exp_gradient_is_the_projects():
    from pvd.activation import make_trunc_exp
    te = make_trunc_exp("cpu")
    x = torch.tensor([-13.0, -12.0, -11.9, 0.0, 11.9, 12.0, 13.0], dtype=torch.float64)
    g = torch.linspace(0.5, 2.0, x.numel(), dtype=torch.float64)
    a = x.clone().requires_grad_(True)
    (te(a) * g).sum().backward()
    b = x.clone().requires_grad_(True)
    (h64.trunc_exp64(b) * g).sum().backward()
    assert torch.equal(a.grad, b.grad)
    assert torch.equal(b.grad[[0, 1]], g[[0, 1]] * np.exp(-12.0)) and torch.equal(b.grad[[5, 6]], g[[5, 6]] * np.exp(12.0))


def _torch_clamp_mask(v, lo, hi):
    t = v.clone().double().requires_grad_(True)
    torch.clamp(t, lo, hi).sum().backward()
    return t.grad != 0


@pytest.mark.parametrize("kind", ["vm", "hash"])
def test_clamp_masks_at_the_boundaries_are_torch_clamps(kind):
    """Inputs exactly on sigma_clip_min / sigma_clip_max (-2, 7) and one f16 ulp either side (clamp_boundary_case): every row's
    gradient mask -- g_sigma_raw (VM), d basis_mat[c, r] (VM colour features), d sigma_net.1[0, r] (hash h0) -- is torch.clamp's."""
    vals = h64.f16_neighbours(-2.0) + h64.f16_neighbours(7.0) + [0.5]
    x0, sraw, d, W = h64.clamp_boundary_case(kind, vals, seed=1)
    M = d.shape[0]
    g = torch.Generator().manual_seed(2)
    gs, gr, gf = torch.randn(M, generator=g), torch.randn(M, 3, generator=g), torch.randn(M, 16, generator=g)
    out = h64.head_ref64(kind, x0, sraw, d, W, g_sigma=gs, g_rgb=gr, g_feat16=gf)
    r = torch.arange(M)
    n = len(vals)
    v = torch.tensor(vals)
    if kind == "vm":
        assert torch.equal(out["feat16"][:, 0], torch.clamp(sraw.double(), -2.0, 7.0))
        assert torch.equal(out["g_sigma_raw"] != 0, _torch_clamp_mask(v[r % n], -2.0, 7.0))
        feat = v[(r[None, :] + torch.arange(15)[:, None]) % n]  # [15, M]: colour feature c of row r
        assert torch.equal(out["feat16"][:, 1:].T, torch.clamp(feat.double(), -2.0, 7.0))
        assert torch.equal(out["gWa1"][:, :M] != 0, _torch_clamp_mask(feat, -2.0, 7.0))
    else:
        assert torch.equal(out["feat16"][:, 0], torch.clamp(v[r % n].double(), -2.0, 7.0))
        assert torch.equal(out["gWa2"][0, :M] != 0, _torch_clamp_mask(v[r % n], -2.0, 7.0))


@pytest.mark.parametrize("kind", ["vm", "hash"])
def test_gradients_are_the_derivatives_of_the_forward(kind):
    """Central differences in float64 (h = 1e-6: truncation ~h^2, cancellation ~1e-16 / h) on a few entries of every weight matrix
    and input; the rows keep every ReLU and clamp away from its kink by far more than h."""
    g = torch.Generator().manual_seed(3)
    M = 5
    K = 144 if kind == "vm" else 28
    x0 = torch.rand(M, K, generator=g) * (0.2 if kind == "vm" else 1.0)
    sraw = torch.tensor([-1.0, 0.5, 3.0, 6.0, 9.0]) if kind == "vm" else None  # 9.0: outside the clamp (zero gradient)
    d = torch.randn(M, 3, generator=g)
    d = d / d.norm(dim=-1, keepdim=True)
    shapes = [(15, 144), None] if kind == "vm" else [(64, 28), (16, 64)]
    W = [None if s is None else torch.randn(*s, generator=g) * 0.5 for s in shapes] + [torch.randn(64, 31, generator=g) * 0.5,
                                                                                    torch.randn(64, 64, generator=g) * 0.3,
                                                                                    torch.randn(3, 64, generator=g) * 0.3]
    gs, gr, gf = torch.randn(M, generator=g), torch.randn(M, 3, generator=g), torch.randn(M, 16, generator=g)
    kw = dict(g_sigma=gs, g_rgb=gr, g_feat16=gf, round_f16=False)
    ref = h64.head_ref64(kind, x0, sraw, d, W, **kw)

    def loss(x0_, sraw_, W_):
        o = h64.head_ref64(kind, x0_, sraw_, d, W_, grads=False, round_f16=False)
        return float((o["sigma"] * gs.double()).sum() + (o["rgb"] * gr.double()).sum() + (o["feat16"] * gf.double()).sum())

    h = 1e-6
    names = ["gWa1", "gWa2", "gWc1", "gWc2", "gWc3"]
    checked = 0
    for wi, name in enumerate(names):
        if W[wi] is None:
            continue
        for flat in torch.randperm(W[wi].numel(), generator=g)[:4].tolist():
            Wp = [None if w is None else w.double().clone() for w in W]
            Wm = [None if w is None else w.double().clone() for w in W]
            Wp[wi].view(-1)[flat] += h
            Wm[wi].view(-1)[flat] -= h
            fd = (loss(x0.double(), sraw, Wp) - loss(x0.double(), sraw, Wm)) / (2 * h)
            an = float(ref[name].reshape(-1)[flat])
            assert abs(fd - an) <= 1e-6 * max(1.0, abs(an)), (name, flat, fd, an)
            checked += 1
    for flat in torch.randperm(x0.numel(), generator=g)[:6].tolist():
        xp, xm = x0.double().clone(), x0.double().clone()
        xp.view(-1)[flat] += h
        xm.view(-1)[flat] -= h
        fd = (loss(xp, sraw, W) - loss(xm, sraw, W)) / (2 * h)
        an = float(ref["g_x0"].reshape(-1)[flat])
        assert abs(fd - an) <= 1e-6 * max(1.0, abs(an)), ("g_x0", flat, fd, an)
    if kind == "vm":
        for i in range(M):
            sp, sm = sraw.double().clone(), sraw.double().clone()
            sp[i] += h
            sm[i] -= h
            fd = (loss(x0.double(), sp, W) - loss(x0.double(), sm, W)) / (2 * h)
            an = float(ref["g_sigma_raw"][i])
            assert abs(fd - an) <= 1e-6 * max(1.0, abs(an)), ("g_sigma_raw", i, fd, an)
        assert float(ref["g_sigma_raw"][4]) == 0.0
    assert checked >= 16


def test_row_weight_and_layouts():
    """row_weight = indicator of some rows == the helper on those rows alone; the hash g_x0 comes back level-major [14, M, 2]"""
    g = torch.Generator().manual_seed(4)
    M = 37
    x0 = (torch.rand(14, M, 2, generator=g) * 2 - 1).half()
    d = torch.randn(M, 3, generator=g)
    d = d / d.norm(dim=-1, keepdim=True)
    W = (torch.randn(64, 28, generator=g) * 0.5, torch.randn(16, 64, generator=g) * 0.5, torch.randn(64, 31, generator=g) * 0.3,
         torch.randn(64, 64, generator=g) * 0.3, torch.randn(3, 64, generator=g) * 0.3)
    gs, gr, gf = torch.randn(M, generator=g), torch.randn(M, 3, generator=g), torch.randn(M, 16, generator=g)
    rows = torch.zeros(M)
    rows[16:32] = 1.0
    full = h64.head_ref64("hash", x0, None, d, W, g_sigma=gs, g_rgb=gr, g_feat16=gf, row_weight=rows)
    part = h64.head_ref64("hash", x0[:, 16:32], None, d[16:32], W, g_sigma=gs[16:32], g_rgb=gr[16:32], g_feat16=gf[16:32])
    assert full["g_x0"].shape == (14, M, 2)
    assert torch.equal(full["g_x0"][:, 16:32], part["g_x0"]) and not full["g_x0"][:, :16].any() and not full["g_x0"][:, 32:].any()
    for n in ("gWa1", "gWa2", "gWc1", "gWc2", "gWc3"):
        assert torch.allclose(full[n], part[n], rtol=1e-12, atol=1e-14), n
    # [14, M, 2] and [M, 28] inputs are the same rows
    flat = h64.head_ref64("hash", x0.permute(1, 0, 2).reshape(M, 28), None, d, W, g_sigma=gs, g_rgb=gr, g_feat16=gf, row_weight=rows)
    assert torch.equal(flat["g_x0"], h64.x0_rows("hash", full["g_x0"]))
