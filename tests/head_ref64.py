"""A float64 restatement of the sigma / colour head of the hash and VM models, forward and backward (test helper, like oracle_ops.py).

The formulation is NeRFNetwork.forward under autocast (pvd/network.py:356-367 for vm, :387-400 for hash): bias-free Linear layers,
ReLU, clamp, trunc_exp, SH degree 4 and sigmoid.  What the fused kernel and autocast consume is rounded to f16 first (the products /
encoder features and every weight matrix); the direction, the VM's raw sigma feature and the upstream gradients stay fp32.  After
that everything is float64 with no intermediate rounding, and the gradients come from float64 autograd:

* trunc_exp has the custom backward g * exp(clamp(x, -12, 12)) (pvd/activation.py);
* torch.clamp's backward keeps the gradient where min <= x <= max (inclusive at both ends);
* SH degree 4 is evaluated from the reference's per-term polynomial table (tests/golden/reference_constants.npz).

Works on any device (the GPU tests run it on the device).  Nothing here imports the kernel's binding."""
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
WEIGHT_NAMES = {"vm": ("Wa1", "Wc1", "Wc2", "Wc3"), "hash": ("Wa1", "Wa2", "Wc1", "Wc2", "Wc3")}
_SH_TERMS = None


def _kind(kind):
    return {0: "hash", 1: "vm"}.get(kind, kind)


def _sh_terms():
    global _SH_TERMS
    if _SH_TERMS is None:
        g = np.load(os.path.join(HERE, "golden", "reference_constants.npz"))
        keep = g["sh_term_output"] < 16  # family 0 (values), bands l < 4
        _SH_TERMS = (g["sh_term_output"][keep].astype(np.int64), g["sh_term_exponents"][keep].astype(np.int64),
                     g["sh_term_coefficient"][keep].astype(np.float64))
    return _SH_TERMS


def sh4(d):
    """[M,3] directions -> [M,16] degree-4 SH basis in float64 (index l*l + l + m, the shencoder's order)."""
    out_idx, ex, coef = _sh_terms()
    d = d.to(torch.float64)
    dev = d.device
    ex = torch.as_tensor(ex, device=dev)
    mono = d[:, None, 0] ** ex[None, :, 0] * d[:, None, 1] ** ex[None, :, 1] * d[:, None, 2] ** ex[None, :, 2]
    out = torch.zeros(d.shape[0], 16, dtype=torch.float64, device=dev)
    out.index_add_(1, torch.as_tensor(out_idx, device=dev), mono * torch.as_tensor(coef, device=dev)[None, :])
    return out


class _TruncExp64(torch.autograd.Function):
    """pvd/activation.py's trunc_exp in float64: exp forward, backward with the exponent clamped to [-12, 12]."""

    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return torch.exp(x)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        return g * torch.exp(x.clamp(-12, 12))


trunc_exp64 = _TruncExp64.apply


def f16_64(t):
    """round to f16, then widen to float64 (what the kernel and autocast consume)"""
    return t.detach().to(torch.float16).to(torch.float64)


def x0_rows(kind, x0):
    """the kernel's input layout -> [M, K] rows: VM products [M,144]; hash encoder output [14,M,2] (level-major) -> [M,28]"""
    if _kind(kind) == "hash" and x0.dim() == 3:
        return x0.permute(1, 0, 2).reshape(x0.shape[1], 28)
    return x0


def head_ref64(kind, x0, sigma_raw, dirs, weights, clips=(-2.0, -2.0, 7.0), g_sigma=None, g_rgb=None, g_feat16=None, g_rgb2=None,
               row_weight=None, grads=True, round_f16=True):
    """kind "vm" / "hash" (or 1 / 0).  x0 in the kernel's layout (VM [M,144], hash [14,M,2] or [M,28]); sigma_raw [M] (VM);
    weights (Wa1, Wa2, Wc1, Wc2, Wc3) fp32 masters (Wa2 None for VM); clips (clip_sigma_min, clip_feat_min, clip_max) as the kernel
    takes them (the hash head clamps channel 0 with clip_sigma_min).  Upstream gradients: any of g_sigma [M], g_rgb [M,3],
    g_rgb2 [M,3] (a second consumer of rgb), g_feat16 [M,16]; None = no gradient.  row_weight [M]: multiplies every row's upstream
    gradients (0 drops a row).  round_f16=False takes x0 and the weights as they are (finite differences).

    Returns a dict of float64 tensors: sigma, rgb, feat16 and, with grads, g_x0 (the kernel's layout), g_sigma_raw (VM), the weight
    gradients gWa1 / gWa2 (hash) / gWc1 / gWc2 / gWc3, and inter_max: the largest |gradient| the kernel stores in f16 on the way
    (pre-activation gradients of every layer and g_x0)."""
    kind = _kind(kind)
    smin, fmin, cmax = clips
    hash_layout = kind == "hash" and x0.dim() == 3
    widen = f16_64 if round_f16 else (lambda t: t.detach().to(torch.float64).clone())
    X = widen(x0_rows(kind, x0))
    M = X.shape[0]
    Wa1, Wa2, Wc1, Wc2, Wc3 = [None if w is None else widen(w) for w in weights]
    leaves = [X, Wa1, Wc1, Wc2, Wc3] + ([Wa2] if kind == "hash" else [])
    sraw = None
    if kind == "vm":
        sraw = sigma_raw.detach().to(torch.float64)
        leaves.append(sraw)
    if grads:
        for t in leaves:
            t.requires_grad_(True)
    inter = []
    keep = (lambda t: (t.retain_grad(), inter.append(t))) if grads else (lambda t: None)
    with torch.enable_grad() if grads else torch.no_grad():
        if kind == "vm":
            raw = X @ Wa1.T                          # basis_mat
            keep(raw)
            cf = torch.clamp(raw, fmin, cmax)
            sf = torch.clamp(sraw, smin, cmax)
            feat = torch.cat([sf.unsqueeze(-1), cf], dim=-1)
        else:
            h1 = X @ Wa1.T                           # sigma_net.0
            keep(h1)
            h = torch.relu(h1) @ Wa2.T               # sigma_net.1
            keep(h)
            sf = torch.clamp(h[:, 0], smin, cmax)    # channel 0 only (network.py:393)
            cf = h[:, 1:]
            feat = torch.cat([sf.unsqueeze(-1), cf], dim=-1)
        sigma = trunc_exp64(sf)
        c1 = torch.cat([sh4(dirs), cf], dim=-1) @ Wc1.T
        keep(c1)
        c2 = torch.relu(c1) @ Wc2.T
        keep(c2)
        c3 = torch.relu(c2) @ Wc3.T
        keep(c3)
        rgb = torch.sigmoid(c3)
        out = {"sigma": sigma.detach(), "rgb": rgb.detach(), "feat16": feat.detach()}
        if not grads:
            return out
        w = (lambda g: g.to(torch.float64)) if row_weight is None else \
            (lambda g: g.to(torch.float64) * row_weight.to(torch.float64).reshape(-1, *([1] * (g.dim() - 1))))
        loss = torch.zeros((), dtype=torch.float64, device=X.device)
        if g_sigma is not None:
            loss = loss + (sigma * w(g_sigma)).sum()
        for g in (g_rgb, g_rgb2):
            if g is not None:
                loss = loss + (rgb * w(g)).sum()
        if g_feat16 is not None:
            loss = loss + (feat * w(g_feat16)).sum()
        if not loss.requires_grad:
            loss = loss + 0.0 * rgb.sum()
        loss.backward()
    gx = X.grad
    if hash_layout:
        gx = gx.reshape(M, 14, 2).permute(1, 0, 2).contiguous()
    out["g_x0"] = gx
    out["gWa1"], out["gWc1"], out["gWc2"], out["gWc3"] = Wa1.grad, Wc1.grad, Wc2.grad, Wc3.grad
    if kind == "vm":
        out["g_sigma_raw"] = sraw.grad
    else:
        out["gWa2"] = Wa2.grad
    mx = max([float(t.grad.abs().max()) if t.grad is not None and t.numel() else 0.0 for t in inter] + [float(X.grad.abs().max()) if M else 0.0])
    out["inter_max"] = mx
    return out


def clamp_boundary_case(kind, values, seed=0, device="cpu"):
    """Inputs whose clamped pre-activations hit `values` EXACTLY in every formulation (f16 values, one-hot inputs, fp32 sums of one
    non-zero product), and where the weight gradient shows each row's clamp mask on its own.

    VM: row r has prod[r] = one-hot at column r and sigma_raw[r] = values[r % n]; basis_mat[c, r] = values[(r + c) % n], so the colour
    feature c of row r is values[(r + c) % n] and d basis_mat[c, r] is that row's masked feature gradient alone.
    Hash: row r has encoder feature r = 1 (M <= 28); sigma_net.0 passes feature k through hidden unit k (weight 1, the rest 0) and
    sigma_net.1[0, k] = values[k % n], so h0 of row r is values[r % n] and d sigma_net.1[0, r] is that row's masked h0 gradient alone.
    Returns (x0 in the kernel's layout as f16, sigma_raw or None, dirs, (Wa1, Wa2, Wc1, Wc2, Wc3) fp32)."""
    kind = _kind(kind)
    g = torch.Generator().manual_seed(seed)
    vals = torch.tensor([float(v) for v in values], dtype=torch.float32)
    n = vals.numel()
    assert bool((vals.half().float() == vals).all()), "boundary values must be f16 numbers"
    M = 144 if kind == "vm" else 28
    rnd = lambda *s: (torch.randn(*s, generator=g) * 0.3).half().float()
    d = torch.randn(M, 3, generator=g)
    d = d / d.norm(dim=-1, keepdim=True)
    Wc1, Wc2, Wc3 = rnd(64, 31), rnd(64, 64), rnd(3, 64)
    r = torch.arange(M)
    X = torch.zeros(M, M)
    X[r, r] = 1.0
    if kind == "vm":
        Wa1 = vals[(r[None, :] + torch.arange(15)[:, None]) % n].clone()  # [15, 144]
        sraw = vals[r % n].clone()
        x0, Wa2 = X.half(), None
    else:
        Wa1 = torch.zeros(64, 28)
        Wa1[r, r] = 1.0
        Wa2 = rnd(16, 64)
        Wa2[0, :] = 0.0
        Wa2[0, :28] = vals[r % n]
        sraw = None
        x0 = X.half().reshape(M, 14, 2).permute(1, 0, 2).contiguous()
    to = lambda t: None if t is None else t.to(device)
    return to(x0), to(sraw), to(d), tuple(to(w) for w in (Wa1, Wa2, Wc1, Wc2, Wc3))


def f16_neighbours(v):
    """[the f16 number one ulp below v, v, the one one ulp above] (v a non-zero f16 number)"""
    b = int(torch.tensor([float(v)], dtype=torch.float16).view(torch.int16))
    step = 1 if v > 0 else -1  # (sign-magnitude bits: for v < 0 a larger magnitude is a lower number)
    return [float(torch.tensor([b + k * step], dtype=torch.int16).view(torch.float16)) for k in (-1, 0, 1)]
