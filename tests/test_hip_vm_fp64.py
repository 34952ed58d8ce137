"""The VM plane x line lookup (pvd_vm_forward / pvd_vm_backward: the register-window walk of csrc/vmencoder.hip and vm_lookup.h)
against the float64 restatement in tests/vm_ref64.py, element by element, under the bound derived there:

    |kernel - fp64| <= eps32 ((16 + n) Y_abs + 2 (S - 1) Y_w)      (+ 2^-11 |ref| + 2^-25 for f16 products)

The inputs are scripted in texel space so that every plane move (same, +x, -x, +y, -y, jump) and line move (same, +1, -1, jump)
of every factor set that the table sizes admit (vm_ref64.reachable: all of them except on the (1, 2, 5) tables) occurs on the
interior fast path and on the generic path at least 8 times whatever chunk length the launch picks (asserted from the reference's
own coordinates, vm_ref64.assert_coverage, for the walk cases and, on the CPU, for their tilings to 32 767 and 65 536 rows; the
short prefixes M <= 65 of the run-length test necessarily cover less), each face of the box is crossed out and back by single
texels, and run lengths end on, before and behind every chunk boundary and every threshold of the chunk choice.  Both
table layouts (dense, interleaved [H][W][64]), both product types, a non-unit asymmetric aabb, axes of size 1 and 2, the
device-side row count and the write guards of outputs and gradient buffers go through pvd_hip.vm_forward / vm_backward directly.

Every test prints its max(err / bound) line (pytest -s); profiles/vm_fp64_pin.txt keeps the lines of one run on the MI355X next to
the same ratios of torch's float32 grid_sample formulation on the CPU.  Those numbers are a record; the threshold is the bound.

Out of scope: the persistent render's per-row lookup (sample_ctl / issue6 / finish6 of vm_lookup.h), which has no entry point of
its own (tests/test_hip_infer_rounds.py compares the render); the found_inf word of the backward rider (test_hip_head_fp64.py);
inf / nan coordinates.  No hipGraph is recorded here."""
import functools

import numpy as np
import pytest
import torch

import vm_ref64 as v

pytestmark = pytest.mark.gpu

SIZES = [(9, 17, 33), (24, 31, 45), (1, 2, 5)]
CASES = [(res, box) for res in SIZES for box in ("unit", "asym")] + [((9, 17, 33), "lattice")]
FWD_NAMES = ["sigma_feat", "color_prod"]
PAD = 192  # sentinel floats around the guarded forward outputs


def _case(res, box):
    return v.lattice(res) if box == "lattice" else v.walk_case(res, box)


def _say(capsys, line):
    with capsys.disabled():
        print("\n" + line, end="")


def _device_tables(tables, layout):
    """the twelve factors on the device, channels-last; interleaved: sigma and colour factor of the same texels share one buffer"""
    from vmencoder.vm import interleave_factors, to_channels_last_param
    tabs = [to_channels_last_param(t.cuda()) for t in tables]
    if layout == "interleaved":
        for j in range(6):
            tabs[j], tabs[6 + j] = interleave_factors(tabs[j], tabs[6 + j])
    return tabs


def _grad_buffers(tabs, layout, prefill=None):
    from vmencoder.vm import interleave_factors
    src = [torch.zeros(t.shape, device="cuda") if prefill is None else prefill[j].cuda() for j, t in enumerate(tabs)]
    if layout == "interleaved":
        out = [None] * 12
        for j in range(6):
            out[j], out[6 + j] = interleave_factors(src[j], src[6 + j])
        return out
    out = [torch.empty_strided(t.shape, t.stride(), dtype=torch.float32, device="cuda") for t in tabs]
    for o, s in zip(out, src):
        o.copy_(s)
    return out


def _forward(xyz, aabb, tabs, res, f16=False, rows_dev=None, out=None):
    import pvd_hip
    M = xyz.shape[0]
    if out is None:
        out = (torch.full((M,), float("nan"), device="cuda"), torch.full((M, 144), float("nan"), dtype=torch.float16 if f16 else torch.float32, device="cuda"))
    pvd_hip.vm_forward(xyz, list(aabb), tabs, list(res), out[0], out[1], rows_dev=rows_dev)
    return out


def _backward(xyz, aabb, tabs, res, gs, gp, grads):
    import pvd_hip
    pvd_hip.vm_backward(xyz, list(aabb), tabs, list(res), gs, gp, grads)
    return grads


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def _where_forward(case_xyz, aabb, res, got_prod, out):
    """bookkeeping of the worst forward row, for the failure message"""
    err = (got_prod.detach().cpu().double() - out.y).abs() / v.bound(out, max(res)).clamp_min(1e-300)
    m = int(err.amax(1).argmax())
    i0 = v.coords(case_xyz, aabb, res).i0.numpy()
    return "; ".join(v.describe(i0, res, c, m) for c in v.CHUNKS)


def _check(capsys, label, xyz_np, aabb, res, tables, layout="dense", f16=False, fwd=None, bwd=None, grads_in=None, do_forward=True, do_backward=True):
    """forward and backward of one case through the binding against the float64 reference; prints the ratio lines"""
    S = max(res)
    xyz = torch.from_numpy(xyz_np).cuda()
    tabs = _device_tables(tables, layout)
    result = {}
    if do_forward:
        sig, prod = _forward(xyz, aabb, tabs, res, f16)
        outs = [fwd["sigma_feat"], fwd["color_prod"]]
        line, worst = v.report("hip fwd %s %s %s" % (label, "f16" if f16 else "f32", layout), FWD_NAMES, [sig, prod], outs, S, f16)
        _say(capsys, line)
        assert worst <= 1.0, (line, _where_forward(xyz_np, aabb, res, prod, outs[1]))
        result["fwd"] = (sig, prod)
    if do_backward:
        gs, gp = grads_in
        grads = _backward(xyz, aabb, tabs, res, gs.cuda(), gp.cuda(), _grad_buffers(tabs, layout))
        line, worst = v.report("hip bwd %s %s %s" % (label, "f16" if f16 else "f32", layout), v.TABLE_NAMES, grads, bwd, S)
        _say(capsys, line)
        assert worst <= 1.0, line
        result["bwd"] = grads
    return result


# ---------------------------------------------------------------------------------------------- scripted walks, lattice points
@pytest.mark.parametrize("layout", ["dense", "interleaved"])
@pytest.mark.parametrize("f16", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("res,box", CASES)
def test_scripted_walks_and_lattice_points_forward_and_backward(res, box, f16, layout, capsys):
    case = _case(res, box)
    if box != "lattice":
        v.assert_coverage(case.C.i0.numpy(), res)
    r = _check(capsys, case.label, case.xyz, case.aabb, res, case.tables, layout, f16, case.fwd, case.bwd(f16), case.grads(f16))
    if layout == "interleaved":  # same values, same operation order: the dense launch's outputs bit for bit
        sig_d, prod_d = _forward(torch.from_numpy(case.xyz).cuda(), case.aabb, _device_tables(case.tables, "dense"), res, f16)
        assert torch.equal(_bits(r["fwd"][0]), _bits(sig_d)) and torch.equal(_bits(r["fwd"][1]), _bits(prod_d))


# ---------------------------------------------------------------------------------------------- run lengths
# pick_chunk(), csrc/vmencoder.hip ("static uint32_t pick_chunk(uint32_t M, bool backward)"):
#   backward: chunk = 64, halved while chunk > 16 && 3 M / chunk < 3072  ->  32 from M = 32 768, 64 from M = 65 536
#   forward : chunk = 16, doubled while chunk < 64 && M / chunk > 256 * 32  ->  32 from M = 131 088, 64 from M = 262 176
BWD_THRESHOLDS = [32768, 65536]
FWD_THRESHOLDS = [131088, 262176]


@functools.lru_cache(maxsize=2)
def _tiled(res, box, M):
    case = v.walk_case(res, box)
    return v.tile_case(case.meta, M)


def _sub_reference(case, xyz_np, rows=None, backward=True, f16=False):
    C = v.coords(xyz_np if rows is None else xyz_np[rows], case.aabb, case.res)
    fwd = v.forward(C, case.tables, case.res)
    if not backward:
        return fwd, None, None
    gs, gp = v.make_grads(xyz_np.shape[0], case.grad_seed + 1, f16)
    return fwd, v.backward(C, case.tables, case.res, gs, gp), (gs, gp)


@pytest.mark.parametrize("M", [1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 4099])
def test_run_lengths_around_every_chunk_length(M, capsys):
    case = v.walk_case((24, 31, 45), "unit")
    xyz = _tiled(case.res, "unit", 4099)[:M].copy()
    fwd, bwd, g = _sub_reference(case, xyz)
    _check(capsys, "M=%d %s" % (M, case.label), xyz, case.aabb, case.res, case.tables, fwd=fwd, bwd=bwd, grads_in=g)


@pytest.mark.parametrize("M", [t + d for t in BWD_THRESHOLDS for d in (-1, 0)])
def test_backward_either_side_of_each_chunk_threshold(M, capsys):
    """the whole backward against float64 (the walk repeated cyclically, every other repetition with its rays in reverse order)"""
    case = v.walk_case((24, 31, 45), "asym")
    xyz = _tiled(case.res, "asym", max(BWD_THRESHOLDS))[:M].copy()
    _, bwd, g = _sub_reference(case, xyz)
    _check(capsys, "M=%d %s" % (M, case.label), xyz, case.aabb, case.res, case.tables, bwd=bwd, grads_in=g, do_forward=False)


@pytest.mark.parametrize("M", [t + d for t in FWD_THRESHOLDS for d in (-1, 0)])
def test_forward_either_side_of_each_chunk_threshold(M, capsys):
    """rows are independent in the forward: the first and last 4096 rows and 8192 rows drawn from between are compared"""
    case = v.walk_case((9, 17, 33), "asym")
    xyz_np = _tiled(case.res, "asym", max(FWD_THRESHOLDS))[:M].copy()
    rng = np.random.default_rng(M)
    rows = np.concatenate([np.arange(4096), np.sort(rng.choice(np.arange(4096, M - 4096), 8192, replace=False)), np.arange(M - 4096, M)])
    fwd, _, _ = _sub_reference(case, xyz_np, rows, backward=False)
    sig, prod = _forward(torch.from_numpy(xyz_np).cuda(), case.aabb, _device_tables(case.tables, "dense"), case.res)
    sel = torch.from_numpy(rows).cuda()
    line, worst = v.report("hip fwd M=%d %s f32 dense" % (M, case.label), FWD_NAMES, [sig[sel], prod[sel]], [fwd["sigma_feat"], fwd["color_prod"]], case.S)
    _say(capsys, line)
    assert worst <= 1.0, line
    assert not torch.isnan(sig).any() and not torch.isnan(prod).any()  # every row was written


# ---------------------------------------------------------------------------------------------- hot texel, random points
def _conservation(capsys, label, grads, bwd, S):
    """sum(grad_table) per factor equals the reference's within the bound summed over the table: a double flush shows here even if
    spread thin"""
    parts = []
    for nm, g, o in zip(v.TABLE_NAMES, grads, bwd):
        err = abs(float(g.detach().cpu().double().sum() - o.y.sum()))
        lim = float(v.bound(o, S).sum())
        parts.append((nm, err / lim if lim > 0 else (0.0 if err == 0 else float("inf"))))
    line = "hip sum %s | " % label + " ".join("%s=%.3g" % p for p in parts)
    _say(capsys, line)
    assert max(r for _, r in parts) <= 1.0, line


@pytest.mark.parametrize("which,res,box", [("hot", (24, 31, 45), "unit"), ("hot", (9, 17, 33), "asym"), ("uniform", (24, 31, 45), "asym"),
                                           ("uniform", (1, 2, 5), "unit")])
def test_hot_texel_and_uniform_random_points(which, res, box, capsys):
    """What the hot texel can see: with n = 65 536 contributions per texel the bound is about eps32 * 65 552 * Y_abs, 0.8 % of the
    element -- a texel flushed to the wrong place, a run lost altogether at a border of the footprint, a weight applied to the wrong
    tap (all 100 % of an element) and accumulation that degrades with n.  What it cannot see: ONE run of 64 rows flushed twice is
    0.1 % of the element, inside the bound of both the element and the sum; a double flush is caught where n is small, by the
    scripted walks and the uniform points (n of a few to a few hundred per texel, where one run is a large share of the element),
    and by the conservation sum of those cases."""
    case = v.walk_case(res, box)
    xyz = v.hot_case(65536, case.aabb) if which == "hot" else v.uniform_case(20011, case.aabb, seed=13)
    fwd, bwd, g = _sub_reference(case, xyz)
    label = "%s M=%d %s %s" % (which, xyz.shape[0], "x".join(map(str, res)), box)
    r = _check(capsys, label, xyz, case.aabb, res, case.tables, fwd=fwd, bwd=bwd, grads_in=g)
    _conservation(capsys, label, r["bwd"], bwd, case.S)


# ---------------------------------------------------------------------------------------------- accumulation
@pytest.mark.parametrize("layout", ["dense", "interleaved"])
def test_backward_accumulates_into_prefilled_buffers(layout, capsys):
    case = v.walk_case((9, 17, 33), "unit")
    g = torch.Generator().manual_seed(17)
    prefill = [torch.randn(t.shape, generator=g) for t in case.tables]
    tabs = _device_tables(case.tables, layout)
    gs, gp = case.grads()
    grads = _backward(torch.from_numpy(case.xyz).cuda(), case.aabb, tabs, case.res, gs.cuda(), gp.cuda(), _grad_buffers(tabs, layout, prefill))
    want = [v.Out(o.y + p.double(), o.y_abs, o.y_w, o.n) for o, p in zip(case.bwd(), prefill)]
    line, worst = v.report("hip bwd prefilled %s %s" % (case.label, layout), v.TABLE_NAMES, grads, want, case.S,
                           extras=[v.EPS32 * p.double().abs() for p in prefill])
    _say(capsys, line)
    assert worst <= 1.0, line


# ---------------------------------------------------------------------------------------------- rows_dev, write guards
def _guarded(shape, dtype):
    """a contiguous view of `shape` in the middle of a NaN-filled buffer -> (buffer, view)"""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * PAD,), float("nan"), dtype=dtype, device="cuda")
    return buf, buf[PAD:PAD + n].view(shape)


def _margins_untouched(buf, n):
    nan = _bits(torch.full((1,), float("nan"), dtype=buf.dtype, device="cuda"))[0]
    b = _bits(buf)
    return bool((b[:PAD] == nan).all()) and bool((b[PAD + n:] == nan).all())


@pytest.mark.parametrize("f16", [False, True], ids=["f32", "f16"])
def test_device_row_count_and_forward_write_guards(f16):
    case = v.walk_case((24, 31, 45), "asym")
    M = 1000
    xyz = torch.from_numpy(case.xyz[:M].copy()).cuda()
    tabs = _device_tables(case.tables, "dense")
    dt = torch.float16 if f16 else torch.float32
    sig0, prod0 = _forward(xyz, case.aabb, tabs, case.res, f16)
    assert not torch.isnan(sig0).any() and not torch.isnan(prod0.float()).any()
    for c in (0, 1, 17, M - 1, M, M + 500):
        sbuf, sig = _guarded((M,), torch.float32)
        pbuf, prod = _guarded((M, 144), dt)
        _forward(xyz, case.aabb, tabs, case.res, f16, rows_dev=torch.tensor([c], dtype=torch.int32, device="cuda"), out=(sig, prod))
        k = min(c, M)
        assert torch.equal(_bits(sig[:k]), _bits(sig0[:k])) and torch.equal(_bits(prod[:k]), _bits(prod0[:k])), c
        assert torch.isnan(sig[k:]).all() and torch.isnan(prod[k:].float()).all(), c
        assert _margins_untouched(sbuf, M) and _margins_untouched(pbuf, M * 144), c


GRAD_SENTINEL = 1.0  # finite: the backward only ever ADDS to gradient memory, and NaN + a keeps NaN's bits


def _guarded_grad(buf_floats, pad, views):
    """a buffer of pad + buf_floats + pad floats filled with GRAD_SENTINEL, its middle zeroed -> (buffer, [as_strided views])"""
    buf = torch.full((buf_floats + 2 * pad,), GRAD_SENTINEL, device="cuda")
    buf[pad:pad + buf_floats] = 0.0
    return buf, [torch.as_strided(buf, t.shape, t.stride(), pad + off) for t, off in views]


def _grad_margins_untouched(buf, n, pad):
    want = _bits(torch.full((1,), GRAD_SENTINEL, device="cuda"))[0]
    b = _bits(buf)
    return bool((b[:pad] == want).all()) and bool((b[pad + n:] == want).all())


@pytest.mark.parametrize("layout", ["dense", "interleaved"])
@pytest.mark.parametrize("res", [(24, 31, 45), (1, 2, 5)])
def test_gradient_buffers_inside_sentinel_margins(res, layout, capsys):
    """The twelve gradient tables are views into larger buffers whose margins hold a finite sentinel (1.0: the walk's contributions
    are O(1) and reach memory only through atomic adds, so any stray add changes the bits).  Each margin is two rows plus two texels
    of the case's widest plane at the layout's texel stride, so a flush at y = -1 or y = H (any x of the footprint), or at x = -1 /
    x = W of the first / last row, lands inside it.  Such a write changes no in-table element: the float64 comparison alone would not
    see it.  The face crossings and the far-outside stretches of the walk must leave every margin as it was, and the views hold the
    reference's gradients."""
    case = v.walk_case(res, "unit")
    tabs = _device_tables(case.tables, layout)
    pad = (2 * max(res) + 2) * 64
    bufs, grads = [], [None] * 12
    for j in range(6):
        ts, tc = tabs[j], tabs[6 + j]
        H, W = ts.shape[2:]
        if layout == "interleaved":
            n = H * W * 64
            buf, (grads[j], grads[6 + j]) = _guarded_grad(n, pad, [(ts, 0), (tc, v.RS)])
            bufs.append((buf, n))
        else:
            for jj, t in ((j, ts), (6 + j, tc)):
                buf, (grads[jj],) = _guarded_grad(t.numel(), pad, [(t, 0)])
                bufs.append((buf, t.numel()))
    for g, t in zip(grads, tabs):
        assert g.stride() == t.stride() and not g.any()
    gs, gp = case.grads()
    _backward(torch.from_numpy(case.xyz).cuda(), case.aabb, tabs, res, gs.cuda(), gp.cuda(), grads)
    for buf, n in bufs:
        assert _grad_margins_untouched(buf, n, pad)
    stray = bufs[0][0].clone()
    stray[pad - 1] += 1e-3  # (the check itself: one small add just outside a table is seen)
    assert not _grad_margins_untouched(stray, bufs[0][1], pad)
    line, worst = v.report("hip bwd guarded %s %s" % (case.label, layout), v.TABLE_NAMES, grads, case.bwd(), case.S)
    _say(capsys, line)
    assert worst <= 1.0, line
