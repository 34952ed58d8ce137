"""The Plenoxel lookup and its SH colour head (pvd_plenoxel_forward / pvd_plenoxel_backward: the register-window walk of
csrc/plenoxel.hip) against the float64 restatement in tests/plenoxel_ref64.py, element by element, under the bound derived there:

    |kernel - fp64| <= eps32 ((K + n) Y_abs + 2 (S - 1) Y_w) + extra      (K = 11 features, 12 / 14 / 16 head, 9 gradient)

The inputs are scripted in voxel space so that every move of the 2x2x2 footprint (open, same, +-x, +-y, +-z, jump) that the volume
admits occurs with the footprint inside, partly outside and wholly outside the volume at least 8 times whatever chunk length the
launch picks (plenoxel_ref64.assert_coverage, from the reference's own coordinates; the tilings to the thresholds of the chunk choice
are asserted on the CPU), each face is crossed out and back by single voxels, run lengths end on, before and behind every chunk
boundary, and 131 087 / 131 088 / 262 175 / 262 176 rows sit either side of the two thresholds of px_chunk.  Every forward form
(features, head, both) and every backward form (g_feat alone without directions, every non-empty subset of g_sigma / g_sigma_l /
g_rgb, all four) into a zero and into a prefilled buffer, both clip ranges ([-2, 7] active on both sides; [-15, 15] with |h0| > 12,
where the backward's +-12 clamp decides), the lattice points where h0 equals a clip value exactly, a non-unit asymmetric aabb, axes
of size 1 and 2, degrees 1 to 3, the largest volume of the 24-bit offset form and the smallest of the 64-bit form go through
pvd_hip.plenoxel_forward / plenoxel_backward directly.  Outputs and gradient buffers lie between sentinel margins; buffers a call
must not depend on are NaN-poisoned.

Every test prints its max(err / bound) line (pytest -s); profiles/plenoxel_fp64_pin.txt keeps the lines of one run on the MI355X next
to the same ratios of torch's float32 grid_sample formulation on the CPU and the measured expf figure.  Those numbers are a record;
the threshold is the bound.

Out of scope: k_infer_px_persistent, which has no entry point per row (tests/test_hip_infer_rounds.py compares the render); inf / nan
coordinates; the autograd wrappers of plenoxel/volume.py (tests/test_hip_plenoxel.py keeps covering them).  No graph is recorded."""
import functools
import itertools

import numpy as np
import pytest
import torch

import plenoxel_ref64 as R
import vm_ref64 as v

pytestmark = pytest.mark.gpu

WALKS = [((9, 7, 5), 3), ((33, 17, 65), 3), ((1, 2, 5), 3), ((20, 24, 28), 2), ((9, 7, 5), 1)]
CASES = [(dims, deg, box, "narrow") for dims, deg in WALKS for box in ("unit", "asym")] + [((9, 17, 33), 3, "lattice", "narrow")] + \
        [((9, 7, 5), 3, "unit", "wide"), ((9, 7, 5), 3, "asym", "wide"), ((20, 24, 28), 2, "unit", "wide")]
FWD_NAMES = ["feat", "h0_raw", "sigma_l", "sigma", "rgb"]
HEAD_NAMES = FWD_NAMES[1:]
HEAD_GRADS = ("g_sigma", "g_sigma_l", "g_rgb")
ALL = ("g_feat",) + HEAD_GRADS
BWD_FORMS = [("g_feat",)] + [c for r in (1, 2, 3) for c in itertools.combinations(HEAD_GRADS, r)] + [ALL]
THRESHOLDS = [131087, 131088, 262175, 262176]  # px_chunk(): 32 from M / 16 > 8192, 64 from M / 32 > 8192
PAD = 192  # sentinel floats around the forward outputs
GRAD_SENTINEL = 1.0  # finite: the backward only ever ADDS to gradient memory, and NaN + a keeps NaN's bits
NAN = float("nan")


def _case(dims, deg, box, clip="narrow"):
    return R.lattice(dims, deg) if box == "lattice" else R.walk_case(dims, box, deg, clip)


def _say(capsys, line):
    with capsys.disabled():
        print("\n" + line, end="")


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---------------------------------------------------------------------------------------------- device buffers
def _as_param(flat, dims, C, offset=0):
    """a [1,C,D,H,W] view with channels-last strides over a flat float buffer"""
    D, H, W = dims
    return torch.as_strided(flat, (1, C, D, H, W), (C * D * H * W, 1, H * W * C, W * C, C), offset)


def _device_volume(rows, dims):
    return _as_param(rows.cuda().contiguous().view(-1), dims, rows.shape[1])


def _guarded(shape):
    """a contiguous view of `shape` in the middle of a NaN-filled buffer -> (buffer, view)"""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * PAD,), NAN, device="cuda")
    return buf, buf[PAD:PAD + n].view(shape)


def _margins(buf, n, pad, value):
    want = _bits(torch.full((1,), value, device="cuda"))[0]
    b = _bits(buf)
    return bool((b[:pad] == want).all()) and bool((b[pad + n:] == want).all())


def _grad_pad(dims, C):
    """one layer, one row and two voxels: a flush one voxel outside the volume in any direction lands in the margin"""
    return (dims[1] * dims[2] + dims[2] + 2) * C


def _grad_buffer(dims, C, prefill=None):
    """the gradient volume with the parameter's strides between margins of GRAD_SENTINEL -> (buffer, [1,C,D,H,W] view, pad)"""
    n, pad = int(np.prod(dims)) * C, _grad_pad(dims, C)
    buf = torch.full((n + 2 * pad,), GRAD_SENTINEL, device="cuda")
    if prefill is None:
        buf[pad:pad + n] = 0.0
    else:
        buf[pad:pad + n] = prefill.cuda().reshape(-1)
    return buf, _as_param(buf, dims, C, pad), pad


def _forward(case, xyz, dirs, vol, form):
    """one call of the binding -> {name: tensor}; outputs between NaN margins, which the call must leave alone"""
    import pvd_hip
    M, C = xyz.shape[0], R.channels(case.degree)
    shapes = {"feat": (M, C), "h0_raw": (M,), "sigma_l": (M,), "sigma": (M,), "rgb": (M, 3)}
    names = {"features": ["feat"], "head": HEAD_NAMES, "both": FWD_NAMES}[form]
    bufs = {nm: _guarded(shapes[nm]) for nm in names}
    o = {nm: bufs[nm][1] if nm in bufs else None for nm in FWD_NAMES}
    pvd_hip.plenoxel_forward(xyz, None if form == "features" else dirs, list(case.aabb), vol, case.degree, case.clip[0], case.clip[1],
                             o["feat"], o["h0_raw"], o["sigma_l"], o["sigma"], o["rgb"])
    for nm in names:
        assert _margins(bufs[nm][0], int(np.prod(shapes[nm])), PAD, NAN), nm
    return {nm: o[nm] for nm in names}


def _backward(case, xyz, dirs, names, inputs, grad):
    """one call of the binding.  inputs: {h0_raw, rgb, g_*} on the device.  Without a head gradient the call gets no directions (then
    only g_feat counts); a teacher-forced input the result must not depend on is NaN-poisoned"""
    import pvd_hip
    head = any(nm != "g_feat" for nm in names)
    M = xyz.shape[0]
    h0 = rgb = None
    if head:
        h0 = inputs["h0_raw"] if ("g_sigma" in names or "g_sigma_l" in names) else torch.full((M,), NAN, device="cuda")
        rgb = inputs["rgb"] if "g_rgb" in names else torch.full((M, 3), NAN, device="cuda")
    g = {nm: (inputs[nm] if nm in names else None) for nm in ALL}
    pvd_hip.plenoxel_backward(xyz, dirs if head else None, list(case.aabb), case.degree, case.clip[0], case.clip[1], h0, rgb,
                              g["g_feat"], g["g_sigma"], g["g_sigma_l"], g["g_rgb"], grad)


def _grad_rows(grad):
    """[1,C,D,H,W] channels-last -> rows [V,C]"""
    return grad[0].permute(1, 2, 3, 0).reshape(-1, grad.shape[1])


def _where(case, M, got, val):
    err = ((got.detach().cpu().double().reshape(val.y.shape) - val.y).abs() / val.b.clamp_min(1e-300)).reshape(M, -1)
    m = int(err.amax(1).argmax())
    return "; ".join(R.describe(case.C.i0.numpy()[:M], case.dims, c, m) for c in R.CHUNKS)


def _device_inputs(case, M=None):
    M = case.M if M is None else M
    h0, rgb = case.forced()
    d = {"h0_raw": h0[:M], "rgb": rgb[:M]}
    d.update({k: t[:M] for k, t in case.grads.items()})
    return {k: t.contiguous().cuda() for k, t in d.items()}


# ---------------------------------------------------------------------------------------------- the library allowance
def _expf_ulps(sigma_l, sigma):
    """device expf as the forward used it: sigma against numpy's float64 exp of the same float32 argument, in float32 ulps"""
    x = sigma_l.detach().cpu().numpy().astype(np.float64)
    want = np.exp(x)
    return float((np.abs(sigma.detach().cpu().numpy().astype(np.float64) - want) / np.spacing(want.astype(np.float32)).astype(np.float64)).max())


def test_device_expf_allowance(capsys):
    """EXPF_ULPS of plenoxel_ref64: twice the largest distance of the kernel's expf from numpy's float64 exp over the arguments of
    the wide-clip walks and the lattice case ([-15, 15]) and 4096 arguments spread over [-15, 15] by way of the volume itself"""
    worst = 0.0
    for case in [R.walk_case((9, 7, 5), "unit", 3, "wide"), R.walk_case((20, 24, 28), "unit", 2, "wide"), R.lattice()]:
        o = _forward(case, torch.from_numpy(case.xyz).cuda(), torch.from_numpy(case.dirs).cuda(), _device_volume(case.rows, case.dims), "head")
        worst = max(worst, _expf_ulps(o["sigma_l"], o["sigma"]))
    # a one-voxel-thick line of voxels whose channel 0 sweeps [-15, 15]; samples at the voxel centres read the values themselves
    n = 4097
    rows = torch.zeros(n, 4)
    rows[:, 0] = torch.linspace(-15.0, 15.0, n)
    xyz = np.zeros((n, 3), np.float32)
    xyz[:, 0] = (2.0 * np.arange(n) / (n - 1) - 1.0).astype(np.float32)
    line = R.Case("expf sweep", xyz, (1, 1, n), v.UNIT_AABB, 1, (-15.0, 15.0), rows)
    o = _forward(line, torch.from_numpy(line.xyz).cuda(), torch.from_numpy(line.dirs).cuda(), _device_volume(rows, line.dims), "head")
    assert R.ratio(o["sigma_l"], line.fwd["sigma_l"]) <= 1.0
    worst = max(worst, _expf_ulps(o["sigma_l"], o["sigma"]))
    _say(capsys, "[plenoxel fp64] device expf(x), x in [-15, 15]: max %.3f float32 ulp from numpy's float64 exp; EXPF_ULPS = %.3g" % (worst, R.EXPF_ULPS))
    assert 2 * worst <= R.EXPF_ULPS, "plenoxel_ref64.EXPF_ULPS must be twice the measured %.3f" % worst


# ---------------------------------------------------------------------------------------------- every form on every scripted case
def _check_forward(capsys, case, xyz, dirs, vol, M, fwd, label):
    outs = {}
    for form in ("features", "head", "both"):
        o = _forward(case, xyz, dirs, vol, form)
        line, worst = R.report("hip fwd %s %s" % (form, label), list(o), list(o.values()), [fwd[nm] for nm in o])
        _say(capsys, line)
        assert worst <= 1.0, (line, _where(case, M, o.get("feat", o.get("rgb")), fwd["feat" if "feat" in o else "rgb"]))
        outs[form] = o
    for nm in HEAD_NAMES:  # the same expressions in the same order, with or without the feature store
        assert torch.equal(_bits(outs["head"][nm]), _bits(outs["both"][nm])), nm
    assert torch.equal(_bits(outs["features"]["feat"]), _bits(outs["both"]["feat"]))
    return outs


def _check_backward(capsys, case, xyz, dirs, M, names, inputs, G, label, prefill=None):
    C = R.channels(case.degree)
    buf, grad, pad = _grad_buffer(case.dims, C, prefill)
    _backward(case, xyz, dirs, names, inputs, grad)
    assert _margins(buf, int(np.prod(case.dims)) * C, pad, GRAD_SENTINEL), ("a write outside the gradient volume", names)
    got = _grad_rows(grad)
    line, worst = R.report("hip bwd %s %s%s" % ("+".join(nm[2:] for nm in names), label, " prefilled" if prefill is not None else ""),
                           ["g_volume"], [got], [R.Val(G.y, G.b)])
    _say(capsys, line)
    assert worst <= 1.0, line
    return got


@pytest.mark.parametrize("dims,deg,box,clip", CASES)
def test_scripted_walks_and_lattice_points_every_forward_and_backward_form(dims, deg, box, clip, capsys):
    case = _case(dims, deg, box, clip)
    if box != "lattice":
        R.assert_coverage(case.C.i0.numpy(), dims)
    h0 = case.fwd["h0_raw"].y
    lo, hi = case.clip
    if clip == "wide":
        assert ((h0.abs() > 12) & (h0.abs() <= 15)).sum() >= 20 and (h0 > hi).any() and (h0 < lo).any()
    else:
        assert (h0 < lo).sum() >= 10 and (h0 > hi).sum() >= 10 and ((h0 > lo) & (h0 < hi)).sum() >= 10
    xyz, dirs = torch.from_numpy(case.xyz).cuda(), torch.from_numpy(case.dirs).cuda()
    _check_forward(capsys, case, xyz, dirs, _device_volume(case.rows, case.dims), case.M, case.fwd, case.label)
    inputs = _device_inputs(case)
    g = torch.Generator().manual_seed(17)
    prefill = torch.randn(int(np.prod(dims)), R.channels(deg), generator=g)
    for names in BWD_FORMS:
        _check_backward(capsys, case, xyz, dirs, case.M, names, inputs, case.bwd(names), case.label)
        _check_backward(capsys, case, xyz, dirs, case.M, names, inputs, case.bwd(names, prefill), case.label, prefill)


# ---------------------------------------------------------------------------------------------- kernel forward into kernel backward
def _clear_of_the_clips(case):
    """clip values near the case's own such that no reference h0 lies within its bound of either: decided from the reference alone"""
    h0, b = case.fwd["h0_raw"].y, case.fwd["h0_raw"].b
    out = []
    for c in case.clip:
        j = 0
        while bool(((h0 - (c + j * 2.0 ** -9)).abs() <= 4.0 * b).any()):
            j += 1
        out.append(c + j * 2.0 ** -9)
    return tuple(out)


@pytest.mark.parametrize("dims,deg,box,clip", [((9, 7, 5), 3, "asym", "narrow"), ((20, 24, 28), 2, "unit", "wide")])
def test_chained_kernel_forward_into_kernel_backward(dims, deg, box, clip, capsys):
    """The backward reads the forward kernel's own h0_raw and rgb.  The clip values are moved (by multiples of 2^-9) until no
    reference h0 lies within four times its bound of either, so the kernel's mask is the reference's on every sample; the bounds of
    h0_raw and rgb enter the gradient's bound through exp and (1 - y) y.  No sample is left out."""
    base = _case(dims, deg, box, clip)
    case = R.Case(base.label + " chained", base.xyz, dims, base.aabb, deg, _clear_of_the_clips(base), base.rows, base.meta)
    f = case.fwd
    h0, b = f["h0_raw"].y, f["h0_raw"].b
    assert all(bool(((h0 - c).abs() > 4.0 * b).all()) for c in case.clip) and (h0 < case.clip[0]).any() and (h0 > case.clip[1]).any()
    xyz, dirs = torch.from_numpy(case.xyz).cuda(), torch.from_numpy(case.dirs).cuda()
    o = _check_forward(capsys, case, xyz, dirs, _device_volume(case.rows, dims), case.M, f, case.label)["both"]
    inputs = _device_inputs(case)
    inputs.update(h0_raw=o["h0_raw"].clone(), rgb=o["rgb"].clone())
    G = R.backward(case.C, dims, deg, case.clip, idx=case.idx, dirs=case.dirs, h0_raw=h0, rgb=f["rgb"].y, b_h0=b, b_rgb=f["rgb"].b, **case.grads)
    _check_backward(capsys, case, xyz, dirs, case.M, ALL, inputs, G, case.label)


# ---------------------------------------------------------------------------------------------- run lengths
@pytest.mark.parametrize("M", [1, 15, 16, 17, 31, 32, 33, 63, 64, 65])
def test_run_lengths_around_every_chunk_length(M, capsys):
    """an empty second half-wave (M <= 16) and the last stream ending on, before and behind a chunk boundary"""
    case = R.walk_case((9, 7, 5), "unit", 3)
    start = 150  # (a stretch of the walk that is inside the volume)
    sub = R.Case("M=%d %s" % (M, case.label), case.xyz[start:start + M], case.dims, case.aabb, case.degree, case.clip, case.rows)
    assert (R.footprint_position(sub.C.i0.numpy(), sub.dims) < 2).any()
    xyz, dirs = torch.from_numpy(sub.xyz).cuda(), torch.from_numpy(sub.dirs).cuda()
    _check_forward(capsys, sub, xyz, dirs, _device_volume(sub.rows, sub.dims), M, sub.fwd, sub.label)
    inputs = _device_inputs(sub)
    for names in (("g_feat",), ALL):
        _check_backward(capsys, sub, xyz, dirs, M, names, inputs, sub.bwd(names), sub.label)


@functools.lru_cache(maxsize=1)
def _tiled():
    """the walk on (9, 7, 5) tiled to the largest threshold, its float64 head and the additive parts of its gradient by segment"""
    base = R.walk_case((9, 7, 5), "asym", 3)
    case = R.Case("tiled " + base.label, R.tile_case(base, max(THRESHOLDS)), base.dims, base.aabb, base.degree, base.clip, base.rows)
    h0, rgb = case.forced()
    names = ("g_sigma", "g_sigma_l", "g_rgb")
    g, ga, ge = R.sample_gradient(case.degree, case.clip, dirs=case.dirs, h0_raw=h0, rgb=rgb, **{nm: case.grads[nm] for nm in names})
    parts, total, at = {}, None, 0
    for M in THRESHOLDS:
        rows = slice(at, M)
        seg = R.scatter(v.take(case.C, rows), case.dims, g[rows], ga[rows], ge[rows], case.idx)
        total = seg if total is None else R.add_parts(total, seg)
        parts[M], at = total, M
    return case, names, parts


@pytest.mark.parametrize("M", THRESHOLDS)
def test_either_side_of_each_chunk_threshold_head_only(M, capsys):
    """px_chunk picks 16, 32, 32, 64 here.  Head only, no feature output; the reference is one vectorised float64 pass over the
    262 176 rows, shared by the four cases (the gradient is additive over rows).  With thousands of contributions per voxel the
    gradient's bound is a few 1e-3 of an element: what this case sees in the backward is a stream that is not run at all or run
    twice; single flushes are the business of the short cases."""
    case, names, parts = _tiled()
    assert R.px_chunk(M) == {131087: 16, 131088: 32, 262175: 32, 262176: 64}[M]
    xyz, dirs = torch.from_numpy(case.xyz[:M]).cuda(), torch.from_numpy(case.dirs[:M]).cuda()
    o = _forward(case, xyz, dirs, _device_volume(case.rows, case.dims), "head")
    line, worst = R.report("hip fwd head M=%d %s" % (M, case.label), HEAD_NAMES, [o[nm] for nm in HEAD_NAMES],
                           [R.Val(case.fwd[nm].y[:M], case.fwd[nm].b[:M]) for nm in HEAD_NAMES])
    _say(capsys, line)
    assert worst <= 1.0, line
    _check_backward(capsys, case, xyz, dirs, M, names, _device_inputs(case, M), R.grad_of(parts[M], case.dims), "M=%d %s" % (M, case.label))


# ---------------------------------------------------------------------------------------------- offset paths
@pytest.mark.parametrize("dims", [(255, 256, 256), (256, 256, 256)], ids=["24-bit", "64-bit"])
def test_offset_forms_on_the_largest_small_and_the_smallest_large_volume(dims, capsys):
    """degree 1 (C = 4): 256 MiB per buffer.  The volume is filled on the device from a seeded generator and only the touched voxels
    are read back for the reference; the gradient is compared on the touched voxels and the rest must be exactly zero."""
    deg, C = 1, 4
    assert R.is_small(dims, C) == (dims[0] == 255)
    V = int(np.prod(dims))
    flat = torch.empty(V * C, device="cuda").normal_(generator=torch.Generator(device="cuda").manual_seed(R.VOLUME_SEED)) * 3.0
    rows_dev = flat.view(V, C)
    case = R.corner_case(dims, "unit", deg, rows=lambda idx: rows_dev[torch.as_tensor(idx).cuda()].cpu().numpy())
    assert int(case.idx[0]) == 0 and int(case.idx[-1]) == V - 1
    xyz, dirs = torch.from_numpy(case.xyz).cuda(), torch.from_numpy(case.dirs).cuda()
    _check_forward(capsys, case, xyz, dirs, _as_param(flat, dims, C), case.M, case.fwd, case.label)
    G = case.bwd(ALL)
    buf, grad, pad = _grad_buffer(dims, C)
    _backward(case, xyz, dirs, ALL, _device_inputs(case), grad)
    assert _margins(buf, V * C, pad, GRAD_SENTINEL)
    rows = buf[pad:pad + V * C].view(V, C)
    touched = case.idx.cuda()
    line, worst = R.report("hip bwd feat+sigma+sigma_l+rgb %s" % case.label, ["g_volume"], [rows[touched]], [R.Val(G.y, G.b)])
    _say(capsys, line)
    assert worst <= 1.0, line
    rows[touched] = 0.0
    assert not bool(rows.any()), "a gradient outside the touched voxels"


# ---------------------------------------------------------------------------------------------- error returns
def test_no_rows_returns_without_touching_a_poisoned_buffer():
    import pvd_hip
    case = R.walk_case((9, 7, 5), "unit", 3)
    C = R.channels(case.degree)
    xyz, dirs = torch.empty(0, 3, device="cuda"), torch.empty(0, 3, device="cuda")
    vol = _device_volume(case.rows, case.dims)
    o = _forward(case, xyz, dirs, vol, "both")  # (checks the margins; the views are empty)
    assert all(t.numel() == 0 for t in o.values())
    poison = {nm: torch.full(s, NAN, device="cuda") for nm, s in [("feat", (4, C)), ("h0_raw", (4,)), ("sigma_l", (4,)), ("sigma", (4,)), ("rgb", (4, 3))]}
    pvd_hip.plenoxel_forward(xyz, dirs, list(case.aabb), vol, case.degree, -2.0, 7.0, *[poison[nm] for nm in FWD_NAMES])
    assert all(bool(torch.isnan(t).all()) for t in poison.values())
    buf, grad, pad = _grad_buffer(case.dims, C, torch.full((int(np.prod(case.dims)), C), 0.5))
    before = buf.clone()
    pvd_hip.plenoxel_backward(xyz, dirs, list(case.aabb), case.degree, -2.0, 7.0, poison["h0_raw"], poison["rgb"], poison["feat"],
                              poison["sigma"], poison["sigma_l"], poison["rgb"], grad)
    pvd_hip.plenoxel_backward(xyz, None, list(case.aabb), case.degree, -2.0, 7.0, None, None, poison["feat"], None, None, None, grad)
    assert torch.equal(_bits(buf), _bits(before))
