"""tests/plenoxel_ref64.py earns its place before it judges a kernel (CPU only): the float64 restatement equals float64 grid_sample,
float64 autograd of the torch formulation and central finite differences; its SH polynomials equal scipy's and the spot values
tests/test_oracle_pins.py pins; torch's float32 grid_sample formulation and a float32 restatement of the kernels' own order (window
walk included) stay inside the derived bound on every scripted case (the bound is not vacuous); injected faults of that restatement
leave the bound or break an exact part (the bound has teeth); the committed seeds reach every reachable move class at every chunk
length, tiled to the thresholds of the chunk choice too.

Every bound test prints one line of max(err / bound) (pytest -s); profiles/plenoxel_fp64_pin.txt keeps one run."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import plenoxel_ref64 as R
import vm_ref64 as v

WALKS = [((9, 7, 5), 3), ((33, 17, 65), 3), ((1, 2, 5), 3), ((20, 24, 28), 2), ((9, 7, 5), 1)]
CASES = [(dims, deg, box) for dims, deg in WALKS for box in ("unit", "asym")] + [((9, 17, 33), 3, "lattice")]
FWD_NAMES = ["feat", "h0_raw", "sigma_l", "sigma", "rgb"]
ALL = ("g_feat", "g_sigma", "g_sigma_l", "g_rgb")
THRESHOLDS = [131087, 131088, 262175, 262176]


def _case(dims, deg, box, clip="narrow"):
    return R.lattice(dims, deg) if box == "lattice" else R.walk_case(dims, box, deg, clip)


def _say(capsys, line):
    with capsys.disabled():
        print("\n" + line, end="")


# ---------------------------------------------------------------------------------------------- anchors
def _torch_formulation(case, xn, rows, dtype, dirs, weights):
    """the "tensors" branch in torch on the CPU: grid_sample, clamp, trunc_exp, SH product, sigmoid -> outputs, volume gradient"""
    from pvd.activation import make_trunc_exp
    K2 = case.degree ** 2
    vol = R.logical(rows.to(dtype), case.dims).requires_grad_(True)
    x = torch.as_tensor(np.asarray(xn)).to(dtype)
    h = F.grid_sample(vol, x.view(1, 1, -1, 1, 3), mode="bilinear", padding_mode="zeros", align_corners=True).view(vol.shape[1], -1).T
    sigma_l = torch.clamp(h[:, 0], case.clip[0], case.clip[1])
    sigma = make_trunc_exp("cpu")(sigma_l)
    enc = torch.from_numpy(R.sh_basis(dirs, case.degree)[0]).to(dtype)
    rgb = torch.sigmoid((h[:, 1:].view(-1, 3, K2) * enc.unsqueeze(1)).sum(-1))
    out = {"feat": h, "h0_raw": h[:, 0], "sigma_l": sigma_l, "sigma": sigma, "rgb": rgb}
    loss = sum((out[nm] * w.to(dtype)).sum() for nm, w in weights.items())
    (g,) = torch.autograd.grad(loss, vol)
    return {k: t.detach() for k, t in out.items()}, g.detach()[0].permute(1, 2, 3, 0).reshape(-1, vol.shape[1])


WEIGHT_OF = {"g_feat": "feat", "g_sigma": "sigma", "g_sigma_l": "sigma_l", "g_rgb": "rgb"}


@pytest.mark.parametrize("dims,deg", [((20, 24, 28), 2), ((1, 2, 5), 3), ((5, 3, 2), 3), ((9, 7, 5), 1)])
@pytest.mark.parametrize("clip", ["narrow", "wide"])
def test_reference_equals_float64_grid_sample_and_autograd_of_the_torch_formulation(dims, deg, clip):
    """the same float32-derived x_n into both, positions and everything after in float64: features, head and the volume gradient of
    every gradient input within 1e-12 of the element's magnitude form (an element nothing contributes to is exactly 0)"""
    case = R.walk_case(dims, "asym", deg, clip)
    rng = np.random.default_rng(1)
    xn = np.concatenate([v.normalise32(case.xyz, case.aabb), rng.uniform(-1.4, 1.4, (1500, 3)).astype(np.float32),
                         np.array([[1, 1, 1], [-1, -1, -1], [0, 0, 0], [1, -1, 0.5]], np.float32)])
    M = xn.shape[0]
    dirs = R.make_dirs(M, 2)
    C = v.coords_from_xn(xn, R.res_of(dims), np.float64)
    f = R.forward(C, dims, case.vol, deg, dirs, case.clip)
    g = {k: t.double() for k, t in R.make_grads(M, deg, 2).items()}
    for names in [ALL, ("g_feat",), ("g_sigma",), ("g_rgb", "g_sigma_l")]:
        want, gvol = _torch_formulation(case, xn, case.rows, torch.float64, dirs, {WEIGHT_OF[nm]: g[nm] for nm in names})
        for nm in FWD_NAMES:
            scale = f[nm].b / R.EPS32  # (a magnitude form of the element, up to the factor K)
            assert ((f[nm].y - want[nm]).abs() <= 1e-12 * scale).all(), nm
        b = R.backward(C, dims, deg, case.clip, idx=case.idx, dirs=dirs, h0_raw=f["h0_raw"].y, rgb=f["rgb"].y, **{nm: g[nm] for nm in names})
        assert ((b.y - gvol).abs() <= 1e-12 * b.b / R.EPS32).all(), names
        assert (gvol[b.b == 0] == 0).all() and (b.b > 0).any()
    assert (f["feat"].y.abs().amax(1) == 0).any() and ((f["h0_raw"].y < case.clip[0]) | (f["h0_raw"].y > case.clip[1])).any()


def test_sh_polynomials_against_scipy_and_the_pinned_spot_values():
    from scipy.special import sph_harm_y
    rng = np.random.RandomState(9)
    d = rng.randn(200, 3)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    Y, Ym = R.sh_basis(d, 3)
    theta, phi = np.arccos(np.clip(d[:, 2], -1, 1)), np.arctan2(d[:, 1], d[:, 0])
    for l in range(3):
        for m in range(-l, l + 1):
            S = sph_harm_y(l, abs(m), theta, phi)
            ref = S.real if m == 0 else (np.sqrt(2) * (S.real if m > 0 else S.imag))
            np.testing.assert_allclose(Y[:, l * l + l + m], ref, atol=1e-13)
    assert (Ym * (1 + 1e-15) >= np.abs(Y)).all()
    for deg in (1, 2):
        assert np.array_equal(R.sh_basis(d, deg)[0], Y[:, :deg * deg])
    # the spot values of tests/test_oracle_pins.py (non-unit inputs see the polynomials, r = 1 baked in)
    z = R.sh_basis(np.zeros((1, 3)), 3)[0][0]
    assert abs(z[0] - 0.28209479177387814) < 1e-15 and abs(z[6] + 0.31539156525251999) < 1e-15 and np.all(z[[1, 2, 3, 4, 5, 7, 8]] == 0)
    x, y, zz = 0.3, -0.2, 0.5
    p = R.sh_basis(np.array([[x, y, zz]]), 3)[0][0]
    assert abs(p[1] - (-0.48860251190291987 * y)) < 1e-15 and abs(p[3] - (-0.48860251190291987 * x)) < 1e-15
    assert abs(p[8] - 0.54627421529603959 * (x * x - y * y)) < 1e-15
    # ... and the float32 evaluation in the kernel's order stays within the allowance on the terms' magnitudes
    d32 = R.make_dirs(500, 3)
    Y, Ym = R.sh_basis(d32, 3)
    assert (np.abs(R.sh32(d32, 3).astype(np.float64) - Y) <= R.EPS32 * R.SH_ROUNDINGS * Ym).all()


def test_volume_gradient_against_central_finite_differences():
    dims, deg, clip = (3, 4, 5), 2, (-2.0, 7.0)
    rng = np.random.default_rng(4)
    M = 48
    xn = rng.uniform(-1.2, 1.2, (M, 3)).astype(np.float32)
    dirs = R.make_dirs(M, 5)
    rows = R.make_volume(dims, deg, 6, scale0=3.0).double()
    C = v.coords_from_xn(xn, R.res_of(dims), np.float64)
    g = {k: t.double() for k, t in R.make_grads(M, deg, 7).items()}

    def loss(r):
        f = R.forward(C, dims, R.DenseVol(r), deg, dirs, clip)
        return float((f["feat"].y * g["g_feat"]).sum() + (f["sigma"].y * g["g_sigma"]).sum() + (f["sigma_l"].y * g["g_sigma_l"]).sum()
                     + (f["rgb"].y * g["g_rgb"]).sum())

    f = R.forward(C, dims, R.DenseVol(rows), deg, dirs, clip)
    h0 = f["h0_raw"].y
    assert min((h0 - clip[0]).abs().min(), (h0 - clip[1]).abs().min()) > 1e-3 and (h0 < clip[0]).any()  # no kink inside a difference
    b = R.backward(C, dims, deg, clip, idx=torch.arange(rows.shape[0]), dirs=dirs, h0_raw=h0, rgb=f["rgb"].y, **g)
    eps, checked = 1e-6, 0
    for j in rng.choice(rows.numel(), 60, replace=False):
        vx, ch = divmod(int(j), rows.shape[1])
        up, dn = rows.clone(), rows.clone()
        up[vx, ch] += eps
        dn[vx, ch] -= eps
        fd = (loss(up) - loss(dn)) / (2 * eps)
        assert abs(fd - float(b.y[vx, ch])) <= 1e-6 * (1.0 + abs(fd)), (vx, ch, fd, float(b.y[vx, ch]))
        checked += b.y[vx, ch] != 0
    assert checked >= 30


# ---------------------------------------------------------------------------------------------- the bound is not vacuous
def _bwd_line(label, got_rows, G):
    return R.report(label, ["g_volume"], [got_rows], [R.Val(G.y, G.b)])


@pytest.mark.parametrize("dims,deg,box", CASES)
def test_float32_grid_sample_formulation_stays_inside_the_bound(dims, deg, box, capsys):
    case = _case(dims, deg, box)
    assert case.M <= 4608
    h0, rgb = case.forced()
    want, gvol = _torch_formulation(case, v.normalise32(case.xyz, case.aabb), case.rows, torch.float32, case.dirs,
                                    {WEIGHT_OF[nm]: case.grads[nm] for nm in ALL})
    l1, w1 = R.report("cpu-f32 fwd " + case.label, FWD_NAMES, [want[nm] for nm in FWD_NAMES], [case.fwd[nm] for nm in FWD_NAMES])
    # (autograd is not teacher-forced: its h0 and rgb are its own float32 values, inside their bounds)
    G = R.backward(case.C, case.dims, deg, case.clip, idx=case.idx, dirs=case.dirs, h0_raw=want["h0_raw"], rgb=want["rgb"], **case.grads)
    l2, w2 = _bwd_line("cpu-f32 bwd " + case.label, gvol, G)
    _say(capsys, l1 + "\n" + l2)
    assert max(w1, w2) <= 1.0, (l1, l2)


def _model(case, chunk, M=None, fault=None, fault_stream=None, head=True):
    M = case.M if M is None else M
    return R.Model32(case.xyz[:M], case.aabb, case.dims, case.degree, case.clip, case.rows32, case.dirs[:M] if head else None, chunk, fault, fault_stream)


def _reference(case, M, names, prefill=None):
    """forward Vals of the first M rows and the Grad of them for the gradient inputs `names`"""
    fwd = {nm: R.Val(case.fwd[nm].y[:M], case.fwd[nm].b[:M]) for nm in FWD_NAMES}
    head = any(nm != "g_feat" for nm in names)
    h0, rgb = case.forced()
    kw = {nm: case.grads[nm][:M] for nm in names}
    if head:
        kw.update(dirs=case.dirs[:M], h0_raw=h0[:M], rgb=rgb[:M])
    return fwd, R.backward(v.take(case.C, slice(0, M)), case.dims, case.degree, case.clip, idx=case.idx, prefill=prefill, **kw), kw


def _run(case, chunk, names=ALL, M=None, fault=None, fault_stream=None, prefill=None):
    """model32 forward and backward of the first M rows -> (worst forward ratio, backward ratio, stray voxels)"""
    M = case.M if M is None else M
    fwd, G, kw = _reference(case, M, names, None if prefill is None else torch.from_numpy(prefill(case.idx.numpy())))
    head = "dirs" in kw
    m = _model(case, chunk, M, fault, fault_stream, head)
    o = m.forward()
    rf = max(R.ratio(o[nm], fwd[nm]) for nm in (FWD_NAMES if head else ["feat"]))
    kw.pop("dirs", None)
    sparse = m.backward(prefill=None if prefill is None else (lambda vx: prefill(np.array([vx]))[0]), **{k: np.asarray(t) for k, t in kw.items()})
    got, stray = R.grad_rows(sparse, case.idx.numpy(), m.Cn)
    if prefill is not None:  # voxels no flush reached keep what they held
        untouched = np.array([int(vx) not in sparse for vx in case.idx.tolist()])
        got[untouched] = prefill(case.idx.numpy())[untouched]
    return rf, R.ratio(got, R.Val(G.y, G.b)), stray


@pytest.mark.parametrize("dims,deg,box", CASES)
def test_float32_restatement_of_the_kernels_order_stays_inside_the_bound(dims, deg, box, capsys):
    case = _case(dims, deg, box)
    chunk = R.CHUNKS[(case.M + deg) % 3]
    rf, rb, stray = _run(case, chunk)
    rf2, rb2, stray2 = _run(case, chunk, ("g_feat",), M=case.M - 7)
    _say(capsys, "[plenoxel fp64] model32 %-50s max err/bound: fwd=%.3g bwd(all)=%.3g | features only: fwd=%.3g bwd=%.3g" % (
        case.label + " chunk %d" % chunk, rf, rb, rf2, rb2))
    assert max(rf, rb, rf2, rb2) <= 1.0 and not stray and not stray2


def test_float32_restatement_on_wide_clips_prefilled_buffers_corners_and_both_offset_paths(capsys):
    wide = R.walk_case((9, 7, 5), "unit", 3, "wide")
    h0 = wide.fwd["h0_raw"].y
    assert ((h0.abs() > 12) & (h0.abs() < 15)).sum() >= 20 and (h0.abs() > 15).sum() >= 5
    pre = lambda idx: R.hashed_rows(idx, wide.vol.rows.shape[1], 77)
    lines = []
    for label, case, kw in [("wide", wide, {}), ("wide prefilled", wide, {"prefill": pre}), ("corner small", R.corner_case((255, 256, 256)), {}),
                            ("corner 64-bit", R.corner_case((256, 256, 256)), {})]:
        rf, rb, stray = _run(case, 16, **kw)
        lines.append("[plenoxel fp64] model32 %-50s max err/bound: fwd=%.3g bwd(all)=%.3g" % (label + " " + case.label, rf, rb))
        assert max(rf, rb) <= 1.0 and not stray, lines[-1]
    _say(capsys, "\n".join(lines))
    assert R.is_small((255, 256, 256), 4) and not R.is_small((256, 256, 256), 4)
    big = R.corner_case((256, 256, 256))
    assert int(big.idx.max()) == 256 ** 3 - 1 and int(big.idx.min()) == 0


# ---------------------------------------------------------------------------------------------- the bound has teeth
def _stream_ending_inside(case, chunk, M):
    """a stream (not the last) whose last sample's footprint is inside the volume"""
    pos = R.footprint_position(case.C.i0.numpy()[:M], case.dims)
    ends = [j for j in range((M - 1) // chunk) if pos[(j + 1) * chunk - 1] == 0]
    return ends[len(ends) // 2]


def _rows_ending_inside(case):
    pos = R.footprint_position(case.C.i0.numpy(), case.dims)
    return int(np.nonzero(pos == 0)[0][-1]) + 1


FAULT_CASES = {  # fault -> (case, gradient inputs, what must leave the bound: "fwd", "bwd" or both)
    "lost_flush_chunk": ("walk", ALL, "bwd"), "lost_flush_M": ("walk", ALL, "bwd"),
    "rename+x": ("walk", ALL, "fwd bwd"), "rename-x": ("walk", ALL, "fwd bwd"), "rename+y": ("walk", ALL, "fwd bwd"),
    "rename-y": ("walk", ALL, "fwd bwd"), "rename+z": ("walk", ALL, "fwd bwd"), "rename-z": ("walk", ALL, "fwd bwd"),
    "leave_at_new": ("walk", ALL, "bwd"), "clamp_tap": ("walk", ALL, "fwd bwd"), "mask_lt": ("lattice", ("g_sigma_l",), "bwd"),
    "no_exp_clamp": ("wide", ("g_sigma",), "bwd"), "tree_drops_last": ("walk", ALL, "fwd"), "wrong_colour": ("walk", ("g_rgb",), "bwd"),
    "gfeat_ignored": ("walk", ALL, "bwd"), "offset_mod24": ("big", ALL, "fwd bwd"),
}


@pytest.mark.parametrize("fault", R.FAULTS)
def test_injected_faults_leave_the_bound_or_break_an_exact_part(fault, capsys):
    assert set(FAULT_CASES) == set(R.FAULTS)
    which, names, must = FAULT_CASES[fault]
    case = {"walk": lambda: R.walk_case((9, 7, 5), "unit", 3), "lattice": lambda: R.lattice(), "wide": lambda: R.walk_case((9, 7, 5), "unit", 3, "wide"),
            "big": lambda: R.corner_case((256, 256, 256))}[which]()
    for chunk in ((16,) if which in ("big", "lattice") else R.CHUNKS):
        M = _rows_ending_inside(case) if fault == "lost_flush_M" else case.M
        stream = _stream_ending_inside(case, chunk, M) if fault == "lost_flush_chunk" else None
        clean = _run(case, chunk, names, M)
        assert max(clean[:2]) <= 1.0 and not clean[2]
        rf, rb, stray = _run(case, chunk, names, M, fault, stream)
        _say(capsys, "[plenoxel fp64] fault %-18s chunk %d on %-34s fwd x %.3g, bwd x %.3g, %d stray voxels" % (fault, chunk, case.label, rf, rb, len(stray)))
        if "fwd" in must:
            assert rf > 1.0, (fault, chunk, rf)
        if "bwd" in must:
            assert rb > 1.0 or stray, (fault, chunk, rb)
        if must == "bwd":
            assert rf <= 1.0  # (a backward fault: the forward is untouched)
    if fault == "tree_drops_last":  # ... at degree 2 as well (K2 = 4: two levels)
        c2 = R.walk_case((20, 24, 28), "unit", 2)
        assert _run(c2, 32, ALL, 600, fault)[0] > 1.0


# ---------------------------------------------------------------------------------------------- coverage
@pytest.mark.parametrize("dims,deg", WALKS[:4])
@pytest.mark.parametrize("box", ["unit", "asym"])
def test_scripted_walks_reach_every_class_under_every_chunk_length(dims, deg, box):
    case = R.walk_case(dims, box, deg)
    i0 = case.C.i0.numpy()
    R.assert_coverage(i0, dims)
    res = R.res_of(dims)
    tiled = R.coords(R.tile_case(case, max(THRESHOLDS)), case.aabb, dims).i0.numpy()
    for M in THRESHOLDS:  # the tilings of the GPU file's threshold test keep it
        R.assert_coverage(tiled[:M], dims)
    multi = [a for a in range(3) if res[a] > 1]
    for a in multi:  # each face is crossed out and back by single voxels
        assert {-2, -1, 0, res[a] - 2, res[a] - 1, res[a]} <= set(int(x) for x in i0[:, a])
    xn = v.normalise32(case.xyz, case.aabb)
    assert np.isfinite(case.xyz).all() and 20 < np.abs(xn).max() <= 110  # far outside: the rays start within +-50 extents and walk on
    f64 = v.coords_from_xn(xn, res, np.float64).i0.numpy()
    assert (f64[:, multi] == i0[:, multi]).all()  # float32 and float64 agree on i0
    r = R.reachable(dims)
    assert r.all() == (min(dims) >= 2)


def test_reachable_and_bookkeeping_on_a_hand_made_sequence():
    dims = (5, 5, 5)
    i0 = np.array([[1, 1, 1], [2, 1, 1], [2, 1, 1], [2, 0, 1], [2, 0, 3], [3, 0, 3], [4, 0, 3], [3, 1, 3], [3, 1, 2], [3, 1, 9], [3, 1, 8], [3, 1, 8]])
    mc = R.move_classes(i0, dims, 4)
    assert [R.CLASSES[c] for c in mc["class"]] == ["open", "+x", "same", "-y", "open", "+x", "+x", "jump", "open", "jump", "-z", "same"]
    assert [R.POSITIONS[p] for p in mc["position"]] == ["inside"] * 6 + ["partly", "inside", "inside", "outside", "outside", "outside"]
    assert mc["left"].tolist() == [-1, 0, 0, 0, -1, 0, 0, 1, -1, 0, 2, 2]
    r = R.reachable((1, 2, 5))  # z has the single position 0, its second tap outside
    assert not r[:, 0].any() and r[0, 1] and r[1, 2] and r[2, 1] and r[4, 2] and not r[6].any() and not r[7].any() and r[8, 1:].all()
    assert R.reachable((1, 1, 1)).tolist() == [[False, True, False]] * 2 + [[False] * 3] * 7
    assert [R.px_chunk(M) for M in THRESHOLDS] == [16, 32, 32, 64] and R.px_chunk(1) == 16


def test_lattice_points_are_exact_and_meet_the_clip_values_and_their_neighbours():
    case = R.lattice()
    lo, hi = (np.float32(c) for c in case.clip)
    h0 = case.fwd["h0_raw"].y.numpy()
    centre = (case.C.w1.numpy() == 0).all(1) & (R.footprint_position(case.C.i0.numpy(), case.dims) < 2)
    assert centre.sum() >= 100
    for val in case.meta["special_h0"]:  # clip_min, clip_max and one float32 ulp either side of each, met exactly
        assert (h0[centre] == np.float64(val)).sum() >= 2, val
    assert (case.fwd["feat"].b[torch.from_numpy(centre)] > 0).any()  # (the bound there is the element's own: a few eps32)
    sl = case.fwd["sigma_l"].y.numpy()
    assert ((sl == np.float64(lo)) & (h0 < np.float64(lo))).any() and ((sl == np.float64(hi)) & (h0 > np.float64(hi))).any()
    for a, s in enumerate(R.res_of(case.dims)):
        for e in case.meta["special"][a]:
            assert (case.xyz[:, a] == e).sum() >= 2


def test_corner_points_reach_the_last_and_the_first_voxel():
    for dims in [(9, 7, 5), (255, 256, 256), (256, 256, 256)]:
        xyz = R.corner_points(dims, v.UNIT_AABB)
        C = R.coords(xyz, v.UNIT_AABB, dims)
        idx = R.touched(C, dims)
        assert int(idx[0]) == 0 and int(idx[-1]) == int(np.prod(dims)) - 1
        tp = R.taps(C, dims)
        assert all(((i == int(np.prod(dims)) - 1) & ok).any() for i, ok, _, _ in tp)  # the last voxel as every tap of the footprint
