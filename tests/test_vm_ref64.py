"""tests/vm_ref64.py earns its place before it judges a kernel (CPU only): the float64 restatement equals float64 grid_sample and its
autograd; the oracle's and torch's own float32 formulations stay inside the derived bound (the bound is not vacuous); modelled
faults of the kernel's window walk -- a lost flush, a flush to the neighbouring texel, swapped weights, a dropped tap at i0 = -1, a
zeroed last sample of a chunk -- are all flagged (the bound has teeth); the committed generator seeds reach every branch.

Every bound test prints one line of max(err / bound) per output tensor (pytest -s); profiles/vm_fp64_pin.txt keeps one run."""
import numpy as np
import pytest
import torch

import vm_ref64 as v

SIZES = [(9, 17, 33), (24, 31, 45), (1, 2, 5)]
WALKS = [(res, box) for res in SIZES for box in ("unit", "asym")]
FWD_NAMES = ["sigma_feat", "color_prod"]


def _leaves(tables, dtype):
    return [t.to(dtype).clone().requires_grad_(True) for t in tables]


def _formulation(case, dtype, xn=None):
    """grid_sample forward + autograd backward of a case in `dtype` on the CPU -> (sigma, prod, [12 grads])"""
    tabs = _leaves(case.tables, dtype)
    xn = v.normalise32(case.xyz, case.aabb) if xn is None else xn
    sig, prod = v.grid_sample_formulation(xn, tabs, dtype)
    gs, gp = case.grads()
    grads = torch.autograd.grad((sig * gs.to(dtype)).sum() + (prod * gp.to(dtype)).sum(), tabs)
    return sig.detach(), prod.detach(), [g.detach() for g in grads]


@pytest.mark.parametrize("res", [(24, 31, 45), (1, 2, 5), (5, 3, 2)])
def test_reference_equals_float64_grid_sample_forward_and_autograd(res):
    """same float32-derived x_n into both, positions and everything after in float64: every element within 1e-12 of its own
    magnitude form y_abs (an element nothing contributes to is exactly 0)"""
    case = v.walk_case(res, "asym")
    rng = np.random.default_rng(1)
    xn = np.concatenate([v.normalise32(case.xyz, case.aabb), rng.uniform(-1.4, 1.4, (1500, 3)).astype(np.float32),
                         np.array([[1, 1, 1], [-1, -1, -1], [0, 0, 0], [1, -1, 0.5]], np.float32)])
    M = xn.shape[0]
    C = v.coords_from_xn(xn, res, np.float64)
    g = torch.Generator().manual_seed(2)
    gs, gp = torch.randn(M, generator=g, dtype=torch.float64), torch.randn(M, 144, generator=g, dtype=torch.float64)
    tabs = _leaves(case.tables, torch.float64)
    sig, prod = v.grid_sample_formulation(xn, tabs, torch.float64)
    grads = torch.autograd.grad((sig * gs).sum() + (prod * gp).sum(), tabs)
    f = v.forward(C, case.tables, res)
    b = v.backward(C, case.tables, res, gs, gp)
    assert (prod.abs().max(1).values == 0).any() and prod.abs().max() > 0.5  # points outside and inside
    for name, o, want in [("sigma_feat", f["sigma_feat"], sig), ("color_prod", f["color_prod"], prod)] + \
                         [(nm, o, gr) for nm, o, gr in zip(v.TABLE_NAMES, b, grads)]:
        want = want.detach()
        assert o.y.shape == want.shape, name
        assert ((o.y - want).abs() <= 1e-12 * o.y_abs).all(), (name, ((o.y - want).abs() / o.y_abs.clamp_min(1e-300)).max().item())


def test_magnitude_forms_dominate_and_counts_add_up():
    case = v.walk_case((24, 31, 45), "unit")
    for o in list(case.fwd.values()) + case.bwd():
        assert (o.y.abs() <= o.y_abs * (1 + 1e-12)).all() and (o.y_w >= 0).all()
    # every in-range tap of every sample is counted exactly once
    C, res = case.C, case.res
    for i in range(3):
        taps = sum(int(valid.sum()) for _, valid, _, _ in v._plane_taps(C, i, res))
        assert int(case.bwd()[i].n.sum()) == taps == int(case.bwd()[6 + i].n.sum())


@pytest.mark.parametrize("box", ["unit", "asym"])
def test_oracle_vm_forward_is_inside_the_bound(box, capsys):
    import oracle
    for res in SIZES:
        case = v.walk_case(res, box)
        sig, prod = oracle.vm_forward(case.xyz, case.aabb, [t.numpy() for t in case.tables], res)
        line, worst = v.report("oracle fwd " + case.label, FWD_NAMES, [torch.from_numpy(sig), torch.from_numpy(prod)],
                               [case.fwd["sigma_feat"], case.fwd["color_prod"]], case.S)
        with capsys.disabled():
            print("\n" + line, end="")
        assert worst <= 1.0, line


def _cpu_f32_lines(case):
    sig, prod, grads = _formulation(case, torch.float32)
    l1, w1 = v.report("cpu-f32 fwd " + case.label, FWD_NAMES, [sig, prod], [case.fwd["sigma_feat"], case.fwd["color_prod"]], case.S)
    l2, w2 = v.report("cpu-f32 bwd " + case.label, v.TABLE_NAMES, grads, case.bwd(), case.S)
    return [l1, l2], max(w1, w2)


@pytest.mark.parametrize("res,box", WALKS + [((9, 17, 33), "lattice")])
def test_float32_grid_sample_stays_inside_the_bound(res, box, capsys):
    """The bound is not vacuous: torch's own float32 formulation on the CPU, forward and autograd backward, meets it on every
    scripted case (M <= 4096)."""
    case = v.lattice(res) if box == "lattice" else v.walk_case(res, box)
    assert case.M <= 4096
    lines, worst = _cpu_f32_lines(case)
    with capsys.disabled():
        print("\n" + "\n".join(lines), end="")
    assert worst <= 1.0, lines


# ---------------------------------------------------------------------------------------------- the bound has teeth
def _worst(gots, outs, S):
    return max(v.ratio(g, o, S) for g, o in zip(gots, outs))


def _run_backward(case, rows):
    gs, gp = case.grads()
    return v.backward(v.take(case.C, rows), case.tables, case.res, gs[rows], gp[rows])


def _border_mask(H, W):
    m = torch.zeros(H, W, dtype=torch.bool)
    m[0], m[-1], m[:, 0], m[:, -1] = True, True, True, True
    return m


def _lost_flush_event(case, i, chunk=16):
    """(table index, run contribution [1,R,H,W], y, x) of the first run that reaches a border texel of colour plane i"""
    t = 6 + i
    H, W = case.tables[t].shape[2:]
    border = _border_mask(H, W)
    for r in range(case.M // chunk):
        rows = torch.arange(r * chunk, (r + 1) * chunk)
        contrib = _run_backward(case, rows)[t]
        hit = (contrib.n[0, 0] > 0) & border & (contrib.y.abs().amax((0, 1)) > 0)
        if hit.any():
            y, x = [int(c) for c in hit.nonzero()[0]]
            return t, contrib.y, y, x
    return None


@pytest.mark.parametrize("res,box", WALKS)
def test_modelled_faults_of_the_walk_are_flagged(res, box):
    case = v.walk_case(res, box)
    ref_b, S = case.bwd(), case.S
    ys = [o.y for o in ref_b]
    assert _worst(ys, ref_b, S) == 0.0
    events = 0
    # a lost flush: one run's contributions to one border texel are dropped ... or land on the neighbouring texel
    for i in range(3):
        ev = _lost_flush_event(case, i)
        if ev is None:
            continue
        events += 1
        t, contrib, y, x = ev
        H, W = contrib.shape[2:]
        lost = [a.clone() for a in ys]
        lost[t][0, :, y, x] -= contrib[0, :, y, x]
        assert v.ratio(lost[t], ref_b[t], S) > 1.0, ("lost flush", i, y, x)
        ny, nx = (y, x + 1 if x + 1 < W else x - 1) if W > 1 else (y + 1 if y + 1 < H else y - 1, x)
        moved = [a.clone() for a in lost]
        moved[t][0, :, ny, nx] += contrib[0, :, y, x]
        assert v.ratio(moved[t], ref_b[t], S) > 1.0, ("misplaced flush", i, y, x)
        assert abs(float(moved[t].sum() - ys[t].sum())) < 1e-9 * float(ref_b[t].y_abs.sum())  # (conservation alone would not see it)
    assert events == 3
    i0 = case.C.i0
    size = torch.tensor(res)
    inside = (i0 >= 0) & (i0 + 1 < size)
    seen = (i0 + 1 >= 0) & (i0 < size)  # at least one tap of the axis in range
    gs, gp = case.grads()

    def with_coords(C2):
        f = v.forward(C2, case.tables, res)
        b = v.backward(C2, case.tables, res, gs, gp)
        return _worst([f["sigma_feat"].y, f["color_prod"].y], [case.fwd["sigma_feat"], case.fwd["color_prod"]], S), _worst([o.y for o in b], ref_b, S)

    # w0 / w1 swapped for one sample on one axis
    for a in range(3):
        if res[a] < 2:
            continue
        m = int((seen.all(1) & inside[:, a]).nonzero()[0])
        w0, w1 = case.C.w0.clone(), case.C.w1.clone()
        w0[m, a], w1[m, a] = case.C.w1[m, a], case.C.w0[m, a]
        rf, rb = with_coords(v.Coords(i0, w0, w1))
        assert rf > 1.0 and rb > 1.0, ("swapped weights", a, m, rf, rb)
    # tap 1 dropped where i0 = -1 (the only tap of that axis in range)
    dropped = 0
    for a in range(3):
        cand = (seen.all(1) & (i0[:, a] == -1)).nonzero()
        if cand.numel() == 0:
            assert res[a] == 1
            continue
        dropped += 1
        m = int(cand[0])
        w1 = case.C.w1.clone()
        w1[m, a] = 0.0
        rf, rb = with_coords(v.Coords(i0, case.C.w0, w1))
        assert rf > 1.0 and rb > 1.0, ("dropped tap", a, m, rf, rb)
    assert dropped >= 2
    # the last sample of one chunk is zeroed
    for chunk in v.CHUNKS:
        last = torch.arange(chunk - 1, case.M, chunk)
        m = int(last[(case.fwd["color_prod"].y_abs[last].amax(1) > 0)][0])
        prod = case.fwd["color_prod"].y.clone()
        prod[m] = 0.0
        assert v.ratio(prod, case.fwd["color_prod"], S) > 1.0
        one = _run_backward(case, torch.tensor([m]))
        assert _worst([y - o.y for y, o in zip(ys, one)], ref_b, S) > 1.0, ("zeroed sample", chunk, m)


# ---------------------------------------------------------------------------------------------- coverage
@pytest.mark.parametrize("res,box", WALKS)
def test_scripted_walks_reach_every_branch_under_every_chunk_length(res, box):
    case = v.walk_case(res, box)
    i0 = case.C.i0.numpy()
    v.assert_coverage(i0, res)
    for M in (32767, 65536):  # the tiled cases of the GPU tests keep it (and gain phases)
        v.assert_coverage(v.coords(v.tile_case(case.meta, M), case.aabb, res).i0.numpy(), res)
    # all 27 step combinations occur inside rays, and multi-texel jumps are mixed in
    multi = [a for a in range(3) if res[a] > 1]
    steps, jumps = set(), 0
    for name, a, b in case.meta["rays"]:
        d = np.diff(i0[a:b], axis=0)
        jumps += int((np.abs(d) > 1).any(1).sum())
        steps |= {tuple(int(x) for x in s) for s in d[(np.abs(d) <= 1).all(1)][:, multi]}
    assert len(steps) == 3 ** len(multi) and jumps >= 20
    # each face is crossed out and back: i0 takes -2, -1, 0 and size-2, size-1, size on every axis that has texels
    for a in multi:
        assert {-2, -1, 0, res[a] - 2, res[a] - 1, res[a]} <= set(int(x) for x in i0[:, a])
    xn = v.normalise32(case.xyz, case.aabb)
    assert np.isfinite(case.xyz).all() and 20 < np.abs(xn).max() <= 102  # far outside, within +-50 extents
    variants = {n.rstrip("+-012") for n, _, _ in case.meta["rays"]}
    assert variants == {"interior", "face", "far"}


def test_interior_variant_stays_interior_and_far_variant_mostly_outside():
    res = (24, 31, 45)
    c = v.scripted_case(res, v.UNIT_AABB, 1, variants=("interior",))
    i0 = v.coords(c["xyz"], v.UNIT_AABB, res).i0.numpy()
    assert ((i0 >= 0) & (i0 + 1 < np.array(res))).all()
    c = v.scripted_case(res, v.UNIT_AABB, 1, variants=("far",))
    i0 = v.coords(c["xyz"], v.UNIT_AABB, res).i0.numpy()
    assert (((i0 < -1) | (i0 >= np.array(res))).any(1)).mean() > 0.6


def test_lattice_points_are_exact_and_hit_every_special_position():
    case = v.lattice()
    x = case.xyz
    for a, s in enumerate(case.res):
        for e in case.meta["special"][a]:
            assert (x[:, a] == e).sum() >= 2
        centres = (2.0 * np.arange(s) / (s - 1) - 1.0).astype(np.float32)
        assert set(centres.tolist()) <= set(x[:, a].tolist())
        on = np.isin(x[:, a], centres)
        w1 = case.C.w1.numpy()[on, a]
        assert (w1 == 0).all()  # texel centres: dyadic, exact, weight 1 on one tap
    i0 = case.C.i0.numpy()
    assert (i0 == -1).any() and (i0 == np.array(case.res) - 1).any()


def test_bookkeeping_on_a_hand_made_sequence():
    res = (5, 5, 5)
    i0 = np.array([[1, 1, 1], [2, 1, 1], [2, 1, 1], [2, 0, 1], [2, 0, 3], [3, 0, 3], [4, 0, 3], [3, 1, 3]])
    mc = v.move_classes(i0, res, 4)
    assert mc["first"].tolist() == [True, False, False, False, True, False, False, False]
    assert [v.PLANE_CLASSES[c] for c in mc["plane"][1:4, 0]] == ["+x", "same", "-y"]       # set 0 = (x, y)
    assert [v.PLANE_CLASSES[c] for c in mc["plane"][5:, 1]] == ["+x", "+x", "-x"]          # set 1 = (x, z)
    assert [v.PLANE_CLASSES[c] for c in mc["plane"][5:, 0]] == ["+x", "+x", "jump"]
    assert [v.LINE_CLASSES[c] for c in mc["line"][1:4, 1]] == ["same", "same", "-1"]       # line 1 = y
    assert mc["plane_interior"][5, 1] and not mc["plane_interior"][6, 1] and not mc["plane_interior"][7, 1]  # x = 4: tap 5 is outside
    assert [v.LINE_CLASSES[c] for c in mc["line"][4:5, 0]] == ["jump"] and mc["line_interior"][5, 2] and not mc["line_interior"][6, 2]
    rp, rl = v.reachable((1, 2, 5))
    assert not rp[0, :, 1].any() and rp[2, 0, 1] and rp[2, 3, 1] and not rp[2, 1, 1] and rp[2, 5, 1]
    assert not rl[2, 1:, :].any() and rl[0, :, :].all() and rl[1, 1, 0] and not rl[1, 1, 1]
