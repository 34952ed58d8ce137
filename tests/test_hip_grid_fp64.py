"""The hash-grid encoder's table gradient (pvd_grid_encode_backward / _affine: k_grid_bwd_lps2, k_grid_bwd_coarse and k_grid_bwd of
csrc/gridencoder.hip) against the float64 restatement in tests/grid_ref64.py, element by element, under the bound derived there:

    |kernel - fp64| <= gamma(k + 1, u) s_abs + 8 * 2^-24 s_abs + k a        (u = 2^-11 | 2^-24, a = 2^-25 | 0 for f16 | f32)

and BIT FOR BIT on the exact cases (dyadic positions, integer gradients: every order and grouping of the sums is exact), which carry
the scripted run shapes of grid_ref64.script: runs of 1, 2, 3, 31, 32, 33 and a whole wave, runs across a wave and a workgroup
boundary, runs that end on and one before the last lane, A B A, dead samples inside and between runs, a dead wave.  An element that
no contribution lands in must keep its bits (zero, or the prefill).  tests/test_grid_ref64.py holds, on the CPU, what makes these
checks mean something: the oracle inside the same bound, sensitivity of every tolerance case to one dropped contribution, the
mutations caught, the run shapes present.

Paths (the knobs are process-wide; `knobs` restores them in a finally and then asserts that a default call gives the bits it gave
before):
  1  f16 D 3 C 2 default                                        k_grid_bwd_lps2
  2  grid_set_fwd_kernel(2, 4096 | 1 << 29)                      k_grid_bwd_coarse on every level
  3  2 + grid_set_variant(1 << 29)                               k_grid_bwd_coarse below scale 300, k_grid_bwd above
  4  2 + grid_set_variant(1 << 30), and with bit 0               k_grid_bwd on every level, plain and XCD-aware schedule
  5  grid_encode_backward_affine, (add, div) = (2, 4)            k_grid_bwd_lps2 mapping the positions itself
  6  every other (type, D, C) by default dispatch                k_grid_bwd_coarse<T, D, C>; with calc_grad_inputs the input-gradient
                                                                 kernel rides behind (its own result: test_hip_parity.py)
Tiled grids and align_corners go through each of the three kernels (f16 tolerance cases on paths 1, 2, 4; bit-exact in f32 on the
coarse and the plain kernel).  Unreachable through the bindings and therefore not here: k_grid_bwd_coarse / k_grid_bwd with an
affine map (refused: PVD_ERR_UNSUPPORTED) and the plain kernel together with the two-lane kernel in one call.

Every test prints its max(err / bound) lines (pytest -s); profiles/grid_fp64_pin.txt keeps the lines of one run on the MI355X next to
the oracle's.  Those numbers are a record; the threshold is the bound.  No hipGraph, no inf / nan, no found_inf rider."""
import contextlib

import numpy as np
import pytest
import torch

import grid_ref64 as G

pytestmark = pytest.mark.gpu

GUARD = 64  # sentinel rows in front of offsets[0] and behind offsets[L]
COARSE = (2, 4096 | (1 << 29))


@pytest.fixture(scope="module")
def hip():
    import pvd_hip
    assert torch.cuda.is_available()
    return pvd_hip


def _say(capsys, line):
    with capsys.disabled():
        print("\n" + line, end="")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ibits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def _scatter(hip, case, guard=0, calc=False):
    """one backward call of the case through the binding; returns the whole output buffer [guard + rows + guard, C]"""
    td = torch.float16 if case.dtype == np.float16 else torch.float32
    rows = int(case.offsets[-1])
    buf = torch.full((rows + 2 * guard, case.C), 7.25, dtype=td, device="cuda")
    mid = buf[guard:guard + rows]
    if case.prefill is None:
        mid.zero_()
    else:
        mid.copy_(_dev(case.prefill))
    offs = _dev(case.offsets + np.int32(guard))
    g, x = _dev(case.g), _dev(case.x)
    a = (g, x)
    shape = (case.B, case.D, case.C, case.L, case.S, case.H)
    if case.affine is not None:
        assert not calc
        hip.grid_encode_backward_affine(g, x, case.affine[0], case.affine[1], buf, offs, buf, *shape, case.gridtype, case.align)
    elif calc:
        dy_dx = torch.zeros(case.B, case.L * case.D * case.C, dtype=td, device="cuda")
        gi = torch.empty(case.B, case.D, dtype=td, device="cuda")
        hip.grid_encode_backward(g, x, buf, offs, buf, *shape, True, dy_dx, gi, case.gridtype, case.align)
    else:
        dummy = buf[:1]
        hip.grid_encode_backward(g, x, buf, offs, buf, *shape, False, dummy, dummy, case.gridtype, case.align)
    torch.cuda.synchronize()
    del a
    return buf


def _check(capsys, label, case, buf, guard=0, a=None):
    """the table part of buf against the case's reference: bit-equal (exact cases) or within the bound, untouched elements untouched;
    compared on the device except for the touched elements"""
    r = case.ref
    rows = int(case.offsets[-1])
    if guard:
        edge = torch.cat([buf[:guard], buf[guard + rows:]])
        assert torch.equal(edge, torch.full_like(edge, 7.25)), "%s %s: a sentinel row around the table changed" % (label, case.name)
    flat = buf[guard:guard + rows].reshape(-1)
    idx = _dev(r.idx)
    got_t = flat[idx]
    if case.prefill is None:
        rest_ok = int(torch.count_nonzero(_ibits(flat))) == int(torch.count_nonzero(_ibits(got_t)))
    else:
        before, after = _dev(case.prefill).reshape(-1).clone(), flat.clone()
        before[idx], after[idx] = 0, 0
        rest_ok = torch.equal(_ibits(before), _ibits(after))
    got_np = got_t.cpu().numpy()
    if case.exact:
        want = r.t_ref.astype(case.dtype)
        bad = np.nonzero(G._bits(got_np) != G._bits(want))[0]
        line = "%-34s %-44s %s" % (label, case.name, "bit-equal" if not len(bad) and rest_ok else "NOT bit-equal (%d elements)" % len(bad))
        _say(capsys, line)
        assert not len(bad), (line, G.describe(r, r.idx[bad[0]], flat.cpu().numpy()))
    else:
        worst, at = G.ratio(got_np, r, prefill=case.prefill, a=a, touched_only=True)
        line = "%-34s %-44s max(err/bound) %.4f  (k max %d, %d elements)" % (label, case.name, worst, r.t_k.max(), len(r.idx))
        _say(capsys, line)
        assert worst <= 1.0, (line, G.describe(r, at, flat.cpu().numpy()))
    assert rest_ok, "%s %s: an element that no contribution lands in changed its bits" % (label, case.name)


def _run(capsys, hip, label, name, **kw):
    case = G.case(name)
    if not case.exact and name != "subnormal":
        G.assert_sensitive(case)  # a condition of the case, from the reference alone
    _check(capsys, label, case, _scatter(hip, case, **kw))


def _default_bits(hip):
    return _scatter(hip, G.case("exact[:257]"))


@contextlib.contextmanager
def knobs(hip, fwd_kernel=None, variant=None):
    before = _default_bits(hip)
    try:
        if fwd_kernel is not None:
            hip.grid_set_fwd_kernel(*fwd_kernel)
        if variant is not None:
            hip.grid_set_variant(variant)
        yield
    finally:
        hip.grid_set_variant(0)
        hip.grid_set_fwd_kernel()
    assert torch.equal(_ibits(before), _ibits(_default_bits(hip))), "the default path changed after the knobs were restored"


# ---------------------------------------------------------------------------------------------- the plain kernel's schedule, restated
def schedule_blocks(scales, nb, row_bytes, D, xcd_aware):
    """make_schedule of csrc/gridencoder.hip: (total_blocks, exclusive rounds, shared levels)"""
    big = [l for l, s in enumerate(scales) if xcd_aware and (np.ceil(float(s)) + 2.0) ** D * row_bytes >= 512 * 1024]
    n_excl = len(big) // 8
    n_shared = len(scales) - n_excl * 8
    return (n_excl * nb + -(-n_shared * nb // 8)) * 8, n_excl, n_shared


def test_schedule_needs_more_than_one_round(hip):
    """paths 3 and 4 run k_grid_bwd under LevelSchedule::locate.  With f16 C 2 rows, L 14 and the product's scales, levels 3..13 are
    'big' (>= 512 KiB): eight of them exclusive, the other three and the three small ones shared.  B = 941 (the scripted cases) gives nb = 4: 4 exclusive slots per
    XCD, 24 shared items over 8 XCDs = 3 more, total_blocks = 56: seven rounds of 8, and B = 3000 (nb = 12) 168.  The plain schedule has
    14 shared levels: 56 and 168 blocks as well.  Anything above B = 256 (nb >= 2) leaves the first round."""
    scales = G.level_scales(14, np.log2(G.PRODUCT_PLS), 16)
    for B, want in ((941, 56), (3000, 168)):
        nb = -(-B // 256)
        for aware in (False, True):
            total, n_excl, n_shared = schedule_blocks(scales, nb, 4, 3, aware)
            assert total == want and total > 8 and (n_excl, n_shared) == ((1, 6) if aware else (0, 14))
    assert min(G.case(n).B for n in G.MAIN) > 512


# ---------------------------------------------------------------------------------------------- paths 1 to 4: f16, D 3, C 2
@pytest.mark.parametrize("name", G.MAIN)
def test_path1_two_lane_kernel(capsys, hip, name):
    _run(capsys, hip, "lps2", name)


@pytest.mark.parametrize("name", G.MAIN)
def test_path2_run_merging_kernel_on_every_level(capsys, hip, name):
    with knobs(hip, COARSE):
        _run(capsys, hip, "coarse", name)


@pytest.mark.parametrize("name", G.MAIN)
def test_path3_run_merging_below_scale_300_plain_above(capsys, hip, name):
    with knobs(hip, COARSE, 1 << 29):
        _run(capsys, hip, "coarse<300|plain", name)


@pytest.mark.parametrize("xcd", [0, 1])
@pytest.mark.parametrize("name", G.MAIN)
def test_path4_plain_kernel_on_every_level(capsys, hip, name, xcd):
    with knobs(hip, COARSE, (1 << 30) | xcd):
        _run(capsys, hip, "plain xcd-aware" if xcd else "plain", name)


@pytest.mark.parametrize("name", G.AFFINE_CASES)
def test_path5_affine(capsys, hip, name):
    _run(capsys, hip, "lps2 affine", name)


@pytest.mark.parametrize("dt,D,C", G.OTHER)
def test_path6_default_dispatch_of_the_other_instantiations(capsys, hip, dt, D, C):
    for name in G.other_names(dt, D, C):
        _run(capsys, hip, "coarse<%s,%d,%d>" % (dt, D, C), name)


def test_path6_input_gradient_kernel_riding_behind(capsys, hip):
    """calc_grad_inputs: f16 D 3 C 2 then goes through k_grid_bwd_coarse with k_grid_input_bwd behind it; the table gradient stays in bound"""
    for name in ("exact", "random-T10", "prefilled"):
        _run(capsys, hip, "coarse + input bwd", name, calc=True)
    _run(capsys, hip, "coarse<float32,3,4> + input bwd", "random-float32-D3C4", calc=True)


@pytest.mark.parametrize("name", ["exact-f32-tiled", "exact-f32-align", "exact-f32-wrap"])
def test_tiled_align_and_wrapped_levels_bit_exact_f32(capsys, hip, name):
    _run(capsys, hip, "coarse<float32,3,2>", name)
    with knobs(hip, None, 1 << 30):
        _run(capsys, hip, "plain<float32,3,2>", name)
    with knobs(hip, None, (1 << 30) | 1):
        _run(capsys, hip, "plain<float32,3,2> xcd-aware", name)


# ---------------------------------------------------------------------------------------------- sizes, guard rows, subnormals
def test_sizes_around_wave_and_workgroup_edges_bit_exact(capsys, hip):
    """B around 32, 64, 128, 256 on the exact inputs: the two-lane kernel's 2 B lanes cross its wave and workgroup edges at half of them"""
    for variant, label in ((None, "lps2"), (0, "coarse"), (1 << 30, "plain")):
        with knobs(hip, None if variant is None else COARSE, variant):
            for B in G.SIZES:
                _run(capsys, hip, label, "exact[:%d]" % B)


def test_guard_rows_stay(capsys, hip):
    for variant, label in ((None, "lps2 guarded"), (0, "coarse guarded"), ((1 << 30) | 1, "plain guarded")):
        with knobs(hip, None if variant is None else COARSE, variant):
            for name in ("exact", "scripted-T11", "prefilled"):
                case = G.case(name)
                _check(capsys, label, case, _scatter(hip, case, guard=GUARD), guard=GUARD)
    for name in ("affine-prefilled", "random-float32-D2C8", "random-float16-D3C1"):
        case = G.case(name)
        _check(capsys, "default guarded", case, _scatter(hip, case, guard=GUARD), guard=GUARD)


def test_subnormal_contributions_and_sums(capsys, hip):
    """f16 contributions and sums below 2^-14, a = 2^-25: the packed f16 atomic and the conversions keep gradual underflow"""
    case = G.case("subnormal")
    assert G.subnormal_rate(case.ref) > 0.5
    _check(capsys, "lps2", case, _scatter(hip, case))
    with knobs(hip, COARSE):
        _check(capsys, "coarse", case, _scatter(hip, case))
    with knobs(hip, COARSE, 1 << 30):
        _check(capsys, "plain", case, _scatter(hip, case))
