"""The float64 restatement of the hash-grid table gradient (tests/grid_ref64.py) against the CPU oracle, and the checker against
itself, on every case that tests/test_hip_grid_fp64.py runs on the GPU.  No GPU.

* The oracle's backward (ascending-sample order, one legal order of the atomics) lies within grid_ref64.bound of the float64
  reference on every tolerance case and is bit-equal on every exact case: that ties the numpy restatement of scale, position, cell,
  bounds rule and LevelIndex to the oracle, which the forward tests tie bit for bit to the kernels, and shows that the reference
  stays inside its own bound.  (The oracle starts from a zero table: prefilled cases are compared without their prefill; the affine
  cases on the positions mapped in float32.)
* assert_sensitive holds for every tolerance case, the exactness conditions for every exact case, the subnormal rate stays below 1 %.
* A dropped contribution, a doubled tail lane, two runs merged across a dead sample and a skipped block of 256 samples on the finest
  level, applied to the reference's own contribution list, are caught in the cases "exact" and "scripted-T11".
* The scripted cases contain every run shape of grid_ref64.FEATURES_ONE_LANE / FEATURES_TWO_LANE.

`pytest -s` prints the oracle's max(err / bound) per case; profiles/grid_fp64_pin.txt keeps them next to the MI355X's."""
import numpy as np
import pytest

import grid_ref64 as G
import oracle


def _say(capsys, line):
    with capsys.disabled():
        print("\n" + line, end="")


def test_scales_and_offsets_are_the_hosts():
    from gridencoder.grid import level_offsets
    for S in (1.0, float(np.log2(G.PRODUCT_PLS)), 0.5):
        want, _ = oracle.grid_level_params(14, S, 16)
        assert np.array_equal(G.level_scales(14, S, 16), want), S
    for D in (2, 3):
        for pls in (2.0, G.PRODUCT_PLS):
            for log2 in (10, 12, 19):
                for align in (False, True):
                    assert np.array_equal(G.level_offsets(D, 14, pls, 16, log2, align), np.array(level_offsets(D, 14, pls, 16, log2, align), np.int32))


def _oracle(case):
    x = case.ref.geo.x01 if case.affine is not None else case.x
    emb = np.zeros((int(case.offsets[-1]), case.C), case.dtype)
    got, _ = oracle.grid_encode_backward(case.g, x, emb, case.offsets, case.S, case.H, gridtype=case.gridtype, align_corners=case.align)
    return got


@pytest.mark.parametrize("name", list(G.CASES))
def test_oracle_within_bound_and_case_conditions(capsys, name):
    case = G.case(name)
    got = _oracle(case)
    r = case.ref
    if case.exact:
        G.assert_exact(case)
        assert G.bit_equal(got, r), G.describe(r, G.ratio(got, r)[1], got)
        _say(capsys, "%-34s %-44s bit-equal" % ("oracle", case.name))
        return
    a = None
    if name == "subnormal":
        assert G.subnormal_rate(r) > 0.5 and np.mean(np.abs(r.t_ref) < 2.0 ** -14) > 0.5
    else:
        G.assert_sensitive(case)
        assert G.subnormal_rate(r) < 0.01
    worst, at = G.ratio(got, r, a=a)
    _say(capsys, "%-34s %-44s max(err/bound) %.4f  (k max %d, %d elements)" % ("oracle", case.name, worst, r.t_k.max(), len(r.idx)))
    assert worst <= 1.0, G.describe(r, at, got)


@pytest.mark.parametrize("name", ["exact", "scripted-T11"])
@pytest.mark.parametrize("kind", ["drop", "double", "merge", "skip"])
def test_mutations_are_caught(name, kind):
    case = G.case(name)
    assert not G.caught(case, case.ref.t_ref.copy())
    for j in ((0, 1, 3) if kind == "skip" else (0,)):
        assert G.caught(case, G.mutate(case.ref, kind, j)), (name, kind, j)


@pytest.mark.parametrize("name", ["exact", "scripted", "scripted-T11", "scripted-tiled-align", "affine-scripted", "exact-f32-tiled", "exact-f32-align", "exact-f32-wrap"]
                         + [n for dt, D, C in G.OTHER for n in G.other_names(dt, D, C)[:2]])
def test_scripted_cases_contain_every_run_shape(name):
    geo = G.case(name).ref.geo
    one = G.coverage(geo, 64, 256)
    assert not (G.FEATURES_ONE_LANE - one), sorted(G.FEATURES_ONE_LANE - one)
    two = G.coverage(geo, 32, 128)
    assert not (G.FEATURES_TWO_LANE - two), sorted(G.FEATURES_TWO_LANE - two)


def test_exact_levels_wrap_as_the_kernels_uint32():
    """S = 1, H = 16: the stride product of levels 12 and 13 wraps at 2^32 and the levels come out dense; the f32 exact cases keep them"""
    geo = G.case("exact-f32-wrap").ref.geo
    assert geo.L == 14 and geo.hashed[11] and not geo.hashed[12] and not geo.hashed[13]
