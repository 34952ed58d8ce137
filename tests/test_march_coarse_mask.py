"""The coarse occupancy mask never hides a sample (CPU): a numpy restatement of the mask build and of the marcher's 64-point test
(tests/coarse_mask_ref.py, mirroring pvd_occ_coarse_mask and coarse_confine in csrc/raymarching.hip) against the oracle's serial
walk.  For every grid and 2000 rays: a ray the test calls empty has oracle count 0, and every oracle sample's t lies below the
lowered far.  No exception is tolerated: these are conditions, not tolerances.

The samples' t are rebuilt from the oracle's own outputs: deltas[k, 1] = fl(t_after_k - t_after_{k-1}) (t0 for the first), so
t_k = t0 + sum_{i<=k} deltas[i, 1] - deltas[k, 0] in float64, off by at most n 2^-24 dt < 1e-6; the lowered far exceeds every
possibly-occupied lattice point by about half a sample spacing (span / 126 >= 1e-3 for any ray that samples), so the comparison
is not at risk from that."""
import numpy as np
import pytest

import oracle

import coarse_mask_ref as ref

H, N = 128, 2000


def _t0(nears, dt_min, perturb):
    if not perturb:
        return nears.copy()
    u = np.array([oracle.pcg32_stream(42, n, 1)[1][0] for n in range(len(nears))], np.float32)  # ray_t0: seed 42, advance(n)
    return (np.float64(dt_min) * u.astype(np.float64) + nears.astype(np.float64)).astype(np.float32)  # one fused operation


def _check(name, dense, bound, max_steps=1024, perturb=False, min_near=0.2):
    C = dense.shape[0]
    bits = ref.bitfield_of(dense)
    mask = ref.coarse_mask(bits, C, H)
    o, d = ref.rays(N, bound, dense, seed=len(name))
    aabb = np.array([-bound] * 3 + [bound] * 3, np.float32)
    nears, fars = oracle.near_far_from_aabb(o, d, aabb, min_near)
    M = N * max_steps + 1
    _, _, deltas, rays, counter = oracle.march_rays_train(o, d, bits, bound, C, H, nears, fars, M, perturb=perturb, max_steps=max_steps)
    assert np.array_equal(rays[:, 0], np.arange(N))
    dt_min, _, _ = ref.step_constants(max_steps, C, H)
    t0 = _t0(nears, dt_min, perturb)
    stated, empty, far2 = ref.confine(mask, o, d, t0, fars, bound, C, H, max_steps)
    cnt = rays[:, 2]
    bad_empty = np.flatnonzero(empty & (cnt > 0))
    assert bad_empty.size == 0, "%s: rays called empty that sample: %s (counts %s)" % (name, bad_empty[:8], cnt[bad_empty[:8]])
    worst, n_cut = -np.inf, 0
    for n in np.flatnonzero(stated & (cnt > 0)):
        dl = deltas[rays[n, 1]:rays[n, 1] + cnt[n]].astype(np.float64)
        t = np.float64(t0[n]) + np.cumsum(dl[:, 1]) - dl[:, 0]
        worst = max(worst, float((t - np.float64(far2[n])).max()))
        n_cut += far2[n] < fars[n]
        assert (t < far2[n]).all(), "%s: ray %d samples at t = %r, beyond the lowered far %r (far %r)" % (name, n, t.max(), far2[n], fars[n])
    return dict(stated=int(stated.sum()), empty=int(empty.sum()), sampled=int((cnt > 0).sum()), cut=int(n_cut), worst=worst,
                samples=int(counter[0]))


@pytest.fixture(scope="module", params=[1.0, 2.0], ids=["bound1", "bound2"])
def setup(request):
    bound = request.param
    C = 1 + int(np.ceil(np.log2(bound)))
    return bound, ref.grids(C, H, seed=int(bound))


def test_mask_restatement_on_hand_cases():
    """One occupied cell: exactly the blocks within one block of its own are set, clamped at the grid's border."""
    for cell, want in (((0, 0, 0), 8), ((64, 64, 64), 27), ((127, 63, 0), 12), ((127, 127, 127), 8)):
        dense = np.zeros((1, H, H, H), bool)
        dense[(0,) + cell] = True
        bits = ref.bitfield_of(dense)
        assert np.unpackbits(bits).sum() == 1
        assert np.array_equal(ref.dense_of(bits, 1, H), dense)
        m = ref.coarse_mask(bits, 1, H).reshape(16, 16, 16)
        assert m.sum() == want
        bx, by, bz = (c // 8 for c in cell)
        assert m[max(bx - 1, 0):bx + 2, max(by - 1, 0):by + 2, max(bz - 1, 0):bz + 2].all()
    # the oracle's own packbits agrees with the restatement's bit order
    g = np.random.RandomState(0).rand(H ** 3).astype(np.float32)
    dense = np.zeros((1, H, H, H), bool)
    dense.reshape(-1)[:] = (g > 0.5)[ref.morton_of_cells(H).reshape(-1)]
    assert np.array_equal(ref.bitfield_of(dense), oracle.packbits(g, 0.5))


def test_no_ray_called_empty_samples_and_no_sample_beyond_the_lowered_far(setup, capsys):
    bound, grids = setup
    lines = []
    for name, dense in grids.items():
        r = _check(name, dense, bound)
        lines.append("%-16s stated %4d empty %4d sampled %4d cut %4d samples %8d worst t - far' %.4g" %
                     (name, r["stated"], r["empty"], r["sampled"], r["cut"], r["samples"], r["worst"]))
        if name == "empty":
            assert r["samples"] == 0 and r["empty"] == r["stated"] > N // 2
        if name == "full":
            assert r["empty"] == 0
    with capsys.disabled():
        print("\nbound %g\n%s" % (bound, "\n".join(lines)))


@pytest.mark.parametrize("max_steps,perturb,min_near", [(1024, True, 0.2), (8, False, 0.2), (8, True, 0.2), (1024, True, 0.01), (64, False, 0.05)])
def test_with_perturbed_starts_small_step_budgets_and_near_starts(setup, max_steps, perturb, min_near):
    """perturb moves t0 (and with it the whole lattice); max_steps 8 makes dt = dt_max and the cap bind (and lifts the level the step
    size asks for); a small min_near starts rays deep inside occupied blocks."""
    bound, grids = setup
    for name in ("random5", "blocky_odd", "full", "cell_127_63_0"):
        _check(name, grids[name], bound, max_steps=max_steps, perturb=perturb, min_near=min_near)
