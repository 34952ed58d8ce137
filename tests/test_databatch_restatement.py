"""tests/databatch_restatement.py -- the numpy restatement the kernels of include/pvd_hip_data.h are compared against -- tied piece by
piece to the project's CPU code: its PCG32 to the oracle's, the cell-to-pixel map and the EMA to pvd.scene, the blend to
pvd.provider.training_target, and the exponential-race draw to torch.multinomial's distribution.  No GPU."""
import numpy as np
import pytest
import torch

import databatch_restatement as R


@pytest.mark.parametrize("initseq", [1, 2])
@pytest.mark.parametrize("seed", [0, 1234, 0x9E3779B97F4A7C15, 2 ** 64 - 1])
def test_the_numpy_pcg32_is_the_oracles(seed, initseq):
    import oracle
    advances = [0, 1, 7, 8, 800, 16383, 8 * 4095, 2 ** 33 + 5]
    g = R.Pcg32(np.full(len(advances), seed, np.uint64), initseq).advance(np.array(advances, np.uint64))
    got_u = np.stack([g.next() for _ in range(3)], -1)
    got_f = g.next_float()
    for i, adv in enumerate(advances):
        u, f = oracle.pcg32_stream(seed, adv, 4, initseq=initseq)
        assert np.array_equal(got_u[i], u[:3]) and got_f[i] == f[3], (seed, initseq, adv)
    assert got_f.dtype == np.float32 and (got_f >= 0).all() and (got_f < 1).all()


def test_the_batch_key_wraps_like_uint64_arithmetic():
    assert int(R.batch_initstate(5, 0)) == (5 + R.GOLDEN) & (2 ** 64 - 1)
    assert int(R.batch_initstate(2 ** 64 - 1, 3)) == (2 ** 64 - 1 + 4 * R.GOLDEN) % 2 ** 64
    assert np.array_equal(R.batch_initstate(7, np.array([0, 3])), np.array([R.batch_initstate(7, 0), R.batch_initstate(7, 3)]))


def test_cell_to_pixel_and_ema_are_scene_pys_arithmetic(monkeypatch):
    """sample_pixels_by_error (grid 128) on shared draws: its multinomial and its two rand calls are replaced by the restatement's
    cells and jitters, so only the arithmetic is compared; then update_error_map against ema()."""
    from pvd import scene
    H, W, N, G = 100, 75, 300, 128 * 128
    rng = np.random.RandomState(0)
    w = rng.uniform(0.0, 5.0, size=(1, G)).astype(np.float32)
    w[0, rng.choice(G, 4000, replace=False)] = 0.0
    cells = R.select(R.keys64(w[0], R.cell_uniforms(11, 3, G)), N)
    _, u1, u2, _ = R.ray_draws(11, 3, N)
    u1[:3], u2[:3] = np.float32(1.0) - np.float32(2.0 ** -24), np.float32(0.0)  # the clamp at H - 1 / W - 1 and the cell's first pixel
    feed = [torch.from_numpy(u1)[None], torch.from_numpy(u2)[None]]
    monkeypatch.setattr(torch, "multinomial", lambda *a, **k: torch.from_numpy(cells)[None])
    monkeypatch.setattr(torch, "rand", lambda *a, **k: feed.pop(0))
    inds, coarse = scene.sample_pixels_by_error(torch.from_numpy(w), N, H, W)
    monkeypatch.undo()
    assert np.array_equal(coarse[0].numpy(), cells)
    mine = R.cell_to_pixel(cells, u1, u2, H, W, 128)
    assert np.array_equal(inds[0].numpy(), mine) and mine.max() < H * W and mine.min() >= 0
    # cells of the last grid row / column land on the last pixel row / column at most
    assert (mine // W).max() <= H - 1 and (mine % W).max() <= W - 1

    pred, gt = rng.rand(N, 3).astype(np.float32), rng.rand(N, 3).astype(np.float32)
    err = ((torch.from_numpy(pred) - torch.from_numpy(gt)) ** 2).mean(-1)[None]
    new = scene.update_error_map(torch.from_numpy(w.copy()), torch.from_numpy(cells)[None], err)[0].numpy()
    mine = R.ema(w[0, cells], pred, gt)
    ulp = np.spacing(np.abs(new[cells]).astype(np.float32))
    assert (np.abs(new[cells] - mine) <= 2 * ulp).all()  # (torch's mean sums in its own order and multiplies by 1/3)
    untouched = np.ones(G, bool)
    untouched[cells] = False
    assert np.array_equal(new[untouched], w[0, untouched])


def test_the_blend_is_training_target_bit_for_bit(monkeypatch):
    from pvd.provider import training_target
    rng = np.random.RandomState(1)
    px = rng.randint(0, 256, size=(1, 500, 4)).astype(np.uint8)
    px[0, :20, 3], px[0, 20:40, 3] = 0, 255
    bg = rng.rand(1, 500, 3).astype(np.float32)
    images = torch.from_numpy(np.asarray(px, dtype=np.float32) / 255.0)  # what BlenderScene keeps
    monkeypatch.setattr(torch, "rand", lambda *a, **k: torch.from_numpy(bg))  # shared draws
    gt, bg_t = training_target(images)
    monkeypatch.undo()
    assert np.array_equal(gt.numpy(), R.blend(px, bg)) and np.array_equal(bg_t.numpy(), bg)
    gt3, white = training_target(images[..., :3])
    assert np.array_equal(gt3.numpy(), R.blend(px[..., :3], None)) and white == 1
    # the bytes come back exactly from the float images (DeviceBatcher.from_scene)
    assert np.array_equal((images * 255.0).round().to(torch.uint8).numpy(), px)
    assert np.array_equal((images.half().float() * 255.0).round().to(torch.uint8).numpy(), px)


def test_selection_takes_the_largest_keys_with_ties_to_the_lower_cell():
    keys = np.array([0.0, 3.0, 0.0, 3.0, 7.0, 0.0, np.inf, 3.0])
    assert R.select(keys, 1).tolist() == [6]
    assert R.select(keys, 3).tolist() == [1, 4, 6]
    assert R.select(keys, 4).tolist() == [1, 3, 4, 6]
    assert R.select(keys, 6).tolist() == [0, 1, 3, 4, 6, 7]
    k = R.keys64(np.array([1.0, 0.0, -2.0, np.nan, 4.0], np.float32), np.array([0.5, 0.5, 0.5, 0.5, 0.0], np.float32))
    assert k[1] == 0 and k[2] == 0 and k[3] == 0 and k[4] == np.inf and abs(k[0] - 1 / np.log(2)) < 1e-15


# Seeds of the distribution test, fixed after checking that two independent torch.multinomial runs stay inside the bound with them
SEED_RESTATEMENT, SEED_TORCH_A, SEED_TORCH_B = 2023, 101, 202


def _inclusion(cells, G):
    return np.bincount(np.asarray(cells).ravel(), minlength=G) / float(cells.shape[0])


def test_the_exponential_race_draws_from_torch_multinomials_distribution():
    """g = 8, weights 1..50, N = 16 cells per batch, T = 4000 batches: each cell's inclusion frequency under the restatement's draw
    against torch.multinomial(replacement=False) with a generator of its own.  Two frequencies of the same inclusion probability p
    from T independent batches each differ by a variable of standard deviation sqrt(2 p (1 - p) / T); the bound is five of them,
    with the pooled frequency for p.  Two independent torch runs are held to the same bound."""
    g, N, T = 8, 16, 4000
    G = g * g
    w = (1.0 + 49.0 * np.random.RandomState(4).rand(G) ** 2).astype(np.float32)
    w[0], w[-1] = 1.0, 50.0
    u = R.cell_uniforms(SEED_RESTATEMENT, np.arange(T), G)
    mine = _inclusion(R.select(R.keys64(w[None], u), N), G)
    wt = torch.from_numpy(w).expand(T, G).contiguous()
    ta = _inclusion(torch.multinomial(wt, N, replacement=False, generator=torch.Generator().manual_seed(SEED_TORCH_A)).numpy(), G)
    tb = _inclusion(torch.multinomial(wt, N, replacement=False, generator=torch.Generator().manual_seed(SEED_TORCH_B)).numpy(), G)

    def inside(fa, fb):
        p = 0.5 * (fa + fb)
        return np.abs(fa - fb) <= 5.0 * np.sqrt(2.0 * p * (1.0 - p) / T)
    assert inside(ta, tb).all(), "the two torch runs disagree: the seeds do not serve"
    assert inside(mine, ta).all(), (np.abs(mine - ta).max(), np.flatnonzero(~inside(mine, ta)))
    assert inside(mine, tb).all()
    assert abs(mine.sum() - N) < 1e-9 and mine[np.argmax(w)] > 3 * mine[np.argmin(w)]  # (not the uniform draw)
