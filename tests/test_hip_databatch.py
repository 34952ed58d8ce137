"""pvd_image_batch / pvd_error_map_update (include/pvd_hip_data.h) and pvd.batcher.DeviceBatcher on the GPU against the numpy
restatement (tests/databatch_restatement.py, itself tied to the project's CPU code by tests/test_databatch_restatement.py), and
inside TeacherTrainer's recorded 16-step block."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import databatch_restatement as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
V, H, W = 3, 20, 28  # g = 8 divides neither side
INTR = (30.0, 31.0, 14.0, 10.0)
SEED = 0xC0FFEE


def _images(C, v=V, h=H, w=W, seed=0):
    rng = np.random.RandomState(seed)
    im = rng.randint(0, 256, size=(v, h, w, C)).astype(np.uint8)
    if C == 4:
        im[..., 3][rng.rand(v, h, w) < 0.2] = 0
        im[..., 3][rng.rand(v, h, w) < 0.2] = 255
    return im


def _batcher(images, N, error_map=False, grid=8, order=None):
    from pvd.batcher import DeviceBatcher
    from pvd.scene import synthetic_poses
    poses = torch.from_numpy(synthetic_poses(np.random.RandomState(0))[:images.shape[0]]).float()
    src = DeviceBatcher(torch.from_numpy(images).to(DEV), poses.to(DEV), INTR, [-1, -1, -1, 1, 1, 1.0], 0.2, N, SEED, error_map=error_map, grid=grid)
    if order is not None:
        src.order.copy_(torch.tensor(order, dtype=torch.int32))
    return src


def _check_rays(src, b):
    """rays and near/far: get_rays on the returned pixel ids + near_far_from_aabb (as test_make_ray_batch_matches_get_rays_and_near_far)."""
    import pvd_hip
    import raymarching
    N = src.num_rays
    fx, fy, cx, cy = src.intrinsics
    ro, rd = torch.empty(N, 3, device=DEV), torch.empty(N, 3, device=DEV)
    pvd_hip.get_rays(src.poses[int(b.view[0])].contiguous(), fx, fy, cx, cy, b.inds, src.W, N, ro, rd)
    assert torch.equal(b[0].view(N, 3), ro) and torch.equal(b[1].view(N, 3), rd)
    n2, f2 = raymarching.near_far_from_aabb(ro, rd, src.aabb, src.min_near)
    assert torch.equal(b.nears, n2) and torch.equal(b.fars, f2)
    assert bool((b.nears < 1e30).any())  # (some rays do meet the box)


def _check_against_restatement(src, images, b, position, counter, cells=None):
    want = R.image_batch(images, src.order.cpu().numpy(), position, counter, SEED, src.num_rays, src.grid, cells)
    assert int(b.view[0]) == want["view"]
    assert np.array_equal(b.inds.cpu().numpy(), want["inds"])
    assert np.array_equal(b[2].view(-1, 3).cpu().numpy(), want["gt"])
    if images.shape[-1] == 4:
        assert np.array_equal(b[3].view(-1, 3).cpu().numpy(), want["bg"])


@pytest.mark.parametrize("C", [4, 3])
def test_uniform_batches_are_the_restatements_and_walk_through_the_order(C):
    N, order = 100, [2, 0, 1]
    images = _images(C)
    src = _batcher(images, N, order=order)
    b = src.new_batch()
    if C == 3:
        assert torch.equal(b[3], torch.ones(1, N, 3, device=DEV))  # white, as training_target gives for RGB images
    for it in range(4):
        src.fill(b)
        assert src.state.tolist() == [(it + 1) % V, it + 1, 0]
        assert int(b.view[0]) == order[it % V]
        _check_against_restatement(src, images, b, it, it)
        _check_rays(src, b)
        if C == 3:
            assert torch.equal(b[3], torch.ones(1, N, 3, device=DEV))  # not touched
    assert b.inds_coarse is None
    src.shuffle(torch.Generator(device=DEV).manual_seed(1))
    assert sorted(src.order.tolist()) == list(range(V)) and src.order.dtype == torch.int32


# The keys against float64.  key = w / e, e = 0 - logf(1 - u):
#   1 - u is exact (u is a multiple of 2^-23 in [0, 1)) and so is 0 - x;
#   logf: 2 ulp, the figure of the single-precision table of the HIP math API reference in ROCm's documentation, which reports the
#   device library's error (the library takes the hardware's base-2 logarithm, 1 ulp by the ISA guide, and multiplies by ln 2 held
#   as two floats: v_log_f32, v_mul, two v_fma and one v_add in the kernel's code); an ulp is at most 2^-23 of the value, so the
#   relative error of e is at most 2 * 2^-23;
#   the division rounds to nearest: a further factor (1 + 2^-24).
# Together |key / key64 - 1| <= (1 + 2^-24) / (1 - 2^-22) - 1 < 2.5 * 2^-23 * (1 + 2^-20).
# (A first version of this bound took logf for 1 ulp, 1.5 * 2^-23 in all; the full-width case measured 1.52 * 2^-23 on the MI355X.)
KEY_REL_BOUND = 2.5 * 2.0 ** -23 * (1.0 + 2.0 ** -20)


def _weights(kind, v, G, seed=5):
    rng = np.random.RandomState(seed)
    if kind == "equal":
        return np.full((v, G), 0.37, np.float32)
    w = (0.01 + 20.0 * rng.rand(v, G) ** 3).astype(np.float32)
    if kind == "ten":  # only 10 positive cells per view: the rest of a batch comes from the zero keys, lowest cells first
        keep = np.zeros((v, G), bool)
        for i in range(v):
            keep[i, rng.choice(G, 10, replace=False)] = True
        w[~keep] = 0.0
        w[:, 1] = -3.0  # (not > 0: key 0 as well)
    return w


CASES = [("random", 8, H, W, 1), ("random", 8, H, W, 16), ("random", 8, H, W, 37), ("random", 8, H, W, 64),
         ("equal", 8, H, W, 16), ("ten", 8, H, W, 16), ("random", 128, 100, 100, 4096)]


@pytest.mark.parametrize("kind,g,h,w,N", CASES, ids=["%s-g%d-N%d" % (c[0], c[1], c[4]) for c in CASES])
def test_error_map_draw_keys_selection_and_pixels(kind, g, h, w, N):
    images = _images(4, V, h, w)
    src = _batcher(images, N, error_map=True, grid=g, order=[1, 2, 0])
    G = g * g
    assert torch.equal(src.error_map, torch.ones(V, G, device=DEV))  # provider.py:232-237
    weights = _weights(kind, V, G)
    src.error_map.copy_(torch.from_numpy(weights))
    b = src.new_batch()
    worst = 0.0
    for it in range(2):
        keys = torch.full((G,), -1.0, device=DEV)
        src.fill(b, keys_out=keys)
        view = int(b.view[0])
        assert view == [1, 2, 0][it] and src.state.tolist() == [it + 1, it + 1, 0]
        keys = keys.cpu().numpy()
        # arithmetic: the keys against the float64 restatement
        k64 = R.keys64(weights[view], R.cell_uniforms(SEED, it, G))
        finite = np.isfinite(k64) & (k64 > 0)
        assert np.array_equal(keys[~finite].astype(np.float64), k64[~finite])  # zeros (and +inf, should u be 0) exactly
        ratio = np.abs(keys[finite].astype(np.float64) / k64[finite] - 1.0)
        worst = max(worst, float(ratio.max()))
        assert ratio.max() <= KEY_REL_BOUND, (ratio.max(), KEY_REL_BOUND)
        # selection: exactly the N largest of the kernel's own keys, ties to the lower cell, ascending and distinct
        cells = b.inds_coarse.cpu().numpy()
        assert np.array_equal(cells, R.select(keys, N))
        assert (np.diff(cells) > 0).all() and cells[0] >= 0 and cells[-1] < G
        if kind == "ten":
            positive = np.flatnonzero(weights[view] > 0)
            rest = np.setdiff1d(np.arange(G), positive)[:N - len(positive)]
            assert np.array_equal(cells, np.sort(np.concatenate([positive, rest])))
        # pixels, ground truth and background follow from the cells exactly
        _check_against_restatement(src, images, b, it, it, cells)
        row, col = b.inds.cpu().numpy() // w, b.inds.cpu().numpy() % w
        assert (row * g // h <= cells // g).all() and (col * g // w <= cells % g).all()  # (inside its cell, up to the clamp at the edge)
        _check_rays(src, b)
    print("largest |key / key64 - 1| = %.3g (%.2f of the bound %.3g)" % (worst, worst / KEY_REL_BOUND, KEY_REL_BOUND))
    assert torch.equal(src.error_map, torch.from_numpy(weights).to(DEV))  # the draw only reads the map


def test_error_map_update_is_update_error_map_and_touches_nothing_else():
    import pvd_hip
    from pvd.scene import update_error_map
    g, N, view = 8, 37, 1
    G = g * g
    rng = np.random.RandomState(9)
    emap = (rng.rand(V, G) * 3).astype(np.float32)
    cells = np.sort(rng.choice(G, N, replace=False)).astype(np.int64)
    pred, gt = rng.rand(N, 3).astype(np.float32), rng.rand(N, 3).astype(np.float32)
    dmap = torch.from_numpy(emap).to(DEV)
    pvd_hip.error_map_update(dmap, torch.tensor([view], dtype=torch.int32, device=DEV), torch.from_numpy(cells).to(DEV),
                             torch.from_numpy(pred).to(DEV), torch.from_numpy(gt).to(DEV), N)
    got = dmap.cpu().numpy()
    err = ((torch.from_numpy(pred) - torch.from_numpy(gt)) ** 2).mean(-1)[None]
    want = update_error_map(torch.from_numpy(emap[view:view + 1].copy()), torch.from_numpy(cells)[None], err)[0].numpy()
    assert (np.abs(got[view, cells] - want[cells]) <= 2 * np.spacing(np.abs(want[cells]))).all()
    assert np.array_equal(got[view, cells], R.ema(emap[view, cells], pred, gt))  # (the restatement has the kernel's operation order)
    untouched = np.ones((V, G), bool)
    untouched[view, cells] = False
    assert np.array_equal(got[untouched], emap[untouched])


def test_device_batcher_refuses_what_the_kernels_cannot_take():
    from pvd.batcher import DeviceBatcher
    poses = torch.eye(4, device=DEV).repeat(V, 1, 1)
    im = torch.from_numpy(_images(4)).to(DEV)
    with pytest.raises(ValueError):
        DeviceBatcher(im.float(), poses, INTR, [-1, -1, -1, 1, 1, 1.0], 0.2, 16, 0)
    with pytest.raises(ValueError):
        DeviceBatcher(im, poses, INTR, [-1, -1, -1, 1, 1, 1.0], 0.2, 65, 0, error_map=True, grid=8)
    with pytest.raises(ValueError):
        DeviceBatcher(im, poses, INTR, [-1, -1, -1, 1, 1, 1.0], 0.2, 16, 0, error_map=True, grid=129)
    src = DeviceBatcher(im, poses, INTR, [-1, -1, -1, 1, 1, 1.0], 0.2, 16, 0)
    src.feedback(src.fill(src.new_batch()), torch.zeros(1, 16, 3, device=DEV))  # no map: nothing to do
    assert src.error_map is None and src.state.tolist() == [1, 1, 0]


# ---------------------------------------------------------------- inside the recorded 16-step block (a child interpreter records the graphs)
@pytest.fixture(scope="module")
def block_run(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("databatch") / "block.npz")
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "databatch_block_child.py")
    proc = subprocess.run([sys.executable, child, out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert proc.returncode == 0, proc.stdout.decode(errors="replace")[-6000:]
    return dict(np.load(out))


def _block_checks(d, name, error_map):
    import databatch_block_child as child
    g = lambda k: d["%s_%s" % (name, k)]
    images, order = g("images"), g("order")
    nV = images.shape[0]
    assert g("state_eager").tolist() == [16 % nV, 16, 0] and np.array_equal(g("state_captured"), g("state_eager"))
    assert g("state").tolist() == [48 % nV, 48, 0] and int(g("global_step")) == 48  # 32 batches beyond the eager block
    assert np.isfinite(g("losses")).all() and len(g("losses")) == 18
    for k in range(16):
        counter = 32 + k  # the second replay's batches
        cells = g("cells%d" % k) if error_map else None
        want = R.image_batch(images, order, counter % nV, counter, child.SEED, child.N, child.GRID, cells)
        assert int(g("view%d" % k)[0]) == want["view"] == int(order[counter % nV]), k
        assert np.array_equal(g("inds%d" % k), want["inds"]), k
        assert np.array_equal(g("bg%d" % k), want["bg"]) and np.array_equal(g("gt%d" % k), want["gt"]), k
        if error_map:
            assert (np.diff(cells) > 0).all() and cells[0] >= 0 and cells[-1] < child.GRID ** 2


def test_recorded_block_draws_fresh_uniform_batches(block_run):
    _block_checks(block_run, "uniform", False)


def test_recorded_block_draws_by_the_error_map_and_feeds_it_back(block_run):
    d = block_run
    _block_checks(d, "errmap", True)
    emap, before, drawn = d["errmap_map"], d["errmap_map_before"], d["errmap_drawn"]
    assert drawn.any() and (emap[~drawn] == 1.0).all()  # only cells some batch drew have moved
    assert (emap[drawn] != 1.0).mean() > 0.99
    # the last recorded step: its cells hold the EMA of what they held before the replay (no other step of the replay drew from
    # this view: 17 views, 16 steps) and the error of the prediction read back
    view, cells = int(d["errmap_view15"][0]), d["errmap_cells15"]
    want = R.ema(before[view, cells], d["errmap_pred"], d["errmap_gt15"])
    assert (np.abs(emap[view, cells] - want) <= 2 * np.spacing(np.abs(want))).all()
    views = [int(d["errmap_view%d" % k][0]) for k in range(16)]
    assert len(set(views)) == 16
