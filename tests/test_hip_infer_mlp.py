"""The inference render of a frozen `mlp` (NeRF trunk) model three ways -- the reference-shaped host loop with one read-back per round
(distill_mutual/renderer.py:450-543), the rounds with their state on the device (NeRFRenderer._run_rounds_device over
pvd_mlp_head_forward_fused_rows) and ONE persistent launch (pvd_infer_image_mlp, include/pvd_hip_mlp.h).  A sample's value is one column
of Y^T = W X^T and a ray's sums depend on nothing but the ray: the persistent image must be the host loop's bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _mlp_model(seed=3, scene_scale=1.0, **cfg):
    """An `mlp` model with non-zero biases (nn.Linear's) whose weights are scaled so that a render has something to compare: the default
    initialisation shrinks the signal by ~0.4 per ReLU layer (trunk matrices x 2.3 keep activations O(1): finite in f16), and the
    sigma / colour heads are widened so that log-sigma spans its clamp [-2, 7] (rays both saturated and semi-transparent)."""
    from pvd.config import PVDConfig
    from pvd.ops import hip_ops
    from pvd.scene import ChairScene
    from pvd.workload import install_occupancy, make_model
    torch.manual_seed(seed)
    opt = PVDConfig(model_type="mlp", resolution0=64, **cfg)
    opt.stage_iters = {"stage1": -1, "stage2": -1}
    m = make_model(hip_ops(), opt, "mlp", False, torch.device(DEV))
    with torch.no_grad():
        for layer in m.nerf_mlp:
            layer.weight.mul_(2.3)
            assert layer.bias.abs().max().item() > 0
        for layer in m.sigma_net:
            layer.weight.mul_(6.0)
        for layer in m.color_net:
            layer.weight.mul_(3.0)
    install_occupancy(m, ChairScene(scale=scene_scale), opt)
    return m.eval()


def _rays(n, full_image=False):
    from pvd.scene import BLENDER_INTRINSICS, get_rays, synthetic_poses
    poses = torch.from_numpy(synthetic_poses(np.random.RandomState(2))).to(DEV)
    if full_image:  # every pixel of a 200 x 200 view (same field of view): most rays miss the object, some cross all of it
        r = get_rays(poses[9][None], (277.775, 277.775, 100.0, 100.0), 200, 200, -1)
    else:
        r = get_rays(poses[9][None], BLENDER_INTRINSICS, 800, 800, n, generator=torch.Generator(device=DEV).manual_seed(8))
    return r["rays_o"], r["rays_d"]


def _render(m, o, d, mode, monkeypatch, max_steps=1024, dt_gamma=0):
    """mode: "host" (the reference-shaped loop), "device" (round state on the device) or "persistent" (one launch).  Asserts that the
    requested path -- and no other -- was TAKEN, through what each path leaves on the model."""
    monkeypatch.setenv("PVD_INFER_PERSISTENT", "1" if mode == "persistent" else "0")
    monkeypatch.setenv("PVD_INFER_DEVICE_ROUNDS", "0" if mode == "host" else "1")
    for k in ("_last_infer_workspace", "_last_rounds"):
        m.__dict__.pop(k, None)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        out = m.render(o, d, staged=False, bg_color=1, perturb=False, dt_gamma=dt_gamma, max_steps=max_steps)
    assert hasattr(m, "_last_infer_workspace") == (mode == "persistent"), mode
    assert hasattr(m, "_last_rounds") == (mode == "device"), mode
    return out["image"].float(), out["depth"].float()


def _assert_same_bits(a, b):
    (img0, dep0), (img1, dep1) = a, b
    assert torch.isfinite(img0).all() and torch.isfinite(img1).all()
    assert torch.equal(img0, img1), (img0 - img1).abs().max().item()
    assert torch.equal(torch.isnan(dep0), torch.isnan(dep1)) and torch.equal(torch.nan_to_num(dep0), torch.nan_to_num(dep1))


def _persistent_is_the_round_loop(m, monkeypatch):
    """test 1's comparison: 5000 random rays of an 800 x 800 view and every pixel of a 200 x 200 view, all-miss rays, the first render again"""
    for full_image in (False, True):
        o, d = _rays(5000, full_image)
        host = _render(m, o, d, "host", monkeypatch)
        pers = _render(m, o, d, "persistent", monkeypatch)
        assert host[0].std().item() > 0.02
        _assert_same_bits(host, pers)
        miss = _render(m, o + 100.0, d, "persistent", monkeypatch)[0]
        assert torch.equal(miss, torch.ones_like(miss))  # all background
        _assert_same_bits(pers, _render(m, o, d, "persistent", monkeypatch))  # the caches of the first call serve the next
    return host


def test_persistent_mlp_render_is_the_round_loops_image(monkeypatch):
    m = _mlp_model()
    assert len(m.nerf_mlp) == 8 and m.skips == 3
    o, d = _rays(5000)
    img, _ = _persistent_is_the_round_loop(m, monkeypatch)
    # the model is worth comparing on: rays that saturate and rays that stay semi-transparent (white background, weights_sum = 1 - T)
    monkeypatch.setenv("PVD_INFER_PERSISTENT", "1")
    from pvd.ops import hip_ops
    rm = hip_ops().raymarching
    oo, dd = o.contiguous().view(-1, 3), d.contiguous().view(-1, 3)
    nears, fars = rm.near_far_from_aabb(oo, dd, m.aabb_infer, m.min_near)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        ws, _, _ = hip_ops().fused_head.mlp_infer_image(m, oo, dd, nears, fars, 0, 1024)
    assert (ws > 1 - 1e-4).sum().item() > 20 and ((ws > 0.05) & (ws < 0.95)).sum().item() > 20


@pytest.mark.parametrize("num,skip", [(5, 1), (5, 2), (5, 0)])
def test_persistent_mlp_render_of_other_layer_structures(num, skip, monkeypatch):
    """n_before / n_after = 1 / 1, 2 / 0 (no hidden layer behind the skip layer) and 0 / 2 (the skip layer follows the first)"""
    m = _mlp_model(nerf_layer_num=num, skip=skip)
    from pvd.ops import hip_ops
    assert hip_ops().fused_head.mlp_supported(m) and len(m.nerf_mlp) - 3 - m.skips == {1: 1, 2: 0, 0: 2}[skip]
    _persistent_is_the_round_loop(m, monkeypatch)


@pytest.mark.parametrize("n_rays,shuffle", [(1, 7919), (63, 7919), (2 * 7919, 7919), (777, 1)])
def test_persistent_mlp_render_renders_every_ray_once(n_rays, shuffle, monkeypatch):
    m = _mlp_model()
    o, d = _rays(n_rays)
    monkeypatch.setenv("PVD_INFER_SHUFFLE", str(shuffle))
    _assert_same_bits(_render(m, o, d, "host", monkeypatch), _render(m, o, d, "persistent", monkeypatch))


def test_persistent_mlp_render_of_a_whole_400x400_view(monkeypatch):
    from pvd.scene import get_rays, synthetic_poses
    m = _mlp_model()
    poses = torch.from_numpy(synthetic_poses(np.random.RandomState(2))).to(DEV)
    r = get_rays(poses[40][None], (555.55, 555.55, 200.0, 200.0), 400, 400, -1)
    host = _render(m, r["rays_o"], r["rays_d"], "host", monkeypatch)
    pers = _render(m, r["rays_o"], r["rays_d"], "persistent", monkeypatch)
    assert host[0].numel() == 3 * 160000
    assert host[0].std().item() > 0.02
    _assert_same_bits(host, pers)
    queued = int(m._last_infer_workspace[0])
    rounds, rows, walk_only, workgroups = m._last_infer_workspace[-10:-6].tolist()
    print("mlp 400x400: rays queued %d, workgroups %d, local rounds %d (walk-only %d), rows shaded %d, rows per shading round %.1f of 192"
          % (queued, workgroups, rounds, walk_only, rows, rows / max(rounds - walk_only, 1)))
    assert workgroups >= 100 and rows > queued > 0


def test_persistent_mlp_render_with_two_cascades_and_a_growing_step(monkeypatch):
    """bound 2 (two cascades of the occupancy grid; positions up to +-2 into the encoding) and dt_gamma = 1/256"""
    m = _mlp_model(seed=4, scene_scale=1.9, bound=2.0, dt_gamma=1.0 / 256)
    o, d = _rays(4096)
    o = o * 1.9
    host = _render(m, o, d, "host", monkeypatch, dt_gamma=1.0 / 256)
    pers = _render(m, o, d, "persistent", monkeypatch, dt_gamma=1.0 / 256)
    assert host[0].std().item() > 0.02
    _assert_same_bits(host, pers)


def test_persistent_mlp_render_with_a_small_step_budget_differs_from_the_rounds_only_as_documented(monkeypatch):
    """include/pvd_hip_mlp.h: the round loop stops ALL rays once the rounds' n_step add up to max_steps, the persistent render stops a
    ray after ITS OWN max_steps samples.  Rays that end before either cap must agree bit for bit."""
    m = _mlp_model()
    o, d = _rays(3000)
    full_r, full_p = _render(m, o, d, "host", monkeypatch)[0], _render(m, o, d, "persistent", monkeypatch)[0]
    assert torch.equal(full_r, full_p)
    cap_r, cap_p = _render(m, o, d, "host", monkeypatch, max_steps=24)[0], _render(m, o, d, "persistent", monkeypatch, max_steps=24)[0]
    # the round loop alone already separates the two groups on this model (two renders, 24 against 1024 steps)
    assert (cap_r == full_r).all(-1).float().mean().item() > 0.3 and (cap_r != full_r).any()
    done_early = (cap_r == full_r).all(-1) & (cap_p == full_p).all(-1)  # rays neither cap touched
    print("small budget: done early %.4f of %d rays" % (done_early.float().mean().item(), done_early.numel()))
    assert done_early.float().mean().item() > 0.3 and (~done_early).any()
    assert torch.equal(cap_r[done_early], cap_p[done_early])
    for cap in (cap_r, cap_p):
        assert ((cap - full_r)[~done_early].abs().max().item()) > 0
    assert torch.isfinite(cap_p).all()


@pytest.mark.parametrize("full_image", [False, True])
def test_device_rounds_of_the_mlp_model_match_the_host_synchronised_loop(full_image, monkeypatch):
    m = _mlp_model()
    o, d = _rays(3000, full_image)
    (img0, dep0) = _render(m, o, d, "host", monkeypatch)
    (img1, dep1) = _render(m, o, d, "device", monkeypatch)
    assert m._last_rounds > 3  # the device loop ran (several rounds, no per-round read-back)
    assert torch.isfinite(img1).all() and img0.std().item() > 0.02
    assert (img0 - img1).abs().max().item() <= 1e-5
    assert torch.equal(torch.isnan(dep0), torch.isnan(dep1))
    assert (torch.nan_to_num(dep0) - torch.nan_to_num(dep1)).abs().max().item() <= 1e-5


def _plain_launch_inputs(m, M):
    import fusedhead
    import pvd_hip
    g = torch.Generator(device=DEV).manual_seed(11)
    x = torch.rand(M, 3, device=DEV, generator=g) * 2 - 1
    dirs = torch.nn.functional.normalize(torch.randn(M, 3, device=DEV, generator=g), dim=-1).contiguous()
    enc = m.encoder_nerf_pe
    pts = pvd_hip.freq_encode(x, enc.freq_bands, enc.include_input, torch.float16, 64)
    ws = [l.weight.detach().contiguous() for l in (m.sigma_net[0], m.sigma_net[1], m.color_net[0], m.color_net[1], m.color_net[2])]
    return pts, fusedhead.mlp_weight_stream(m), m.skips, len(m.nerf_mlp) - 3 - m.skips, dirs, ws


def test_plain_mlp_launch_takes_a_device_side_row_count():
    """pvd_mlp_head_forward_fused_rows: rows below *rows_dev are the plain launch's, bit for bit; rows at and above it are not written"""
    import pvd_hip
    m = _mlp_model()
    M = 20011
    pts, stream, nb, na, dirs, ws = _plain_launch_inputs(m, M)
    a = m.args
    f = lambda *s: torch.full(s, -777.0, device=DEV)
    ref = (f(M), f(M, 3), f(M, 16))
    pvd_hip.mlp_head_forward_fused(pts, stream, nb, na, dirs, M, *ws, a.sigma_clip_min, a.sigma_clip_max, *ref)
    assert all(torch.isfinite(t).all() and not (t == -777.0).any() for t in ref)
    for count in (0, 1, 47, 48, 191, 192, 193, M):
        out = (f(M), f(M, 3), f(M, 16))
        rows_dev = torch.tensor([count], dtype=torch.int32, device=DEV)
        pvd_hip.mlp_head_forward_fused(pts, stream, nb, na, dirs, M, *ws, a.sigma_clip_min, a.sigma_clip_max, *out, rows_dev=rows_dev)
        for got, want in zip(out, ref):
            assert torch.equal(got[:count], want[:count]), count
            assert (got[count:] == -777.0).all(), count
    # a count beyond M is clamped to M
    out = (f(M), f(M, 3), f(M, 16))
    pvd_hip.mlp_head_forward_fused(pts, stream, nb, na, dirs, M, *ws, a.sigma_clip_min, a.sigma_clip_max, *out,
                                   rows_dev=torch.tensor([M + 500], dtype=torch.int32, device=DEV))
    assert all(torch.equal(g, w) for g, w in zip(out, ref))


def test_persistent_mlp_render_follows_weights_changed_in_place(monkeypatch):
    """the weight stream and the head's weight image are cached on the model: keyed so that an in-place change is seen"""
    m = _mlp_model()
    o, d = _rays(3000)
    before = _render(m, o, d, "persistent", monkeypatch)
    with torch.no_grad():
        m.nerf_mlp[2].weight[:, 7] += 0.25   # a trunk weight column
        m.nerf_mlp[5].bias[:64] -= 0.2       # biases
        m.color_net[1].weight[3] *= -2.0     # a head weight row
    after = _render(m, o, d, "persistent", monkeypatch)
    assert not torch.equal(before[0], after[0])
    fresh = _mlp_model()  # a fresh model carrying the changed weights, rendered by the host loop
    fresh.load_state_dict(m.state_dict())
    _assert_same_bits(_render(fresh, o, d, "host", monkeypatch), after)


@pytest.mark.parametrize("case", ["wide128", "pe6", "fused_off"])
def test_models_outside_the_supported_structure_keep_the_host_loop(case, monkeypatch):
    cfg = {"wide128": dict(nerf_layer_wide=128), "pe6": dict(PE=6), "fused_off": {}}[case]
    if case == "fused_off":
        monkeypatch.setenv("PVD_MLP_FUSED", "0")
    m = _mlp_model(**cfg)
    assert not m.supports_device_rows()
    o, d = _rays(1500)
    monkeypatch.setenv("PVD_INFER_PERSISTENT", "1")
    monkeypatch.setenv("PVD_INFER_DEVICE_ROUNDS", "1")
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        img = m.render(o, d, staged=False, bg_color=1, perturb=False, dt_gamma=0, max_steps=1024)["image"].float()
    assert torch.isfinite(img).all()
    assert not hasattr(m, "_last_infer_workspace") and not hasattr(m, "_last_rounds")  # neither new path was entered


def test_mlp_entry_points_reject_bad_arguments_without_a_launch():
    import pvd_hip
    m = _mlp_model()
    M = 64
    pts, stream, nb, na, dirs, ws = _plain_launch_inputs(m, M)
    a = m.args
    f = lambda *s: torch.full(s, -777.0, device=DEV)
    out = (f(M), f(M, 3), f(M, 16))
    one = torch.ones(1, dtype=torch.int32, device=DEV)
    with pytest.raises(pvd_hip.PvdHipError):  # a stream of the wrong length for the stated layer structure
        pvd_hip.mlp_head_forward_fused(pts, stream[:-8].contiguous(), nb, na, dirs, M, *ws, a.sigma_clip_min, a.sigma_clip_max, *out, rows_dev=one)
    with pytest.raises(pvd_hip.PvdHipError):  # ... or the structure misstated
        pvd_hip.mlp_head_forward_fused(pts, stream, nb + 1, na, dirs, M, *ws, a.sigma_clip_min, a.sigma_clip_max, *out, rows_dev=one)
    with pytest.raises(pvd_hip.PvdHipError):  # the row count must be a device int32
        pvd_hip.mlp_head_forward_fused(pts, stream, nb, na, dirs, M, *ws, a.sigma_clip_min, a.sigma_clip_max, *out, rows_dev=one.long())
    # the persistent render
    N = 32
    o, d = _rays(N)
    o, d = o.contiguous().view(-1, 3), d.contiguous().view(-1, 3)
    from pvd.ops import hip_ops
    nears, fars = hip_ops().raymarching.near_far_from_aabb(o, d, m.aabb_infer, m.min_near)
    acc = (f(N), f(N), f(N, 3))
    wsp = torch.zeros(2 * N + 12, dtype=torch.int32, device=DEV)
    bands = [float(b) for b in m.encoder_nerf_pe.freq_bands]
    call = lambda bands=bands, stream=stream, wsp=wsp, nb=nb: pvd_hip.infer_image_mlp(
        o, d, nears, fars, m.density_bitfield, float(m.bound), 0.0, 1024, int(m.cascade), int(m.grid_size), float(m.density_scale), bands, stream,
        nb, na, *ws, a.sigma_clip_min, a.sigma_clip_max, wsp, *acc)
    with pytest.raises(pvd_hip.PvdHipError):  # n_freqs != 10: PVD_ERR_UNSUPPORTED from the library
        call(bands=bands[:6])
    with pytest.raises(pvd_hip.PvdHipError):
        call(stream=stream[:-8].contiguous())
    with pytest.raises(pvd_hip.PvdHipError):
        call(wsp=wsp[:2 * N])
    with pytest.raises(pvd_hip.PvdHipError):
        call(nb=nb + 1)
    # NULL pointers reach the library's own checks only through the raw symbol: PVD_ERR_INVALID
    u32, f32, vp = ctypes.c_uint32, ctypes.c_float, ctypes.c_void_p
    p = lambda t: vp(t.data_ptr())
    cb = (ctypes.c_float * 10)(*bands)
    raw = lambda wstream: pvd_hip._lib.pvd_infer_image_mlp(
        p(o), p(d), p(nears), p(fars), u32(N), p(m.density_bitfield), f32(1.0), f32(0.0), u32(1024), u32(1), u32(128), f32(1.0), cb, u32(10), wstream,
        u32(nb), u32(na), p(ws[0]), p(ws[1]), p(ws[2]), p(ws[3]), p(ws[4]), vp(0), f32(-2.0), f32(7.0), p(wsp), p(acc[0]), p(acc[1]), p(acc[2]), vp(0))
    assert raw(vp(0)) == -1
    torch.cuda.synchronize()
    assert all((t == -777.0).all() for t in out + acc) and int(wsp.abs().sum()) == 0  # nothing was launched
