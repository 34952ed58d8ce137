"""The student-independent prefix of G steps in one launch per stage (include/pvd_hip_prefix.h) is, segment by segment, bit for bit
what G sequential single-step launches produce (GPU).  Everything in the prefix is deterministic -- integer slot allocation, no float
atomics -- so every comparison is torch.equal on the bit patterns.

* batches: G = 3, N = 64 rays, V = 5 poses, starting at pose 4 (wraps): rays, background, near/far and the device state afterwards.
* march: the 128^3 bitfield of the chair, N = 64, G = 3; one segment's budget below its sample count (its trailing rays drop, the
  others are untouched), one segment aimed away from the box (no samples), perturb on / off, fresh and pre-zeroed outputs.
* boundary: G = 257 segments of 64 rays = 16 448 rays, past the 16 384 rays one single launch's record path takes.
* teacher forward + compositing over G = 3 slices of M = 256 rows (padded rows and dropped rays included) against per-slice launches.
* whole step: vm student, 256 rays, 4 steps per graph recorded back to back, G in {2, 4} against the G = 1 recording: rays, samples and
  the teacher's image and feature rows of all 8 replayed steps and the student's ring of step counters bit for bit; loss and parameters within the bars
  tests/test_hip_amp_parity.py uses for graph replay against eager (the table scatter's float atomics are unordered in both)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N, G3 = 64, 3


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _workload(num_rays=256, **kw):
    from pvd.config import PVDConfig
    from pvd.ops import hip_ops
    from pvd.workload import DistillWorkload
    opt = PVDConfig(num_rays=num_rays, resolution0=64, iters=300, model_type="vm", **kw)
    torch.cuda.manual_seed(1234)
    return DistillWorkload(hip_ops(), torch.device(DEV), opt, teacher_pretrain_steps=0, seed=0)


@pytest.fixture(scope="module")
def scene():
    """One workload for the kernel-level tests: the chair's 128^3 bitfield and coarse mask, cameras, a hash teacher off its initialisation."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import pvd_hip
    w = _workload()
    g = torch.Generator(device=DEV).manual_seed(5)
    with torch.no_grad():
        w.tea.encoder.embeddings.copy_((torch.rand(w.tea.encoder.embeddings.shape, device=DEV, generator=g) - 0.5) * 0.6)
    pvd_hip.note_weights_changed(list(w.tea.parameters()))
    assert w.tea.grid_size == 128
    return w


def _batch_args(w, V=5):
    from pvd.scene import BLENDER_INTRINSICS
    return w.poses[:V].float().contiguous(), BLENDER_INTRINSICS, w.stu.aabb_train, w.stu.min_near


def _group_batch(w, G, n=N, start=(4, 7, 0), seed=0x5eed):
    import pvd_hip
    poses, (fx, fy, cx, cy), aabb, min_near = _batch_args(w)
    state = torch.tensor(start, dtype=torch.int64, device=DEV)
    f = lambda *s: torch.full(s, 7.0, dtype=torch.float32, device=DEV)
    out = dict(inds=torch.full((G, n), -1, dtype=torch.int64, device=DEV), rays_o=f(G, n, 3), rays_d=f(G, n, 3), bg=f(G, n, 3), nears=f(G, n), fars=f(G, n))
    pvd_hip.make_ray_batch_group(poses, state, seed, fx, fy, cx, cy, 800, 800, n, G, aabb, min_near, *out.values())
    return out, state


def test_batches_of_a_group_are_the_sequential_batches(scene):
    import pvd_hip
    w = scene
    grp, gstate = _group_batch(w, G3)
    poses, (fx, fy, cx, cy), aabb, min_near = _batch_args(w)
    state = torch.tensor([4, 7, 0], dtype=torch.int64, device=DEV)
    for j in range(G3):
        f = lambda *s: torch.full(s, 9.0, dtype=torch.float32, device=DEV)
        one = dict(inds=torch.full((N,), -1, dtype=torch.int64, device=DEV), rays_o=f(N, 3), rays_d=f(N, 3), bg=f(N, 3), nears=f(N), fars=f(N))
        pvd_hip.make_ray_batch(poses, state, 0x5eed, fx, fy, cx, cy, 800, 800, N, aabb, min_near, *one.values())
        for k, v in one.items():
            assert _same(grp[k][j], v), (j, k)
    assert torch.equal(gstate, state) and state.tolist() == [(4 + G3) % 5, 7 + G3, 0]
    assert not _same(grp["rays_o"][0], grp["rays_o"][1])  # (pose 4, then pose 0)


def _march_single(w, o, d, nears, fars, M, perturb, fresh, budget, mask):
    import pvd_hip
    tea = w.tea
    fill = (lambda *s: torch.full(s, 3.0, device=DEV)) if fresh else (lambda *s: torch.zeros(*s, device=DEV))
    xyzs, dirs, deltas = fill(M, 3), fill(M, 3), fill(M, 2)
    rays = torch.full((o.shape[0], 3), -5, dtype=torch.int32, device=DEV)
    counter = torch.full((2,), 11 if fresh else 0, dtype=torch.int32, device=DEV)
    pvd_hip.march_rays_train(o.contiguous(), d.contiguous(), tea.density_bitfield, tea.bound, 0.0, 1024, o.shape[0], tea.cascade, tea.grid_size, M,
                             nears.contiguous(), fars.contiguous(), xyzs, dirs, deltas, rays, counter, perturb, fresh=fresh, budget_dev=budget,
                             coarse_mask=mask)
    return dict(xyzs=xyzs, dirs=dirs, deltas=deltas, rays=rays, counter=counter)


def _march_group(w, b, G, M, perturb, fresh, budget, mask, n=N):
    import pvd_hip
    tea = w.tea
    fill = (lambda *s: torch.full(s, 5.0, device=DEV)) if fresh else (lambda *s: torch.zeros(*s, device=DEV))
    xyzs, dirs, deltas = fill(G * M, 3), fill(G * M, 3), fill(G * M, 2)
    rays = torch.full((G, n, 3), -9, dtype=torch.int32, device=DEV)
    counter = torch.full((G, 2), 13 if fresh else 0, dtype=torch.int32, device=DEV)
    pvd_hip.march_rays_train_group(b["rays_o"], b["rays_d"], tea.density_bitfield, tea.bound, 0.0, 1024, n, G, tea.cascade, tea.grid_size, M,
                                   b["nears"], b["fars"], xyzs, dirs, deltas, rays, counter, perturb, fresh=fresh, budget_dev=budget, coarse_mask=mask)
    return dict(xyzs=xyzs.view(G, M, 3), dirs=dirs.view(G, M, 3), deltas=deltas.view(G, M, 2), rays=rays, counter=counter)


def _away(w, b, j):
    """Segment j looks away from the box: no ray of it has a sample."""
    import pvd_hip
    b["rays_d"][j] = -b["rays_d"][j]
    pvd_hip.near_far_from_aabb(b["rays_o"][j], b["rays_d"][j], w.stu.aabb_train, N, w.stu.min_near, b["nears"][j], b["fars"][j])


@pytest.mark.parametrize("fresh", [True, False], ids=["fresh", "zeroed"])
@pytest.mark.parametrize("perturb", [True, False], ids=["perturb", "noperturb"])
def test_march_segments_are_the_sequential_marches(scene, perturb, fresh):
    w = scene
    M = 2048
    b, _ = _group_batch(w, G3)
    _away(w, b, 1)
    mask = w.tea.coarse_mask()
    full = _march_group(w, b, G3, M, perturb, True, None, mask)
    counts = full["counter"][:, 0].tolist()
    assert counts[0] > 256 and counts[1] == 0 and counts[2] > 256 and max(counts) < M, counts
    budget = torch.tensor([M, M, counts[2] // 2], dtype=torch.int32, device=DEV)  # segment 2 drops its trailing rays
    grp = _march_group(w, b, G3, M, perturb, fresh, budget, mask)
    for j in range(G3):
        one = _march_single(w, b["rays_o"][j], b["rays_d"][j], b["nears"][j], b["fars"][j], M, perturb, fresh, budget[j:j + 1], mask)
        for k, v in one.items():
            assert _same(grp[k][j], v), (j, k)
    r2 = grp["rays"][2]
    dropped = (r2[:, 2] > 0) & (r2[:, 1] + r2[:, 2] >= counts[2] // 2)
    assert bool(dropped.any()) and _same(grp["xyzs"][0], full["xyzs"][0]) and _same(grp["rays"][0], full["rays"][0])
    # one budget for every segment (stride 0) is the single call's one device budget
    b1 = budget[2:3].clone()
    grp1 = _march_group(w, b, G3, M, perturb, fresh, b1, mask)
    one = _march_single(w, b["rays_o"][0], b["rays_d"][0], b["nears"][0], b["fars"][0], M, perturb, fresh, b1, mask)
    assert all(_same(grp1[k][0], v) for k, v in one.items())


def test_march_group_past_the_single_launch_boundary(scene):
    w = scene
    G, M = 257, 2048
    assert G * N == 16448 > 16384
    b, _ = _group_batch(w, G)
    mask = w.tea.coarse_mask()
    grp = _march_group(w, b, G, M, True, True, None, mask)
    for j in (0, 128, 256):
        one = _march_single(w, b["rays_o"][j], b["rays_d"][j], b["nears"][j], b["fars"][j], M, True, True, None, mask)
        for k, v in one.items():
            assert _same(grp[k][j], v), (j, k)
    assert int(grp["counter"][:, 0].min()) > 0 and grp["counter"][:, 1].tolist() == [N] * G


def test_teacher_forward_and_compositing_over_slices(scene):
    import pvd_hip
    w = scene
    tea = w.tea.train()
    w.opt.global_step = w.opt.stage_iters["stage2"]  # (stage 3: the forward returns densities and colours)
    M = 256  # (below a batch's sample count: trailing rays dropped, tail rows cleared -- the padded rows the teacher still computes)
    b, _ = _group_batch(w, G3)
    grp = _march_group(w, b, G3, M, True, True, None, tea.coarse_mask())
    xyzs, dirs, deltas = grp["xyzs"].reshape(-1, 3), grp["dirs"].reshape(-1, 3), grp["deltas"].reshape(-1, 2)
    names = ("feature_sigma_color", "sigma_l", "color_l")
    with torch.autocast("cuda", dtype=torch.float16), torch.no_grad():
        sig, rgb = tea(xyzs, dirs)
        attrs = {k: getattr(tea, k) for k in names}
        sig, rgb = sig.float().contiguous(), rgb.float().contiguous()
        ws, depth, image = (torch.full((G3, N, c), 2.0, device=DEV).squeeze(-1) for c in (1, 1, 3))
        pvd_hip.composite_rays_train_bg_forward_group(sig, rgb, deltas, grp["rays"], M, N, G3, b["bg"], 0.0, b["nears"], b["fars"], 1e-6, ws, depth, image)
        for j in range(G3):
            sl = slice(j * M, (j + 1) * M)
            s1, c1 = tea(xyzs[sl].contiguous(), dirs[sl].contiguous())
            assert _same(sig[sl], s1.float()) and _same(rgb[sl], c1.float()), j
            for k in names:
                assert _same(attrs[k][sl].float(), getattr(tea, k).float()), (j, k)
            w1, d1, i1 = (torch.full((N, c), 4.0, device=DEV).squeeze(-1) for c in (1, 1, 3))
            pvd_hip.composite_rays_train_bg_forward(s1.float().contiguous(), c1.float().contiguous(), deltas[sl].contiguous(), grp["rays"][j].contiguous(), M, N,
                                                    b["bg"][j].contiguous(), 0.0, b["nears"][j].contiguous(), b["fars"][j].contiguous(), 1e-6, w1, d1, i1)
            assert _same(ws[j], w1) and _same(depth[j], d1) and _same(image[j], i1), j
    assert float(ws.max()) > 0.0


def _recorded_run(monkeypatch, G, steps_per_graph=4, replays=2):
    """8 replayed steps of a back-to-back recording with groups of G; returns what every step marched and what the teacher made of it."""
    monkeypatch.setenv("PVD_FORKED_GRAPHS", "0")
    monkeypatch.setenv("PVD_PREFIX_GROUP", str(G))
    w = _workload()
    tr, stu = w.trainer, w.stu
    seen = []
    render, closs = stu.render, tr.compute_loss

    def render_spy(rays_o, rays_d, **kw):
        out = render(rays_o, rays_d, **kw)
        seen.append(dict(rays_o=rays_o, rays_d=rays_d, **dict(zip(("xyzs", "dirs", "deltas", "rays"), out["inherited_params"]))))
        return out

    def closs_spy(*a, **kw):
        res = closs(*a, **kw)
        seen[-1].update(pred_tea=res[3], tea_fea=w.tea.feature_sigma_color)
        return res
    stu.render, tr.compute_loss = render_spy, closs_spy
    p0 = torch.cat([p.detach().float().reshape(-1) for p in stu.parameters() if p.requires_grad]).clone()
    w.enable_graph(steps_per_graph=steps_per_graph)
    assert getattr(tr, "prefix_group", 1) == G and not getattr(tr, "pipelined_ingraph", False)
    static = seen[-steps_per_graph:]  # (the recorded steps' tensors: kept alive here, so the pool does not hand their memory on)
    steps, losses = [], []
    for _ in range(replays):
        losses.append(float(w.step()[0]))
        torch.cuda.synchronize()
        steps += [{k: v.detach().clone().reshape(-1) for k, v in s.items()} for s in static]
    getattr(stu, "_pvd_flush_params", lambda: None)()
    p1 = torch.cat([p.detach().float().reshape(-1) for p in stu.parameters() if p.requires_grad])
    return steps, np.array(losses), p0, p1, stu.step_counter.detach().clone()


@pytest.fixture(scope="module")
def per_step_recording():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    mp = pytest.MonkeyPatch()
    try:
        return _recorded_run(mp, 1)
    finally:
        mp.undo()


@pytest.mark.parametrize("G", [2, 4])
def test_whole_step_grouped_recording_against_per_step(per_step_recording, monkeypatch, G):
    ref_steps, ref_loss, p0, ref_p, ref_ring = per_step_recording
    steps, loss, q0, p, ring = _recorded_run(monkeypatch, G)
    # the student's ring of step counters (mean_count's source, the benchmark's samples per step) is what the single marches leave
    assert torch.equal(ring, ref_ring) and int((ring[:, 0] > 0).sum()) == 3 + 4, ring
    assert torch.equal(p0, q0) and len(steps) == len(ref_steps) == 8
    for i, (a, b) in enumerate(zip(steps, ref_steps)):
        for k in ("rays_o", "rays_d", "xyzs", "dirs", "deltas", "rays", "pred_tea", "tea_fea"):
            assert _same(a[k], b[k]), (i, k)
    assert not _same(steps[0]["rays_o"], steps[1]["rays_o"])
    upd = (ref_p - p0).norm().item()
    print("G=%d: loss %s vs %s, |dp|/upd %.3e" % (G, loss, ref_loss, (p - ref_p).norm().item() / upd))
    assert upd > 0 and np.isfinite(loss).all()
    assert np.allclose(loss, ref_loss, rtol=2e-3), (loss, ref_loss)
    assert (p - ref_p).norm().item() / upd < 0.08
