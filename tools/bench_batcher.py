#!/usr/bin/env python3
"""Cost of the data side of a teacher step: batches made on the device (pvd.batcher.DeviceBatcher, csrc/databatch.hip) against the
host-side refill of the same static slots, on one GPU.

  python tools/bench_batcher.py [--scene DIR] [--views 40 --res 200] [--rays 4096 --reps 30 --warmup 5 --out profiles/data_batcher.txt]

Without --scene the synthetic chair is written to a temporary directory by tools/make_blender_scene.py (a child process).
  (a) pvd_image_batch alone, uniform pixels and by the error map (grid 128), hipEvents around every call;
  (b) pvd_error_map_update alone;
  (c) one 16-step teacher block with the batches made inside the graph (capture_block(batches, source)), without and with the map;
  (d) the same block fed from the host: 16 x (BlenderScene.batch + training_target + copy_ into the static slots), then train_block();
  (e) train_block() replaying frozen batches: the floor.
(c), (d) and (e) are host wall clock around train_block() -- the occupancy-grid update and one graph launch -- ending in a
synchronise, taken alternately in the same process (each variant on a trainer of its own, all started from the same seed)."""
import argparse
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "aaai2023-pvd_amd"), os.path.join(REPO, "tests")]

import pvd_hip  # noqa: E402  (before torch touches the device)
import torch  # noqa: E402


def stats(ms):
    ms = np.asarray(ms, dtype=np.float64)
    return "median %8.4f  min %8.4f  p10 %8.4f  p90 %8.4f" % (np.median(ms), ms.min(), np.percentile(ms, 10), np.percentile(ms, 90))


def event_times(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        ev.append((e0, e1))
    torch.cuda.synchronize()
    return np.array([a.elapsed_time(b) for a, b in ev])


def burst_times(fn, reps, burst=50):
    """Per-call time with `burst` calls queued back to back between two events: the launches' own time, without the wait for the host
    that a single call between two events on an idle stream includes."""
    return event_times(lambda: [fn() for _ in range(burst)], reps, 2) / burst


def make_trainer(dev, rays):
    """The hash teacher of bench.py's teacher workload."""
    from pvd.config import PVDConfig
    from pvd.ops import hip_ops
    from pvd.trainer import TeacherTrainer
    from pvd.workload import DistillWorkload, measure_mean_count
    torch.manual_seed(0)
    opt = PVDConfig(num_rays=rays, fp16=True)
    w = DistillWorkload(hip_ops(), dev, opt, teacher_pretrain_steps=0)
    topt = PVDConfig(**{**opt.__dict__, "model_type": opt.teacher_type, "iters": 30000, "stage_iters": {"stage1": -1, "stage2": -1}})
    tea = w.tea
    tea.teacher_variant = True
    tea.requires_grad_(True).train()
    tea.args = tea.opt = topt
    tr = TeacherTrainer(topt, tea, dev, fp16=True)
    tea.mean_count = measure_mean_count(tea, w.poses, opt, generator=w.gen)
    return w, tr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default=None, help="a Blender-format scene; default: the synthetic chair written to a temporary directory")
    ap.add_argument("--views", type=int, default=40)
    ap.add_argument("--res", type=int, default=200)
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "data_batcher.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_batcher.py measures on a GPU; none is visible")
    tmp = None
    if a.scene is None:
        tmp = tempfile.TemporaryDirectory(prefix="pvd_chair_")
        a.scene = tmp.name
        subprocess.run([sys.executable, os.path.join(REPO, "tools", "make_blender_scene.py"), a.scene, "--views", str(a.views), "--res", str(a.res)],
                       check=True, timeout=600)
    from pvd.batcher import DeviceBatcher
    from pvd.provider import BlenderScene, training_target
    import databatch_restatement as R
    dev = torch.device("cuda:0")
    N = a.rays
    lines = ["tools/bench_batcher.py on %s" % torch.cuda.get_device_name(0), ""]

    trainers = {name: make_trainer(dev, N) for name in ("graph", "graph+map", "host")}
    w0, tr0 = trainers["host"]
    opt = w0.opt
    scene = BlenderScene(a.scene, "train", scale=opt.scale, device=dev, num_rays=N)
    aabb = tr0.model.aabb_train
    f32_bytes, u8_bytes = scene.images.numel() * scene.images.element_size(), scene.images.numel()
    lines.append("scene: %d train views of %d x %d x %d; image stack %.2f MB as float32 (BlenderScene), %.2f MB as uint8 (DeviceBatcher): %.1fx"
                 % (len(scene), scene.H, scene.W, scene.images.shape[-1], f32_bytes / 1e6, u8_bytes / 1e6, f32_bytes / u8_bytes))
    lines.append("%d rays per batch, %d repetitions after %d warm-up (all times in ms)" % (N, a.reps, a.warmup))
    lines.append("")

    # ---- (a), (b): the entry points alone
    reps_k = max(200, a.reps)
    a_ms, b_ms = {}, 0.0
    for label, emap in (("uniform", False), ("error map, grid 128", True)):
        src = DeviceBatcher.from_scene(scene, aabb, 0.2, num_rays=N, seed=1, error_map=emap)
        b = src.new_batch()
        ms = event_times(lambda: src.fill(b), reps_k, 20)
        lines.append("(a) pvd_image_batch, %-20s %s  (%d single calls)" % (label + ":", stats(ms), reps_k))
        ms = burst_times(lambda: src.fill(b), a.reps)
        a_ms["map" if emap else "uniform"] = float(np.median(ms))
        lines.append("    %-36s %s  (per call, 50 calls back to back, %d times)" % ("", stats(ms), a.reps))
        if emap:
            pred = torch.rand(1, N, 3, device=dev)
            ms = event_times(lambda: src.feedback(b, pred), reps_k, 20)
            lines.append("(b) pvd_error_map_update:               %s  (%d single calls)" % (stats(ms), reps_k))
            ms = burst_times(lambda: src.feedback(b, pred), a.reps)
            b_ms = float(np.median(ms))
            lines.append("    %-36s %s  (per call, 50 calls back to back, %d times)" % ("", stats(ms), a.reps))
            # the keys of the draw against float64 (tests/test_hip_databatch.py states the bound)
            worst = 0.0
            src.error_map.copy_(0.01 + 20.0 * torch.rand(src.error_map.shape, device=dev) ** 3)
            for _ in range(4):
                counter, pos = int(src.state[1]), int(src.state[0])
                keys = torch.empty(128 * 128, device=dev)
                src.fill(b, keys_out=keys)
                k64 = R.keys64(src.error_map[int(src.order[pos])].cpu().numpy(), R.cell_uniforms(1, counter, 128 * 128))
                ok = np.isfinite(k64) & (k64 > 0)
                worst = max(worst, float(np.abs(keys.cpu().numpy()[ok].astype(np.float64) / k64[ok] - 1.0).max()))
            lines.append("    keys of the draw against float64: largest |key / key64 - 1| = %.4g = %.3f x 2^-23 (bound 2.5 x 2^-23: logf 2 ulp, one rounding of the division)" % (worst, worst * 2 ** 23))
    lines.append("")

    # ---- (c), (d), (e): the 16-step block
    sources, slots = {}, {}
    for name, (w, tr) in trainers.items():
        gen = w.gen
        if name == "host":
            bs = []
            for it in range(16):
                bt = scene.batch([it % len(scene)], generator=gen)
                gt, bg = training_target(bt["images"], generator=gen)
                bs.append((bt["rays_o"].contiguous(), bt["rays_d"].contiguous(), gt.contiguous(), bg.contiguous()))
            for it in range(16):
                tr.train_step(*bs[it])
            tr.capture_block(bs)
        else:
            src = DeviceBatcher.from_scene(scene, tr.model.aabb_train, 0.2, num_rays=N, seed=1, error_map=name == "graph+map")
            bs = [src.new_batch() for _ in range(16)]
            for it in range(16):
                src.fill(bs[it])
                _, pred = tr.train_step(*bs[it])
                src.feedback(bs[it], pred)
            tr.capture_block(bs, src)
            sources[name] = src
        slots[name] = bs
    step = {"n": 0}

    def host_refill():
        w, _ = trainers["host"]
        for k in range(16):
            bt = scene.batch([(step["n"] + k) % len(scene)], generator=w.gen)
            gt, bg = training_target(bt["images"], generator=w.gen)
            s = slots["host"][k]
            s[0].copy_(bt["rays_o"]), s[1].copy_(bt["rays_d"]), s[2].copy_(gt), s[3].copy_(bg)
        step["n"] += 16

    def block(name, refill=False):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if refill:
            host_refill()
        loss, _ = trainers[name][1].train_block()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, float(loss)

    variants = [("(c) in-graph batches, uniform", "graph", False), ("(c) in-graph batches, error map", "graph+map", False),
                ("(d) host refill + replay", "host", True), ("(e) frozen batches (floor)", "host", False)]
    times, last = {v[0]: [] for v in variants}, {}
    for r in range(a.warmup + a.reps):  # alternating, so that a drift of the machine hits all variants alike
        for label, name, refill in variants:
            ms, loss = block(name, refill)
            if r >= a.warmup:
                times[label].append(ms)
            last[label] = loss
    lines.append("one block = occupancy-grid update + 16 training steps in one graph launch (%s), host wall clock incl. synchronise"
                 % ("next step's march forked" if trainers["graph"][1].pipelined_block else "steps back to back"))
    for label, _, _ in variants:
        lines.append("%-34s %s  per step %.4f  (last loss %.4g)" % (label + ":", stats(times[label]), np.median(times[label]) / 16, last[label]))
    med = {k: float(np.median(v)) for k, v in times.items()}
    c, c2, d, e = (med[v[0]] for v in variants)
    spread = max(np.percentile(times[v[0]], 90) - np.percentile(times[v[0]], 10) for v in (variants[0], variants[2]))
    lines.append("(d) - (c) = %.4f ms per block (%.1f %% of (d)); larger p90 - p10 spread of the two: %.4f ms -> (c) is %s"
                 % (d - c, 100 * (d - c) / d, spread, "below (d) by more than the spread" if d - c > spread else "NOT below (d) by more than the spread"))
    lines.append("(c) - (e) = %.4f ms per block = %.4f ms per step, uniform; %.4f ms per block = %.4f ms per step with the error map"
                 % (c - e, (c - e) / 16, c2 - e, (c2 - e) / 16))
    lines.append("(d) - (e) = %.4f ms per block: the host refill" % (d - e))
    spread_ce = max(np.percentile(times[v[0]], 90) - np.percentile(times[v[0]], 10) for v in (variants[0], variants[3]))
    lines.append("16 x (a) = %.4f ms (uniform), %.4f ms (error map, + 16 x (b) = %.4f ms); p90 - p10 spread of (c) and (e): %.4f ms -> (c) - (e) is %s"
                 % (16 * a_ms["uniform"], 16 * a_ms["map"], 16 * b_ms, spread_ce,
                    "resolved by the block timing" if abs(c - e) > spread_ce else "below what the block timing resolves"))
    for name, src in sources.items():
        lines.append("%s: %d batches drawn on the device" % (name, int(src.state[1])))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    if tmp is not None:
        tmp.cleanup()


if __name__ == "__main__":
    main()
