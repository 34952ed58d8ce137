#!/usr/bin/env python3
"""Time of one 800 x 800 inference render (640 000 rays) of the hash teacher, the VM student, the Plenoxel student and the NeRF-MLP teacher:
the reference-shaped loop (one device-to-host read-back per round) vs the rounds whose state stays on the device (pvd_infer_*) vs the
whole loop as one persistent launch (pvd_infer_image_hash / pvd_infer_image_vm / pvd_infer_image_plenoxel / pvd_infer_image_mlp).
For the mlp model the persistent launch's MFMA rate (rows shaded x 0.87 MFLOP / launch time) is printed next to that of the plain
trunk + head launch (pvd_mlp_head_forward_fused) on as many rows: the gap is what under-full rounds and the march cost."""
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "aaai2023-pvd_amd"), os.path.join(REPO, "tests")]
import numpy as np
import torch

from pvd.scene import BLENDER_INTRINSICS, get_rays, synthetic_poses
from test_hip_infer_rounds import _model

dev = torch.device("cuda:0")
poses = torch.from_numpy(synthetic_poses(np.random.RandomState(2))).to(dev)
r = get_rays(poses[9][None], BLENDER_INTRINSICS, 800, 800, -1)
ONLY = os.environ.get("PVD_RENDER_ONLY")  # "p": the persistent renders alone (profiling); PVD_RENDER_KIND=hash|vm|tensors|mlp: one model
for kind in ("hash", "vm", "tensors", "mlp"):
    if os.environ.get("PVD_RENDER_KIND", kind) != kind:
        continue
    if kind == "mlp":
        from test_hip_infer_mlp import _mlp_model
        m = _mlp_model()
    else:
        m = _model(kind)
    for mode in ("0", "1", "p"):
        if (ONLY and mode != ONLY) or (kind == "tensors" and mode == "1"):  # (no device-side round state for the Plenoxel model)
            continue
        os.environ["PVD_INFER_DEVICE_ROUNDS"] = "0" if mode == "0" else "1"
        os.environ["PVD_INFER_PERSISTENT"] = "1" if mode == "p" else "0"
        times = []
        for it in range(4):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
                out = m.render(r["rays_o"], r["rays_d"], staged=False, bg_color=1, perturb=False, dt_gamma=0, max_steps=1024)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        if mode == "p":
            wsp = m._last_infer_workspace
            st = wsp[-10:-6].tolist()
            ph = wsp[-6:-1].tolist()
            if any(ph) and kind != "mlp":
                print("      workgroup 0, us: refill+scan %.0f  march %.0f  lookup %.0f  head %.0f  blend %.0f" % tuple(v / 100.0 for v in ph))
            print("      persistent launch: %d rays queued of %d; %d workgroups, %d local rounds (%d walk-only), %d rows shaded = %.1f rows per shading round"
                  % (int(wsp[0]), r["rays_o"].shape[1], st[3], st[0], st[2], st[1], st[1] / max(st[0] - st[2], 1)))
            if kind == "mlp" and st[1] > 0 and hasattr(m.ops.fused_head, "mlp_infer_image"):
                # the launch alone (events around the entry point: no near/far, no compositing of the background) ...
                fh, rm = m.ops.fused_head, m.ops.raymarching
                o, d = r["rays_o"].contiguous().view(-1, 3), r["rays_d"].contiguous().view(-1, 3)
                nears, fars = rm.near_far_from_aabb(o, d, m.aabb_infer, m.min_near)
                def timed(fn, n=4):
                    best = 1e9
                    for _ in range(n):
                        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        a.record(); fn(); b.record(); torch.cuda.synchronize()
                        best = min(best, a.elapsed_time(b))
                    return best
                with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
                    t_p = timed(lambda: fh.mlp_infer_image(m, o, d, nears, fars, 0, 1024))
                    # ... and the plain trunk + head launch (pvd_mlp_head_forward_fused alone, rows already encoded) on as many rows
                    import pvd_hip
                    from test_hip_infer_mlp import _plain_launch_inputs
                    M = int(st[1])
                    pts, stream, nb, na, dirs, hw = _plain_launch_inputs(m, M)
                    outs = (torch.empty(M, device=dev), torch.empty(M, 3, device=dev), torch.empty(M, 16, device=dev))
                    t_f = timed(lambda: pvd_hip.mlp_head_forward_fused(pts, stream, nb, na, dirs, M, *hw, m.args.sigma_clip_min, m.args.sigma_clip_max, *outs))
                print("      persistent launch alone %.3f ms: %d rows x 0.87 MFLOP = %.1f TFLOP/s;  plain trunk + head launch on %d rows %.3f ms = %.1f TFLOP/s"
                      % (t_p, M, M * 0.868352e6 / (t_p * 1e-3) / 1e12, M, t_f, M * 0.868352e6 / (t_f * 1e-3) / 1e12))
        print("%-5s 800x800 render, %s: %.2f ms (best of 3 after warm-up), %s rounds" % (
            kind, {"1": "round state on the device", "0": "host read-back per round ", "p": "ONE persistent launch     "}[mode], min(times[1:]) * 1e3,
            getattr(m, "_last_rounds", "?") if mode == "1" else "n/a"))
