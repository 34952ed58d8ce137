#!/usr/bin/env python3
"""Accuracy and time of the fused image metrics (pvd_image_metrics, csrc/metrics.hip) on one GPU.

  python tools/bench_metrics.py [--size 800 --reps 50 --warmup 10 --out profiles/image_metrics.txt]

1. Error ratios: per test case, |kernel - float64| / E_ref with E_ref = |float32 restatement on the CPU - float64|
   (tests/ssim_restatement.py; the bar of tests/test_hip_metrics.py is 4 E_ref + 2e-6).
2. Time of SSIM + MSE of one size x size x 3 pair, three ways in the same run, alternating, hipEvents around every call:
     fused      pvd.metrics.image_metrics(a, b, None): max + SSIM/MSE + final sum, three launches, no read-back
     torch      the plain-torch composition of pvd/metrics.py (ssim_torch + mean squared error), max_val kept as a tensor
     reference  the same composition with max_val = max(a.max().item(), b.max().item()) as the reference's evaluate takes it
   Per variant: the median and the minimum of the per-call event times, and the host's wall clock per call over the whole loop
   (ending in a synchronise), which is what a sweep over views pays."""
import argparse
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "aaai2023-pvd_amd"), os.path.join(REPO, "tests")]

from pvd.metrics import image_metrics, ssim_torch  # noqa: E402


def error_ratios(dev, lines):
    import pvd_hip
    from ssim_restatement import cpu_checked_cases, host_max, pair_random, yardstick
    T = pvd_hip.METRICS_TILE
    cases = dict(cpu_checked_cases())
    for h, w in ((T - 1, T - 1), (T, T), (T + 1, T + 1), (2 * T + 1, 2 * T + 1)):
        cases["seam_%dx%d" % (h, w)] = pair_random((1, h, w, 3), 100 + h)
    lines.append("%-16s %-16s %11s %11s %7s %11s %11s" % ("case", "[B,H,W,C]", "map error", "E_ref(map)", "ratio", "mean error", "E_ref(mean)"))
    for name, (a, b) in cases.items():
        mv = host_max(a, b)
        truth_mean, truth_map, e_mean, e_map = yardstick(a, b, mv)
        ssim, _, ssim_map = image_metrics(a.to(dev), b.to(dev), mv, return_map=True)
        err_map = float((ssim_map.cpu().double() - truth_map).abs().max())
        err_mean = float((ssim.cpu().double() - truth_mean).abs().max())
        lines.append("%-16s %-16s %11.3e %11.3e %7.2f %11.3e %11.3e" % (name, str(list(a.shape)), err_map, e_map, err_map / max(e_map, 1e-30),
                                                                          err_mean, float(e_mean.max())))


def timings(dev, size, reps, warmup, lines):
    g = torch.Generator().manual_seed(0)
    a = F.interpolate(torch.rand(1, 3, size // 8, size // 8, generator=g), size=(size, size), mode="bilinear").permute(0, 2, 3, 1).contiguous()
    b = (a + 0.02 * torch.randn(a.shape, generator=g)).clamp(0, 1)
    a, b = a.to(dev), b.to(dev)

    def fused():
        s, m, _ = image_metrics(a, b, None)
        return s, m

    def composed(max_val):
        s, _ = ssim_torch(a, b, max_val)
        return s, ((a - b) ** 2).reshape(1, -1).mean(-1)

    variants = [("fused", fused), ("torch", lambda: composed(None)), ("reference", lambda: composed(max(a.max().item(), b.max().item())))]
    results = {n: f() for n, f in variants}
    for _ in range(warmup):
        for _, f in variants:
            f()
    torch.cuda.synchronize()
    events = {n: [] for n, _ in variants}
    for _ in range(reps):  # alternating, so that a drift of the machine hits all three alike
        for n, f in variants:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            events[n].append((e0, e1))
    torch.cuda.synchronize()
    wall = {}
    for n, f in variants:
        t0 = time.perf_counter()
        for _ in range(reps):
            f()
        torch.cuda.synchronize()
        wall[n] = (time.perf_counter() - t0) / reps * 1e3
    lines.append("SSIM + MSE of one %d x %d x 3 pair, %d repetitions after %d warm-up calls (ms per call)" % (size, size, reps, warmup))
    lines.append("%-10s %12s %12s %12s   %s" % ("variant", "event median", "event min", "host wall", "ssim, mse"))
    med = {}
    for n, _ in variants:
        ms = np.array([e0.elapsed_time(e1) for e0, e1 in events[n]])
        med[n] = float(np.median(ms))
        lines.append("%-10s %12.4f %12.4f %12.4f   %.6f, %.6e" % (n, med[n], ms.min(), wall[n], float(results[n][0][0]), float(results[n][1][0])))
    lines.append("fused vs torch: %.1fx by event median, %.1fx by host wall; fused vs reference: %.1fx, %.1fx"
                 % (med["torch"] / med["fused"], wall["torch"] / wall["fused"], med["reference"] / med["fused"], wall["reference"] / wall["fused"]))
    # the entry point alone (its launches, without the wrapper's allocations), with and without the maximum's launch
    import pvd_hip
    entry = {}
    for label, mv in (("max on the device", None), ("max_val given", 1.0)):
        with pvd_hip.KernelTimer({"pvd_image_metrics"}) as kt:
            for _ in range(reps):
                image_metrics(a, b, mv)
            entry[label] = kt.mean_ms("pvd_image_metrics")
        lines.append("pvd_image_metrics alone, %s: %.4f ms per call (mean of %d)" % (label, entry[label], reps))
    # what the algorithm needs: both images read once; per pixel and channel 5 moments x taps fused multiply-adds in each pass
    # (the W pass also runs on the halo rows: (tile + taps - 1) / tile as many)
    nbytes = 2 * a.numel() * 4
    T, fs = pvd_hip.METRICS_TILE, 11
    flops = 2.0 * a.numel() * 5 * fs * (1.0 + (T + fs - 1) / T)
    t = entry["max_val given"] * 1e-3
    lines.append("needed: %.2f MB read, %.3f GFLOP in the tap sums; over the time with max_val given: %.0f GB/s, %.2f TFLOP/s (f32)"
                 % (nbytes / 1e6, flops / 1e9, nbytes / t / 1e9, flops / t / 1e12))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "image_metrics.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_metrics.py measures on a GPU; none is visible")
    if a.reps < 20:
        raise SystemExit("--reps must be at least 20")
    dev = torch.device("cuda:0")
    lines = ["tools/bench_metrics.py on %s" % torch.cuda.get_device_name(0), ""]
    error_ratios(dev, lines)
    lines.append("")
    timings(dev, a.size, a.reps, a.warmup, lines)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
