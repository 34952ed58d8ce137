#!/usr/bin/env python3
"""Time of the mesh extraction (pvd_mesh_count / pvd_mesh_emit, csrc/mesh.hip) of a sphere's density volume on one GPU.

  python tools/bench_mesh.py [--sizes 256,512 --reps 30 --warmup 5 --out profiles/mesh_extract.txt]

Per resolution R, hipEvents around every call, after `warmup` untimed rounds, the median and the minimum over `reps` rounds of
  count+scan  pvd_mesh_count: the count pass, the scan of the per-workgroup sums and the offsets pass (three launches)
  emit        pvd_mesh_emit: vertices and triangles
next to the floor of reading the field once, R^3 * 4 B at the 6.29 TB/s the project measured for a device copy, and
the ratio of the two calls' sum to that floor.  The lines are appended to --out."""
import argparse
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "aaai2023-pvd_amd")]

HBM_COPY_TBS = 6.29  # measured copy rate, BASELINE.md


def sphere(R, dev, radius=0.6):
    x = torch.linspace(-1.0, 1.0, R, device=dev)
    X, Y, Z = torch.meshgrid(x, x, x, indexing="ij")
    return (radius - torch.sqrt(X * X + Y * Y + Z * Z)).contiguous()


def bench(R, dev, reps, warmup):
    import pvd_hip
    u = sphere(R, dev)
    ws = torch.empty(pvd_hip.mesh_workspace_bytes(R), dtype=torch.uint8, device=dev)
    totals = torch.zeros(2, dtype=torch.int32, device=dev)
    lo, hi = torch.full((3,), -1.0, device=dev), torch.full((3,), 1.0, device=dev)
    pvd_hip.mesh_count(u, R, 0.0, ws, totals)
    V, T = totals.tolist()
    verts = torch.empty(V, 3, device=dev)
    tris = torch.empty(T, 3, dtype=torch.int32, device=dev)
    times = {"count+scan": [], "emit": []}
    for it in range(warmup + reps):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        ev[0].record()
        pvd_hip.mesh_count(u, R, 0.0, ws, totals)
        ev[1].record()
        pvd_hip.mesh_emit(u, R, 0.0, lo, hi, ws, verts, tris)
        ev[2].record()
        torch.cuda.synchronize()
        if it >= warmup:
            times["count+scan"].append(ev[0].elapsed_time(ev[1]))
            times["emit"].append(ev[1].elapsed_time(ev[2]))
    floor_ms = R ** 3 * 4 / (HBM_COPY_TBS * 1e12) * 1e3
    med = {k: float(np.median(v)) for k, v in times.items()}
    line = ("mesh R=%d sphere: V=%d T=%d  count+scan %.3f ms (min %.3f)  emit %.3f ms (min %.3f)  sum %.3f ms  floor (field once at %.2f TB/s) "
            "%.3f ms  ratio %.1f  [median of %d, %d warm-up]"
            % (R, V, T, med["count+scan"], min(times["count+scan"]), med["emit"], min(times["emit"]), med["count+scan"] + med["emit"],
               HBM_COPY_TBS, floor_ms, (med["count+scan"] + med["emit"]) / floor_ms, reps, warmup))
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,512")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mesh_extract.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_mesh.py measures on a GPU; there is no CPU path"
    dev = torch.device("cuda:0")
    lines = [bench(int(R), dev, a.reps, a.warmup) for R in a.sizes.split(",")]
    for ln in lines:
        print(ln, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
