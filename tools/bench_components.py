#!/usr/bin/env python3
"""Time of labelling and filtering the connected components (pvd_components_label / pvd_components_filter, csrc/components.hip) of a
sphere plus seeded noise on one GPU, next to the mesh passes on the same field.

  python tools/bench_components.py [--sizes 256,512 --reps 30 --warmup 5 --noise 0.02 --out profiles/mesh_components.txt]

Per resolution R, hipEvents around every call, after `warmup` untimed rounds, the median and the minimum over `reps` rounds of
  label       pvd_components_label: init, merge, flatten + count, largest (five launches)
  filter      pvd_components_filter with min_points = 8 (two launches)
  mesh        pvd_mesh_count + pvd_mesh_emit of the unfiltered field, as tools/bench_mesh.py times them
next to the floor of reading the field once and writing the labels, R^3 * 8 B, at the device copy rate measured in the same run
(a copy of R^3 floats: 8 B of traffic per point as well), and the ratio of label to that floor.  The lines are appended to --out."""
import argparse
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "aaai2023-pvd_amd")]


def sphere_plus_noise(R, dev, noise, radius=0.6, seed=0):
    x = torch.linspace(-1.0, 1.0, R, device=dev)
    X, Y, Z = torch.meshgrid(x, x, x, indexing="ij")
    u = radius - torch.sqrt(X * X + Y * Y + Z * Z)
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    floaters = torch.rand(R, R, R, device=dev, generator=g) < noise
    return torch.where(floaters, torch.full_like(u, 0.25), u).contiguous()


def bench(R, dev, reps, warmup, noise):
    import pvd_hip
    u = sphere_plus_noise(R, dev, noise)
    N = R ** 3
    labels = torch.empty(N, dtype=torch.int32, device=dev)
    sizes = torch.empty(N, dtype=torch.int32, device=dev)
    stats = torch.zeros(4, dtype=torch.int32, device=dev)
    kept = torch.zeros(2, dtype=torch.int32, device=dev)
    out, copy = torch.empty_like(u), torch.empty_like(u)
    ws = torch.empty(pvd_hip.mesh_workspace_bytes(R), dtype=torch.uint8, device=dev)
    totals = torch.zeros(2, dtype=torch.int32, device=dev)
    lo, hi = torch.full((3,), -1.0, device=dev), torch.full((3,), 1.0, device=dev)
    pvd_hip.mesh_count(u, R, 0.0, ws, totals)
    V, T = totals.tolist()
    verts = torch.empty(V, 3, device=dev)
    tris = torch.empty(T, 3, dtype=torch.int32, device=dev)
    times = {"label": [], "filter": [], "mesh": [], "copy": []}
    for it in range(warmup + reps):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
        ev[0].record()
        pvd_hip.components_label(u, R, 0.0, labels, sizes, stats)
        ev[1].record()
        pvd_hip.components_filter(u, labels, sizes, stats, R, 0.0, 8, False, out, kept)
        ev[2].record()
        pvd_hip.mesh_count(u, R, 0.0, ws, totals)
        pvd_hip.mesh_emit(u, R, 0.0, lo, hi, ws, verts, tris)
        ev[3].record()
        copy.copy_(u)
        ev[4].record()
        torch.cuda.synchronize()
        if it >= warmup:
            for q, k in enumerate(("label", "filter", "mesh", "copy")):
                times[k].append(ev[q].elapsed_time(ev[q + 1]))
    med = {k: float(np.median(v)) for k, v in times.items()}
    rate = N * 8 / (med["copy"] * 1e-3) / 1e12
    st, kp = stats.tolist(), kept.tolist()
    return ("components R=%d sphere + %.3g noise: %d components (%d inside points, largest %d), kept %d (%d points) at min_points 8  "
            "label %.3f ms (min %.3f)  filter %.3f ms (min %.3f)  mesh count+emit %.3f ms (min %.3f)  floor (8 B/point at the copy's "
            "%.2f TB/s) %.3f ms  label/floor %.1f  label/mesh %.2f  [median of %d, %d warm-up]"
            % (R, noise, st[0], st[1], st[2], kp[0], kp[1], med["label"], min(times["label"]), med["filter"], min(times["filter"]),
               med["mesh"], min(times["mesh"]), rate, med["copy"], med["label"] / med["copy"], med["label"] / med["mesh"], reps, warmup))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,512")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--noise", type=float, default=0.02, help="fraction of lattice points turned into floaters")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mesh_components.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_components.py measures on a GPU; there is no CPU path"
    dev = torch.device("cuda:0")
    lines = [bench(int(R), dev, a.reps, a.warmup, a.noise) for R in a.sizes.split(",")]
    for ln in lines:
        print(ln, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
