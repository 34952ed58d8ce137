#!/usr/bin/env python3
"""Time of the vertex-normal pass (pvd_mesh_normals, csrc/mesh.hip) next to the emit pass of the mesh it belongs to, on one GPU.

  python tools/bench_mesh_attr.py [--sizes 256,512 --fields sphere,smooth --reps 30 --warmup 5 --out profiles/mesh_normals.txt]

Per field and resolution R, hipEvents around every call, after `warmup` untimed rounds, the median and the minimum over `reps` rounds of
  normals     pvd_mesh_normals: one launch, one lane per lattice point, the normals of the vertices the point owns
  emit        pvd_mesh_emit: vertices and triangles of the same workspace
  field once  a device copy of the field (R^3 * 4 B read and written), the measured cost of touching every sample
next to the floor of reading the field once at the 6.29 TB/s the project measured for a device copy, the ratio
normals / emit, and the bytes the pass must move (mask and field once, per vertex one offset read and 12 B written) over its time.
No gate: the figures are appended to --out."""
import argparse
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "aaai2023-pvd_amd")]

HBM_COPY_TBS = 6.29  # measured copy rate, BASELINE.md


def make_field(kind, R, dev):
    x = torch.linspace(-1.0, 1.0, R, device=dev)
    X, Y, Z = torch.meshgrid(x, x, x, indexing="ij")
    if kind == "sphere":
        return (0.6 - torch.sqrt(X * X + Y * Y + Z * Z)).contiguous()
    if kind == "smooth":  # a sum of products of sines: a surface with many sheets that leaves the box through every face
        rng = np.random.RandomState(7)
        u = torch.zeros_like(X)
        for _ in range(4):
            f, ph = rng.uniform(0.5, 3.0, 3), rng.uniform(0, 2 * np.pi, 3)
            u += float(rng.uniform(0.3, 1.0)) * torch.sin(f[0] * X + ph[0]) * torch.sin(f[1] * Y + ph[1]) * torch.sin(f[2] * Z + ph[2])
        return u.contiguous()
    raise KeyError(kind)


def bench(kind, R, dev, reps, warmup):
    import pvd_hip
    u = make_field(kind, R, dev)
    ws = torch.empty(pvd_hip.mesh_workspace_bytes(R), dtype=torch.uint8, device=dev)
    totals = torch.zeros(2, dtype=torch.int32, device=dev)
    lo, hi = torch.full((3,), -1.0, device=dev), torch.full((3,), 1.0, device=dev)
    pvd_hip.mesh_count(u, R, 0.0, ws, totals)
    V, T = totals.tolist()
    verts = torch.empty(V, 3, device=dev)
    tris = torch.empty(T, 3, dtype=torch.int32, device=dev)
    normals = torch.empty(V, 3, device=dev)
    copy = torch.empty_like(u)
    times = {"normals": [], "emit": [], "field once": []}
    for it in range(warmup + reps):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        ev[0].record()
        pvd_hip.mesh_emit(u, R, 0.0, lo, hi, ws, verts, tris)
        ev[1].record()
        pvd_hip.mesh_normals(u, R, 0.0, lo, hi, ws, normals)
        ev[2].record()
        copy.copy_(u)
        ev[3].record()
        torch.cuda.synchronize()
        if it >= warmup:
            times["emit"].append(ev[0].elapsed_time(ev[1]))
            times["normals"].append(ev[1].elapsed_time(ev[2]))
            times["field once"].append(ev[2].elapsed_time(ev[3]))
    med = {k: float(np.median(v)) for k, v in times.items()}
    floor_ms = R ** 3 * 4 / (HBM_COPY_TBS * 1e12) * 1e3
    must_move = R ** 3 * 5 + V * 16  # mask byte + field once per point; first vertex index and 12 B of normal per vertex (lower bound)
    return ("mesh normals R=%d %s: V=%d T=%d  normals %.3f ms (min %.3f)  emit %.3f ms (min %.3f)  normals/emit %.2f  copy of the field "
            "%.3f ms (min %.3f)  floor (field once at %.2f TB/s) %.3f ms  normals: %.2f TB/s of the %.1f MB it must move  "
            "[median of %d, %d warm-up]"
            % (R, kind, V, T, med["normals"], min(times["normals"]), med["emit"], min(times["emit"]), med["normals"] / med["emit"],
               med["field once"], min(times["field once"]), HBM_COPY_TBS, floor_ms, must_move / (med["normals"] * 1e-3) / 1e12,
               must_move / 1e6, reps, warmup))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,512")
    ap.add_argument("--fields", default="sphere,smooth")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mesh_normals.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_mesh_attr.py measures on a GPU; there is no CPU path"
    dev = torch.device("cuda:0")
    lines = [bench(kind, int(R), dev, a.reps, a.warmup) for kind in a.fields.split(",") for R in a.sizes.split(",")]
    for ln in lines:
        print(ln, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
