#!/usr/bin/env python3
"""Time of the point-to-mesh distance (pvd_mesh_dist_build / pvd_mesh_dist_query, csrc/mesh_dist.hip) on one GPU.

  python tools/bench_mesh_dist.py [--size 256 --grids 16,32,64,128,256 --reps 20 --warmup 5 --out profiles/mesh_dist.txt]

The mesh is the sphere of radius 0.6 extracted at size^3; the queries are the vertices of the same sphere shifted by
(0.004, -0.003, 0.002), extracted the same way: the case compare_meshes runs, every point within a lattice spacing of the surface.
Per G, hipEvents around every call, after `warmup` untimed rounds, the median and the minimum over `reps` rounds of
  build   pvd_mesh_dist_build: count, block sums, scan, offsets, fill, and the two memsets
  query   pvd_mesh_dist_query: one launch, one lane per point
  copy    a device copy of the triangle array (T * 12 B read and written): the memory floor of touching the mesh once
next to h_min and rho at that G, and a last line for the default grid rule (pvd/mesh.py: default_grid).  The results of every G
are compared bit for bit with those of the first.
No gate: the figures are appended to --out."""
import argparse
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "aaai2023-pvd_amd")]


def sphere_mesh(R, centre, dev):
    from pvd.mesh import extract_mesh
    x = torch.linspace(-1.0, 1.0, R, device=dev)
    X, Y, Z = torch.meshgrid(x, x, x, indexing="ij")
    u = (0.6 - torch.sqrt((X - centre[0]) ** 2 + (Y - centre[1]) ** 2 + (Z - centre[2]) ** 2)).contiguous()
    return extract_mesh(u, 0.0, (-1.0,) * 3, (1.0,) * 3)


def bench(R, grids, dev, reps, warmup):
    import pvd_hip
    from pvd.mesh import _finite_box, default_grid
    verts, tris = sphere_mesh(R, (0.0, 0.0, 0.0), dev)
    points = sphere_mesh(R, (0.004, -0.003, 0.002), dev)[0]
    T, N = int(tris.shape[0]), int(points.shape[0])
    lo, hi = _finite_box(verts)
    copy = torch.empty_like(tris)
    dist, tri = torch.empty(N, device=dev), torch.empty(N, dtype=torch.int32, device=dev)
    lines, first = [], None
    for G in grids + [default_grid(T)]:
        ws = torch.empty(pvd_hip.mesh_dist_workspace_bytes(T, G), dtype=torch.uint8, device=dev)
        times = {"build": [], "query": [], "copy": []}
        for it in range(warmup + reps):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            ev[0].record()
            pvd_hip.mesh_dist_build(verts, tris, lo, hi, G, ws)
            ev[1].record()
            pvd_hip.mesh_dist_query(points, T, G, ws, 1.0, dist, tri)
            ev[2].record()
            copy.copy_(tris)
            ev[3].record()
            torch.cuda.synchronize()
            if it >= warmup:
                for q, k in enumerate(("build", "query", "copy")):
                    times[k].append(ev[q].elapsed_time(ev[q + 1]))
        got = (dist.cpu().numpy().tobytes(), tri.cpu().numpy().tobytes())
        first = first or got
        same = got == first
        med = {k: float(np.median(v)) for k, v in times.items()}
        h = float((hi - lo).min()) / G
        rho = float(ws[:4].view(torch.float32)[0])  # the first word of the workspace header
        lines.append("mesh dist R=%d sphere: T=%d N=%d G=%d%s  h_min %.5f rho %.5f  build %.3f ms (min %.3f)  query %.3f ms (min %.3f)  "
                     "%.1f M points/s  copy of the triangles %.3f ms (min %.3f)  workspace %.1f MB  mean dist %.6f  bits equal to G=%d: %s  "
                     "[median of %d, %d warm-up]"
                     % (R, T, N, G, " (default_grid)" if G == default_grid(T) and G not in grids else "", h, rho, med["build"],
                        min(times["build"]), med["query"], min(times["query"]), N / med["query"] / 1e3, med["copy"], min(times["copy"]),
                        ws.numel() / 1e6, float(dist.double().mean()), grids[0], same, reps, warmup))
        print(lines[-1], flush=True)
        del ws
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--grids", default="16,32,64,128,256")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mesh_dist.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_mesh_dist.py measures on a GPU; there is no CPU path"
    lines = bench(a.size, [int(g) for g in a.grids.split(",")], torch.device("cuda:0"), a.reps, a.warmup)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
