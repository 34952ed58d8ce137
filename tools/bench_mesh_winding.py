#!/usr/bin/env python3
"""Time of the winding numbers of a mesh (pvd_mesh_winding_count / _build / _points / _lattice, csrc/mesh_winding.hip) on one GPU.

  python tools/bench_mesh_winding.py [--size 256 --lattices 256,512 --grids 256,1024 --reps 10 --warmup 3 --out profiles/mesh_winding.txt]

The mesh is the sphere of radius 0.6 extracted at size^3 (the mesh of tools/bench_mesh_dist.py); the lattice lies over the box
-1 .. 1.  Per lattice resolution R and grid G, hipEvents around every call, after `warmup` untimed rounds, the median and the
minimum over `reps` rounds of
  build     pvd_mesh_winding_count + pvd_mesh_winding_build (without the read-back of the totals between them)
  lattice   pvd_mesh_winding_lattice: one launch, one wave per column
  copy      a device copy of an R^3 int32 array: the floor of writing the answer
  points    pvd_mesh_winding_points on the same R^3 lattice points, 2^24 at a time (the points are made beforehand, untimed)
  dist      pvd_mesh_dist_query of the same points against the mesh at default_grid(T), max_dist one lattice spacing
and the ratios lattice / copy, points / lattice, dist / lattice.  The lattice is compared with the points query bit for bit.
No gate: the figures are appended to --out."""
import argparse
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "aaai2023-pvd_amd"), os.path.join(REPO, "tools")]
CHUNK = 1 << 24


def lattice_points(R, lo, hi, s, e, dev):
    """Rows s .. e of the R^3 lattice of include/pvd_hip_mesh_winding.h, made on the device (a tensor divisor: a true division)."""
    steps = torch.arange(R, dtype=torch.float32, device=dev)[:, None] / torch.full((1, 1), float(R - 1), dtype=torch.float32, device=dev)
    axes = steps * (hi - lo)[None, :] + lo[None, :]
    n = torch.arange(s, e, dtype=torch.int64, device=dev)
    return torch.stack([axes[n // (R * R), 0], axes[(n // R) % R, 1], axes[n % R, 2]], dim=1).contiguous()


def bench(size, lattices, grids, dev, reps, warmup):
    import pvd_hip
    from bench_mesh_dist import sphere_mesh
    from pvd.mesh import _finite_box, default_grid
    verts, tris = sphere_mesh(size, (0.0, 0.0, 0.0), dev)
    T = int(tris.shape[0])
    box_lo, box_hi = _finite_box(verts)
    lo, hi = torch.full((3,), -1.0, device=dev), torch.full((3,), 1.0, device=dev)
    Gd = default_grid(T)
    ws_d = torch.empty(pvd_hip.mesh_dist_workspace_bytes(T, Gd), dtype=torch.uint8, device=dev)
    pvd_hip.mesh_dist_build(verts, tris, box_lo, box_hi, Gd, ws_d)
    totals2, totals4 = torch.zeros(2, dtype=torch.int64, device=dev), torch.zeros(4, dtype=torch.int64, device=dev)
    lines = []
    for R in lattices:
        N = R ** 3
        w, w_p, copy = (torch.empty(N, dtype=torch.int32, device=dev) for _ in range(3))
        dist, dtri = torch.empty(min(N, CHUNK), device=dev), torch.empty(min(N, CHUNK), dtype=torch.int32, device=dev)
        for G in grids:
            pvd_hip.mesh_winding_count(verts, tris, box_lo, box_hi, G, totals2)
            pairs, outside = totals2.tolist()
            ws = torch.empty(pvd_hip.mesh_winding_workspace_bytes(T, G, pairs), dtype=torch.uint8, device=dev)
            times = {"build": [], "lattice": [], "copy": [], "points": [], "dist": []}
            for it in range(warmup + reps):
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
                ev[0].record()
                pvd_hip.mesh_winding_count(verts, tris, box_lo, box_hi, G, totals2)
                pvd_hip.mesh_winding_build(verts, tris, box_lo, box_hi, G, pairs, ws)
                ev[1].record()
                pvd_hip.mesh_winding_lattice(R, lo, hi, T, G, pairs, ws, w, totals4)
                ev[2].record()
                copy.copy_(w)
                ev[3].record()
                t_points = t_dist = 0.0
                for s in range(0, N, CHUNK):
                    e = min(s + CHUNK, N)
                    pts = lattice_points(R, lo, hi, s, e, dev)
                    ep = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
                    ep[0].record()
                    pvd_hip.mesh_winding_points(pts, T, G, pairs, ws, w_p[s:e])
                    ep[1].record()
                    pvd_hip.mesh_dist_query(pts, T, Gd, ws_d, 2.0 / (R - 1), dist[:e - s], dtri[:e - s])
                    ep[2].record()
                    torch.cuda.synchronize()
                    t_points += ep[0].elapsed_time(ep[1])
                    t_dist += ep[1].elapsed_time(ep[2])
                    del pts
                torch.cuda.synchronize()
                if it >= warmup:
                    for q, k in enumerate(("build", "lattice", "copy")):
                        times[k].append(ev[q].elapsed_time(ev[q + 1]))
                    times["points"].append(t_points)
                    times["dist"].append(t_dist)
            med = {k: float(np.median(v)) for k, v in times.items()}
            names = dict(zip(pvd_hip.MESH_WINDING_TOTALS, totals4.tolist()))
            lines.append("mesh winding %d^3 sphere T=%d, lattice %d^3 (%.1f M points), G=%d: pairs %d (%.2f per triangle) outside %d  build %.3f ms "
                         "(min %.3f)  lattice %.3f ms (min %.3f)  %.0f M points/s  copy of R^3 int32 %.3f ms  lattice / copy = %.1f  "
                         "points query %.3f ms  points / lattice = %.1f  mesh_distance query at G=%d, max_dist one spacing %.3f ms  "
                         "dist / lattice = %.1f  inside %d leaky %d  workspace %.1f MB  lattice == points query: %s  [median of %d, %d warm-up]"
                         % (size, T, R, N / 1e6, G, pairs, pairs / max(T, 1), outside, med["build"], min(times["build"]), med["lattice"],
                            min(times["lattice"]), N / med["lattice"] / 1e3, med["copy"], med["lattice"] / med["copy"], med["points"],
                            med["points"] / med["lattice"], Gd, med["dist"], med["dist"] / med["lattice"], names["inside"], names["leaky_columns"],
                            ws.numel() / 1e6, bool(torch.equal(w, w_p)), reps, warmup))
            print(lines[-1], flush=True)
            del ws
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--lattices", default="256,512")
    ap.add_argument("--grids", default="256,1024")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mesh_winding.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_mesh_winding.py measures on a GPU; there is no CPU path"
    lines = bench(a.size, [int(r) for r in a.lattices.split(",")], [int(g) for g in a.grids.split(",")], torch.device("cuda:0"), a.reps, a.warmup)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
