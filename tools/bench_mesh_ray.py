#!/usr/bin/env python3
"""Time of ray casting against a mesh (pvd_mesh_ray_count / _build / _cast, csrc/mesh_ray.hip) on one GPU.

  python tools/bench_mesh_ray.py [--size 256 --view 800 --grids 1,16,32,64,128,256 --reps 20 --warmup 5 --out profiles/mesh_ray.txt]

The mesh is the sphere of radius 0.6 extracted at size^3 (the mesh of tools/bench_mesh_dist.py); the rays are one view x view
get_rays image from a pose_spherical camera at distance 2.5 with the Blender field of view, in row-major pixel order.  Per G,
hipEvents around every call, after `warmup` untimed rounds, the median and the minimum over `reps` rounds of
  build   pvd_mesh_ray_count + pvd_mesh_ray_build (without the read-back of the totals between them)
  cast    pvd_mesh_ray_cast: one launch, one lane per ray
  dist    pvd_mesh_dist_query of the mesh's own vertices against the mesh at default_grid(T): the neighbouring primitive
  copy    a device copy of the triangle array (T * 12 B read and written): the memory floor of touching the mesh once
and a last line for the default grid rule (pvd/mesh.py: mesh_raycast).  The results of every G are compared bit for bit with those
of the first; the last line states cast(G = 1) / cast(default G) where G = 1 was asked for (one cell is brute force, N x T tests:
it gets 2 rounds after 1 warm-up).
No gate: the figures are appended to --out."""
import argparse
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "aaai2023-pvd_amd"), os.path.join(REPO, "tools")]


def bench(R, view, grids, dev, reps, warmup):
    import pvd_hip
    from bench_mesh_dist import sphere_mesh
    from pvd.mesh import _finite_box, default_grid
    from pvd.scene import BLENDER_INTRINSICS, get_rays, nerf_matrix_to_ngp, pose_spherical
    verts, tris = sphere_mesh(R, (0.0, 0.0, 0.0), dev)
    T, V = int(tris.shape[0]), int(verts.shape[0])
    lo, hi = _finite_box(verts)
    pose = torch.from_numpy(nerf_matrix_to_ngp(pose_spherical(35.0, -30.0, 2.5), scale=1.0)).to(dev)
    s = view / 800.0
    r = get_rays(pose[None], tuple(x * s for x in BLENDER_INTRINSICS), view, view, -1)
    o, d = r["rays_o"].reshape(-1, 3).contiguous(), r["rays_d"].reshape(-1, 3).contiguous()
    N = int(o.shape[0])
    copy = torch.empty_like(tris)
    t, tri, bary = torch.empty(N, device=dev), torch.empty(N, dtype=torch.int32, device=dev), torch.empty(N, 2, device=dev)
    totals = torch.zeros(2, dtype=torch.int64, device=dev)
    Gd = default_grid(T)
    ws_d = torch.empty(pvd_hip.mesh_dist_workspace_bytes(T, Gd), dtype=torch.uint8, device=dev)
    pvd_hip.mesh_dist_build(verts, tris, lo, hi, Gd, ws_d)
    dist, dtri = torch.empty(V, device=dev), torch.empty(V, dtype=torch.int32, device=dev)
    lines, first, cast_ms = [], None, {}
    for G in grids + [Gd]:
        pvd_hip.mesh_ray_count(verts, tris, lo, hi, G, totals)
        pairs, outside = totals.tolist()
        ws = torch.empty(pvd_hip.mesh_ray_workspace_bytes(T, G, pairs), dtype=torch.uint8, device=dev)
        times = {"build": [], "cast": [], "dist": [], "copy": []}
        w_, r_ = (1, 2) if G == 1 else (warmup, reps)  # one cell is brute force, N x T tests: seconds per cast
        for it in range(w_ + r_):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
            ev[0].record()
            pvd_hip.mesh_ray_count(verts, tris, lo, hi, G, totals)
            pvd_hip.mesh_ray_build(verts, tris, lo, hi, G, pairs, ws)
            ev[1].record()
            pvd_hip.mesh_ray_cast(o, d, T, G, pairs, ws, 0.0, float("inf"), t, tri, bary)
            ev[2].record()
            pvd_hip.mesh_dist_query(verts, T, Gd, ws_d, 1.0, dist, dtri)
            ev[3].record()
            copy.copy_(tris)
            ev[4].record()
            torch.cuda.synchronize()
            if it >= w_:
                for q, k in enumerate(("build", "cast", "dist", "copy")):
                    times[k].append(ev[q].elapsed_time(ev[q + 1]))
        got = (t.cpu().numpy().tobytes(), tri.cpu().numpy().tobytes(), bary.cpu().numpy().tobytes())
        first = first or got
        med = {k: float(np.median(v)) for k, v in times.items()}
        cast_ms[G] = med["cast"]
        lines.append("mesh ray R=%d sphere, %dx%d view: T=%d N=%d G=%d%s  pairs %d (%.2f per triangle) outside %d  build %.3f ms (min %.3f)  "
                     "cast %.3f ms (min %.3f)  %.1f M rays/s  %d pixels hit  mesh_distance query of %d vertices at G=%d %.3f ms (%.1f M points/s)  "
                     "copy of the triangles %.3f ms  workspace %.1f MB  bits equal to G=%d: %s  [median of %d, %d warm-up]"
                     % (R, view, view, T, N, G, " (default)" if G == Gd and G not in grids else "", pairs, pairs / max(T, 1), outside,
                        med["build"], min(times["build"]), med["cast"], min(times["cast"]), N / med["cast"] / 1e3, int((tri >= 0).sum()), V, Gd,
                        med["dist"], V / med["dist"] / 1e3, med["copy"], ws.numel() / 1e6, grids[0], got == first, r_, w_))
        print(lines[-1], flush=True)
        del ws
    if 1 in cast_ms:
        lines.append("mesh ray R=%d sphere: cast at G=1 %.3f ms / cast at the default G=%d %.3f ms = %.1f"
                     % (R, cast_ms[1], Gd, cast_ms[Gd], cast_ms[1] / cast_ms[Gd]))
        print(lines[-1], flush=True)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--view", type=int, default=800)
    ap.add_argument("--grids", default="16,32,64,128,256")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mesh_ray.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_mesh_ray.py measures on a GPU; there is no CPU path"
    lines = bench(a.size, a.view, [int(g) for g in a.grids.split(",")], torch.device("cuda:0"), a.reps, a.warmup)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
