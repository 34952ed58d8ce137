#!/usr/bin/env python3
"""Time of the exposure query (pvd_mesh_expose, csrc/mesh_expose.hip) on one GPU, next to the only way to get its result without it.

  python tools/bench_mesh_expose.py [--size 256 --grids 32,64,128,256 --dirs 64 --reps 5 --warmup 2 --out profiles/mesh_expose.txt]

Two meshes: the sphere of radius 0.6 extracted at size^3 (the mesh of tools/bench_mesh_dist.py) and a hollow variant of it (a
spherical shell, radii 0.6 and 0.35: the cavity wall is hidden).  Per mesh and G, hipEvents around every call, after `warmup` untimed
rounds, the median and the minimum over `reps` rounds of
  expose    pvd_mesh_expose at D directions, S = 1: one launch, one wave per triangle, the rays never leave the registers
  compose   the same rays through pvd_mesh_ray_cast: centroids, side test and the T x D rays built in torch (24 T D bytes, a chunk of
            triangles at a time), the first hit from t_min = 2^-20 of the box's diagonal (the cast cannot leave out the ray's own
            triangle), the four counts by torch sums.  Its exposed set is compared with the kernel's, not expected to be equal to the bit
  copy      a device copy of the triangle array (T * 12 B read and written): the memory floor of touching the mesh once
The build of the grid is outside all three (both queries read the same workspace).  The counts of every G are compared byte for byte with
those of the first; the default grid of the mesh (pvd/mesh.py: default_grid) is tagged, and added where --grids does not hold it.  Within a
round the kernel runs before the composition.  The last line per mesh states compose / expose at the default grid.  No gate: the figures are appended to --out."""
import argparse
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "aaai2023-pvd_amd"), os.path.join(REPO, "tools")]
CHUNK = 1 << 16  # triangles per cast of the composition: 4.2 M rays at D = 64


def hollow_mesh(R, dev):
    from pvd.mesh import extract_mesh
    x = torch.linspace(-1.0, 1.0, R, device=dev)
    X, Y, Z = torch.meshgrid(x, x, x, indexing="ij")
    r = torch.sqrt(X ** 2 + Y ** 2 + Z ** 2)
    return extract_mesh(torch.minimum(0.6 - r, r - 0.35).contiguous(), 0.0, (-1.0,) * 3, (1.0,) * 3)


def compose(verts, tris, dirs, T, G, pairs, ws, t_min):
    """counts [T,4] int32 from pvd_mesh_ray_cast, the rays built in torch."""
    import pvd_hip
    D = int(dirs.shape[0])
    counts = torch.empty(T, 4, dtype=torch.int32, device=verts.device)
    for s in range(0, T, CHUNK):
        c = verts[tris[s:s + CHUNK].long()]  # [n,3,3]
        n = c.shape[0]
        o = c.double().mean(dim=1).float()
        side = torch.linalg.cross((c[:, 1] - c[:, 0]).double(), (c[:, 2] - c[:, 0]).double()) @ dirs.double().T  # [n,D]
        ro = o[:, None, :].expand(n, D, 3).reshape(-1, 3).contiguous()
        rd = dirs[None, :, :].expand(n, D, 3).reshape(-1, 3).contiguous()
        t = torch.empty(n * D, device=verts.device)
        tri = torch.empty(n * D, dtype=torch.int32, device=verts.device)
        bary = torch.empty(n * D, 2, device=verts.device)
        pvd_hip.mesh_ray_cast(ro, rd, T, G, pairs, ws, t_min, float("inf"), t, tri, bary)
        esc = (tri < 0).reshape(n, D)
        front, back = side > 0, side < 0
        counts[s:s + n] = torch.stack([front.sum(1), (front & esc).sum(1), back.sum(1), (back & esc).sum(1)], dim=1).to(torch.int32)
    return counts


def bench(name, verts, tris, grids, D, dev, reps, warmup):
    import pvd_hip
    from pvd.mesh import _finite_box, default_grid, exposure_directions
    T = int(tris.shape[0])
    lo, hi = _finite_box(verts)
    t_min = float(torch.linalg.norm(hi - lo)) * 2.0 ** -20
    dirs = exposure_directions(D).to(dev)
    copy = torch.empty_like(tris)
    totals2 = torch.zeros(2, dtype=torch.int64, device=dev)
    Gd = default_grid(T)
    lines, first, ratio = [], None, None
    for G in grids + ([] if Gd in grids else [Gd]):
        pvd_hip.mesh_ray_count(verts, tris, lo, hi, G, totals2)
        pairs = int(totals2.tolist()[0])
        ws = torch.empty(pvd_hip.mesh_ray_workspace_bytes(T, G, pairs), dtype=torch.uint8, device=dev)
        pvd_hip.mesh_ray_build(verts, tris, lo, hi, G, pairs, ws)
        counts = torch.empty(T, 4, dtype=torch.int32, device=dev)
        totals = torch.zeros(5, dtype=torch.int64, device=dev)
        times = {"expose": [], "compose": [], "copy": []}
        for it in range(warmup + reps):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            totals.zero_()
            ev[0].record()
            pvd_hip.mesh_expose(dirs, 1, 0, T, T, G, pairs, ws, counts, totals)
            ev[1].record()
            composed = compose(verts, tris, dirs, T, G, pairs, ws, t_min)
            ev[2].record()
            copy.copy_(tris)
            ev[3].record()
            torch.cuda.synchronize()
            if it >= warmup:
                for q, k in enumerate(("expose", "compose", "copy")):
                    times[k].append(ev[q].elapsed_time(ev[q + 1]))
        got = counts.cpu().numpy().tobytes()
        first = first or got
        med = {k: float(np.median(v)) for k, v in times.items()}
        tot = dict(zip(pvd_hip.MESH_EXPOSE_TOTALS, totals.tolist()))
        agree = int(((counts[:, 1] > 0) == (composed[:, 1] > 0)).sum())
        if G == Gd:
            ratio = med["compose"] / med["expose"]
        lines.append("mesh expose R=%s %s: T=%d D=%d S=1 G=%d%s  pairs %d  expose %.2f ms (min %.2f)  %.1f M rays/s  mesh_raycast composition "
                     "%.2f ms (min %.2f)  composition / expose %.2f  copy of the triangles %.3f ms  rays cast %d escaped %d  front-exposed %d "
                     "hidden %d  the composition's exposed set agrees on %d of %d triangles  bytes equal to G=%d: %s  [median of %d, %d warm-up]"
                     % (name[0], name[1], T, D, G, " (default)" if G == Gd else "", pairs, med["expose"], min(times["expose"]),
                        tot["rays_cast"] / med["expose"] / 1e3, med["compose"], min(times["compose"]), med["compose"] / med["expose"], med["copy"],
                        tot["rays_cast"], tot["rays_escaped"], tot["front_exposed"], tot["hidden"], agree, T, grids[0], got == first, reps, warmup))
        print(lines[-1], flush=True)
        del ws
    lines.append("mesh expose R=%s %s: at the default G=%d the mesh_raycast composition takes %.2f times the kernel's time (%s)"
                 % (name[0], name[1], Gd, ratio, "the kernel is faster" if ratio > 1 else "THE KERNEL IS NOT FASTER"))
    print(lines[-1], flush=True)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--grids", default="32,64,128,256")
    ap.add_argument("--dirs", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mesh_expose.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_mesh_expose.py measures on a GPU; there is no CPU path"
    from bench_mesh_dist import sphere_mesh
    dev = torch.device("cuda:0")
    grids = [int(g) for g in a.grids.split(",")]
    lines = []
    for name, (verts, tris) in (("sphere", sphere_mesh(a.size, (0.0, 0.0, 0.0), dev)), ("hollow", hollow_mesh(a.size, dev))):
        lines += bench((a.size, name), verts, tris, grids, a.dirs, dev, a.reps, a.warmup)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
