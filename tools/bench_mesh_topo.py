#!/usr/bin/env python3
"""Time of the mesh topology report and clean-up (pvd_mesh_topo_*, csrc/mesh_topo.hip) on one GPU.

  python tools/bench_mesh_topo.py [--size 256 --grids 64,128 --reps 20 --warmup 5 --out profiles/mesh_topo.txt]

The meshes are the sphere of radius 0.6 extracted at size^3 and its clusterings by simplify_mesh at the given grids.  hipEvents
around every call, after `warmup` untimed rounds, the median and the minimum over `reps` rounds of
  build   pvd_mesh_topo_build: one memset and 18 launches
  clean   pvd_mesh_topo_clean_count + pvd_mesh_topo_clean_emit without a filter (nine and two launches), the outputs allocated for the
          counts of an untimed first call, so that no read-back sits inside the timed region
  copy    a device copy of the vertex and the triangle array: the memory floor of touching the mesh once
  torch   the same edge census composed in torch: the three directed edges of every triangle packed into 64-bit keys
          (smaller << 32 | larger), torch.unique with counts, the boundary / non-manifold counts from the counts.  It takes every
          triangle as it comes: no validity, no groups, no orientation, no shells.
The totals, flags, shells and maps of the last round are compared bit for bit with those of the first.  Each line ends with the
report itself, and with that of the cleaned mesh.  No gate: the figures are appended to --out."""
import argparse
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "aaai2023-pvd_amd")]


def sphere_mesh(R, dev):
    from pvd.mesh import extract_mesh
    x = torch.linspace(-1.0, 1.0, R, device=dev)
    X, Y, Z = torch.meshgrid(x, x, x, indexing="ij")
    u = (0.6 - torch.sqrt(X ** 2 + Y ** 2 + Z ** 2)).contiguous()
    return extract_mesh(u, 0.0, (-1.0,) * 3, (1.0,) * 3)


def torch_census(tris):
    """(edges, boundary, three or more) from packed keys and torch.unique."""
    t = tris.to(torch.int64)
    u, w = torch.cat([t[:, 0], t[:, 1], t[:, 2]]), torch.cat([t[:, 1], t[:, 2], t[:, 0]])
    keys = (torch.minimum(u, w) << 32) | torch.maximum(u, w)
    _, counts = torch.unique(keys, return_counts=True)
    return torch.stack([torch.tensor(counts.numel(), device=tris.device), (counts == 1).sum(), (counts >= 3).sum()])


def short(d):
    return ("F %d Vr %d E %d euler %d boundary %d inconsistent %d non-manifold %d unbalanced %d duplicate %d cancelled %d shells %d closed %s "
            "manifold %s" % (d["survivors"], d["referenced"], d["edges"], d["euler"], d["boundary"], d["inconsistent"], d["non_manifold"],
                             d["unbalanced"], d["duplicate"], d["cancelled"], d["shells"], d["closed"], d["manifold"]))


def bench(label, verts, tris, reps, warmup):
    import pvd_hip
    from pvd.mesh import clean_mesh
    dev = verts.device
    V, T = int(verts.shape[0]), int(tris.shape[0])
    ws = torch.empty(pvd_hip.mesh_topo_workspace_bytes(V, T), dtype=torch.uint8, device=dev)
    totals, counts = torch.zeros(16, dtype=torch.int64, device=dev), torch.zeros(2, dtype=torch.int64, device=dev)
    flags, shell = torch.empty(T, dtype=torch.uint8, device=dev), torch.empty(V, dtype=torch.int32, device=dev)
    pvd_hip.mesh_topo_build(verts, tris, ws, totals, flags, shell)
    pvd_hip.mesh_topo_clean_count(V, T, ws, 0, False, counts)
    nv, nt = (int(x) for x in counts.tolist())  # the one read-back, outside the timed rounds
    out_v, out_t = torch.empty(nv, 3, device=dev), torch.empty(nt, 3, dtype=torch.int32, device=dev)
    vmap, tmap = torch.empty(V, dtype=torch.int32, device=dev), torch.empty(T, dtype=torch.int32, device=dev)
    copy_v, copy_t = torch.empty_like(verts), torch.empty_like(tris)
    names = ("build", "clean", "copy", "torch")
    times, first, got, census = {k: [] for k in names}, None, None, None
    for it in range(warmup + reps):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(names) + 1)]
        ev[0].record()
        pvd_hip.mesh_topo_build(verts, tris, ws, totals, flags, shell)
        ev[1].record()
        pvd_hip.mesh_topo_clean_count(V, T, ws, 0, False, counts)
        pvd_hip.mesh_topo_clean_emit(verts, tris, ws, out_v, out_t, vmap, tmap)
        ev[2].record()
        copy_v.copy_(verts)
        copy_t.copy_(tris)
        ev[3].record()
        census = torch_census(tris)
        ev[4].record()
        torch.cuda.synchronize()
        if it >= warmup:
            for q, k in enumerate(names):
                times[k].append(ev[q].elapsed_time(ev[q + 1]))
        if it in (0, warmup + reps - 1):
            got = tuple(x.cpu().numpy().tobytes() for x in (totals, flags, shell, counts, out_v, out_t, vmap, tmap))
            first = first or got
    med = {k: float(np.median(v)) for k, v in times.items()}
    done = clean_mesh(verts, tris)
    e, b, n3 = (int(x) for x in census.tolist())
    line = ("mesh topo %s: V=%d T=%d  build %.3f ms (min %.3f)  clean count + emit %.3f ms (min %.3f) -> V'=%d T'=%d  copy of vertices and "
            "triangles %.3f ms (min %.3f)  torch edge census (packed keys, unique with counts) %.3f ms (min %.3f): edges %d boundary %d three "
            "or more %d  workspace %.1f MB  bits equal from first to last round: %s  [median of %d, %d warm-up]  report: %s  after clean: %s"
            % (label, V, T, med["build"], min(times["build"]), med["clean"], min(times["clean"]), nv, nt, med["copy"], min(times["copy"]),
               med["torch"], min(times["torch"]), e, b, n3, ws.numel() / 1e6, got == first, reps, warmup, short(done["before"]),
               short(done["after"])))
    print(line, flush=True)
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--grids", default="64,128")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mesh_topo.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_mesh_topo.py measures on a GPU; there is no CPU path"
    from pvd.mesh import simplify_mesh
    dev = torch.device("cuda:0")
    verts, tris = sphere_mesh(a.size, dev)
    lines = [bench("R=%d sphere" % a.size, verts, tris, a.reps, a.warmup)]
    for G in (int(g) for g in a.grids.split(",") if g):
        small = simplify_mesh(verts, tris, G, bmin=(-1.0,) * 3, bmax=(1.0,) * 3)
        lines.append(bench("R=%d sphere clustered at G=%d" % (a.size, G), small["vertices"], small["triangles"], a.reps, a.warmup))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
