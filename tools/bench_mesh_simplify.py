#!/usr/bin/env python3
"""Time of the vertex clustering (pvd_mesh_simplify_count / pvd_mesh_simplify_emit, csrc/mesh_simplify.hip) on one GPU.

  python tools/bench_mesh_simplify.py [--size 256 --grids 32,64,128,256 --reps 20 --warmup 5 --out profiles/mesh_simplify.txt]

The mesh is the sphere of radius 0.6 extracted at size^3 with its normals and a colour made of the position (six attributes), the
box the extraction box.  Per G, hipEvents around every call, after `warmup` untimed rounds, the median and the minimum over `reps`
rounds of
  count   pvd_mesh_simplify_count: the memset of the cell flags, cells, triangle flags, and the two scans (eight launches)
  emit    pvd_mesh_simplify_emit: the memset of the sums, the 64-bit atomic gather, the means, the remapped triangles
  copy    a device copy of the vertex and the triangle array: the memory floor of touching the mesh once
next to the reduction (vertices and triangles after / before) and the measured distance between the two meshes (compare_meshes over
the vertices: Hausdorff, Chamfer) with the cell diagonal that bounds the former.  The outputs of the last round are compared bit for
bit with those of the first.  Only the plain atomics are built: a wave-level pre-sum of equal cells is not, so there is no A/B.
No gate: the figures are appended to --out."""
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
    return extract_mesh(u, 0.0, (-1.0,) * 3, (1.0,) * 3, with_normals=True)


def bench(R, grids, dev, reps, warmup):
    import pvd_hip
    from pvd.mesh import compare_meshes
    verts, tris, normals = sphere_mesh(R, dev)
    V, T = int(verts.shape[0]), int(tris.shape[0])
    attrs = torch.cat([normals, 0.5 + 0.5 * verts], dim=1).contiguous()
    K = int(attrs.shape[1])
    lo, hi = torch.full((3,), -1.0, device=dev), torch.full((3,), 1.0, device=dev)
    copy_v, copy_t = torch.empty_like(verts), torch.empty_like(tris)
    totals = torch.zeros(2, dtype=torch.int32, device=dev)
    vmap = torch.empty(V, dtype=torch.int32, device=dev)
    lines = []
    for G in grids:
        ws = torch.empty(pvd_hip.mesh_simplify_workspace_bytes(V, T, G, K), dtype=torch.uint8, device=dev)
        pvd_hip.mesh_simplify_count(verts, tris, lo, hi, G, K, ws, totals)
        Vn, Tn = (int(x) for x in totals.tolist())
        out_v, out_t = torch.empty(Vn, 3, device=dev), torch.empty(Tn, 3, dtype=torch.int32, device=dev)
        out_a = torch.empty(Vn, K, device=dev)
        times, first = {"count": [], "emit": [], "copy": []}, None
        for it in range(warmup + reps):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            ev[0].record()
            pvd_hip.mesh_simplify_count(verts, tris, lo, hi, G, K, ws, totals)
            ev[1].record()
            pvd_hip.mesh_simplify_emit(verts, tris, attrs, lo, hi, G, ws, out_v, out_a, out_t, vmap)
            ev[2].record()
            copy_v.copy_(verts)
            copy_t.copy_(tris)
            ev[3].record()
            torch.cuda.synchronize()
            if it >= warmup:
                for q, k in enumerate(("count", "emit", "copy")):
                    times[k].append(ev[q].elapsed_time(ev[q + 1]))
            if it in (0, warmup + reps - 1):
                got = tuple(x.cpu().numpy().tobytes() for x in (out_v, out_a, out_t, vmap, totals))
                first = first or got
        med = {k: float(np.median(v)) for k, v in times.items()}
        d = compare_meshes(verts, tris, out_v, out_t, tau=1.0)
        diagonal = float((hi - lo).double().norm()) / G
        lines.append("mesh simplify R=%d sphere: V=%d T=%d K=%d G=%d -> V'=%d T'=%d (%.4f of the vertices, %.4f of the triangles)  "
                     "count %.3f ms (min %.3f)  emit %.3f ms (min %.3f)  %.1f M 64-bit atomics/s in emit  copy of vertices and triangles "
                     "%.3f ms (min %.3f)  workspace %.1f MB  hausdorff %.6f chamfer %.6f cell diagonal %.6f  unmapped vertices %d  "
                     "bits equal from first to last round: %s  plain atomics only (no wave-level pre-sum built)  [median of %d, %d warm-up]"
                     % (R, V, T, K, G, Vn, Tn, Vn / max(V, 1), Tn / max(T, 1), med["count"], min(times["count"]), med["emit"],
                        min(times["emit"]), V * (4 + K) / med["emit"] / 1e3, med["copy"], min(times["copy"]), ws.numel() / 1e6,
                        d["hausdorff"], d["chamfer"], diagonal, int((vmap < 0).sum()), got == first, reps, warmup))
        print(lines[-1], flush=True)
        del ws
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--grids", default="32,64,128,256")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mesh_simplify.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_mesh_simplify.py measures on a GPU; there is no CPU path"
    lines = bench(a.size, [int(g) for g in a.grids.split(",")], torch.device("cuda:0"), a.reps, a.warmup)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
