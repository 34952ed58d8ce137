#!/usr/bin/env python3
"""A PLY mesh as an R^3 volume of winding numbers, made on the device (pvd/mesh.py: voxelize_mesh; csrc/mesh_winding.hip,
include/pvd_hip_mesh_winding.h).  Reads the PLY files write_ply writes.

  python tools/voxelize_mesh.py a.ply --resolution 256 [--bmin x y z --bmax x y z] [--grid G] [--out field.npy]

The lattice lies over the bounding box of the mesh's finite vertices unless --bmin / --bmax say otherwise.  Prints one JSON line:
the four totals (inside: points with w != 0; positive: w > 0; leaky_columns: columns that saw the mesh open or inconsistently
oriented; max_abs), the lattice volume (inside x the volume of a lattice cell) next to the mesh's signed volume (the sum of the
signed tetrahedra, which inconsistently oriented triangles cancel in), and the box.  --out writes (w != 0) as a float32 [R,R,R]
.npy: a field extract_mesh(., 0.5, bmin, bmax), label_components and drop_components accept."""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "aaai2023-pvd_amd")]


def signed_volume(vertices, triangles):
    """The sum over the valid triangles of a . (b x c) / 6, in float64 on the device."""
    v, t = vertices.to(torch.float64), triangles.to(torch.int64)
    ok = ((t >= 0) & (t < v.shape[0])).all(dim=1)
    c = v[t[ok]]
    vol = (c[:, 0] * torch.linalg.cross(c[:, 1], c[:, 2])).sum(dim=1) / 6.0
    return float(vol[torch.isfinite(vol)].sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mesh")
    ap.add_argument("--resolution", type=int, required=True, help="points per axis of the lattice, 2 .. 1024")
    ap.add_argument("--bmin", type=float, nargs=3, default=None)
    ap.add_argument("--bmax", type=float, nargs=3, default=None)
    ap.add_argument("--grid", type=int, default=None, help="cells per axis of the two-dimensional grid (default: default_grid(T))")
    ap.add_argument("--out", default=None, help="write (w != 0) as float32 [R,R,R] to this .npy")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "voxelize_mesh.py runs on a GPU; there is no CPU path"
    from pvd.mesh import _finite_box, read_ply, voxelize_mesh
    dev = torch.device("cuda:0")
    vertices, triangles = (x.to(dev) for x in read_ply(a.mesh)[:2])
    lo, hi = _finite_box(vertices.to(torch.float32).reshape(-1, 3))
    lo = lo if a.bmin is None else torch.tensor(a.bmin, dtype=torch.float32, device=dev)
    hi = hi if a.bmax is None else torch.tensor(a.bmax, dtype=torch.float32, device=dev)
    w, totals = voxelize_mesh(vertices, triangles, a.resolution, lo, hi, grid=a.grid, return_totals=True)
    cell = 1.0
    for l, h in zip(lo.tolist(), hi.tolist()):
        cell *= (h - l) / (a.resolution - 1)
    print(json.dumps(dict(totals, resolution=a.resolution, lattice_volume=totals["inside"] * cell, signed_volume=signed_volume(vertices, triangles),
                          bmin=lo.tolist(), bmax=hi.tolist(), path=a.mesh)))
    if a.out:
        np.save(a.out, (w != 0).to(torch.float32).cpu().numpy())


if __name__ == "__main__":
    main()
