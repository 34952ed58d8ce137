#!/usr/bin/env python3
"""How far apart two meshes are: one-sided mean distances, Chamfer and Hausdorff distance, precision / recall / F-score at a
tolerance, measured on the device (pvd/mesh.py: compare_meshes; csrc/mesh_dist.hip).  Reads the PLY files write_ply writes.

  python tools/compare_meshes.py a.ply b.ply --tau 0.01 [--samples 100000 --seed 0 --max-dist D] [--volume R]

Prints the result as one JSON line.  Without --samples the points are the meshes' vertices.  --volume R adds the volume overlap of
the two meshes voxelised on one R^3 lattice over their joint bounding box (csrc/mesh_winding.hip): iou, volume_a, volume_b, and
leaky_a, leaky_b -- not 0 for a mesh that is open or inconsistently oriented, whose volume figures mean little."""
import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "aaai2023-pvd_amd")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("--tau", type=float, required=True, help="tolerance of precision / recall / F-score, in the meshes' units")
    ap.add_argument("--samples", type=int, default=0, help="surface samples per mesh (0: the vertices)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--max-dist", type=float, default=None, help="search radius (default: the diagonal of the joint bounding box)")
    ap.add_argument("--volume", type=int, default=0, help="also voxelise both meshes at this resolution (2 .. 1024) and report the overlap")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "compare_meshes.py measures on a GPU; there is no CPU path"
    from pvd.mesh import compare_meshes, read_ply
    dev = torch.device("cuda:0")
    va, ta = (t.to(dev) for t in read_ply(a.a)[:2])
    vb, tb = (t.to(dev) for t in read_ply(a.b)[:2])
    print(json.dumps(compare_meshes(va, ta, vb, tb, a.tau, max_dist=a.max_dist, samples=a.samples, seed=a.seed, volume=a.volume)))


if __name__ == "__main__":
    main()
