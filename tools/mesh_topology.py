#!/usr/bin/env python3
"""The topology report of a PLY file: one JSON line of pvd.mesh.mesh_topology (csrc/mesh_topo.hip, include/pvd_hip_mesh_topo.h).

  python tools/mesh_topology.py a.ply [b.ply ...]

valid / invalid / duplicate / cancelled triangles, survivors, referenced vertices, edges and how many of them are boundary,
inconsistent, non-manifold and unbalanced, shells and the largest one, euler, closed, manifold; the file's name is added as "path".
The mesh is read with read_ply (the PLY files write_ply makes) and examined on the device."""
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "aaai2023-pvd_amd")]

from pvd.mesh import mesh_topology, read_ply  # noqa: E402


def main():
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    dev = torch.device("cuda:0")
    for path in sys.argv[1:]:
        vertices, triangles = read_ply(path)[:2]
        top = mesh_topology(vertices.to(dev), triangles.to(dev))
        print(json.dumps(dict(top, path=path)))


if __name__ == "__main__":
    main()
