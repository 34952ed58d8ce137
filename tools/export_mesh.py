#!/usr/bin/env python3
"""A checkpoint as a triangle mesh: the density of the model, sampled on a resolution^3 lattice of its inference box and meshed on
the device (pvd/mesh.py, csrc/mesh.hip), written as a binary PLY.

  python tools/train_distill.py --save-student student.pth [--save-teacher teacher.pth]
  python tools/export_mesh.py student.pth --model-type vm -o student.ply [--resolution 256 --threshold T --resolution0 300]
                              [--min-component N] [--largest-only] [--normals] [--colors] [--simplify G [--simplify-report]]

The checkpoint is the reference's format (pvd/checkpoint.py); --model-type and the size flags must describe the model that wrote it.
The threshold defaults to min(density_thresh, mean_density) of the loaded model (density_thresh where the file carries no mean).
--min-component N drops the connected components of the inside set with fewer than N lattice points ("floaters"), --largest-only
all but the largest one, before meshing (csrc/components.hip); the components found and kept are printed.
--normals adds a smooth unit normal per vertex (nx ny nz: the gradient of the density volume, pvd_mesh_normals), --colors the
model's own colour at the vertex, seen along the normal (red green blue; it computes the normals whether or not they are written).
--simplify G makes the mesh smaller by vertex clustering on G^3 cells of the box (csrc/mesh_simplify.hip; normals and colours are
averaged with the positions; duplicate triangles are not merged and the result is not guaranteed manifold) and prints the vertices
and triangles before and after; --simplify-report also measures the simplified mesh against the original (compare_meshes over the
vertices: Hausdorff, Chamfer) and prints the result next to the cell diagonal, which bounds the former."""
import argparse
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "aaai2023-pvd_amd")]

from pvd.checkpoint import load_student_checkpoint  # noqa: E402
from pvd.config import PVDConfig  # noqa: E402
from pvd.mesh import compare_meshes, default_threshold, extract_mesh, extract_surface, write_ply  # noqa: E402
from pvd.ops import hip_ops  # noqa: E402
from pvd.workload import make_model  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("checkpoint")
    ap.add_argument("-o", "--out", default=None, help="PLY path (default: the checkpoint's name with .ply)")
    ap.add_argument("--model-type", default="vm", choices=["hash", "mlp", "vm", "tensors"])
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--threshold", type=float, default=None)
    ap.add_argument("--resolution0", type=int, default=PVDConfig.resolution0, help="VM: initial resolution (the file's own is loaded)")
    ap.add_argument("--plenoxel-res", default=PVDConfig.plenoxel_res)
    ap.add_argument("--min-component", type=int, default=0, help="drop components of fewer lattice points before meshing")
    ap.add_argument("--largest-only", action="store_true", help="keep the largest component only")
    ap.add_argument("--normals", action="store_true", help="write a unit normal per vertex (nx ny nz)")
    ap.add_argument("--colors", action="store_true", help="write the model's colour per vertex (red green blue)")
    ap.add_argument("--simplify", type=int, default=0, metavar="G", help="cluster the vertices on G^3 cells of the box (1 .. 512)")
    ap.add_argument("--simplify-report", action="store_true", help="measure the simplified mesh against the original")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    opt = PVDConfig(model_type=a.model_type, resolution0=a.resolution0, plenoxel_res=a.plenoxel_res)
    model = make_model(hip_ops(), opt, a.model_type, False, dev)
    missing, unexpected = load_student_checkpoint(model, None, a.checkpoint)
    if missing or unexpected:
        print("state-dict keys missing %s, unexpected %s" % (missing, unexpected), file=sys.stderr)
    model.eval()
    thresh = default_threshold(model) if a.threshold is None else a.threshold
    filtering = a.min_component > 0 or a.largest_only
    m = extract_surface(model, resolution=a.resolution, threshold=thresh, min_points=a.min_component, largest_only=a.largest_only,
                        normals=a.normals, colors=a.colors, simplify=a.simplify)
    out = a.out or os.path.splitext(a.checkpoint)[0] + ".ply"
    write_ply(out, m["vertices"], m["triangles"], normals=m["normals"], colors=m["colors"])
    carries = "positions" + (", normals" if a.normals else "") + (", colours" if a.colors else "")
    print("%s: %d vertices (%s), %d triangles at density %.6g, resolution %d"
          % (out, m["vertices"].shape[0], carries, m["triangles"].shape[0], thresh, a.resolution))
    if filtering:
        print("components: %d found, %d kept, %d points kept" % m["counts"])
    if a.simplify > 0:
        print("simplify G=%d: %d -> %d vertices, %d -> %d triangles"
              % (a.simplify, m["full_counts"][0], m["vertices"].shape[0], m["full_counts"][1], m["triangles"].shape[0]))
        if a.simplify_report:
            aabb = model.aabb_infer
            full_v, full_t = extract_mesh(m["field"], thresh, aabb[:3], aabb[3:])
            diagonal = float((aabb[3:] - aabb[:3]).double().norm()) / a.simplify
            d = compare_meshes(full_v, full_t, m["vertices"], m["triangles"], tau=diagonal)
            print("simplified against original: hausdorff %.6g, chamfer %.6g, cell diagonal %.6g" % (d["hausdorff"], d["chamfer"], diagonal))


if __name__ == "__main__":
    main()
