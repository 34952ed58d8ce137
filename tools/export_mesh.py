#!/usr/bin/env python3
"""A checkpoint as a triangle mesh: the density of the model, sampled on a resolution^3 lattice of its inference box and meshed on
the device (pvd/mesh.py, csrc/mesh.hip), written as a binary PLY.

  python tools/train_distill.py --save-student student.pth [--save-teacher teacher.pth]
  python tools/export_mesh.py student.pth --model-type vm -o student.ply [--resolution 256 --threshold T --resolution0 300]
                              [--min-component N] [--largest-only] [--normals] [--colors] [--simplify G [--simplify-report]]
                              [--smooth N [--smooth-lambda L --smooth-mu M] [--smooth-report]] [--render-check N]
                              [--clean [--min-shell N] [--largest-shell-only]] [--topology-report] [--texture S [--texture-sh L]] [--texture-density D]
                              [--cull-hidden {shells,triangles} [--exposure-dirs D --exposure-samples S] [--exposure-report]]
                              [--tsdf N [--tsdf-res HxW] [--tsdf-trunc K]] [--mesher {tetrahedra,nets}]

The checkpoint is the reference's format (pvd/checkpoint.py); --model-type and the size flags must describe the model that wrote it.
The threshold defaults to min(density_thresh, mean_density) of the loaded model (density_thresh where the file carries no mean).
--min-component N drops the connected components of the inside set with fewer than N lattice points ("floaters"), --largest-only
all but the largest one, before meshing (csrc/components.hip); the components found and kept are printed.
--normals adds a smooth unit normal per vertex (nx ny nz: the gradient of the density volume, pvd_mesh_normals), --colors the
model's own colour at the vertex, seen along the normal (red green blue; it computes the normals whether or not they are written).
--simplify G makes the mesh smaller by vertex clustering on G^3 cells of the box (csrc/mesh_simplify.hip; normals and colours are
averaged with the positions; duplicate triangles are not merged and the result is not guaranteed manifold) and prints the vertices
and triangles before and after; --simplify-report also measures the simplified mesh against the original (compare_meshes over the
vertices: Hausdorff, Chamfer) and prints the result next to the cell diagonal, which bounds the former.
--smooth N runs N iterations of Taubin's lambda|mu filter over the vertices before any simplification (pvd/mesh.py: smooth_mesh,
csrc/mesh_smooth.hip; weights --smooth-lambda 0.5 and --smooth-mu -0.53): the staircase of the lattice goes, the triangles stay as
they are, the colours are those of the unsmoothed vertices and the normals written are recomputed from the faces.  --smooth-report
prints two lines: the Hausdorff and Chamfer distance of the smoothed mesh to the unsmoothed one (compare_meshes over the vertices)
next to the lattice spacing, and the volume the mesh encloses before and after (signed tetrahedra, float64).
--render-check N (needs --colors) renders the coloured mesh (pvd/mesh.py: render_mesh, csrc/mesh_ray.hip) and the model itself from N
pose_spherical views at 200 x 200 and prints the PSNR and SSIM of the mesh's image against the model's volume render, and the mean
absolute difference of the two depths over the pixels where both hit.  Both depths are distances along the ray in world units: the
mesh's is the ray cast's t (unit directions); the model's render returns its composited depth normalised to the ray's interval in
the inference box, clamp(depth - near, 0) / (far - near), and is brought back with near + depth * (far - near), near and far from the
model's own slab test (aabb_infer, min_near).  The composited depth is the weight-summed sample distance, not divided by the
opacity, so it falls short of the surface where the model is not opaque.
--clean runs clean_mesh (pvd/mesh.py, csrc/mesh_topo.hip) last, on the mesh about to be written: invalid and duplicate triangles go,
collapsed sheets -- the duplicates --simplify leaves -- cancel, --min-shell N drops the shells of fewer than N triangles and
--largest-shell-only all but the largest one.  --topology-report prints one JSON line of mesh_topology for the mesh about to be
written (triangle, edge and shell counts, euler, closed, manifold); with --clean two lines, before and after the clean-up.
--texture S bakes a texture atlas for the mesh about to be written (pvd/mesh.py: bake_texture, csrc/mesh_tex.hip: S x S texels per pair of
triangles, S 4 .. 64, the model's colour at the surface point of every texel) and writes an .obj, an .mtl and a .png next to the PLY.
With --render-check N it prints the PSNR and SSIM of three renders against the model's own: the textured mesh, the same mesh with its
vertex colours, and the full-resolution mesh (no --simplify) with its vertex colours -- what the texture wins back of what the
simplification lost.
--cull-hidden shells|triangles drops the geometry no outside view can see (pvd/mesh.py: cull_hidden, csrc/mesh_expose.hip: rays from
--exposure-samples 1 or 4 points of every triangle along --exposure-dirs D directions of a Fibonacci sphere, default 64; a triangle is
exposed when a ray from its front escapes): `shells` drops a shell only when none of its triangles is exposed and keeps a closed mesh
closed, `triangles` drops every unexposed triangle and opens the surface.  It runs after --smooth, --simplify and --clean and BEFORE the
normals are recomputed, the colours are taken and the --texture atlas is baked -- that order is the point: a hidden triangle costs S^2 / 2
texels and as many evaluations of the model.  (With it the colours are therefore those at the vertices of the final mesh.)
--exposure-report prints one JSON line, cull_hidden's report: triangles and vertices before and after, hidden triangles, shells before
and dropped, the ray totals; with --texture also atlas_before and atlas_after, [width, height] of the atlas without and with the cull.
--texture-density D bakes onto an area-adaptive atlas instead (pvd/mesh.py: adaptive_atlas, csrc/mesh_atex.hip): every triangle gets the
smallest cell edge of 4, 8, 16, 32, 64 texels that gives it D texels per unit length along its longest edge (--texture S, one of these, is
then the largest cell edge allowed), and the triangles of one cell size share a band of the image.  It prints the triangles per cell size,
how many were capped, the atlas size and its fill; .obj, .mtl, .png and --render-check work as with --texture.  Not with --texture-sh.
--texture-sh L (1 .. 4, needs --texture S) bakes a view-dependent atlas instead (pvd/mesh.py: bake_sh_texture, csrc/mesh_shtex.hip): L * L
spherical-harmonics coefficients per channel and texel, fitted to the model's colour along 64 directions.  The .png / .obj / .mtl are
written from its view-independent part; the coefficients go to <stem>.shtex.npy ([height, width, L * L, 3] float32, numpy.save) with a
one-line JSON sidecar <stem>.shtex.json carrying S, L and T.  With --render-check N a fourth render is reported next to the three: the
SH-textured mesh, coloured at every pixel for that pixel's ray (the flat atlas of the first line is then baked as well, for the check only).
--tsdf N takes the geometry from what the model RENDERS instead of from a density level: depth and colour maps of N cameras on a Fibonacci
sphere (pvd/mesh.py: tsdf_poses, render_depth_maps; --tsdf-res HxW pixels each, default 400x400) are fused into a truncated signed
distance volume on the same lattice (tsdf_integrate, csrc/mesh_tsdf.hip; the truncation distance is --tsdf-trunc K lattice spacings,
default 3) and its zero level is meshed (extract_surface_tsdf).  No density threshold takes part, what any camera sees through is
carved empty, and --colors are the fused colours of the views -- except with --cull-hidden, which takes the colours after the cull, from
the model's colour head at the vertices that are left, as it does without --tsdf (textures are always baked from the model).  Every other
flag works as before, on that mesh; --threshold is ignored.
With --render-check the line's mean |depth difference| then measures the fused surface against the model's own composited depth.

--project-views N [--project-size HW] [--project-best]: the vertex colours (--colors) and the atlas (--texture S) are taken from N
rendered views (tsdf_poses; the colour maps of render_depth_maps, weighted by the opacity) projected onto the mesh with an occlusion
test (pvd/mesh.py: project_views; csrc/mesh_project.hip), blended by cos^2 times the opacity or, with --project-best, taken from the
best view; the model's colour head seen straight on is only the fallback where no view sees a point.  --render-check reports its usual
lines, so the two bakes can be compared.  (With --simplify the third line's full-resolution mesh keeps the colour head's colours.)
--project-data DIR [--project-split train] [--project-downscale K] projects the photographs of a Blender-format scene with their own
poses (pvd.provider.BlenderScene) instead of renders; an alpha channel is the weight image.
--mesher nets extracts the surface with naive surface nets (pvd/mesh.py: extract_mesh(method="nets"), csrc/mesh_nets.hip: one vertex per
active cell, two triangles per crossing lattice edge -- a fraction of the triangles and no slivers, but not manifold at ambiguous lattice
faces and open where the surface leaves the box) instead of marching tetrahedra, the default.  Every other flag works on the result;
--min-component and --largest-only still follow the tetrahedra's connectivity."""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "aaai2023-pvd_amd")]

from pvd.checkpoint import load_student_checkpoint  # noqa: E402
from pvd.config import PVDConfig  # noqa: E402
from pvd.mesh import (bake_texture, compare_meshes, default_threshold, extract_mesh, extract_surface, extract_surface_tsdf, mesh_topology,  # noqa: E402
                      render_mesh, smooth_mesh, tsdf_poses, write_obj, write_ply, write_png)
from pvd.ops import hip_ops  # noqa: E402
from pvd.workload import make_model  # noqa: E402


@torch.no_grad()
def render_check(model, m, views, res=200, textured=False, texture=None):
    """textured: the mesh is coloured from m["texture"] (render_mesh's texture; `texture` where given: a flat or an SH atlas at the
    cell edge m["texture_cell"]) instead of m["colors"].
    (ImageMeter report of the mesh's colour image against the model's render, mean |depth difference| over the pixels both hit,
    their number), over `views` pose_spherical cameras on a circle at the reference's radius and scale.  Depths in world units along
    the ray: the model's normalised depth d is turned back into near + d (far - near) with the near / far of its own slab test."""
    import numpy as np
    from pvd.metrics import ImageMeter
    from pvd.renderer import near_far_from_aabb_torch
    from pvd.scene import BLENDER_INTRINSICS, get_rays, nerf_matrix_to_ngp, pose_spherical
    intr = tuple(v * res / 800.0 for v in BLENDER_INTRINSICS)
    dev = m["vertices"].device
    meter, diff, both = ImageMeter(), torch.zeros((), dtype=torch.float64, device=dev), torch.zeros((), dtype=torch.int64, device=dev)
    for q in range(views):
        pose = torch.from_numpy(nerf_matrix_to_ngp(pose_spherical(-180.0 + 360.0 * q / views, -30.0, 4.0)).astype(np.float32)).to(dev)
        if textured:
            mesh = render_mesh(m["vertices"], m["triangles"], pose, intr, res, res, bg_color=1.0,
                               texture=m["texture"] if texture is None else texture, texture_cell=m["texture_cell"])
        else:
            mesh = render_mesh(m["vertices"], m["triangles"], pose, intr, res, res, colors=m["colors"], bg_color=1.0)
        r = get_rays(pose[None], intr, res, res, -1)
        with torch.autocast("cuda", dtype=torch.float16):
            vol = model.render(r["rays_o"], r["rays_d"], staged=True, bg_color=1, perturb=False, max_steps=1024)
        meter.update(mesh["color"], vol["image"].float().reshape(res, res, 3))
        if vol.get("depth") is not None:
            near, far = near_far_from_aabb_torch(r["rays_o"].reshape(-1, 3), r["rays_d"].reshape(-1, 3), model.aabb_infer.float(),
                                                 float(model.min_near))
            unit = vol["depth"].float().reshape(-1)
            depth = (near + unit * (far - near)).reshape(res, res)
            hit = mesh["mask"] & (unit > 0).reshape(res, res) & (far > near).reshape(res, res)
            diff += torch.where(hit, (mesh["depth"] - depth).abs(), torch.zeros_like(depth)).double().sum()
            both += hit.sum()
    n = int(both)
    return meter.report(), (float(diff) / n if n else float("nan")), n


def _atlas_cell(m, texture, texture_density):
    """What bake_texture takes as S: the integer cell edge, or with texture_density > 0 the adaptive atlas of the mesh in m (texture:
    its largest cell edge where given, 64 otherwise)."""
    if float(texture_density) > 0.0:
        from pvd.mesh import adaptive_atlas
        return adaptive_atlas(m["vertices"], m["triangles"], float(texture_density), max_cell=int(texture) if int(texture) > 0 else 64)
    return int(texture)


@torch.no_grad()
def cull_surface(model, m, mode, n_dirs=64, samples=1, colors=False, texture=0, from_faces=False, texture_sh=0, texture_density=0.0):
    """--cull-hidden: extract_surface's dict m (taken WITHOUT colours and texture) goes through cull_hidden (pvd/mesh.py,
    csrc/mesh_expose.hip) with exposure_directions(n_dirs) and `samples` points per triangle; only then are the normals recomputed
    (from_faces: face_vertex_normals of what is left, for a smoothed mesh; otherwise the normals it has follow the selection), the
    colours taken (colors: vertex_colors at the vertices that are left) and the atlas baked (texture=S): hidden geometry costs neither
    model evaluations nor texels.  vertex_map and triangle_map, where m has them, are composed with cull_hidden's.  Returns
    cull_hidden's report, with mode, directions and samples, and with atlas_before / atlas_after = [width, height] where texture > 0.
    texture_sh=L > 0: the atlas is bake_sh_texture's, under the keys extract_surface(texture_sh=L) uses.  texture_density=D > 0: the
    atlas is the adaptive one of what is left (atlas_after only)."""
    from pvd.mesh import bake_sh_texture, bake_texture, cull_hidden, exposure_directions, face_vertex_normals, texture_layout, vertex_colors
    T0 = int(m["triangles"].shape[0])
    done = cull_hidden(m["vertices"], m["triangles"], normals=m["normals"], mode=mode,
                       dirs=exposure_directions(n_dirs).to(m["vertices"].device), samples=samples)
    report = dict(done["report"], mode=mode, directions=int(n_dirs), samples=int(samples))
    for key in ("vertex_map", "triangle_map"):
        first = m.get(key)
        if first is not None:  # extracted -> simplified / cleaned -> culled
            m[key] = torch.where(first >= 0, done[key][first.clamp(min=0).long()], torch.full_like(first, -1))
        else:
            m[key] = done[key]
    m.update(vertices=done["vertices"], triangles=done["triangles"], normals=done["normals"], exposure=done["counts"])
    if from_faces and m["normals"] is not None:
        m["normals"] = face_vertex_normals(m["vertices"], m["triangles"])
    if colors:
        m["colors"] = vertex_colors(model, m["vertices"], m["normals"])
    if float(texture_density) > 0.0:
        cell = _atlas_cell(m, texture, texture_density)
        report["atlas_after"] = [cell["layout"]["width"], cell["layout"]["height"]]
        baked = bake_texture(model, m["vertices"], m["triangles"], cell, normals=m["normals"])
        m.update(texture=baked["texture"], uv=baked["uv"], texture_cell=cell)
    elif int(texture) > 0:
        for key, T in (("atlas_before", T0), ("atlas_after", int(m["triangles"].shape[0]))):
            lay = texture_layout(T, int(texture))
            report[key] = [lay["width"], lay["height"]]
        if int(texture_sh) > 0:
            baked = bake_sh_texture(model, m["vertices"], m["triangles"], int(texture), degree=int(texture_sh), normals=m["normals"])
            m.update(texture_degree=int(texture_sh), texture_diffuse=baked["diffuse"])
        else:
            baked = bake_texture(model, m["vertices"], m["triangles"], int(texture), normals=m["normals"])
        m.update(texture=baked["texture"], uv=baked["uv"], texture_cell=int(texture))
    return report


def load_view_data(root, split="train", downscale=1, device="cpu"):
    """--project-data DIR: dict(color [V,H,W,3], weight [V,H,W] or None, poses [V,4,4], intrinsics (fx, fy, cx, cy), H, W) of a
    Blender-format scene (transforms_<split>.json and its frames) through pvd.provider.BlenderScene: the photographs and their exact
    poses, in the model's frame (nerf_matrix_to_ngp at the provider's scale).  An alpha channel becomes the weight image -- a
    transparent pixel shows nothing of the surface -- and the colours are un-premultiplied as stored (PNG stores straight alpha)."""
    from pvd.provider import BlenderScene
    scene = BlenderScene(root, split=split, downscale=int(downscale), device=device, preload=True)
    images = scene.images.float()
    weight = images[..., 3].contiguous() if images.shape[-1] == 4 else None
    return dict(color=images[..., :3].contiguous(), weight=weight, poses=scene.poses.float(), intrinsics=tuple(float(v) for v in scene.intrinsics),
                H=int(scene.H), W=int(scene.W))


@torch.no_grad()
def project_surface(model, m, n_views, size=400, best=False, colors=True, texture=0, min_opacity=0.5, views=None, texture_density=0.0):
    """--project-views N: the colours of extract_surface's dict m from what the model RENDERS, not from its colour head seen straight
    on: N tsdf_poses views of size x size are rendered (render_depth_maps: colour maps, and the opacity as the weight image, 0 below
    min_opacity) and projected onto the mesh (pvd/mesh.py: project_views, csrc/mesh_project.hip) -- the vertex colours (colors), and with
    texture=S the atlas through bake_texture(view_source(...)).  views: load_view_data's dict instead (--project-data): photographs.
    Where no view sees a point the model's own colour is the fallback.  Needs m["normals"].  Leaves m["project_seen"] [V] bool with the
    colours and returns dict(views, size, mode, vertices_seen, vertices_unseen)."""
    import math
    from pvd.mesh import project_views, render_depth_maps, vertex_colors, view_source
    dev = m["vertices"].device
    if views is None:
        poses = tsdf_poses(int(n_views)).to(dev)
        focal = 0.5 * size / math.tan(math.radians(25.0))
        intr = (focal, focal, 0.5 * size, 0.5 * size)
        maps = render_depth_maps(model, poses, intr, size, size, min_opacity=min_opacity)
        color = maps["color"]
        weight = torch.where(maps["opacity"] >= float(min_opacity), maps["opacity"], torch.zeros_like(maps["opacity"]))
        shape = [int(size), int(size)]
    else:
        color, weight, poses, intr = views["color"].to(dev), views["weight"], views["poses"].to(dev), views["intrinsics"]
        weight = None if weight is None else weight.to(dev)
        shape = [int(views["H"]), int(views["W"])]
    kw = dict(weight=weight, mode="best" if best else "blend")
    own = lambda x, n: vertex_colors(model, x, n)  # noqa: E731
    report = dict(views=int(color.shape[0]), size=shape[0] if shape[0] == shape[1] else shape, mode=kw["mode"])
    if colors:
        out = project_views(m["vertices"], m["normals"], m["vertices"], m["triangles"], color, poses, intr, fallback=own, **kw)
        m["colors"], m["project_seen"] = out["colors"], out["seen"]
        report.update(vertices_seen=out["totals"]["seen"], vertices_unseen=out["totals"]["unseen"])
    if int(texture) > 0 or float(texture_density) > 0.0:  # (texture_density: the adaptive atlas, _atlas_cell)
        cell = _atlas_cell(m, texture, texture_density)
        baked = bake_texture(view_source(m["vertices"], m["triangles"], color, poses, intr, fallback=own, **kw), m["vertices"],
                             m["triangles"], cell, normals=m["normals"])
        m.update(texture=baked["texture"], uv=baked["uv"], texture_cell=cell)
    return report


def enclosed_volume(vertices, triangles):
    """The volume a closed mesh encloses: the sum of the signed tetrahedra (origin, a, b, c), float64 in torch."""
    c = vertices.to(torch.float64)[triangles.to(torch.int64)]  # [T,3,3]
    return float((c[:, 0] * torch.linalg.cross(c[:, 1], c[:, 2])).sum() / 6.0)


def main(argv=None):
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
    ap.add_argument("--smooth", type=int, default=0, metavar="N", help="Taubin iterations over the vertices (0 .. 1024)")
    ap.add_argument("--smooth-lambda", type=float, default=0.5)
    ap.add_argument("--smooth-mu", type=float, default=-0.53)
    ap.add_argument("--smooth-report", action="store_true", help="measure the smoothed mesh against the unsmoothed one")
    ap.add_argument("--render-check", type=int, default=0, metavar="N",
                    help="render the coloured mesh and the model from N views and print PSNR, SSIM and the depth difference (needs --colors)")
    ap.add_argument("--clean", action="store_true", help="drop invalid and duplicate triangles and cancel collapsed sheets before writing")
    ap.add_argument("--min-shell", type=int, default=0, metavar="N", help="with --clean: drop the shells of fewer than N triangles")
    ap.add_argument("--largest-shell-only", action="store_true", help="with --clean: keep the largest shell only")
    ap.add_argument("--topology-report", action="store_true", help="print mesh_topology of the mesh about to be written as JSON")
    ap.add_argument("--texture", type=int, default=0, metavar="S",
                    help="bake a texture atlas with S x S texels per pair of triangles (4 .. 64) and write .obj, .mtl and .png next to the PLY")
    ap.add_argument("--texture-density", type=float, default=0.0, metavar="D",
                    help="bake onto an area-adaptive atlas instead: D texels per unit length, a cell edge of 4 .. 64 per triangle "
                         "(--texture S, one of 4 8 16 32 64, caps it); writes .obj, .mtl and .png like --texture")
    ap.add_argument("--texture-sh", type=int, default=0, metavar="L",
                    help="with --texture S: bake L * L spherical-harmonics coefficients per texel (1 .. 4), the colour as a function of the view; "
                         "writes <stem>.shtex.npy and .shtex.json next to the .png, which holds the view-independent part")
    ap.add_argument("--cull-hidden", default=None, choices=["shells", "triangles"],
                    help="drop what no outside view can see: whole unexposed shells, or every unexposed triangle (opens the surface)")
    ap.add_argument("--exposure-dirs", type=int, default=64, metavar="D", help="with --cull-hidden: directions of the Fibonacci sphere (1 .. 1024)")
    ap.add_argument("--exposure-samples", type=int, default=1, choices=[1, 4], metavar="S", help="with --cull-hidden: points per triangle (1 or 4)")
    ap.add_argument("--exposure-report", action="store_true", help="with --cull-hidden: print cull_hidden's report as one JSON line")
    ap.add_argument("--tsdf", type=int, default=0, metavar="N", help="fuse the model's depth maps from N views into a TSDF volume and mesh its zero level")
    ap.add_argument("--tsdf-res", default="400x400", metavar="HxW", help="with --tsdf: the size of the rendered depth maps")
    ap.add_argument("--tsdf-trunc", type=float, default=3.0, metavar="K", help="with --tsdf: the truncation distance in lattice spacings")
    ap.add_argument("--project-views", type=int, default=0, metavar="N",
                    help="colour the mesh (--colors, --texture) from N rendered views projected onto it, occlusion-tested, not from the colour head")
    ap.add_argument("--project-size", type=int, default=400, metavar="HW", help="with --project-views: the side of the rendered views")
    ap.add_argument("--project-best", action="store_true", help="with --project-views: take the best view per point instead of blending")
    ap.add_argument("--project-data", default=None, metavar="DIR",
                    help="project the photographs of a Blender-format scene (transforms_<split>.json, read through pvd.provider) instead of renders")
    ap.add_argument("--project-split", default="train", help="with --project-data: train, val, test, trainval or all")
    ap.add_argument("--project-downscale", type=int, default=1, metavar="K", help="with --project-data: read the photographs at 1 / K of their size")
    ap.add_argument("--mesher", default="tetrahedra", choices=["tetrahedra", "nets"],
                    help="marching tetrahedra (watertight, vertices on lattice edges) or naive surface nets (one vertex per cell, fewer triangles)")
    a = ap.parse_args(argv)
    projecting = a.project_views > 0 or a.project_data is not None
    if a.project_views < 0 or (a.project_views > 0 and a.project_data is not None):
        ap.error("--project-views N must not be negative, and it is either N rendered views or --project-data DIR")
    if a.project_views == 0 and a.project_size != 400:
        ap.error("--project-size needs --project-views N, N > 0")
    if not projecting and a.project_best:
        ap.error("--project-best needs --project-views N or --project-data DIR")
    if a.project_data is None and (a.project_split != "train" or a.project_downscale != 1):
        ap.error("--project-split and --project-downscale need --project-data DIR")
    adaptive = a.texture_density > 0.0
    textured = a.texture > 0 or adaptive
    if not a.texture_density >= 0.0 or a.texture_density == float("inf") or (adaptive and (a.texture_sh > 0 or a.texture not in (0, 4, 8, 16, 32, 64))):
        ap.error("--texture-density must be positive and finite, goes with --texture 4, 8, 16, 32 or 64 only, and not with --texture-sh")
    if projecting and (a.texture_sh > 0 or a.cull_hidden or not (a.colors or textured) or a.project_size < 2 or a.project_downscale < 1):
        ap.error("projection needs --colors or --texture, a size of at least 2, and goes with neither --texture-sh nor --cull-hidden")
    if a.tsdf < 0:
        ap.error("--tsdf N: the number of views must not be negative")
    if a.tsdf == 0 and (a.tsdf_res != "400x400" or a.tsdf_trunc != 3.0):
        ap.error("--tsdf-res and --tsdf-trunc need --tsdf N")
    if a.tsdf > 0 and not (a.tsdf_trunc > 0 and len(a.tsdf_res.lower().split("x")) == 2):
        ap.error("--tsdf-res must be HxW and --tsdf-trunc positive")
    if a.cull_hidden is None and (a.exposure_report or a.exposure_dirs != 64 or a.exposure_samples != 1):
        ap.error("--exposure-dirs, --exposure-samples and --exposure-report need --cull-hidden")
    if not 1 <= a.exposure_dirs <= 1024:
        ap.error("--exposure-dirs must be 1 .. 1024")
    if (a.min_shell > 0 or a.largest_shell_only) and not a.clean:
        ap.error("--min-shell and --largest-shell-only need --clean")
    if a.texture_sh != 0 and (a.texture <= 0 or not 1 <= a.texture_sh <= 4):
        ap.error("--texture-sh must be 1 .. 4 and needs --texture S")
    if a.render_check > 0 and not (a.colors or textured):
        ap.error("--render-check needs --colors or --texture")
    dev = torch.device("cuda:0")
    opt = PVDConfig(model_type=a.model_type, resolution0=a.resolution0, plenoxel_res=a.plenoxel_res)
    model = make_model(hip_ops(), opt, a.model_type, False, dev)
    missing, unexpected = load_student_checkpoint(model, None, a.checkpoint)
    if missing or unexpected:
        print("state-dict keys missing %s, unexpected %s" % (missing, unexpected), file=sys.stderr)
    model.eval()
    thresh = default_threshold(model) if a.threshold is None else a.threshold
    filtering = a.min_component > 0 or a.largest_only
    kw = dict(resolution=a.resolution, threshold=thresh, min_points=a.min_component, largest_only=a.largest_only, smooth=a.smooth,
              smooth_lambda=a.smooth_lambda, smooth_mu=a.smooth_mu, clean=a.clean, min_shell_triangles=a.min_shell,
              largest_shell_only=a.largest_shell_only, **(dict(method=a.mesher) if a.mesher != "tetrahedra" else {}))
    compare = textured and a.render_check > 0  # the three renders need the vertex colours too, written or not
    surface = extract_surface
    if a.tsdf > 0:  # the same dict from fused depth maps: the level is 0 of -field, the TSDF being positive outside
        import math
        th, tw = (int(v) for v in a.tsdf_res.lower().split("x"))
        aabb = model.aabb_infer
        focal = 0.5 * tw / math.tan(math.radians(25.0))
        tau = a.tsdf_trunc * float((aabb[3:] - aabb[:3]).max()) / (a.resolution - 1)

        def surface(model, threshold=None, **kwargs):
            m = extract_surface_tsdf(model, tsdf_poses(a.tsdf), (focal, focal, 0.5 * tw, 0.5 * th), th, tw, tau=tau, **kwargs)
            m["field"] = -m["field"]
            return m
        thresh = 0.0
    if a.cull_hidden:  # the geometry first; normals for the colours' sake too; colours and texture after the cull
        m = surface(model, normals=a.normals or a.colors or compare, colors=False, simplify=a.simplify, **kw)
        exposure = cull_surface(model, m, a.cull_hidden, a.exposure_dirs, a.exposure_samples, colors=a.colors or compare, texture=a.texture,
                                from_faces=a.smooth > 0, texture_sh=a.texture_sh, texture_density=a.texture_density)
    else:
        # (with a projection the colours and the atlas come from the views below: the model's own are not taken first)
        m = surface(model, normals=a.normals or projecting, colors=(a.colors or compare) and not projecting, simplify=a.simplify,
                    **(dict(texture=a.texture) if a.texture > 0 and not projecting else {}),
                    **(dict(texture_density=a.texture_density) if adaptive and not projecting else {}),
                    **(dict(texture_sh=a.texture_sh) if a.texture_sh > 0 else {}), **kw)
    if projecting:  # the colours and the atlas from views projected onto the mesh; the model's own colour is only the fallback
        if m["normals"] is None:  # (a surface function that returned none)
            from pvd.mesh import face_vertex_normals
            m["normals"] = face_vertex_normals(m["vertices"], m["triangles"])
        views = None if a.project_data is None else load_view_data(a.project_data, a.project_split, a.project_downscale, dev)
        projected = project_surface(model, m, a.project_views, a.project_size, a.project_best, colors=a.colors or compare, texture=a.texture,
                                    views=views, texture_density=a.texture_density)
        print("projected %d views at %s (%s)%s: %s" % (projected["views"], projected["size"], projected["mode"],
                                                      "" if views is None else " from " + a.project_data,
                                                      json.dumps({k: v for k, v in projected.items() if k.startswith("vertices")})))
    out = a.out or os.path.splitext(a.checkpoint)[0] + ".ply"
    write_ply(out, m["vertices"], m["triangles"], normals=m["normals"] if a.normals else None, colors=m["colors"] if a.colors else None)
    carries = "positions" + (", normals" if a.normals else "") + (", colours" if a.colors else "")
    print("%s: %d vertices (%s), %d triangles at density %.6g, resolution %d"
          % (out, m["vertices"].shape[0], carries, m["triangles"].shape[0], thresh, a.resolution))
    if a.mesher == "nets":
        print("mesher: surface nets (one vertex per active cell; open where the surface leaves the box)")
    if a.tsdf > 0:
        print("tsdf: %d views at %s, truncation %g spacings; voxels %s" % (m["views"], a.tsdf_res, a.tsdf_trunc, json.dumps(m["tsdf_totals"])))
    if filtering:
        print("components: %d found, %d kept, %d points kept" % m["counts"])
    if a.smooth > 0:
        print("smooth: %d iterations, lambda %g, mu %g" % (a.smooth, a.smooth_lambda, a.smooth_mu))
        if a.smooth_report:
            aabb = model.aabb_infer
            raw_v, raw_t = extract_mesh(m["field"], thresh, aabb[:3], aabb[3:], method=a.mesher)
            new_v = smooth_mesh(raw_v, raw_t, iterations=a.smooth, lam=a.smooth_lambda, mu=a.smooth_mu, bmin=aabb[:3], bmax=aabb[3:])
            spacing = float((aabb[3:] - aabb[:3]).double().max()) / (a.resolution - 1)
            d = compare_meshes(raw_v, raw_t, new_v, raw_t, tau=spacing)
            print("smoothed against unsmoothed: hausdorff %.6g, chamfer %.6g, lattice spacing %.6g" % (d["hausdorff"], d["chamfer"], spacing))
            before, after = enclosed_volume(raw_v, raw_t), enclosed_volume(new_v, raw_t)
            print("enclosed volume: %.6g before, %.6g after (%+.3f %%)" % (before, after, 100.0 * (after - before) / before if before else 0.0))
    if a.simplify > 0:
        print("simplify G=%d: %d -> %d vertices, %d -> %d triangles"
              % (a.simplify, m["full_counts"][0], m["vertices"].shape[0], m["full_counts"][1], m["triangles"].shape[0]))
        if a.simplify_report:
            aabb = model.aabb_infer
            full_v, full_t = extract_mesh(m["field"], thresh, aabb[:3], aabb[3:], method=a.mesher)
            diagonal = float((aabb[3:] - aabb[:3]).double().norm()) / a.simplify
            d = compare_meshes(full_v, full_t, m["vertices"], m["triangles"], tau=diagonal)
            print("simplified against original: hausdorff %.6g, chamfer %.6g, cell diagonal %.6g" % (d["hausdorff"], d["chamfer"], diagonal))
    if a.clean:
        before, after = m["topology"]["before"], m["topology"]["after"]
        print("clean: %d -> %d triangles (%d invalid, %d duplicate, %d cancelled), %d -> %d shells"
              % (before["valid"] + before["invalid"], after["survivors"], before["invalid"], before["duplicate"], before["cancelled"],
                 before["shells"], after["shells"]))
    if a.cull_hidden:
        print("cull hidden (%s, %d directions, %d per triangle): %d -> %d triangles, %d -> %d vertices, %d of %d shells dropped"
              % (a.cull_hidden, a.exposure_dirs, a.exposure_samples, exposure["triangles_before"], exposure["triangles_after"],
                 exposure["vertices_before"], exposure["vertices_after"], exposure["shells_dropped"], exposure["shells_before"]))
        if a.exposure_report:
            print(json.dumps(exposure))
    if a.topology_report:
        for top in ((m["topology"]["before"], m["topology"]["after"]) if a.clean else (mesh_topology(m["vertices"], m["triangles"]),)):
            print(json.dumps(top))
    if textured:
        stem = os.path.splitext(out)[0]
        write_png(stem + ".png", m["texture_diffuse"] if a.texture_sh > 0 else m["texture"])
        write_obj(stem + ".obj", m["vertices"], m["triangles"], m["uv"], os.path.basename(stem + ".png"), normals=m["normals"] if a.normals else None)
        if adaptive:
            atlas = m["texture_cell"]
            proper = sum(n * (c - 3) ** 2 for n, c in zip(atlas["counts"], atlas["layout"]["cell"])) / 2.0  # the triangles proper: m^2 / 2 each
            print("%s.obj, .mtl, .png: adaptive texture %d x %d at %g texels per unit length; triangles per cell edge %s: %s, %d capped; fill %.1f %%"
                  % (stem, m["texture"].shape[1], m["texture"].shape[0], a.texture_density, "/".join(str(c) for c in atlas["layout"]["cell"]),
                     "/".join(str(n) for n in atlas["counts"]), atlas["capped"],
                     100.0 * proper / (m["texture"].shape[0] * m["texture"].shape[1])))
        else:
            print("%s.obj, .mtl, .png: texture %d x %d, %d x %d texels per pair of triangles"
                  % (stem, m["texture"].shape[1], m["texture"].shape[0], a.texture, a.texture))
        if a.texture_sh > 0:
            np.save(stem + ".shtex.npy", m["texture"].cpu().numpy())
            with open(stem + ".shtex.json", "w") as f:
                f.write(json.dumps(dict(S=a.texture, L=a.texture_sh, T=int(m["triangles"].shape[0]))) + "\n")
            print("%s.shtex.npy, .shtex.json: %d SH coefficients per channel and texel (L = %d); the .png holds the view-independent part"
                  % (stem, a.texture_sh ** 2, a.texture_sh))
    if compare:
        full = surface(model, normals=False, colors=True, **kw) if a.simplify > 0 else m
        renders = [("textured mesh", m, True, None), ("vertex-coloured mesh", m, False, None),
                   ("full-resolution vertex-coloured mesh", full, False, None)]
        if a.texture_sh > 0:  # the first line stays the flat atlas, baked for the check; the fourth is the SH atlas
            flat = bake_texture(model, m["vertices"], m["triangles"], a.texture, normals=m["normals"])["texture"]
            renders[0] = ("textured mesh", m, True, flat)
            renders.append(("SH-textured mesh (L = %d)" % a.texture_sh, m, True, m["texture"]))
        for name, mesh, tex, atlas in renders:
            rep = render_check(model, mesh, a.render_check, textured=tex, texture=atlas)[0]
            print("render check, %d views at 200 x 200, %s (%d triangles) against the model's volume render: PSNR %.2f dB, SSIM %.4f"
                  % (a.render_check, name, mesh["triangles"].shape[0], rep["psnr"], rep["ssim"]))
    elif a.render_check > 0:
        rep, depth_diff, n = render_check(model, m, a.render_check)
        print("render check, %d views at 200 x 200, mesh against the model's volume render: PSNR %.2f dB, SSIM %.4f, mean |depth difference| "
              "%.5f (world units along the ray) over %d pixels both hit" % (a.render_check, rep["psnr"], rep["ssim"], depth_diff, n))


if __name__ == "__main__":
    main()
