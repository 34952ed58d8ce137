#!/usr/bin/env python3
"""Time of the area-adaptive texture atlas of a mesh (pvd_mesh_atex_build / _points / _sample, csrc/mesh_atex.hip) on one GPU, next to the
uniform atlas's kernels (csrc/mesh_tex.hip) on the same input.

  python tools/bench_mesh_atex.py [--size 256 --grid 64 --density 96 --view 800 --reps 10 --warmup 3 --inner 200 --out profiles/mesh_atex.txt]

The mesh is the sphere of radius 0.6 extracted at size^3 (the mesh of tools/bench_mesh_dist.py) after simplify_mesh with `grid` cells per
axis and clean_mesh: triangles from about one lattice cell to a cluster's diagonal.  After `warmup` untimed rounds, the median and the
minimum over `reps` rounds of
  build     one call of pvd_mesh_atex_build (three launches) between two hipEvents, next to a device copy of the triangle array
  points    pvd_mesh_atex_points over the whole adaptive atlas, next to pvd_mesh_tex_points (k_mt_points) over the uniform atlas at the cell
            edge S whose texel count is nearest; both as ns per texel too
  sample    pvd_mesh_atex_sample for a view x view image of the mesh (the view of tools/bench_mesh_ray.py; the cast is not timed), next to
            pvd_mesh_tex_sample (k_mt_sample) on the same hits and that S: the adaptive lookup does one more dependent gather per hit
WHAT THE FIGURES ARE.  These kernels last microseconds at this size, so a pair of events around one call of the binding measures the
binding (argument checks, the host-side layout, the launch) as much as the kernel.  points and sample are therefore timed as `inner`
calls back to back between one pair of events, the two versions alternated round by round: the time PER CALL of the binding with the queue
kept full, an upper bound on the kernel's time and still not the kernel's time.  For that, run the tool under a kernel trace in a run of
its own (rocprofv3 --kernel-trace --stats -- python tools/bench_mesh_atex.py --out /dev/null) and read k_ax_* against k_mt_*;
profiles/mesh_atex.txt records both.  No gate: the figures are appended to --out."""
import argparse
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "aaai2023-pvd_amd"), os.path.join(REPO, "tools")]


def timed_pair(fa, fb, reps, warmup, inner):
    """((median, minimum) of fa, the same of fb) in ms per call: `inner` calls back to back between two hipEvents, fa's batch and fb's
    alternated in every round."""
    out = ([], [])
    for it in range(warmup + reps):
        for k, fn in enumerate((fa, fb)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                fn()
            b.record()
            torch.cuda.synchronize()
            if it >= warmup:
                out[k].append(a.elapsed_time(b) / inner)
    return tuple((float(np.median(v)), float(min(v))) for v in out)


def bench(size, grid, density, view, dev, reps, warmup, inner):
    import pvd_hip
    from bench_mesh_dist import sphere_mesh
    from bench_mesh_tex import timed
    from pvd.mesh import adaptive_atlas, clean_mesh, face_vertex_normals, mesh_raycast, simplify_mesh, texture_layout
    from pvd.scene import BLENDER_INTRINSICS, get_rays, nerf_matrix_to_ngp, pose_spherical
    verts, tris = sphere_mesh(size, (0.0, 0.0, 0.0), dev)
    full = int(tris.shape[0])
    small = simplify_mesh(verts, tris, grid, bmin=(-1.0, -1.0, -1.0), bmax=(1.0, 1.0, 1.0))
    done = clean_mesh(small["vertices"], small["triangles"])
    verts, tris = done["vertices"].contiguous(), done["triangles"].contiguous()
    normals = face_vertex_normals(verts, tris)
    T = int(tris.shape[0])
    what = "%d^3 sphere, G=%d clustering, T=%d (of %d)" % (size, grid, T, full)
    lines = []
    # ---- the build against a copy of the triangle array
    slot, order = torch.empty(T, dtype=torch.int32, device=dev), torch.empty(T, dtype=torch.int32, device=dev)
    totals = torch.zeros(6, dtype=torch.int32, device=dev)
    ws = torch.empty(pvd_hip.mesh_atex_workspace_bytes(T), dtype=torch.uint8, device=dev)
    other = torch.empty_like(tris)
    med, low = timed(lambda: pvd_hip.mesh_atex_build(verts, tris, density, 4, ws, slot, order, totals), reps, warmup)
    cmed, clow = timed(lambda: other.copy_(tris), reps, warmup)
    atlas = adaptive_atlas(verts, tris, density)
    lay = atlas["layout"]
    Wt, Ht = lay["width"], lay["height"]
    proper = sum(n * (c - 3) ** 2 for n, c in zip(atlas["counts"], lay["cell"])) / 2.0
    lines.append("mesh atex build %s, density %g: classes %s, %d capped, atlas %d x %d (%.2f M texels, fill %.0f %%)  build %.4f ms (min %.4f)  "
                 "copy of the triangle array %.4f ms (min %.4f)  build / copy = %.1f  [one call between two events: the binding and three launches "
                 "included; median of %d, %d warm-up]"
                 % (what, density, "/".join(str(n) for n in atlas["counts"]), atlas["capped"], Wt, Ht, Wt * Ht / 1e6, 100.0 * proper / (Wt * Ht),
                    med, low, cmed, clow, med / cmed, reps, warmup))
    print(lines[-1], flush=True)
    # ---- the uniform S whose texel count is nearest
    S = min(range(pvd_hip.MESH_TEX_MIN_S, pvd_hip.MESH_TEX_MAX_S + 1),
            key=lambda s: abs(texture_layout(T, s)["width"] * texture_layout(T, s)["height"] - Wt * Ht))
    ulay = texture_layout(T, S)
    Wu, Hu = ulay["width"], ulay["height"]
    # ---- the points kernels
    x, nn = torch.empty(Wt * Ht, 3, device=dev), torch.empty(Wt * Ht, 3, device=dev)
    xu, nu = torch.empty(Wu * Hu, 3, device=dev), torch.empty(Wu * Hu, 3, device=dev)
    (med, low), (umed, ulow) = timed_pair(lambda: pvd_hip.mesh_atex_points(verts, tris, normals, atlas["counts"], atlas["order"], 0, Ht, x, nn),
                                          lambda: pvd_hip.mesh_tex_points(verts, tris, normals, S, 0, Hu, xu, nu), reps, warmup, inner)
    lines.append("mesh atex points %s: adaptive %d x %d (%.2f M texels)  points %.4f ms (min %.4f)  %.3f ns / texel  |  uniform S=%d: %d x %d "
                 "(%.2f M texels)  k_mt_points %.4f ms (min %.4f)  %.3f ns / texel  |  adaptive / uniform per texel = %.2f  "
                 "[per call of the binding, %d calls back to back, alternated; median of %d, %d warm-up]"
                 % (what, Wt, Ht, Wt * Ht / 1e6, med, low, 1e6 * med / (Wt * Ht), S, Wu, Hu, Wu * Hu / 1e6, umed, ulow, 1e6 * umed / (Wu * Hu),
                    (med / (Wt * Ht)) / (umed / (Wu * Hu)), inner, reps, warmup))
    print(lines[-1], flush=True)
    del x, nn, xu, nu
    # ---- the sample kernels on the hits of one view
    pose = torch.from_numpy(nerf_matrix_to_ngp(pose_spherical(35.0, -30.0, 2.5), scale=1.0)).to(dev)
    s = view / 800.0
    r = get_rays(pose[None], tuple(v * s for v in BLENDER_INTRINSICS), view, view, -1)
    o, d = r["rays_o"].reshape(-1, 3).contiguous(), r["rays_d"].reshape(-1, 3).contiguous()
    _, tri, bary = mesh_raycast(o, d, verts, tris)
    N, hits = int(tri.shape[0]), int((tri >= 0).sum())
    bg = torch.ones(3, device=dev)
    tex, texu = torch.rand(Ht, Wt, 3, device=dev), torch.rand(Hu, Wu, 3, device=dev)
    out = torch.empty(N, 3, device=dev)
    (med, low), (umed, ulow) = timed_pair(lambda: pvd_hip.mesh_atex_sample(tex, T, atlas["counts"], atlas["slot"], tri, bary, bg, out),
                                          lambda: pvd_hip.mesh_tex_sample(texu, T, S, tri, bary, bg, out), reps, warmup, inner)
    lines.append("mesh atex sample %s: %d x %d view (%d rays, %d hit)  adaptive %.4f ms (min %.4f)  |  uniform S=%d k_mt_sample %.4f ms "
                 "(min %.4f)  |  adaptive / uniform = %.2f  [per call of the binding, %d calls back to back, alternated; median of %d, %d warm-up]"
                 % (what, view, view, N, hits, med, low, S, umed, ulow, med / umed, inner, reps, warmup))
    print(lines[-1], flush=True)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--grid", type=int, default=64)
    ap.add_argument("--density", type=float, default=96.0)
    ap.add_argument("--view", type=int, default=800)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=200, help="calls back to back between one pair of events (points, sample)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mesh_atex.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_mesh_atex.py measures on a GPU; there is no CPU path"
    lines = bench(a.size, a.grid, a.density, a.view, torch.device("cuda:0"), a.reps, a.warmup, a.inner)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
