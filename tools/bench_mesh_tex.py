#!/usr/bin/env python3
"""Time of the texture atlas of a mesh (pvd_mesh_tex_points / pvd_mesh_tex_sample, csrc/mesh_tex.hip) on one GPU.

  python tools/bench_mesh_tex.py [--size 256 --cells 8,16 --view 800 --reps 10 --warmup 3 --out profiles/mesh_tex.txt]

The mesh is the sphere of radius 0.6 extracted at size^3 (the mesh of tools/bench_mesh_dist.py).  hipEvents around every call, after
`warmup` untimed rounds, the median and the minimum over `reps` rounds of
  points    pvd_mesh_tex_points over a band of at most 2^24 texels of the atlas at the cell edge S, with vertex normals: 24 B stored per
            texel, next to a device copy of the same number of bytes (which reads them as well)
  sample    pvd_mesh_tex_sample for a view x view image of the mesh (the view of tools/bench_mesh_ray.py; the cast is not timed), next to
            render_mesh's torch gather of the vertex colours for the same hits
  bake      the whole bake_texture at every S with a freshly initialised VM model as the source, split by KernelTimer into the points
            kernel's time and the rest (the model's colour queries, the normalisation and the copies)
No gate: the figures are appended to --out."""
import argparse
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "aaai2023-pvd_amd"), os.path.join(REPO, "tools")]
BAND = 1 << 24


def timed(fn, reps, warmup):
    """(median, minimum) ms of fn() by hipEvents."""
    out = []
    for it in range(warmup + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if it >= warmup:
            out.append(a.elapsed_time(b))
    return float(np.median(out)), float(min(out))


def bench(size, cells, view, dev, reps, warmup):
    import pvd_hip
    from bench_mesh_dist import sphere_mesh
    from pvd.config import PVDConfig
    from pvd.mesh import bake_texture, face_vertex_normals, mesh_raycast, texture_layout
    from pvd.ops import hip_ops
    from pvd.scene import BLENDER_INTRINSICS, get_rays, nerf_matrix_to_ngp, pose_spherical
    from pvd.workload import make_model
    verts, tris = sphere_mesh(size, (0.0, 0.0, 0.0), dev)
    normals = face_vertex_normals(verts, tris)
    T = int(tris.shape[0])
    lines = []
    # ---- the points kernel against a copy of what it stores
    for S in cells:
        lay = texture_layout(T, S)
        Wt, Ht = lay["width"], lay["height"]
        rows = max(1, min(Ht, BAND // Wt))
        n = rows * Wt
        x, nn = torch.empty(n, 3, device=dev), torch.empty(n, 3, device=dev)
        src, dst = torch.empty(2 * n, 3, device=dev), torch.empty(2 * n, 3, device=dev)
        med, low = timed(lambda: pvd_hip.mesh_tex_points(verts, tris, normals, S, 0, rows, x, nn), reps, warmup)
        cmed, clow = timed(lambda: dst.copy_(src), reps, warmup)
        lines.append("mesh tex points %d^3 sphere T=%d, S=%d: atlas %d x %d (%.1f M texels, fill %.0f %%), band of %d rows (%.1f M texels, "
                     "%.1f MB stored)  points %.3f ms (min %.3f)  %.0f GB/s of stores  copy of the same bytes %.3f ms (min %.3f)  "
                     "points / copy = %.2f  [median of %d, %d warm-up]"
                     % (size, T, S, Wt, Ht, Wt * Ht / 1e6, 100.0 * (S - 3) ** 2 / S ** 2, rows, n / 1e6, 24 * n / 1e6, med, low,
                        24 * n / med / 1e6, cmed, clow, med / cmed, reps, warmup))
        print(lines[-1], flush=True)
        del x, nn, src, dst
    # ---- the sample kernel against the torch gather of vertex colours
    pose = torch.from_numpy(nerf_matrix_to_ngp(pose_spherical(35.0, -30.0, 2.5), scale=1.0)).to(dev)
    s = view / 800.0
    r = get_rays(pose[None], tuple(v * s for v in BLENDER_INTRINSICS), view, view, -1)
    o, d = r["rays_o"].reshape(-1, 3).contiguous(), r["rays_d"].reshape(-1, 3).contiguous()
    t, tri, bary = mesh_raycast(o, d, verts, tris)
    N, hits = int(tri.shape[0]), int((tri >= 0).sum())
    colors = torch.rand(verts.shape[0], 3, device=dev)
    bg = torch.ones(3, device=dev)

    def gather():  # render_mesh's colour path
        mask = tri >= 0
        idx = tris.to(torch.int64)[tri.clamp(min=0).to(torch.int64)]
        w = torch.stack([1.0 - bary[:, 0] - bary[:, 1], bary[:, 0], bary[:, 1]], dim=1)
        return torch.where(mask[:, None], (w[:, :, None] * colors[idx]).sum(dim=1), bg[None, :])
    gmed, glow = timed(gather, reps, warmup)
    for S in cells:
        lay = texture_layout(T, S)
        tex = torch.rand(lay["height"], lay["width"], 3, device=dev)
        out = torch.empty(N, 3, device=dev)
        med, low = timed(lambda: pvd_hip.mesh_tex_sample(tex, T, S, tri, bary, bg, out), reps, warmup)
        lines.append("mesh tex sample %d^3 sphere T=%d, S=%d: %d x %d view (%d rays, %d hit), texture %.0f MB  sample %.4f ms (min %.4f)  "
                     "%.0f M rays/s  render_mesh's torch gather of vertex colours %.4f ms (min %.4f)  gather / sample = %.1f  "
                     "[median of %d, %d warm-up]"
                     % (size, T, S, view, view, N, hits, tex.numel() * 4 / 1e6, med, low, N / med / 1e3, gmed, glow, gmed / med, reps, warmup))
        print(lines[-1], flush=True)
        del tex, out
    # ---- the whole bake with a VM model
    opt = PVDConfig(model_type="vm")
    model = make_model(hip_ops(), opt, "vm", False, dev).eval()
    for S in cells:
        lay = texture_layout(T, S)
        bake_texture(model, verts, tris, S, normals=normals)  # warm-up: code objects, the allocator
        torch.cuda.synchronize()
        with pvd_hip.KernelTimer({"pvd_mesh_tex_points"}) as kt:
            t0 = time.perf_counter()
            baked = bake_texture(model, verts, tris, S, normals=normals)
            torch.cuda.synchronize()
            total = (time.perf_counter() - t0) * 1e3
            kernel = kt.total_ms("pvd_mesh_tex_points")
            launches = kt.launches("pvd_mesh_tex_points")
        lines.append("mesh tex bake %d^3 sphere T=%d, S=%d, VM model (untrained): atlas %d x %d (%.1f M texels)  bake_texture %.1f ms  "
                     "points kernel %.3f ms in %d bands  model queries and the rest %.1f ms  [one run after one warm-up]"
                     % (size, T, S, lay["width"], lay["height"], lay["width"] * lay["height"] / 1e6, total, kernel, launches, total - kernel))
        print(lines[-1], flush=True)
        del baked
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--cells", default="8,16")
    ap.add_argument("--view", type=int, default=800)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mesh_tex.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_mesh_tex.py measures on a GPU; there is no CPU path"
    lines = bench(a.size, [int(s) for s in a.cells.split(",")], a.view, torch.device("cuda:0"), a.reps, a.warmup)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
