#!/usr/bin/env python3
"""Time of the view-dependent texture atlas (pvd_mesh_shtex_*, csrc/mesh_shtex.hip) on one GPU.

  python tools/bench_mesh_shtex.py [--size 256 --cell 8 --view 800 --reps 10 --warmup 3 --out profiles/mesh_shtex.txt]

The mesh is the sphere of radius 0.6 extracted at size^3 (the mesh of tools/bench_mesh_dist.py).  hipEvents around every call, after
`warmup` untimed rounds, the median and the minimum over `reps` rounds of
  sample    pvd_mesh_shtex_sample at L = 1 .. 4 for a view x view image of the mesh (the view of tools/bench_mesh_ray.py; the cast is
            not timed), next to pvd_mesh_tex_sample on the same hits and a flat atlas, and next to a device copy of the bytes the hits
            touch (4 texels of K * 12 B per hit; the copy reads and writes them)
  project   pvd_mesh_shtex_project over 2^20 texels and a batch of 8 directions, per direction, next to a device copy of the
            coefficient array [M,K,3] -- which the kernel writes once per batch, not per direction
  bake      one whole bake_sh_texture (L = 3, the default 64 directions) with a freshly initialised VM model as the source, split by
            KernelTimer into the time of this feature's kernels and the rest (the model's colour queries and the copies)
No gate: the figures are appended to --out."""
import argparse
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "aaai2023-pvd_amd"), os.path.join(REPO, "tools")]
TEXELS, BATCH = 1 << 20, 8


def bench(size, S, view, dev, reps, warmup):
    import pvd_hip
    from bench_mesh_dist import sphere_mesh
    from bench_mesh_tex import timed
    from pvd.config import PVDConfig
    from pvd.mesh import bake_sh_texture, face_vertex_normals, mesh_raycast, texture_layout
    from pvd.ops import hip_ops
    from pvd.scene import BLENDER_INTRINSICS, get_rays, nerf_matrix_to_ngp, pose_spherical
    from pvd.workload import make_model
    verts, tris = sphere_mesh(size, (0.0, 0.0, 0.0), dev)
    normals = face_vertex_normals(verts, tris)
    T = int(tris.shape[0])
    lay = texture_layout(T, S)
    Wt, Ht = lay["width"], lay["height"]
    lines = []
    # ---- the sample kernel against the flat one and a copy of the bytes the hits touch
    pose = torch.from_numpy(nerf_matrix_to_ngp(pose_spherical(35.0, -30.0, 2.5), scale=1.0)).to(dev)
    s = view / 800.0
    r = get_rays(pose[None], tuple(v * s for v in BLENDER_INTRINSICS), view, view, -1)
    o, d = r["rays_o"].reshape(-1, 3).contiguous(), r["rays_d"].reshape(-1, 3).contiguous()
    t, tri, bary = mesh_raycast(o, d, verts, tris)
    N, hits = int(tri.shape[0]), int((tri >= 0).sum())
    bg = torch.ones(3, device=dev)
    out = torch.empty(N, 3, device=dev)
    flat = torch.rand(Ht, Wt, 3, device=dev)
    fmed, flow = timed(lambda: pvd_hip.mesh_tex_sample(flat, T, S, tri, bary, bg, out), reps, warmup)
    del flat
    for L in (1, 2, 3, 4):
        K = L * L
        tex = torch.rand(Ht, Wt, K, 3, device=dev)
        touched = hits * 4 * K * 3  # floats
        src, dst = torch.empty(touched, device=dev), torch.empty(touched, device=dev)
        med, low = timed(lambda: pvd_hip.mesh_shtex_sample(tex, T, S, L, tri, bary, d, bg, out), reps, warmup)
        cmed, clow = timed(lambda: dst.copy_(src), reps, warmup)
        lines.append("mesh shtex sample %d^3 sphere T=%d, S=%d, L=%d (K=%d): %d x %d view (%d rays, %d hit), texture %.0f MB  sample %.4f ms "
                     "(min %.4f)  %.0f M rays/s  flat pvd_mesh_tex_sample on the same hits %.4f ms (min %.4f)  sh / flat = %.2f  copy of the "
                     "%.1f MB the hits touch %.4f ms (min %.4f)  sh / copy = %.2f  [median of %d, %d warm-up]"
                     % (size, T, S, L, K, view, view, N, hits, tex.numel() * 4 / 1e6, med, low, N / med / 1e3, fmed, flow, med / fmed,
                        touched * 4 / 1e6, cmed, clow, med / cmed, reps, warmup))
        print(lines[-1], flush=True)
        del tex, src, dst
    # ---- the projection, per direction, against a copy of the coefficient array
    rgb = torch.rand(BATCH, TEXELS, 3, device=dev)
    for L in (1, 2, 3, 4):
        K = L * L
        P = torch.randn(K, BATCH, device=dev)
        coef, other = torch.zeros(TEXELS, K, 3, device=dev), torch.empty(TEXELS, K, 3, device=dev)
        med, low = timed(lambda: pvd_hip.mesh_shtex_project(rgb, P, L, coef, False), reps, warmup)
        cmed, clow = timed(lambda: other.copy_(coef), reps, warmup)
        lines.append("mesh shtex project L=%d (K=%d), %d texels, batch of %d directions: %.4f ms (min %.4f), %.4f ms per direction  copy of "
                     "the coefficient array (%.1f MB) %.4f ms (min %.4f)  per direction / copy = %.2f, batch / copy = %.2f  [median of %d, "
                     "%d warm-up]"
                     % (L, K, TEXELS, BATCH, med, low, med / BATCH, coef.numel() * 4 / 1e6, cmed, clow, med / BATCH / cmed, med / cmed, reps,
                        warmup))
        print(lines[-1], flush=True)
        del coef, other
    del rgb
    # ---- the whole bake with a VM model
    opt = PVDConfig(model_type="vm")
    model = make_model(hip_ops(), opt, "vm", False, dev).eval()
    names = {"pvd_mesh_tex_points", "pvd_mesh_shtex_dirs", "pvd_mesh_shtex_project"}
    bake_sh_texture(model, verts, tris[:2048], S, degree=3, normals=normals)  # warm-up: code objects, the allocator
    torch.cuda.synchronize()
    with pvd_hip.KernelTimer(names) as kt:
        t0 = time.perf_counter()
        baked = bake_sh_texture(model, verts, tris, S, degree=3, normals=normals)
        torch.cuda.synchronize()
        total = (time.perf_counter() - t0) * 1e3
        kernel = {n: kt.total_ms(n) for n in sorted(names)}
        launches = {n: kt.launches(n) for n in sorted(names)}
    ours = sum(kernel.values())
    lines.append("mesh shtex bake %d^3 sphere T=%d, S=%d, L=3, 64 directions, VM model (untrained): atlas %d x %d (%.1f M texels, %.0f MB of "
                 "coefficients)  bake_sh_texture %.1f ms  kernels %.2f ms (%s)  model queries and the rest %.1f ms  [one run after a small "
                 "warm-up]"
                 % (size, T, S, Wt, Ht, Wt * Ht / 1e6, baked["texture"].numel() * 4 / 1e6, total, ours,
                    ", ".join("%s %.2f ms in %d launches" % (n[len("pvd_mesh_"):], kernel[n], launches[n]) for n in sorted(names)),
                    total - ours))
    print(lines[-1], flush=True)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--cell", type=int, default=8)
    ap.add_argument("--view", type=int, default=800)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mesh_shtex.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_mesh_shtex.py measures on a GPU; there is no CPU path"
    lines = bench(a.size, a.cell, a.view, torch.device("cuda:0"), a.reps, a.warmup)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
