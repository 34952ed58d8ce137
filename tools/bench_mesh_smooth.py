#!/usr/bin/env python3
"""Time of the Taubin smoothing (pvd_mesh_smooth_build / pvd_mesh_smooth_run, csrc/mesh_smooth.hip) on one GPU.

  python tools/bench_mesh_smooth.py [--size 256 --iterations 10 --reps 20 --warmup 5 --out profiles/mesh_smooth.txt]

The mesh is the sphere of radius 0.6 extracted at size^3, the box the extraction box.  hipEvents around every call, after `warmup`
untimed rounds, the median and the minimum over `reps` rounds of
  build   pvd_mesh_smooth_build: two memsets, quantise, row sizes (32-bit atomics), the scan, offsets, fill (six launches)
  run     pvd_mesh_smooth_run with `iterations` iterations: 2 x iterations pass launches and the output launch; the time per pass is
          (run - run with 0 iterations) / (2 x iterations)
  copy    a device copy of the vertex and the triangle array: the memory floor of touching the mesh once
  torch   the same filter in float32 torch on the device: per pass two index_add_ of the neighbours' positions over a prebuilt list
          of directed edges (float atomics: not reproducible), a division and an axpy
The outputs of the last round are compared bit for bit with those of the first.  A second line gives the three figures of the noisy
sphere of tests/mesh_smooth_restatement.py (seed 0, +-0.03; lambda 0.5, mu -0.53, 10 iterations, and 10 plain passes) from this
device run.  The wavefront threshold for long rows is the one constant of the source: no second build, so no A/B.  No gate: the
figures are appended to --out."""
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


class TorchTaubin:
    """The filter as one would write it in torch: directed edges (corner -> each of the other two), index_add_ per pass."""

    def __init__(self, verts, tris):
        t = tris.to(torch.int64)
        self.dst = torch.cat([t[:, 0], t[:, 0], t[:, 1], t[:, 1], t[:, 2], t[:, 2]])
        self.src = torch.cat([t[:, 1], t[:, 2], t[:, 2], t[:, 0], t[:, 0], t[:, 1]])
        n = torch.zeros(verts.shape[0], device=verts.device).index_add_(0, self.dst, torch.ones(self.dst.shape[0], device=verts.device))
        self.has = (n > 0)[:, None]
        self.n = n.clamp(min=1.0)[:, None]

    def one_pass(self, x, w):
        mean = torch.zeros_like(x).index_add_(0, self.dst, x[self.src]) / self.n
        return torch.where(self.has, x + w * (mean - x), x)

    def run(self, x, lam, mu, iterations):
        for _ in range(iterations):
            x = self.one_pass(self.one_pass(x, lam), mu)
        return x


def bench(R, iterations, dev, reps, warmup):
    import pvd_hip
    verts, tris = sphere_mesh(R, dev)
    V, T = int(verts.shape[0]), int(tris.shape[0])
    lo, hi = torch.full((3,), -1.0, device=dev), torch.full((3,), 1.0, device=dev)
    copy_v, copy_t = torch.empty_like(verts), torch.empty_like(tris)
    totals = torch.zeros(2, dtype=torch.int64, device=dev)
    ws = torch.empty(pvd_hip.mesh_smooth_workspace_bytes(V, T), dtype=torch.uint8, device=dev)
    out, out0 = torch.empty_like(verts), torch.empty_like(verts)
    ref = TorchTaubin(verts, tris)
    names = ("build", "run", "run0", "copy", "torch")
    times, first, got = {k: [] for k in names}, None, None
    for it in range(warmup + reps):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(names) + 1)]
        ev[0].record()
        pvd_hip.mesh_smooth_build(verts, tris, lo, hi, None, ws, totals)
        ev[1].record()
        pvd_hip.mesh_smooth_run(verts, T, lo, hi, ws, 0.5, -0.53, iterations, out)
        ev[2].record()
        pvd_hip.mesh_smooth_run(verts, T, lo, hi, ws, 0.5, -0.53, 0, out0)
        ev[3].record()
        copy_v.copy_(verts)
        copy_t.copy_(tris)
        ev[4].record()
        tout = ref.run(verts, 0.5, -0.53, iterations)
        ev[5].record()
        torch.cuda.synchronize()
        if it >= warmup:
            for q, k in enumerate(names):
                times[k].append(ev[q].elapsed_time(ev[q + 1]))
        if it in (0, warmup + reps - 1):
            got = tuple(x.cpu().numpy().tobytes() for x in (out, totals))
            first = first or got
    med = {k: float(np.median(v)) for k, v in times.items()}
    per_pass = (med["run"] - med["run0"]) / (2 * iterations)
    entries, longest = (int(x) for x in totals.tolist())
    # bytes one pass has to move at the least: every 16-byte vertex row read once and written once, every row entry and offset read
    pass_bytes = 32 * V + 4 * entries + 8 * V
    diff = float((tout - out).abs().max())
    line = ("mesh smooth R=%d sphere: V=%d T=%d row entries %d largest row %d  %d iterations (lambda 0.5, mu -0.53)  build %.3f ms (min %.3f)  "
            "run %.3f ms (min %.3f)  output launch alone %.3f ms  per pass %.4f ms = %.1f GB/s of the pass's least bytes (%d)  copy of vertices "
            "and triangles %.3f ms (min %.3f)  torch index_add_ filter, same iterations %.3f ms (min %.3f) = %.4f ms per pass, max |torch - "
            "kernel| %.3g  workspace %.1f MB  bits equal from first to last round: %s  long-row threshold 64 entries (no A/B: one build)  "
            "[median of %d, %d warm-up]"
            % (R, V, T, entries, longest, iterations, med["build"], min(times["build"]), med["run"], min(times["run"]), med["run0"], per_pass,
               pass_bytes / per_pass / 1e6, pass_bytes, med["copy"], min(times["copy"]), med["torch"], min(times["torch"]),
               med["torch"] / (2 * iterations), diff, ws.numel() / 1e6, got == first, reps, warmup))
    print(line, flush=True)
    return [line]


def noisy_sphere_line(dev):
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import mesh_smooth_restatement as mr
    from pvd.mesh import smooth_mesh
    v, t, lo, hi = mr.noisy_sphere(seed=0, amplitude=0.03)
    dv, dt = torch.from_numpy(v.copy()).to(dev), torch.from_numpy(t.copy()).to(dev)
    dlo, dhi = torch.from_numpy(lo.copy()).to(dev), torch.from_numpy(hi.copy()).to(dev)
    taubin = smooth_mesh(dv, dt, iterations=10, lam=0.5, mu=-0.53, bmin=dlo, bmax=dhi).cpu().numpy()
    laplace = smooth_mesh(dv, dt, iterations=10, lam=0.5, mu=0.0, bmin=dlo, bmax=dhi).cpu().numpy()
    same = np.array_equal(taubin.view(np.int32), mr.smooth(v, t, lo, hi, 0.5, -0.53, 10).view(np.int32))
    figures = mr.noisy_sphere_figures(v, taubin, laplace)
    line = ("mesh smooth noisy sphere (614 vertices, seed 0, +-0.03), device run: radius (mean, std) before (%.4f, %.4f), 10 Taubin iterations "
            "(%.4f, %.4f), 10 plain Laplacian passes (%.4f, %.4f)  std after / before %.4f  mean radius change %.5f  plain Laplacian loses "
            "%.4f of the mean radius  bits equal to the numpy restatement: %s"
            % (mr.radii(v) + mr.radii(taubin) + mr.radii(laplace) + figures + (same,)))
    print(line, flush=True)
    return [line]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mesh_smooth.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_mesh_smooth.py measures on a GPU; there is no CPU path"
    dev = torch.device("cuda:0")
    lines = bench(a.size, a.iterations, dev, a.reps, a.warmup) + noisy_sphere_line(dev)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
