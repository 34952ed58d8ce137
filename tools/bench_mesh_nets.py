#!/usr/bin/env python3
"""Kernel times of the surface nets mesher (csrc/mesh_nets.hip) next to the marching tetrahedra (csrc/mesh.hip) on the same field -- the
sphere of tools/bench_mesh.py -- and next to one read of that field, on one GPU.

  python tools/bench_mesh_nets.py [--sizes 256,512 --reps 20 --warmup 5 --out profiles/mesh_nets.txt]

KERNEL DURATIONS, NOT WALL TIME.  Per size the tool starts a fresh child process under `rocprofv3 --kernel-trace` (the program after
`--`; the parent never opens the GPU) which runs warmup + reps rounds of
  nets        pvd_mesh_nets_count (k_nets_count, k_nets_scan, k_nets_offsets), pvd_mesh_nets_emit (k_nets_vertices, k_nets_triangles),
              pvd_mesh_nets_normals (k_nets_normals)
  tetrahedra  pvd_mesh_count (k_mesh_count, k_mesh_scan, k_mesh_offsets), pvd_mesh_emit (k_mesh_emit), pvd_mesh_normals (k_mesh_normals)
  read        torch.max over the field: one pass over R^3 * 4 bytes and nothing written
and reads the per-dispatch start and end stamps of the trace: per kernel the median and the minimum over the LAST `reps` dispatches
(the warm-up rounds are in the trace and are left out).  Four figures per mesher: count + scan (three kernels), vertex emit, triangle
emit (one kernel does both for the tetrahedra), normals.  The lines are appended to --out."""
import argparse
import csv
import glob
import os
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "aaai2023-pvd_amd")]

GROUPS = (("nets", (("count+scan", ("k_nets_count", "k_nets_scan", "k_nets_offsets")), ("vertex emit", ("k_nets_vertices",)),
                    ("triangle emit", ("k_nets_triangles",)), ("normals", ("k_nets_normals",)))),
          ("tetrahedra", (("count+scan", ("k_mesh_count", "k_mesh_scan", "k_mesh_offsets")), ("vertex+triangle emit", ("k_mesh_emit",)),
                          ("normals", ("k_mesh_normals",)))))
READ = "max"  # the name of torch's reduction kernel holds it; the child launches no other reduction


def child(R, reps, warmup):
    import torch
    import pvd_hip
    from bench_mesh import sphere
    dev = torch.device("cuda:0")
    u = sphere(R, dev)
    lo, hi = torch.full((3,), -1.0, device=dev), torch.full((3,), 1.0, device=dev)
    apis = ((pvd_hip.mesh_nets_workspace_bytes, pvd_hip.mesh_nets_count, pvd_hip.mesh_nets_emit, pvd_hip.mesh_nets_normals),
            (pvd_hip.mesh_workspace_bytes, pvd_hip.mesh_count, pvd_hip.mesh_emit, pvd_hip.mesh_normals))
    state = []
    for ws_bytes, count, emit, normals in apis:
        ws = torch.empty(ws_bytes(R), dtype=torch.uint8, device=dev)
        totals = torch.zeros(2, dtype=torch.int32, device=dev)
        count(u, R, 0.0, ws, totals)
        V, T = totals.tolist()
        state.append((count, emit, normals, ws, totals, torch.empty(V, 3, device=dev), torch.empty(T, 3, dtype=torch.int32, device=dev),
                      torch.empty(V, 3, device=dev)))
        print("COUNTS %d %d" % (V, T), flush=True)
    for _ in range(warmup + reps):
        for count, emit, normals, ws, totals, verts, tris, nrm in state:
            count(u, R, 0.0, ws, totals)
            emit(u, R, 0.0, lo, hi, ws, verts, tris)
            normals(u, R, 0.0, lo, hi, ws, nrm)
        u.max()
        torch.cuda.synchronize()


def durations(directory):
    """{kernel name: [ns per dispatch, in dispatch order]} from the kernel trace CSV under `directory`."""
    out = {}
    for path in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
        for r in rows:
            out.setdefault(r["Kernel_Name"], []).append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    return out


def pick(trace, short, reps):
    """The last `reps` durations of the one kernel whose name holds `short`."""
    names = [n for n in trace if short in n]
    if short == READ:
        names = [n for n in trace if "reduce" in n.lower() and short in n.lower()]
    if len(names) != 1:
        raise SystemExit("expected one kernel named *%s* in the trace, found %s" % (short, names))
    return trace[names[0]][-reps:]


def bench(R, reps, warmup):
    import numpy as np
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", tmp, "-o", "nets", "--",
               sys.executable, os.path.abspath(__file__), "--child", str(R), "--reps", str(reps), "--warmup", str(warmup)]
        done = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
        if done.returncode != 0:
            raise SystemExit("the profiled child failed (%d):\n%s" % (done.returncode, done.stdout[-2000:]))
        counts = [ln.split()[1:] for ln in done.stdout.splitlines() if ln.startswith("COUNTS ")]
        trace = durations(tmp)
    read = np.asarray(pick(trace, READ, reps), np.float64) / 1e3
    lines = []
    for (name, groups), (V, T) in zip(GROUPS, counts):
        parts, total = [], 0.0
        for label, kernels in groups:
            d = sum(np.asarray(pick(trace, k, reps), np.float64) for k in kernels) / 1e3
            parts.append("%s %.1f us (min %.1f)" % (label, np.median(d), d.min()))
            total += float(np.median(d))
        lines.append("mesh R=%d sphere, %-10s: V=%s T=%s  %s  sum %.1f us = %.2f x one read of the field (%.1f us, min %.1f, %.2f TB/s)  "
                     "[kernel durations from a kernel trace, median of the last %d dispatches after %d warm-up rounds]"
                     % (R, name, V, T, "  ".join(parts), total, total / np.median(read), np.median(read), read.min(),
                        R ** 3 * 4 / np.median(read) / 1e6, reps, warmup))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,512")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mesh_nets.txt"))
    ap.add_argument("--child", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.reps, a.warmup)
    lines = []
    for R in a.sizes.split(","):
        lines += bench(int(R), a.reps, a.warmup)
    for ln in lines:
        print(ln, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
