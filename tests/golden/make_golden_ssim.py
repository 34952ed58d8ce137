#!/usr/bin/env python3
"""Generate tests/golden/reference_ssim.npz by running the REFERENCE's own compute_ssim (distill_mutual/utils.py:219-300) on the CPU.

Run where the reference tree exists (it does not on the GPU box), as tests/golden/make_golden.py is:

    PYTHONDONTWRITEBYTECODE=1 python -B tests/golden/make_golden_ssim.py [path of the reference tree]

For every image pair of tests/ssim_restatement.py:cpu_checked_cases() the file holds the inputs ([B,H,W,C] float32), the max_val the
reference's evaluate would pass (max of both images, utils.py:1278), and the reference's per-image mean and its map ([B,C,H,W]).
Only data is written; no reference source is copied."""
import importlib
import os
import sys
from unittest.mock import MagicMock

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(REPO, "tests"))

import numpy as np
import torch

from ssim_restatement import cpu_checked_cases, host_max

# stand-ins for what the reference's utils.py imports at its top and this image may lack (none of it is used by compute_ssim)
for name in ("lpips", "tqdm", "tensorboardX", "pandas", "imageio", "cv2", "matplotlib", "matplotlib.pyplot", "trimesh", "mcubes", "rich",
             "rich.console", "torch_ema", "IPython", "packaging", "torch_efficient_distloss", "raymarching", "gridencoder", "shencoder"):
    if name in ("raymarching", "gridencoder", "shencoder"):
        sys.modules[name] = MagicMock()  # the reference's native extensions: never built here
        continue
    try:
        importlib.import_module(name)
    except Exception:  # noqa: BLE001
        sys.modules[name] = MagicMock()

sys.path.insert(0, REF)
from distill_mutual.utils import compute_ssim as ref_compute_ssim  # noqa: E402

torch.manual_seed(0)
out = {"names": np.array(sorted(cpu_checked_cases()))}
for name, (a, b) in cpu_checked_cases().items():
    mv = host_max(a, b)
    with torch.no_grad():
        mean = ref_compute_ssim(a, b, max_val=mv)
        ssim_map = ref_compute_ssim(a, b, max_val=mv, return_map=True)
    out[name + "_img0"], out[name + "_img1"] = a.numpy(), b.numpy()
    out[name + "_max_val"] = np.float64(mv)
    out[name + "_mean"], out[name + "_map"] = mean.numpy(), ssim_map.numpy()
    print("%-14s %-16s max_val %.6f  mean %s" % (name, tuple(a.shape), mv, mean.numpy()))
path = os.path.join(HERE, "reference_ssim.npz")
np.savez_compressed(path, **out)
print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))
