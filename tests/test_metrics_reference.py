"""SSIM on the CPU against the reference's own compute_ssim (tests/golden/reference_ssim.npz, written by
tests/golden/make_golden_ssim.py): the tests' restatement of the formula (tests/ssim_restatement.py) in float32 reproduces the
reference's mean and map to 2e-6 -- which pins the truth the GPU test holds the HIP kernel to, the same restatement in float64 --
and so does the plain-torch composition pvd/metrics.py falls back to."""
import os

import numpy as np
import pytest
import torch

from ssim_restatement import cpu_checked_cases, host_max, ssim_restated, yardstick

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_ssim.npz"))
NAMES = [str(n) for n in GOLD["names"]]
TOL = 2e-6


def _case(name):
    return torch.from_numpy(GOLD[name + "_img0"]), torch.from_numpy(GOLD[name + "_img1"]), float(GOLD[name + "_max_val"])


def test_the_fixture_holds_the_cases_the_tests_build():
    built = cpu_checked_cases()
    assert NAMES == sorted(built)
    for name in NAMES:
        a, b, mv = _case(name)
        assert torch.equal(a, built[name][0]) and torch.equal(b, built[name][1]) and mv == host_max(a, b)
        assert GOLD[name + "_map"].shape == (a.shape[0], a.shape[3], a.shape[1], a.shape[2]) and GOLD[name + "_mean"].shape == (a.shape[0],)


@pytest.mark.parametrize("name", NAMES)
def test_the_float32_restatement_reproduces_the_reference(name):
    a, b, mv = _case(name)
    mean, ssim_map = ssim_restated(a, b, mv, dtype=torch.float32)
    assert np.abs(ssim_map.numpy() - GOLD[name + "_map"]).max() <= TOL
    assert np.abs(mean.numpy() - GOLD[name + "_mean"]).max() <= TOL


@pytest.mark.parametrize("name", NAMES)
def test_the_torch_fallback_reproduces_the_reference(name):
    from pvd.metrics import compute_ssim, ssim_torch
    a, b, mv = _case(name)
    mean, ssim_map = ssim_torch(a, b, mv)
    assert np.abs(ssim_map.numpy() - GOLD[name + "_map"]).max() <= TOL
    assert np.abs(mean.numpy() - GOLD[name + "_mean"]).max() <= TOL
    # ... and through the public signature (CPU tensors take the fallback, they do not raise); max_val=None is the images' maximum
    assert torch.equal(compute_ssim(a, b, mv), mean) and torch.equal(compute_ssim(a, b, mv, return_map=True), ssim_map)
    assert np.abs(compute_ssim(a, b, None).numpy() - GOLD[name + "_mean"]).max() <= TOL


def test_the_float64_restatement_is_where_the_float32_one_converges():
    """The yardstick the GPU test uses: float32 is off from float64 by ~1e-6 on random images and by up to ~1e-3 where
    E[x^2] - mu^2 cancels (near-flat images) -- never by more, or the truth itself would be in doubt."""
    worst = {}
    for name in NAMES:
        a, b, mv = _case(name)
        _, _, e_mean, e_map = yardstick(a, b, mv)
        worst[name] = (float(e_mean.max()), e_map)
    assert worst["random"][1] <= 1e-5 and worst["near_flat"][1] <= 5e-3 and worst["smooth_noise"][1] <= 2e-3, worst
    assert max(v[0] for v in worst.values()) <= 5e-4, worst


def test_fallback_of_what_the_kernel_does_not_take_matches_float64_on_the_cpu():
    from pvd.metrics import compute_ssim
    g = torch.Generator().manual_seed(11)
    a, b = torch.rand(2, 20, 17, 5, generator=g), torch.rand(2, 20, 17, 5, generator=g)
    for kw in (dict(filter_size=11), dict(filter_size=8), dict(filter_size=17, filter_sigma=2.5)):
        truth, _ = ssim_restated(a, b, 1.0, **kw)
        assert (compute_ssim(a, b, 1.0, **kw).double() - truth).abs().max().item() <= 1e-5


def test_image_meter_on_the_cpu_averages_per_image_psnr_and_ssim():
    from pvd.metrics import ImageMeter, compute_ssim
    from pvd.trainer import psnr
    pairs = [cpu_checked_cases()[n] for n in ("random", "smooth_noise", "near_flat")]
    meter = ImageMeter()
    want_psnr, want_ssim = [], []
    for a, b in pairs:
        meter.update(a, b)
        for i in range(a.shape[0]):
            want_psnr.append(float(psnr(a[i], b[i])))
            want_ssim.append(float(compute_ssim(a[i], b[i], host_max(a, b))))
    rep = meter.report()
    assert rep["n"] == 4 and abs(rep["psnr"] - np.mean(want_psnr)) <= 1e-4 and abs(rep["ssim"] - np.mean(want_ssim)) <= 1e-6
    assert ImageMeter().report()["n"] == 0
