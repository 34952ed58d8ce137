"""pvd_image_metrics (csrc/metrics.hip, include/pvd_hip_metrics.h): SSIM + mean squared error of image pairs in one fused pass,
against the float64 restatement of the formula (tests/ssim_restatement.py, pinned to the reference's own compute_ssim by
tests/test_metrics_reference.py).

Tolerance.  float32 SSIM is not uniformly accurate (E[x^2] - mu^2 cancels on flat images), so the bar is relative to a yardstick:
E_ref = |the float32 restatement on the CPU - the float64 one|, for the map's maximum and for each image's mean, and the kernel
must be within 4 E_ref + 2e-6 of float64 -- 4 for another order inside the tap sums and of the two passes.  mse: 1e-6 relative."""
import numpy as np
import pytest
import torch

from ssim_restatement import cpu_checked_cases, host_max, pair_random, ssim_restated, yardstick

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _tile():
    import pvd_hip
    return pvd_hip.METRICS_TILE


def _run(a, b, max_val, return_map=True, **kw):
    from pvd.metrics import image_metrics
    ssim, mse, ssim_map = image_metrics(a.to(DEV), b.to(DEV), max_val, return_map=return_map, **kw)
    return ssim.cpu(), mse.cpu(), (ssim_map.cpu() if ssim_map is not None else None)


def _check_against_float64(a, b, label, **kw):
    mv = host_max(a, b)
    truth_mean, truth_map, e_mean, e_map = yardstick(a, b, mv, **kw)
    ssim, mse, ssim_map = _run(a, b, mv, **kw)
    assert ssim_map.shape == truth_map.shape
    err_map = float((ssim_map.double() - truth_map).abs().max())
    err_mean = (ssim.double() - truth_mean).abs()
    print("%s %s: map error %.3e (E_ref %.3e, ratio %.2f), mean error %.3e (E_ref %.3e)"
          % (label, tuple(a.shape), err_map, e_map, err_map / max(e_map, 1e-30), float(err_mean.max()), float(e_mean.max())))
    assert err_map <= 4 * e_map + 2e-6
    assert bool((err_mean <= 4 * e_mean + 2e-6).all())
    mse64 = ((a.double() - b.double()) ** 2).reshape(a.shape[0], -1).mean(-1)
    assert bool(((mse.double() - mse64).abs() <= 1e-6 * mse64).all())
    # the mean the kernel returns is the mean of the map it returns
    assert float((ssim_map.double().reshape(a.shape[0], -1).mean(-1) - ssim.double()).abs().max()) <= 1e-6


@pytest.mark.parametrize("name", sorted(cpu_checked_cases()))
def test_kernel_matches_float64_on_the_recorded_cases(name):
    """random [2,37,29,3] (non-square, odd, batch index); [1,5,7,3] and [1,1,1,1] (halo larger than the image, all-padding taps);
    [3,40,24,1] and [1,24,40,4] (channel loop and stride); smooth + noise; near-flat white."""
    a, b = cpu_checked_cases()[name]
    _check_against_float64(a, b, name)


def _edge_sizes():
    T = _tile()
    return [(T - 1, T - 1), (T, T), (T + 1, T + 1), (2 * T + 1, 2 * T + 1), (T - 1, 2 * T + 1), (2 * T + 1, T), (T + 1, T - 1), (T, T + 1)]


@pytest.mark.parametrize("k", range(8))
def test_kernel_matches_float64_at_tile_seams(k):
    """H and W = tile - 1, tile, tile + 1 and 2 tile + 1 for the tile the kernel uses: off-by-one at seams, partial last tiles."""
    H, W = _edge_sizes()[k]
    a, b = pair_random((1, H, W, 3), 100 + k)
    _check_against_float64(a, b, "seam")


@pytest.mark.parametrize("fs,sigma", [(1, 1.5), (3, 0.8), (7, 1.0), (15, 2.5)])
def test_other_odd_windows(fs, sigma):
    a, b = pair_random((2, 35, 41, 3), 200 + fs)
    _check_against_float64(a, b, "window %d" % fs, filter_size=fs, filter_sigma=sigma)


def test_identical_images():
    a, _ = pair_random((2, 37, 29, 3), 7)
    ssim, mse, _ = _run(a, a.clone(), None)
    assert bool((mse == 0).all()) and float((ssim - 1).abs().max()) <= 1e-6


def test_two_calls_give_the_same_bits_and_the_device_maximum_is_the_host_one():
    a, b = pair_random((2, 2 * _tile() + 1, 45, 3), 8)
    b = b * 0.7  # the maximum is in img0 ...
    first = _run(a, b, None)
    again = _run(a, b, None)
    given = _run(a, b, host_max(a, b))
    for x, y, z in zip(first, again, given):
        assert torch.equal(x, y) and torch.equal(x, z)
    swapped = _run(b, a, None), _run(b, a, host_max(a, b))  # ... and in img1
    for x, z in zip(*swapped):
        assert torch.equal(x, z)
    # a pointer that is not 16-byte aligned and an element count that is no multiple of 4 (the scalar path of the reduction)
    from pvd.metrics import image_metrics
    flat = torch.zeros(2 * 11 * 13 * 3 + 1, device=DEV)
    av, bv = flat[1:].view(2, 11, 13, 3), (torch.rand(2, 11, 13, 3, device=DEV) * 0.5)
    av.copy_(torch.rand(2, 11, 13, 3, device=DEV))
    assert av.data_ptr() % 16 != 0
    for x, z in zip(image_metrics(av, bv, None), image_metrics(av, bv, float(torch.maximum(av.max(), bv.max())))):
        assert x is None or torch.equal(x, z)


def test_compute_ssim_has_the_reference_signature_and_shapes():
    from pvd.metrics import compute_ssim
    a, b = pair_random((2, 3, 21, 18, 3), 9)  # [..., W, H, C] with two leading dimensions
    out = compute_ssim(a.to(DEV), b.to(DEV), 1.0)
    ssim_map = compute_ssim(a.to(DEV), b.to(DEV), 1.0, return_map=True)
    assert out.shape == (6,) and ssim_map.shape == (6, 3, 21, 18) and out.is_cuda
    truth, truth_map = ssim_restated(a.reshape(6, 21, 18, 3), b.reshape(6, 21, 18, 3), 1.0)
    assert float((out.cpu().double() - truth).abs().max()) <= 1e-5 and float((ssim_map.cpu().double() - truth_map).abs().max()) <= 1e-4


def test_what_the_kernel_does_not_take_is_unsupported_in_the_binding_and_falls_back_in_compute_ssim():
    import pvd_hip
    from pvd.metrics import compute_ssim, gaussian_taps
    for shape, fs in (((1, 20, 17, 3), 8), ((1, 20, 17, 5), 11), ((1, 20, 17, 3), 17)):
        a, b = pair_random(shape, 10 + fs)
        ad, bd = a.to(DEV), b.to(DEV)
        ws = torch.zeros(pvd_hip.image_metrics_workspace_floats(1, 20, 17, 3) + 64, device=DEV)
        out = torch.zeros(2, 1, device=DEV)
        rc = pvd_hip.image_metrics(ad, bd, gaussian_taps(fs, 1.5).tolist(), 0.01, 0.03, 1.0, ws, out[0], out[1], status=True)
        assert rc == -2  # PVD_ERR_UNSUPPORTED
        with pytest.raises(pvd_hip.PvdHipError):
            pvd_hip.image_metrics(ad, bd, gaussian_taps(fs, 1.5).tolist(), 0.01, 0.03, 1.0, ws, out[0], out[1])
        truth, _ = ssim_restated(a, b, 1.0, filter_size=fs)
        got = compute_ssim(ad, bd, 1.0, filter_size=fs)
        assert got.is_cuda and float((got.cpu().double() - truth).abs().max()) <= 1e-5


def test_an_empty_batch_is_ok():
    import pvd_hip
    from pvd.metrics import gaussian_taps
    e = torch.empty(0, 8, 8, 3, device=DEV)
    ws, out = torch.zeros(512, device=DEV), torch.zeros(2, 0, device=DEV)
    assert pvd_hip.image_metrics(e, e.clone(), gaussian_taps(11, 1.5).tolist(), 0.01, 0.03, 1.0, ws, out[0], out[1], status=True) == 0


def test_image_meter_is_the_mean_of_the_single_pair_results():
    from pvd.metrics import ImageMeter, image_metrics
    pairs = [pair_random((1, 33, 47, 3), 20 + i) for i in range(3)]
    meter = ImageMeter()
    psnrs, ssims = [], []
    for a, b in pairs:
        ad, bd = a.to(DEV), (0.5 * a + 0.5 * b).to(DEV)
        meter.update(ad[0], bd[0])
        ssim, mse, _ = image_metrics(ad, bd, None)
        psnrs.append(float(-10.0 * torch.log10(mse[0])))
        ssims.append(float(ssim[0]))
    assert meter._sums.is_cuda  # the sums stay on the device until report()
    rep = meter.report()
    assert rep["n"] == 3 and abs(rep["psnr"] - np.mean(psnrs)) <= 1e-5 and abs(rep["ssim"] - np.mean(ssims)) <= 1e-6


def test_evaluate_views_measures_the_views_the_model_renders():
    """Two 40 x 40 views of one of the small models the inference tests build: PSNR is pvd.trainer.psnr of the same images, SSIM
    the kernel's on the same images."""
    from test_hip_infer_rounds import _model
    from pvd.metrics import evaluate_views, image_metrics
    from pvd.scene import synthetic_poses
    from pvd.trainer import psnr
    m = _model("hash")
    poses = torch.from_numpy(synthetic_poses(np.random.RandomState(2))[[9, 40]]).to(DEV)
    intr = (55.555, 55.555, 20.0, 20.0)
    g = torch.Generator().manual_seed(5)
    truth = torch.rand(2, 40, 40, 3, generator=g).to(DEV)
    rep = evaluate_views(m, poses, intr, 40, 40, truth, keep_images=True, bg_color=1, max_steps=1024)
    assert rep["n"] == 2 and len(rep["images"]) == 2 and rep["images"][0].shape == (40, 40, 3)
    assert not m.training and float(torch.stack(rep["images"]).std()) > 0.01  # something was rendered
    want_psnr = np.mean([float(psnr(i, t)) for i, t in zip(rep["images"], truth)])
    want_ssim = np.mean([float(image_metrics(i[None], t[None], None)[0]) for i, t in zip(rep["images"], truth)])
    assert abs(rep["psnr"] - want_psnr) <= 1e-4 and abs(rep["ssim"] - want_ssim) <= 1e-6
    # a callable truth sees the rays of each view
    seen = []

    def white(rays_o, rays_d):
        seen.append(tuple(rays_o.shape))
        return torch.ones(40 * 40, 3, device=DEV)
    rep2 = evaluate_views(m, poses, intr, 40, 40, white, bg_color=1, max_steps=1024)
    assert rep2["n"] == 2 and seen == [(1, 1600, 3)] * 2 and np.isfinite(rep2["psnr"]) and 0 < rep2["ssim"] <= 1
