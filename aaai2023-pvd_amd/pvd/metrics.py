"""Image metrics of a held-out evaluation: SSIM and PSNR, accumulated on the device.

reference: compute_ssim (distill_mutual/utils.py:219-300), as Trainer.evaluate calls it per view (utils.py:1275-1279, with
max_val = max(preds.max().item(), truths.max().item())), and PSNRMeter (utils.py:491-529).  On a HIP device the pair of images
goes through ONE fused pass of libpvd_hip.so (pvd_image_metrics, include/pvd_hip_metrics.h: SSIM, squared error and, for
max_val=None, the maximum of both images, without a host read-back); what that kernel does not implement (an even window, more
than 15 taps, more than 4 channels) and CPU tensors go through `ssim_torch`, the same formula composed from torch operators.
LPIPS (utils.py:1273-1274) needs pretrained weights and is not part of this module.
"""
import torch
import torch.nn.functional as F


def gaussian_taps(filter_size, filter_sigma, dtype=torch.float32):
    """The normalised 1-D window of utils.py:254-258, computed on the host (float32 unless a test asks for float64)."""
    half = filter_size // 2
    shift = (2 * half - filter_size + 1) / 2
    pos = torch.arange(filter_size).to(dtype) - half + shift
    taps = torch.exp(-0.5 * (pos / filter_sigma) ** 2)
    return taps / taps.sum()


def ssim_torch(img0, img1, max_val=None, filter_size=11, filter_sigma=1.5, k1=0.01, k2=0.03, taps=None):
    """SSIM of img0 / img1 [B,H,W,C] from torch operators, in the images' dtype: (ssim [B], map [B,C,H,W]).
    The window runs along W, then along H, as depthwise convolutions with zero padding (no renormalisation at the borders).
    max_val None: the maximum over both batches, kept as a tensor (no read-back).  With an even window the zero-padded
    convolutions return one more row and column, as the reference's arithmetic does; the mean is then taken over that map."""
    B, H, W, C = img0.shape
    x, y = img0.permute(0, 3, 1, 2), img1.permute(0, 3, 1, 2)
    if taps is None:
        taps = gaussian_taps(filter_size, filter_sigma, x.dtype)
    taps = taps.to(device=x.device, dtype=x.dtype)
    half = taps.numel() // 2
    along_w = taps.view(1, 1, 1, -1).repeat(C, 1, 1, 1)
    along_h = taps.view(1, 1, -1, 1).repeat(C, 1, 1, 1)

    def blur(z):
        z = F.conv2d(z, along_w, padding=[0, half], groups=C)
        return F.conv2d(z, along_h, padding=[half, 0], groups=C)

    if max_val is None:
        max_val = torch.maximum(x.max(), y.max())
    mu0, mu1 = blur(x), blur(y)
    mu00, mu11, mu01 = mu0 * mu0, mu1 * mu1, mu0 * mu1
    s00 = (blur(x ** 2) - mu00).clamp(min=0.0)
    s11 = (blur(y ** 2) - mu11).clamp(min=0.0)
    s01 = blur(x * y) - mu01
    s01 = torch.sign(s01) * torch.minimum(torch.sqrt(s00 * s11), s01.abs())
    c1, c2 = (k1 * max_val) ** 2, (k2 * max_val) ** 2
    ssim_map = ((2 * mu01 + c1) * (2 * s01 + c2)) / ((mu00 + mu11 + c1) * (s00 + s11 + c2))
    return ssim_map.reshape(B, -1).mean(dim=-1), ssim_map


def _kernel_takes(img, filter_size):
    if not img.is_cuda or img.numel() == 0:
        return False
    import pvd_hip
    return filter_size % 2 == 1 and filter_size <= pvd_hip.METRICS_MAX_FILTER and 1 <= img.shape[-1] <= 4


def image_metrics(img0, img1, max_val=None, filter_size=11, filter_sigma=1.5, k1=0.01, k2=0.03, return_map=False):
    """(ssim [B], mse [B], map [B,C,H,W] or None) of img0 / img1 [B,H,W,C]: the fused HIP pass where it applies, torch otherwise.
    max_val None: max(img0.max(), img1.max()), taken on the device."""
    img0, img1 = img0.detach().float().contiguous(), img1.detach().float().contiguous()
    if img0.dim() != 4 or img0.shape != img1.shape:
        raise ValueError("image_metrics: two [B,H,W,C] images of one shape expected, got %s and %s" % (tuple(img0.shape), tuple(img1.shape)))
    if torch.is_tensor(max_val):
        max_val = float(max_val)  # (a read-back the caller asked for; None keeps it on the device)
    B, H, W, C = img0.shape
    if _kernel_takes(img0, filter_size) and img1.device == img0.device:
        import pvd_hip
        dev = img0.device
        ws = torch.empty(pvd_hip.image_metrics_workspace_floats(B, H, W, C), device=dev)
        out = torch.empty(2, B, device=dev)
        ssim_map = torch.empty(B, H, W, C, device=dev) if return_map else None
        pvd_hip.image_metrics(img0, img1, gaussian_taps(filter_size, filter_sigma).tolist(), k1, k2, max_val, ws, out[0], out[1], ssim_map)
        return out[0], out[1], (ssim_map.permute(0, 3, 1, 2) if return_map else None)
    ssim, ssim_map = ssim_torch(img0, img1, max_val, filter_size, filter_sigma, k1, k2)
    mse = ((img0 - img1) ** 2).reshape(B, -1).mean(dim=-1)
    return ssim, mse, (ssim_map if return_map else None)


def compute_ssim(img0, img1, max_val, filter_size=11, filter_sigma=1.5, k1=0.01, k2=0.03, return_map=False):
    """The reference's compute_ssim (utils.py:219-300): images [..., W, H, C] -> each image's mean SSIM [B], or with return_map
    the map [B, C, W, H].  max_val=None: the maximum of both images, taken on the device."""
    W, H, C = img0.shape[-3:]
    ssim, _, ssim_map = image_metrics(img0.reshape(-1, W, H, C), img1.reshape(-1, W, H, C), max_val, filter_size, filter_sigma, k1, k2,
                                      return_map=return_map)
    return ssim_map if return_map else ssim


class ImageMeter:
    """PSNR and SSIM over the views of an evaluation.  update() adds each image's -10 log10(mse) (PSNRMeter.update,
    utils.py:511-519) and SSIM (utils.py:1275-1279) to two sums that stay on the device; report() reads them back once."""

    def __init__(self, max_val=None, **ssim_kw):
        self.max_val, self.ssim_kw = max_val, ssim_kw
        self.clear()

    def clear(self):
        self.n, self._sums = 0, None

    def update(self, pred, truth):
        """pred / truth [..., H, W, C] (one view or a batch of views)."""
        H, W, C = pred.shape[-3:]
        ssim, mse, _ = image_metrics(pred.reshape(-1, H, W, C), truth.reshape(-1, H, W, C), self.max_val, **self.ssim_kw)
        sums = torch.stack(((-10.0 * torch.log10(mse)).sum(), ssim.sum())).double()
        self._sums = sums if self._sums is None else self._sums + sums
        self.n += int(ssim.numel())

    def report(self):
        if self.n == 0:
            return {"psnr": float("nan"), "ssim": float("nan"), "n": 0}
        psnr, ssim = self._sums.tolist()  # the one read-back
        return {"psnr": psnr / self.n, "ssim": ssim / self.n, "n": self.n}


@torch.no_grad()
def evaluate_views(model, poses, intrinsics, H, W, truth, autocast=True, keep_images=False, **render_kw):
    """Render poses [V,4,4] with model.render(..., staged=True, perturb=False, **render_kw) and measure each view against
    `truth`: a tensor [V,H,W,3], or a callable (rays_o, rays_d) -> [H*W,3].  Returns ImageMeter.report() (and, with
    keep_images, the rendered and the true views under "images" / "truths")."""
    from .scene import get_rays
    meter = ImageMeter()
    images, truths = [], []
    was_training = model.training
    model.eval()
    try:
        for v, pose in enumerate(poses):
            r = get_rays(pose[None], intrinsics, H, W, -1)
            with torch.autocast("cuda", dtype=torch.float16, enabled=autocast):
                img = model.render(r["rays_o"], r["rays_d"], staged=True, perturb=False, **render_kw)["image"]
            img = img.float().reshape(H, W, 3)
            gt = truth(r["rays_o"], r["rays_d"]) if callable(truth) else truth[v]
            gt = gt.to(img.device).float().reshape(H, W, 3)
            meter.update(img, gt)
            if keep_images:
                images.append(img), truths.append(gt)
    finally:
        model.train(was_training)
    out = meter.report()
    if keep_images:
        out["images"], out["truths"] = images, truths
    return out
