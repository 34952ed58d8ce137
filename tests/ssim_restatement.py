"""The SSIM formula restated for the tests, in the dtype it is asked for (float64: the truth the HIP kernel is held to; float32 on
the CPU: the yardstick E_ref of how far a float32 evaluation may be from that truth), and the image pairs the tests use.

The formula (distill_mutual/utils.py:219-300): a normalised Gaussian window of `filter_size` taps; the five moments E[x], E[y],
E[x^2], E[y^2], E[xy] blurred along W, then along H, as depthwise convolutions with ZERO padding; variances clamped at 0, the
covariance clamped to the geometric mean of the variances; c1 = (k1 max_val)^2, c2 = (k2 max_val)^2;
map = (2 mu01 + c1)(2 s01 + c2) / ((mu00 + mu11 + c1)(s00 + s11 + c2)); the mean of the map per image.
Images are [B,H,W,C]; the map comes back as [B,C,H,W].  With an even window the padded convolutions give one more row and column
and the mean is taken over that map."""
import torch
import torch.nn.functional as F


def window(filter_size, filter_sigma, dtype):
    """The taps are float32 numbers in every dtype (the reference computes them so, and so does the wrapper of the kernel): the
    float64 evaluation is the exact-arithmetic answer for THOSE taps, and E_ref is the rounding of the float32 arithmetic alone."""
    half = filter_size // 2
    centre = half - (2 * half - filter_size + 1) / 2
    g = torch.exp(-0.5 * ((torch.arange(filter_size).to(torch.float32) - centre) / filter_sigma) ** 2)
    return (g / torch.sum(g)).to(dtype)


def ssim_restated(img0, img1, max_val, filter_size=11, filter_sigma=1.5, k1=0.01, k2=0.03, dtype=torch.float64):
    """(mean [B], map [B,C,H,W]) on the CPU in `dtype`; max_val a Python float."""
    p = img0.detach().cpu().to(dtype).permute(0, 3, 1, 2)
    q = img1.detach().cpu().to(dtype).permute(0, 3, 1, 2)
    C = p.shape[1]
    g = window(filter_size, filter_sigma, dtype)
    half = filter_size // 2
    row = g.view(1, 1, 1, -1).repeat(C, 1, 1, 1)
    col = g.view(1, 1, -1, 1).repeat(C, 1, 1, 1)

    def expect(z):
        return F.conv2d(F.conv2d(z, row, padding=[0, half], groups=C), col, padding=[half, 0], groups=C)

    ep, eq = expect(p), expect(q)
    pp, qq, pq = ep * ep, eq * eq, ep * eq
    var_p = torch.clamp(expect(p ** 2) - pp, min=0.0)
    var_q = torch.clamp(expect(q ** 2) - qq, min=0.0)
    cov = expect(p * q) - pq
    cov = torch.sign(cov) * torch.min(torch.sqrt(var_p * var_q), torch.abs(cov))
    c1 = (k1 * max_val) ** 2
    c2 = (k2 * max_val) ** 2
    m = (2 * pq + c1) * (2 * cov + c2) / ((pp + qq + c1) * (var_p + var_q + c2))
    return m.reshape(m.shape[0], -1).mean(dim=-1), m


def yardstick(img0, img1, max_val, **kw):
    """(truth mean, truth map, E_ref of the mean [B], E_ref of the map): float64, and |float32 on the CPU - float64|."""
    mean64, map64 = ssim_restated(img0, img1, max_val, dtype=torch.float64, **kw)
    mean32, map32 = ssim_restated(img0, img1, max_val, dtype=torch.float32, **kw)
    return mean64, map64, (mean32.double() - mean64).abs(), float((map32.double() - map64).abs().max())


# ---------------------------------------------------------------- the image pairs, float32 [B,H,W,C] on the CPU, seeded
def pair_random(shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(*shape, generator=g), torch.rand(*shape, generator=g)


def pair_smooth_noise(shape=(1, 45, 70, 3), seed=1):
    """Bilinear-upsampled 6 x 9 noise, and the same + 0.02 randn clamped to [0, 1]: the regime real renders are in."""
    g = torch.Generator().manual_seed(seed)
    B, H, W, C = shape
    a = F.interpolate(torch.rand(B, C, 6, 9, generator=g), size=(H, W), mode="bilinear", align_corners=False).permute(0, 2, 3, 1).contiguous()
    b = (a + 0.02 * torch.randn(*shape, generator=g)).clamp(0.0, 1.0)
    return a, b


def pair_near_flat(shape=(1, 40, 40, 3), seed=2):
    """ones against ones - 1e-3 rand: E[x^2] - mu^2 cancels almost completely (white-background renders)."""
    g = torch.Generator().manual_seed(seed)
    a = torch.ones(*shape)
    return a, a - 1e-3 * torch.rand(*shape, generator=g)


def cpu_checked_cases():
    """name -> (img0, img1): the cases tests/golden/reference_ssim.npz records the reference's own result for."""
    return {
        "random": pair_random((2, 37, 29, 3), 0),
        "small": pair_random((1, 5, 7, 3), 3),
        "one_pixel": pair_random((1, 1, 1, 1), 4),
        "one_channel": pair_random((3, 40, 24, 1), 5),
        "four_channels": pair_random((1, 24, 40, 4), 6),
        "smooth_noise": pair_smooth_noise(),
        "near_flat": pair_near_flat(),
    }


def host_max(img0, img1):
    return max(float(img0.max()), float(img1.max()))
