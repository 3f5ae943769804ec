"""Restatement of the image metrics in torch on the CPU, and the seeded test images (tests/test_metrics_cpu.py, tests/test_gpu_metrics.py).

SSIM is torchmetrics.functional.structural_similarity_index_measure(preds, target) with every default, as published, on [B, C, H, W]:
data_range = max(preds.max() - preds.min(), target.max() - target.min()) over the whole batch tensor, c1 = (0.01 data_range)^2,
c2 = (0.03 data_range)^2; an 11 x 11 Gaussian window, sigma 1.5, normalised to sum 1 (outer product of the 1-D window); both images
reflect-padded by 5; p, t, p p, t t, p t filtered per channel by a grouped valid convolution; variances clamped at 0, covariance not;
the map cropped by 5 on every side, averaged per image, then over the batch.  torchmetrics itself is not a dependency: this file is the pin.

Images here are channel last, [B, H, W, C], as the renderer produces them; maps come back as [B, H-10, W-10, C]."""
import torch
import torch.nn.functional as F

WINDOW, SIGMA, PAD = 11, 1.5, 5


def window(dtype=torch.float64):
    dist = torch.arange((1 - WINDOW) / 2, (1 + WINDOW) / 2, 1, dtype=dtype)
    g = torch.exp(-torch.pow(dist / SIGMA, 2) / 2)
    return g / g.sum()


def _moments(p, t, dtype):
    """E[p], E[t], E[pp], E[tt], E[pt] of [B, C, h, w] by the grouped valid convolution -> five [B, C, h-10, w-10]."""
    B, C = p.shape[:2]
    g = window(dtype).to(p.device)
    kernel = torch.matmul(g[:, None], g[None, :]).expand(C, 1, WINDOW, WINDOW)
    out = F.conv2d(torch.cat((p, t, p * p, t * t, p * t)), kernel, groups=C)
    return out.split(B)


def _ssim(pred, truth, dtype, data_range, pad):
    p = pred.permute(0, 3, 1, 2).to(dtype)
    t = truth.permute(0, 3, 1, 2).to(dtype)
    if data_range is None:
        data_range = torch.max(p.max() - p.min(), t.max() - t.min())
    c1 = (0.01 * data_range) ** 2
    c2 = (0.03 * data_range) ** 2
    if pad:
        p = F.pad(p, (PAD, PAD, PAD, PAD), mode="reflect")
        t = F.pad(t, (PAD, PAD, PAD, PAD), mode="reflect")
    mu_p, mu_t, e_pp, e_tt, e_pt = _moments(p, t, dtype)
    sigma_p = torch.clamp(e_pp - mu_p.pow(2), min=0.0)
    sigma_t = torch.clamp(e_tt - mu_t.pow(2), min=0.0)
    sigma_pt = e_pt - mu_p * mu_t
    full = ((2 * mu_p * mu_t + c1) * (2 * sigma_pt + c2)) / ((mu_p.pow(2) + mu_t.pow(2) + c1) * (sigma_p + sigma_t + c2))
    if pad:
        full = full[..., PAD:-PAD, PAD:-PAD]
    per_image = full.reshape(full.shape[0], -1).mean(-1)
    return per_image.mean(), per_image, full.permute(0, 2, 3, 1).contiguous()


def ssim_literal(pred, truth, dtype=torch.float64, data_range=None):
    """The literal sequence (reflect pad, grouped valid convolution, crop), every operation in `dtype` ->
    (batch mean 0-d, per-image means [B], map [B, H-10, W-10, C])."""
    return _ssim(pred, truth, dtype, data_range, pad=True)


def ssim_valid(pred, truth, dtype=torch.float64, data_range=None):
    """The same without the padding: a valid convolution over the bare image.  Every window that survives the crop lies inside the image."""
    return _ssim(pred, truth, dtype, data_range, pad=False)


def sse(pred, truth):
    """Per image sum (double)(float(p - t))^2 -> [B] float64."""
    d = (pred.to(torch.float32) - truth.to(torch.float32)).to(torch.float64)
    return (d * d).reshape(d.shape[0], -1).sum(-1)


def psnr(pred, truth):
    """-10 log10(mean squared error over the whole tensor), from `sse` (float64)."""
    return -10.0 * torch.log10(sse(pred, truth).sum() / pred.numel())


KINDS = {"wm": 1e-3, "mid": 3e-2, "noise": None}
SIZES = [(100, 100), (400, 400), (75, 133)]
NINE = [(kind, size) for kind in KINDS for size in SIZES]


def images(kind, size, seed=0, channels=3):
    """(pred, truth) float32 [1, H, W, channels] in [0, 1].  'wm' / 'mid': truth is a smooth pattern inside a disc of radius 0.4 on a white
    background (large exactly flat areas, like the synthetic scenes), pred adds N(0, sigma^2) noise inside the disc, clamped.
    'noise': two independent U[0, 1) images."""
    H, W = size
    gen = torch.Generator().manual_seed(seed * 1000003 + H * 1009 + W)
    if kind == "noise":
        pred, truth = torch.rand(H, W, 3, generator=gen, dtype=torch.float64), torch.rand(H, W, 3, generator=gen, dtype=torch.float64)
    else:
        y, x = torch.meshgrid(torch.linspace(0, 1, H, dtype=torch.float64), torch.linspace(0, 1, W, dtype=torch.float64), indexing="ij")
        pattern = torch.stack((0.5 + 0.4 * torch.sin(7 * x + 3 * y), 0.5 + 0.4 * torch.cos(5 * x * y + 1), 0.3 + 0.3 * torch.sin(40 * x) * torch.sin(33 * y)), -1)
        disc = ((x - 0.5) ** 2 + (y - 0.5) ** 2 < 0.16)[..., None]
        white = torch.ones_like(pattern)
        noise = KINDS[kind] * torch.randn(H, W, 3, generator=gen, dtype=torch.float64)
        truth = torch.where(disc, pattern, white)
        pred = torch.where(disc, pattern + noise, white).clamp(0, 1)
    return pred[None, ..., :channels].float().contiguous(), truth[None, ..., :channels].float().contiguous()


def mixed_batch(size=(100, 100)):
    """B = 3: the three kinds in one batch."""
    pairs = [images(kind, size) for kind in KINDS]
    return torch.cat([p for p, _ in pairs]), torch.cat([t for _, t in pairs])
