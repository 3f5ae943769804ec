"""Image metrics of rendered views on the device: PSNR and SSIM (the reference's PSNRMeter / SSIMMeter, nerf/utils_wtmk_disen.py:211-282).

The reference copies every view to the host for PSNR and calls torchmetrics' structural_similarity_index_measure for SSIM.  Here both are
HIP kernels (csrc/metrics.hip) over the renderer's own [B, H, W, C] tensors, and an evaluation reads the host once, at its end.

    psnr(pred, truth)                                    -> 0-d float64 device tensor, -10 log10(sum of squared errors / numel) (one value per call)
    ssim(pred, truth, data_range=None, return_map=False) -> 0-d float64 device tensor, the batch mean (and the map [B, H-10, W-10, C] fp32)
    ssim_images(...)                                     -> the per-image values [B] float64 that `ssim` averages
    ImageMetrics(device)                                 update(pred, truth) per view, measure() -> {"psnr_db", "ssim", "n"}, clear()

SSIM is torchmetrics' definition with every default, restated in DESIGN.md section 15 (torchmetrics is not a dependency): Gaussian 11 x 11
window with sigma 1.5, k1 = 0.01, k2 = 0.03, data_range from the extrema of the two batch tensors unless given.  Both images constant
(data range 0) or non-finite pixels give a non-finite result.  There is no CPU path and no gradient (a meter, not a loss).
"""
import torch

from . import _native as nv

WINDOW = 11


def _device_images(pred, truth, what, dims=None):
    for name, t in (("pred", pred), ("truth", truth)):
        if not isinstance(t, torch.Tensor):
            raise nv.NativeError(f"{what}: {name} must be a tensor on the GPU, got {type(t).__name__}")
        if not t.is_cuda:
            raise nv.NativeError(f"{what}: {name} is a CPU tensor; the metrics run on the GPU only (there is no CPU path)")
    if pred.shape != truth.shape:
        raise ValueError(f"{what}: pred {tuple(pred.shape)} and truth {tuple(truth.shape)} differ in shape")
    if pred.device != truth.device:
        raise ValueError(f"{what}: pred is on {pred.device}, truth on {truth.device}")
    if dims is not None and pred.dim() != dims:
        raise ValueError(f"{what}: expected [B, H, W, C] images, got shape {tuple(pred.shape)}")
    return pred.detach().to(torch.float32).contiguous(), truth.detach().to(torch.float32).contiguous()


def range_sse(pred, truth):
    """(extrema float32 [4] = pred min, pred max, truth min, truth max over the whole batch; SSE float64 [B] = per leading index the sum of
    (double)(float(p - t))^2) of two equally shaped device tensors [B, ...].  Device tensors back, no host read."""
    pred, truth = _device_images(pred, truth, "range_sse")
    if pred.dim() < 1 or pred.numel() == 0:
        raise ValueError(f"range_sse: empty input of shape {tuple(pred.shape)}")
    B = int(pred.shape[0])
    n = pred.numel() // B
    dev = pred.device
    with torch.cuda.device(dev):
        scratch = torch.empty(int(nv.fn("im_range_scratch_bytes")(B, n)), dtype=torch.uint8, device=dev)
        extrema = torch.empty(4, dtype=torch.float32, device=dev)
        sse = torch.empty(B, dtype=torch.float64, device=dev)
        nv.call("im_range_sse", nv.ptr(pred), nv.ptr(truth), B, n, nv.ptr(scratch), nv.ptr(extrema), nv.ptr(sse), nv.stream())
    return extrema, sse


def psnr(pred, truth):
    """-10 log10(mean squared error over the whole tensor): the reference's one value per PSNRMeter.update.  0-d float64 device tensor."""
    _, sse = range_sse(pred, truth)
    return -10.0 * torch.log10(sse.sum() / pred.numel())


def _ssim_launch(pred, truth, extrema, data_range, return_map):
    B, H, W, C = (int(s) for s in pred.shape)
    if not 1 <= C <= 4:
        raise ValueError(f"ssim: 1 to 4 channels (last dimension), got shape {tuple(pred.shape)}")
    if H < WINDOW or W < WINDOW:
        raise ValueError(f"ssim: images of at least {WINDOW} x {WINDOW} pixels, got shape {tuple(pred.shape)}")
    if B < 1:
        raise ValueError("ssim: empty batch")
    dev = pred.device
    with torch.cuda.device(dev):
        scratch = torch.empty(int(nv.fn("im_ssim_scratch_bytes")(B, H, W, C)), dtype=torch.uint8, device=dev)
        out = torch.empty(B, dtype=torch.float64, device=dev)
        smap = torch.empty(B, H - WINDOW + 1, W - WINDOW + 1, C, dtype=torch.float32, device=dev) if return_map else None
        nv.call("im_ssim", nv.ptr(pred), nv.ptr(truth), B, H, W, C, nv.ptr(extrema), 0.0 if data_range is None else float(data_range),
                nv.ptr(scratch), nv.ptr(out), nv.ptr(smap), nv.stream())
    return out, smap


def ssim_images(pred, truth, data_range=None, return_map=False):
    """Per-image mean SSIM [B] float64 of device images [B, H, W, C] (1 <= C <= 4; H, W >= 11), and with return_map the values of every
    window inside the image, [B, H-10, W-10, C] float32.  data_range None: max(pred.max() - pred.min(), truth.max() - truth.min()) over the
    batch, taken by a first launch and read by the second on the device."""
    pred, truth = _device_images(pred, truth, "ssim", dims=4)
    if data_range is not None and not float(data_range) >= 0.0:
        raise ValueError(f"ssim: data_range must be a number >= 0, got {data_range!r}")
    extrema = range_sse(pred, truth)[0] if data_range is None else None
    out, smap = _ssim_launch(pred, truth, extrema, data_range, return_map)
    return (out, smap) if return_map else out


def ssim(pred, truth, data_range=None, return_map=False):
    """torchmetrics.functional.structural_similarity_index_measure(pred.permute(0, 3, 1, 2), truth.permute(0, 3, 1, 2)) for channel-last device
    images: the mean over the batch of `ssim_images`, a 0-d float64 device tensor (with return_map: and the map)."""
    r = ssim_images(pred, truth, data_range, return_map)
    return (r[0].mean(), r[1]) if return_map else r.mean()


class ImageMetrics:
    """PSNR and SSIM of an evaluation's views with one host read: update() queues the kernels of one view (or batch of views) and adds the
    view's two values to a device accumulator; measure() reads it.  Averages per update, as the reference's meters do."""

    def __init__(self, device=None):
        self.device = device
        self.n = 0
        self._sum = None          # float64 [2] on the device: sum of per-update PSNR, sum of per-update SSIM (allocated by the first update)

    def clear(self):
        self.n = 0
        self._sum = None

    def update(self, pred, truth):
        if self.device is not None and isinstance(pred, torch.Tensor) and isinstance(truth, torch.Tensor):
            pred, truth = pred.to(self.device), truth.to(self.device)
        pred, truth = _device_images(pred, truth, "ImageMetrics.update", dims=4)
        extrema, sse = range_sse(pred, truth)
        per_image, _ = _ssim_launch(pred, truth, extrema, None, False)
        v = torch.stack((-10.0 * torch.log10(sse.sum() / pred.numel()), per_image.mean()))
        self._sum = v if self._sum is None else self._sum + v
        self.n += 1

    def measure(self):
        """{"psnr_db", "ssim", "n"}: the means over the updates (the evaluation's one host read)."""
        if self.n == 0:
            raise ZeroDivisionError("ImageMetrics.measure: no update yet")
        p, s = (self._sum / self.n).tolist()
        return {"psnr_db": p, "ssim": s, "n": self.n}
