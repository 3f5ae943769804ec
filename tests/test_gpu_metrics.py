"""Image metrics on the GPU (csrc/metrics.hip) against the fp64 restatement of tests/ssim_ref.py.

The bars are measured here, on the CPU, from the reference's own arithmetic: E32 / M32 = the largest |literal fp32 - fp64| of the mean / of a
map element over the nine test images (one number for the set).  Every GPU mean must be within 2 E32 of fp64 (2: the GPU sums in another
order than the CPU's convolution), every GPU map element within M32."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ssim_ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

CASES = {f"{kind}-{h}x{w}": (kind, (h, w)) for kind, (h, w) in ssim_ref.NINE}
CASES.update({"wm-11x11": ("wm", (11, 11)), "wm-11x40": ("wm", (11, 40)), "wm-756x1008": ("wm", (756, 1008)), "mixed-batch": ("batch", (100, 100)),
              "one-channel": ("c1", (100, 100))})


@functools.lru_cache(maxsize=None)
def _inputs(case):
    kind, size = CASES[case]
    if kind == "batch":
        return ssim_ref.mixed_batch(size)
    if kind == "c1":
        return ssim_ref.images("wm", size, channels=1)
    return ssim_ref.images(kind, size)


@functools.lru_cache(maxsize=None)
def _fp64(case, data_range=None):
    return ssim_ref.ssim_literal(*_inputs(case), dtype=torch.float64, data_range=data_range)


@functools.lru_cache(maxsize=None)
def _bars():
    """(E32, M32) over the nine images."""
    e32 = m32 = 0.0
    for kind, (h, w) in ssim_ref.NINE:
        case = f"{kind}-{h}x{w}"
        mean64, _, map64 = _fp64(case)
        mean32, _, map32 = ssim_ref.ssim_literal(*_inputs(case), dtype=torch.float32)
        e32 = max(e32, abs(float(mean32.double() - mean64)))
        m32 = max(m32, float((map32.double() - map64).abs().max()))
    print(f"\n[bars] E32 = {e32:.3e} (bar 2 E32 = {2 * e32:.3e}), M32 = {m32:.3e}")
    return e32, m32


def _gpu(case, **kw):
    from nerf_signature_amd import metrics
    pred, truth = (x.to(DEV) for x in _inputs(case))
    per_image, smap = metrics.ssim_images(pred, truth, return_map=True, **kw)
    mean = metrics.ssim(pred, truth, **kw)
    return mean.cpu(), per_image.cpu(), smap.cpu()


def _check_against_fp64(case, data_range=None):
    e32, m32 = _bars()
    kw = {} if data_range is None else {"data_range": data_range}
    mean, per_image, smap = _gpu(case, **kw)
    mean64, per64, map64 = _fp64(case, data_range)
    assert mean.dtype == torch.float64 and mean.dim() == 0 and per_image.dtype == torch.float64 and smap.dtype == torch.float32
    assert smap.shape == map64.shape and per_image.shape == per64.shape
    err_mean = max(abs(float(mean - mean64)), float((per_image - per64).abs().max()))
    err_map = float((smap.double() - map64).abs().max())
    print(f"\n[{case}{'' if data_range is None else f' data_range={data_range}'}] fp64 {float(mean64):.6f}  |mean - fp64| = {err_mean:.3e} (bar {2 * e32:.3e})  "
          f"max |map - fp64| = {err_map:.3e} (bar {m32:.3e})")
    assert torch.isfinite(smap).all()
    assert err_mean <= 2 * e32
    assert err_map <= m32
    # the returned per-image value is the mean of the same numbers the map holds, one reduction
    assert float((smap.double().reshape(smap.shape[0], -1).mean(-1) - per_image).abs().max()) <= 1e-12
    return mean, per_image, smap


@pytest.mark.parametrize("case", list(CASES))
def test_ssim_against_fp64(case):
    """Mean and map of every test image against fp64 (items 4, 5 and 9 of the issue's list: the single-window image and the single-row map too)."""
    _, per_image, smap = _check_against_fp64(case)
    kind, (h, w) = CASES[case]
    assert smap.shape[1:3] == (h - 10, w - 10)


@pytest.mark.parametrize("case", ["wm-100x100", "mid-75x133", "noise-100x100", "mixed-batch"])
def test_explicit_data_range(case):
    _check_against_fp64(case, data_range=1.0)


def test_batch_with_explicit_range_is_the_mean_of_its_images():
    """With the range given, an image's value does not depend on its batch: the same bits alone as inside the batch."""
    from nerf_signature_amd import metrics
    pred, truth = (x.to(DEV) for x in _inputs("mixed-batch"))
    per_image, smap = metrics.ssim_images(pred, truth, data_range=1.0, return_map=True)
    singles = [metrics.ssim_images(pred[i:i + 1], truth[i:i + 1], data_range=1.0, return_map=True) for i in range(pred.shape[0])]
    assert torch.equal(per_image, torch.cat([s[0] for s in singles]))
    assert torch.equal(smap, torch.cat([s[1] for s in singles]))
    assert torch.equal(metrics.ssim(pred, truth, data_range=1.0), torch.cat([s[0] for s in singles]).mean())


@pytest.mark.parametrize("case", ["mid-400x400", "wm-756x1008", "mixed-batch", "wm-11x11"])
def test_range_and_squared_error(case):
    from nerf_signature_amd import metrics
    pred, truth = _inputs(case)
    extrema, sse = metrics.range_sse(pred.to(DEV), truth.to(DEV))
    want = torch.stack((pred.min(), pred.max(), truth.min(), truth.max()))
    assert extrema.dtype == torch.float32 and torch.equal(extrema.cpu().view(torch.int32), want.view(torch.int32))
    ref = ssim_ref.sse(pred, truth)
    rel = float(((sse.cpu() - ref).abs() / ref).max())
    db, ref_db = float(metrics.psnr(pred.to(DEV), truth.to(DEV))), float(ssim_ref.psnr(pred, truth))
    print(f"\n[{case}] SSE relative error {rel:.3e}, PSNR {db:.6f} dB (restatement {ref_db:.6f})")
    assert sse.dtype == torch.float64 and rel <= 1e-9
    assert abs(db - ref_db) <= 1e-8


def test_unaligned_image_size_takes_the_scalar_loads():
    """75 x 133 x 3 values per image is not a multiple of 4 (no 16-byte loads), and a batch of those puts the second image off alignment."""
    from nerf_signature_amd import metrics
    pred = torch.cat([ssim_ref.images(kind, (75, 133))[0] for kind in ("wm", "mid")])
    truth = torch.cat([ssim_ref.images(kind, (75, 133))[1] for kind in ("wm", "mid")])
    assert (pred[0].numel() % 4) != 0
    extrema, sse = metrics.range_sse(pred.to(DEV), truth.to(DEV))
    assert torch.equal(extrema.cpu(), torch.stack((pred.min(), pred.max(), truth.min(), truth.max())))
    ref = ssim_ref.sse(pred, truth)
    assert float(((sse.cpu() - ref).abs() / ref).max()) <= 1e-9


@pytest.mark.parametrize("case", ["mid-400x400", "noise-75x133", "mixed-batch"])
def test_same_bits_every_run_and_with_the_images_swapped(case):
    """No atomics, fixed reduction order: two runs agree in every bit.  pred and truth enter every expression of the kernel symmetrically
    (products and sums commute, d = p - t only changes sign), so swapping them changes no bit either."""
    from nerf_signature_amd import metrics
    pred, truth = (x.to(DEV) for x in _inputs(case))
    a, a_map = metrics.ssim_images(pred, truth, return_map=True)
    b, b_map = metrics.ssim_images(pred, truth, return_map=True)
    c, c_map = metrics.ssim_images(truth, pred, return_map=True)
    assert torch.equal(a, b) and torch.equal(a_map.view(torch.int32), b_map.view(torch.int32))
    assert torch.equal(a, c) and torch.equal(a_map.view(torch.int32), c_map.view(torch.int32))
    assert torch.equal(metrics.psnr(pred, truth), metrics.psnr(pred, truth)) and torch.equal(metrics.psnr(pred, truth), metrics.psnr(truth, pred))


def test_other_input_layouts_are_converted():
    """Inputs that are not contiguous fp32 are converted by the wrapper: same result as their contiguous fp32 copies."""
    from nerf_signature_amd import metrics
    pred, truth = (x.to(DEV) for x in _inputs("mid-100x100"))
    want = metrics.ssim(pred, truth)
    nchw_p, nchw_t = pred.permute(0, 3, 1, 2).contiguous(), truth.permute(0, 3, 1, 2).contiguous()
    assert torch.equal(metrics.ssim(nchw_p.permute(0, 2, 3, 1), nchw_t.permute(0, 2, 3, 1)), want)
    assert torch.equal(metrics.ssim(pred.double(), truth.double()), want)
    with pytest.raises(ValueError):
        metrics.ssim(pred[0], truth[0])
    with pytest.raises(ValueError):
        metrics.ssim(pred[:, :10], truth[:, :10])


def test_image_metrics_accumulates_on_the_device():
    """Ten views through ImageMetrics == the ten single results averaged in double; update() returns nothing and reads nothing back."""
    from nerf_signature_amd import metrics, trainer
    kinds = ["wm", "mid", "noise", "wm", "mid", "wm", "mid", "noise", "wm", "mid"]
    views = [tuple(x.to(DEV) for x in ssim_ref.images(kind, (100, 100) if i % 2 else (75, 133), seed=i)) for i, kind in enumerate(kinds)]
    singles = [(float(metrics.psnr(p, t)), float(metrics.ssim(p, t))) for p, t in views]
    meter, ssim_meter = metrics.ImageMetrics(DEV), trainer.SSIMMeter(DEV)
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:                      # does this torch build honour the mode?  A host read must raise under it.
            torch.ones(1, device=DEV).item()
            honoured = False
        except RuntimeError:
            honoured = True
        returned = [meter.update(p, t) for p, t in views]
        for p, t in views:
            ssim_meter.update(p, t)
    finally:
        torch.cuda.set_sync_debug_mode(before)
    print(f"\n[ImageMetrics] sync debug mode honoured by this torch build: {honoured}")
    assert returned == [None] * 10
    assert meter._sum.is_cuda and meter._sum.dtype == torch.float64 and ssim_meter.V.is_cuda      # (the whole check where the mode is not honoured)
    m = meter.measure()
    assert set(m) == {"psnr_db", "ssim", "n"} and m["n"] == 10
    assert abs(m["psnr_db"] - sum(s[0] for s in singles) / 10) <= 1e-10 and abs(m["ssim"] - sum(s[1] for s in singles) / 10) <= 1e-14
    assert abs(ssim_meter.measure() - m["ssim"]) <= 1e-14 and ssim_meter.report() == f"SSIM = {m['ssim']:.6f}"
    meter.clear()
    with pytest.raises(ZeroDivisionError):
        meter.measure()


def test_quality_test_image_metrics_end_to_end():
    """quality.test_image_metrics on the watermark stage's own renders: PSNR as quality.test_image reports it (numpy's pairwise fp32 mean of
    4.8e5 squares is within about 1e-6 relative of the double sum: 5e-6 dB; the bar is 1e-4 dB), SSIM as the restatement gives it for the
    rendered tensors, under the bar of the mean."""
    from nerf_signature_amd import quality
    e32, _ = _bars()
    stage = quality.watermark_stage("hotdog", n_poses=1, n_test_poses=2)
    views = [(p.clone(), t.clone()) for p, t in quality.test_views(stage)]
    assert len(views) == 2 and views[0][0].shape == (1, stage["H"], stage["W"], 3)
    m = quality.test_image_metrics(stage, views=views)
    assert set(m) == {"psnr_db", "ssim"}
    ref = sum(float(ssim_ref.ssim_literal(p.cpu(), t.cpu())[0]) for p, t in views) / 2
    ref_db = sum(float(ssim_ref.psnr(p.cpu(), t.cpu())) for p, t in views) / 2
    rendered = quality.test_image_metrics(stage)
    host_db = quality.test_image(stage)
    print(f"\n[hotdog, 2 views] PSNR {m['psnr_db']:.6f} dB (restatement {ref_db:.6f}, test_image {host_db:.6f}), SSIM {m['ssim']:.8f} (fp64 {ref:.8f}, "
          f"|diff| = {abs(m['ssim'] - ref):.3e}, bar {2 * e32:.3e}); rendered again: {rendered['psnr_db']:.6f} dB, {rendered['ssim']:.8f}")
    assert abs(m["ssim"] - ref) <= 2 * e32
    assert abs(m["psnr_db"] - ref_db) <= 1e-8
    assert abs(rendered["psnr_db"] - host_db) <= 1e-4
    assert abs(rendered["ssim"] - ref) <= 2 * e32
