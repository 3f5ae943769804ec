"""Image metrics without a GPU: the fp64 restatement (tests/ssim_ref.py) is self-consistent, the new C entry points are declared, loaded,
exported and validate their arguments before any GPU call, and the meters have the reference's interface."""
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ssim_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["im_range_scratch_bytes", "im_range_sse", "im_ssim", "im_ssim_scratch_bytes"]


@pytest.fixture(scope="module")
def native():
    from nerf_signature_amd import build, _native
    build.build()
    return _native


def test_window():
    g = ssim_ref.window(torch.float64)
    assert g.shape == (11,) and abs(float(g.sum()) - 1.0) < 1e-15
    assert torch.equal(g, g.flip(0)) and float(g[5]) == float(g.max())
    assert abs(float(g[4] / g[5]) - float(torch.exp(torch.tensor(-1.0 / (2 * 1.5 ** 2), dtype=torch.float64)))) < 1e-15


@pytest.mark.parametrize("kind,size", ssim_ref.NINE)
def test_padding_never_reaches_the_result(kind, size):
    """Pad 5, valid filter, crop 5 == valid filter over the bare image: identical maps in fp64, so the kernel needs no padding."""
    pred, truth = ssim_ref.images(kind, size)
    assert pred.shape == (1, *size, 3) and pred.dtype == torch.float32 and 0.0 <= float(pred.min()) and float(pred.max()) <= 1.0
    mean_l, per_l, map_l = ssim_ref.ssim_literal(pred, truth)
    mean_v, per_v, map_v = ssim_ref.ssim_valid(pred, truth)
    assert map_l.shape == (1, size[0] - 10, size[1] - 10, 3) and map_l.dtype == torch.float64
    assert torch.equal(map_l, map_v) and torch.equal(per_l, per_v) and float(mean_l) == float(mean_v)
    lo, hi = {"wm": (0.999, 1.0), "mid": (0.75, 0.92), "noise": (-0.05, 0.05)}[kind]
    assert lo < float(mean_l) < hi
    db = float(ssim_ref.psnr(pred, truth))
    lo, hi = {"wm": (61.0, 65.0), "mid": (32.0, 35.0), "noise": (7.0, 8.5)}[kind]
    assert lo < db < hi


def test_batch_is_the_mean_of_its_images_given_the_range():
    pred, truth = ssim_ref.mixed_batch()
    mean, per, _ = ssim_ref.ssim_literal(pred, truth, data_range=1.0)
    singles = [float(ssim_ref.ssim_literal(pred[i:i + 1], truth[i:i + 1], data_range=1.0)[0]) for i in range(3)]
    assert per.tolist() == singles and abs(float(mean) - sum(singles) / 3) < 1e-15


def test_symbols_declared_loaded_exported(native):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nerfsig.h")).read(), flags=re.S)
    declared = set(re.findall(r"^(?:int|size_t)\s*(\w+)\s*\(", text, flags=re.M))
    for name in SYMBOLS:
        assert name in declared and name in native.SIGNATURES, name
        assert native.fn(name) is not None


def test_host_queries(native):
    q, r = native.fn("im_ssim_scratch_bytes"), native.fn("im_range_scratch_bytes")
    assert q(1, 11, 11, 3) >= 8 and q(1, 11, 11, 3) % 16 == 0
    assert q(2, 400, 400, 3) >= 2 * 13 * 25 * 8          # one double per 32 x 16 tile of the 390 x 390 map and image
    assert q(0, 400, 400, 3) == 0 and q(1, 10, 400, 3) == 0 and q(1, 400, 10, 3) == 0 and q(1, 400, 400, 0) == 0 and q(1, 400, 400, 5) == 0
    assert r(1, 1) > 0 and r(3, 400 * 400 * 3) >= 3 * 24 and r(0, 100) == 0 and r(1, 0) == 0


def test_argument_validation_needs_no_gpu(native):
    d = native._vp(256)
    with pytest.raises(ValueError, match="null pointer"):
        native.call("im_ssim", None, d, 1, 100, 100, 3, None, 1.0, d, d, None, None)
    with pytest.raises(ValueError, match="null pointer"):
        native.call("im_ssim", d, d, 1, 100, 100, 3, None, 1.0, d, None, None, None)
    with pytest.raises(ValueError, match="channels"):
        native.call("im_ssim", d, d, 1, 100, 100, 0, None, 1.0, d, d, None, None)
    with pytest.raises(ValueError, match="channels"):
        native.call("im_ssim", d, d, 1, 100, 100, 5, None, 1.0, d, d, None, None)
    with pytest.raises(ValueError, match="out of range"):
        native.call("im_ssim", d, d, 1, 10, 100, 3, None, 1.0, d, d, None, None)
    with pytest.raises(ValueError, match="out of range"):
        native.call("im_ssim", d, d, 1, 100, 10, 3, None, 1.0, d, d, None, None)
    with pytest.raises(ValueError, match="batch"):
        native.call("im_ssim", d, d, 0, 100, 100, 3, None, 1.0, d, d, None, None)
    with pytest.raises(ValueError, match="data range"):
        native.call("im_ssim", d, d, 1, 100, 100, 3, None, -1.0, d, d, None, None)
    with pytest.raises(ValueError, match="data range"):
        native.call("im_ssim", d, d, 1, 100, 100, 3, None, float("nan"), d, d, None, None)
    with pytest.raises(ValueError, match="16-byte aligned"):
        native.call("im_ssim", d, d, 1, 100, 100, 3, None, 1.0, native._vp(264), d, None, None)
    with pytest.raises(ValueError, match="null pointer"):
        native.call("im_range_sse", d, None, 1, 100, d, d, d, None)
    with pytest.raises(ValueError, match="batch"):
        native.call("im_range_sse", d, d, 0, 100, d, d, d, None)
    with pytest.raises(ValueError, match="out of range"):
        native.call("im_range_sse", d, d, 1, 0, d, d, d, None)
    with pytest.raises(ValueError, match="16-byte aligned"):
        native.call("im_range_sse", d, d, 1, 100, native._vp(264), d, d, None)


def test_meter_interfaces():
    from nerf_signature_amd import _native, metrics, trainer
    ssim_meter, both = trainer.SSIMMeter(), metrics.ImageMetrics("cuda:0")      # constructing either touches no GPU (there is none here)
    for name in ("clear", "update", "measure", "report", "write"):
        assert callable(getattr(ssim_meter, name)), name
    for name in ("clear", "update", "measure"):
        assert callable(getattr(both, name)), name
    with pytest.raises(ZeroDivisionError):          # as PSNRMeter before its first update
        trainer.PSNRMeter().measure()
    with pytest.raises(ZeroDivisionError):
        ssim_meter.measure()
    with pytest.raises(ZeroDivisionError):
        both.measure()
    ssim_meter.V, ssim_meter.N = torch.tensor(1.5, dtype=torch.float64), 2
    assert ssim_meter.measure() == 0.75 and ssim_meter.report() == "SSIM = 0.750000"
    written = []
    ssim_meter.write(type("W", (), {"add_scalar": lambda self, *a: written.append(a)})(), 7, prefix="test")
    assert written == [(os.path.join("test", "SSIM"), 0.75, 7)]
    ssim_meter.clear()
    assert (ssim_meter.V, ssim_meter.N) == (0, 0)
    both.clear()
    assert both.n == 0


def test_cpu_tensors_are_refused():
    """The product has no CPU path: a CPU tensor is an error, not a slow route."""
    from nerf_signature_amd import _native, metrics, trainer
    pred, truth = ssim_ref.images("mid", (100, 100))
    for call in (lambda: metrics.ssim(pred, truth), lambda: metrics.psnr(pred, truth), lambda: metrics.ImageMetrics().update(pred, truth),
                 lambda: trainer.SSIMMeter().update(pred, truth)):
        with pytest.raises(_native.NativeError, match="CPU tensor"):
            call()


def test_dropin_keeps_the_reference_meter():
    """The drop-in trainer module does not rebind SSIMMeter: a user of the unchanged CLI keeps the reference's meter."""
    text = open(os.path.join(ROOT, "nerf_signature_amd", "dropin", "nerf", "utils_wtmk_disen.py")).read()
    assert not re.search(r"^\s*(class\s+SSIMMeter|SSIMMeter\s*=)", text, flags=re.M)
