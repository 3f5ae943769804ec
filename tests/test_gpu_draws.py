"""The device draws that nothing else pins bit for bit: the distortion layer's single kinds (wm_distort_draw: brightness, blur sigma, rotation, noise) and
stage 1's next-step march offsets (clean_loss's noise_next).  Every word is taken from tests/draw_ref.py -- the 64-bit counter hash in integers -- and the
kernel's float32 operations are redone in numpy float32, each rounded on its own (the library is built without contraction)."""
import math

import numpy as np
import pytest
import torch

import draw_ref as dr
import orbit_ref
import tamper_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STEPS = (0, 1, 2, 255, 256, 65535, 2 ** 31 - 1, 2 ** 32 - 1)          # test_gpu_mixed_distortion.py's
SEEDS = (0, 69, 2 ** 32 + 5, 2 ** 63 + 12345)
F32 = np.float32
# the sequences of a step's key that are the distortion layer's own (csrc/distortion.hip)
UNIT_XOR, ROTATION_MUL = 0xFFFFFFFFFFFFFFFF, 0xA0761D6478BD642F


def _counter(step):
    return torch.tensor([step if step < 2 ** 31 else step - 2 ** 32], dtype=torch.int32, device=DEV)


def _unit(seed, step):
    """the step's one U[0, 1) word as the float32 the kernel forms (exact: 24 bits)"""
    return F32(dr.unit24(dr.mix64(dr.stream_key(seed, step) ^ UNIT_XOR) >> 40))


def _draw(kind, seed, step, shape):
    from nerf_signature_amd.distortion import DistortionLayer
    layer = DistortionLayer(kind, seed)
    layer.draw_on_device(_counter(step), shape, torch.device(DEV))
    return layer


def test_brightness_draw_is_one_half_plus_the_steps_word():
    for seed in SEEDS:
        for step in STEPS:
            got = _draw("brightness", seed, step, (3, 4, 4, 3)).param.cpu().numpy()
            assert got.shape == (1,) and got[0] == F32(0.5) + _unit(seed, step), (seed, step)


def test_blur_sigma_draw_is_the_steps_word_scaled_into_its_range():
    for seed in SEEDS:
        for step in STEPS:
            got = _draw("blurring", seed, step, (3, 4, 4, 3)).param.cpu().numpy()
            assert got.shape == (1,) and got[0] == F32(0.01) + F32(F32(0.49) * _unit(seed, step)), (seed, step)


def test_rotation_draw_is_one_angle_per_image():
    """Three images: the per-image index takes 0, 1, 2.  The float32 angle is reproduced exactly; (cos, sin) against float64 cos and sin of that angle, within
    HIP's documented error of cosf / sinf (orbit_ref.TRIG_ULP ulp of a result of magnitude <= 1: at most TRIG_ULP 2^-23 absolute, as orbit_ref.pose_bound
    takes it)."""
    bound = orbit_ref.TRIG_ULP * 2.0 ** -23
    for seed in SEEDS:
        for step in STEPS:
            got = _draw("rotation", seed, step, (3, 4, 4, 3)).param.cpu().numpy().astype(np.float64).reshape(3, 2)
            key = dr.stream_key(seed, step)
            for i in range(3):
                u = F32(dr.unit24(dr.mix64(key ^ ((ROTATION_MUL * (i + 1)) & dr.MASK64)) >> 40))
                a = float(F32(F32(F32(60.0) * u) - F32(30.0)) * F32(0.0174532925199432958))
                err = max(abs(got[i, 0] - math.cos(a)), abs(got[i, 1] - math.sin(a)))
                assert err <= bound, (seed, step, i, err, bound)


@pytest.mark.parametrize("n", [1, 255, 256, 257])          # the edges of the 256-thread launch
def test_noise_draw_is_the_scaled_unit_normal_of_the_steps_words(n):
    """noise[i] = 0.316227766016837933 (sqrt(0.1)) times the Box-Muller normal of word i of the step's key: against tamper_ref.unit_normal (float64, from the
    same two 24-bit fractions; the tensor index there is the step here) within tamper_ref.EPS_Z -- the project's measured bound on the device's unit normal --
    scaled by the factor, plus one float32 rounding of the product.  (The factor's own float32 rounding, below 2^-25 of it, sits inside EPS_Z's fourfold margin.)"""
    c = 0.316227766016837933
    for seed in SEEDS:
        for step in STEPS:
            layer = _draw("noise", seed, step, (1, n))
            got = layer.noise.cpu().numpy().astype(np.float64).reshape(-1)
            want = c * tamper_ref.unit_normal(seed, step, n)
            bound = c * tamper_ref.EPS_Z + 2.0 ** -24 * np.abs(want)
            err = np.abs(got - want)
            print(f"noise n={n} seed={seed} step={step}: max err {err.max():.3e}, min slack {(bound - err).min():.3e}")
            assert got.shape == (n,) and bool((err <= bound).all()), (seed, step, float(err.max()))


@pytest.mark.parametrize("n_noise", [1, 1023, 1024, 1025])   # the edges of the 1024-thread stride loop
def test_clean_loss_writes_the_next_steps_march_offsets_and_advances_the_count(n_noise):
    """noise_next[i] = float32(word24) * 2^-24 with the word the top 24 bits of draw i of the key of (seed, *step_dev + 1) -- the counter is widened before the
    increment, so step 2^32 - 1 draws from counter 2^32 --, nothing behind n_noise is touched, and *step_dev leaves as step + 1 modulo 2^32."""
    from nerf_signature_amd import _native as nv
    image, gt = torch.full((6,), 0.25, device=DEV), torch.zeros(6, device=DEV)
    loss, g_image = torch.zeros(1, device=DEV), torch.zeros(6, device=DEV)
    for seed in SEEDS:
        for step in (0, 1, 2 ** 32 - 1):
            counter = _counter(step)
            noise = torch.full((n_noise + 3,), -7.0, device=DEV)
            nv.call("clean_loss", nv.ptr(image), nv.ptr(gt), 6, 1.0, nv.ptr(loss), nv.ptr(g_image), nv.ptr(counter), nv.ptr(None), nv.ptr(None), nv.ptr(None), 0,
                    nv.ptr(noise), n_noise, seed, nv.stream())
            got = noise.cpu().numpy()
            words = dr.draw64(dr.stream_key(seed, step + 1), np.arange(n_noise, dtype=np.uint64)) >> np.uint64(40)
            assert np.array_equal(got[:n_noise], dr.unit24(words).astype(F32)) and bool((got[n_noise:] == -7.0).all()), (seed, step)
            assert (int(counter.cpu()[0]) & 0xFFFFFFFF) == (step + 1) & 0xFFFFFFFF
            assert float(loss.cpu()[0]) == 0.0625
