"""Shared by the mixed-distortion tests (test_mixed_distortion_cpu.py, test_gpu_mixed_distortion.py): the sets, the selector's statistical bound and the
single-kind statement a forced mixed step is compared with."""
import math

FIVE = ("noise", "brightness", "blurring", "rotation", "scaling")
SETS = {"five": FIVE, "two": ("noise", "blurring"), "six": ("none",) + FIVE}
SEEDS = (0, 1, 2 ** 32 + 5)
STEPS = 4000


def count_bound(n_members, steps=STEPS):
    """(expected count, allowed deviation) of one member of an n-set over `steps` uniform draws: 5 sigma of Binomial(steps, 1 / n), rounded up -- 127 for the
    5-set (sigma 25.3), 159 for the 2-set (sigma 31.6), 118 for the 6-set (sigma 23.6)."""
    p = 1.0 / n_members
    return steps * p, math.ceil(5.0 * math.sqrt(steps * p * (1.0 - p)))


def forced_parameters(kind, n_images):
    """Host values that make the kind's interesting paths run: a brightness factor that clips some pixels, a sigma that blurs, angles of both signs."""
    if kind == "brightness":
        return {"factor": 1.37}
    if kind == "blurring":
        return {"sigma": 0.45}
    if kind == "rotation":
        return {"radians": [math.radians(-30.0 + 60.0 * (i + 0.5) / n_images) for i in range(n_images)]}
    if kind == "scaling":
        return {"scaling": 1.13}
    return {}


def single_layer(kind, shape, device, params, noise=None):
    """The existing single-kind layer holding the same parameters (None for "none")."""
    from nerf_signature_amd.distortion import DistortionLayer
    if kind == "none":
        return None
    layer = DistortionLayer(kind, 0)
    layer._buffers(shape, device)
    if kind == "noise":
        layer.noise.copy_(noise)
    elif kind == "brightness":
        layer.param.fill_(params["factor"])
    elif kind == "blurring":
        layer.param.fill_(params["sigma"])
    elif kind == "rotation":
        layer.set_rotation(params["radians"])
    else:
        layer.set_scaling(params["scaling"])
    return layer
