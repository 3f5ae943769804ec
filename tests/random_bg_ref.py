"""Host mirror of the stage-1 RGBA step's background draw and blend (csrc/raygen.hip blend_random_background): the counter hash in integers -- sequence 4
of the hash the samplers draw from (tests/draw_ref.py, through tests/error_map_ref.py) -- and the blend gt = rgb * a + bg * (1 - a) in float32 with every operation rounded on its own
(tests/test_rgba_cpu.py, tests/test_gpu_rgba.py)."""
import numpy as np

from error_map_ref import draw_base, draw_word

STREAM = 4


def background(n_rays, seed, step, stream=STREAM):
    """bg [n_rays, 3] float32: word 3 n + c of the step's sequence, its top 24 bits * 2^-24 (exact in float32): U[0, 1) on torch.rand's grid."""
    words = draw_word(draw_base(seed, int(step) & 0xFFFFFFFF, stream), np.arange(3 * n_rays))
    return ((words >> np.uint64(8)).astype(np.float32) * np.float32(1.0 / (1 << 24))).reshape(n_rays, 3)


def blend(rgba, bg):
    """rgb * a + bg * (1 - a), float32, each product and sum rounded separately (numpy rounds every float32 operation: there is nothing to contract)."""
    rgba, bg = np.asarray(rgba, np.float32), np.asarray(bg, np.float32)
    rgb, a = rgba[..., :3], rgba[..., 3:]
    left = (rgb * a).astype(np.float32)
    rest = (np.float32(1.0) - a).astype(np.float32)
    right = (bg * rest).astype(np.float32)
    return (left + right).astype(np.float32)
