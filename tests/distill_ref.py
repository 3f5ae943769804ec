"""rm_finish_u8 restated in numpy float32 from the text of include/nerfsig.h ("the render tail that writes STORE BYTES"): every operation on its own, in the order
written there.  tests/test_distill_cpu.py holds it to exact arithmetic; tests/test_gpu_distill.py compares the kernel with it by equality.  Also: the seeded inputs
both files use, and four mutants of the arithmetic (truncate | premultiplied | clamp_after_scale | alpha_unclamped)."""
from fractions import Fraction

import numpy as np

F = np.float32
MUTANTS = ("truncate", "premultiplied", "clamp_after_scale", "alpha_unclamped")
BGS = ((1.0, 1.0, 1.0), (0.2, 0.6, 1.0))


def _clamp(x):
    return np.fmin(np.fmax(x, F(0)), F(1))


def float_picture(image, weights_sum, channels, bg=(1.0, 1.0, 1.0), mutant=None):
    """The float32 values behind the bytes, [N, channels], BEFORE the clamp of the colours: C = 4 (rgb_0, rgb_1, rgb_2, a), C = 3 (s_0, s_1, s_2)."""
    image = np.asarray(image, F).reshape(-1, 3)
    ws = np.asarray(weights_sum, F).reshape(-1)
    a = ws if mutant == "alpha_unclamped" else _clamp(ws)
    with np.errstate(all="ignore"):
        if channels == 4:
            safe = np.where(a > 0, a, F(1))
            rgb = image if mutant == "premultiplied" else np.where((a > 0)[:, None], image / safe[:, None], F(0)).astype(F)
            return np.concatenate([rgb, a[:, None]], axis=1).astype(F)
        if channels != 3:
            raise ValueError(f"channels={channels} is not 3 or 4")
        behind = ((F(1) - a)[:, None] * np.asarray(bg, F)[None, :]).astype(F)
        return (image + behind).astype(F)


def finish_u8(image, weights_sum, channels, bg=(1.0, 1.0, 1.0), mutant=None):
    """uint8 [N, channels]: rint(255 clamp(x)) of float_picture's values (alpha is in [0, 1] already: its clamp changes nothing)."""
    x = float_picture(image, weights_sum, channels, bg, mutant)
    with np.errstate(all="ignore"):
        if mutant == "clamp_after_scale":
            y = _clamp(F(255) * x)
        else:
            y = F(255) * _clamp(x) if mutant != "alpha_unclamped" else F(255) * np.concatenate([_clamp(x[:, :3]), x[:, 3:]], axis=1)
        codes = np.trunc(y) if mutant == "truncate" else np.rint(y)
    return (codes.astype(np.int64) & 0xFF).astype(np.uint8)


def exact_value(image_c, ws, channels, bg_c=None, alpha=False):
    """255 clamp(.) of one channel in exact rational arithmetic on the float32 inputs (bg_c as the float32 the entry point receives)."""
    a = min(max(Fraction(float(F(ws))), Fraction(0)), Fraction(1))
    if alpha:
        return 255 * a
    v = Fraction(float(F(image_c)))
    x = (v / a if a > 0 else Fraction(0)) if channels == 4 else v + (1 - a) * Fraction(float(F(bg_c)))
    return 255 * min(max(x, Fraction(0)), Fraction(1))


def round_half_even(q):
    return int(round(q))      # (Fraction.__round__ rounds half to even)


def _half_code(k, a):
    """image_c ON the half code between k and k + 1 at alpha a, as float32 can say it: ((k + 0.5) / 255) a."""
    return F(F(F(k + 0.5) / F(255)) * F(a))


def edge_rays():
    """(weights_sum, image) rows that sit on the edges of the arithmetic: alpha exactly 0, a denormal, 1, 1 + 2^-23, a small negative and one well above 1; colours on
    half codes scaled by alpha; colours above alpha; exact 0 and 1; a negative colour."""
    one_up, den = F(1) + F(2.0 ** -23), F(1e-40)
    rows = [(0.0, (0.0, 0.0, 0.0)), (0.0, (0.3, 0.0, 1.0)), (-0.0, (0.0, 0.5, 0.0)),
            (den, (0.0, F(1e-41), den)), (den, (F(3e-41), F(5e-41), F(2e-40))),
            (1.0, (0.0, 1.0, 0.5)), (1.0, (1.0, 0.0, 1.0)), (1.0, tuple(_half_code(k, 1.0) for k in (0, 1, 127))), (1.0, tuple(_half_code(k, 1.0) for k in (128, 253, 254))),
            (one_up, (1.0, one_up, 0.25)), (one_up, (0.0, 0.5, one_up)),
            (-1e-3, (0.1, 0.2, 0.3)), (-1e-3, (0.0, 0.0, 0.0)), (1.5, (0.2, 0.9, 1.2)),
            (0.4, (0.5, 0.41, 0.4)), (0.4, (0.4, F(0.4) + F(2.0 ** -25), 0.39999)), (0.6, (-0.1, 0.0, 0.6)),
            (F(2.0 ** -24), (F(2.0 ** -25), F(2.0 ** -24), 0.0))]
    for a in (0.5, 0.75, 0.3, F(1) - F(2.0 ** -24), 1.0 / 255, 0.5 / 255, 1.5 / 255):
        rows.append((a, tuple(_half_code(k, a) for k in (0, 7, 100))))
        rows.append((a, tuple(_half_code(k, a) for k in (126, 200, 254))))
    return rows


def inputs(N, seed=0):
    """image [N,3], weights_sum [N] (float32): two rays of every three from edge_rays() -- the walk through the table starts at N, so every N sees other edges on its
    last rays and tails -- and every third one seeded at random (alpha in [-0.05, 1.05], colours in [-0.05, 1.1] alpha)."""
    rng = np.random.RandomState(1000 + seed)
    edges = edge_rays()
    image, ws = np.zeros((N, 3), F), np.zeros(N, F)
    for i in range(N):
        if i % 3 == 2:
            ws[i] = F(rng.uniform(-0.05, 1.05))
            image[i] = (rng.uniform(-0.05, 1.1, 3) * max(float(ws[i]), 0.0)).astype(F)
        else:
            a, c = edges[(i + N) % len(edges)]
            ws[i], image[i] = F(a), np.asarray(c, F)
    return image, ws
