"""tests/distill_ref.py -- the restatement of rm_finish_u8 (include/nerfsig.h, "the render tail that writes STORE BYTES") that the GPU tests compare the kernel with --
held to exact arithmetic in fractions.Fraction, to dataset.decode_u8, to the consistency of its two channel counts and to its own mutants; every refusal of the entry
point word for word through the built library.  No GPU."""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import distill_ref as dr  # noqa: E402

F = np.float32
# How far the float32 value 255 clamp(x) can lie from the exact one.  C = 3: 1 - a, its product with bg_c <= 1 and the sum each round by at most 2^-25 where the
# result is in [0, 1] (outside, the clamp decides); the scale by 255 multiplies that by 255 and rounds once more, by at most 2^-17 (half an ulp under 256):
# 255 * 3 * 2^-25 + 2^-17 = 3.0e-5.  C = 4: one division and the scale, 255 * 2^-25 + 2^-17 = 1.5e-5.  2^-14 = 6.1e-5 covers both twice over.
TIE_MARGIN = Fraction(1, 1 << 14)
EXCLUDED_CAP = 0.01


def case_list():
    """6000 seeded rays -- alpha in [-0.05, 1.05], a tenth of them exactly 0 or 1, colours in [-0.05, 1.1] alpha -- and every row of distill_ref.edge_rays() once."""
    rng = np.random.RandomState(26)
    n = 6000
    ws = rng.uniform(-0.05, 1.05, n)
    pick = rng.rand(n)
    ws[pick < 0.05], ws[pick > 0.95] = 0.0, 1.0
    image = rng.uniform(-0.05, 1.1, (n, 3)) * np.maximum(ws, 0.0)[:, None]
    image[pick < 0.05] = rng.uniform(0, 1, (int((pick < 0.05).sum()), 3))      # colour without alpha: straight alpha writes 0
    edges = dr.edge_rays()
    ws = np.concatenate([ws.astype(F), np.array([e[0] for e in edges], F)])
    image = np.concatenate([image.astype(F), np.array([e[1] for e in edges], F)])
    return image, ws


CASES = case_list()


def exact_disagreements(finish):
    """(values whose byte is not the correctly rounded one, values excluded because the exact value is within TIE_MARGIN of a tie, values in all) over CASES, both
    channel counts and both backgrounds of distill_ref.BGS."""
    image, ws = CASES
    wrong = excluded = total = 0
    for C, bg in ((4, dr.BGS[0]), (3, dr.BGS[0]), (3, dr.BGS[1])):
        got = finish(image, ws, C, bg)
        for i in range(len(ws)):
            for c in range(C):
                q = dr.exact_value(image[i, c] if c < 3 else 0.0, ws[i], C, bg[c] if c < 3 else None, alpha=(c == 3))
                total += 1
                if abs(q - (int(q) + Fraction(1, 2))) <= TIE_MARGIN:
                    excluded += 1
                elif int(got[i, c]) != dr.round_half_even(q):
                    wrong += 1
    return wrong, excluded, total


def decode_disagreements(finish):
    """Values where dataset.decode_u8 of the byte lies more than half a code (and 2^-20 for the float32 roundings on both sides) from the float picture."""
    from nerf_signature_amd import dataset as ds
    image, ws = CASES
    bad = 0
    for C, bg in ((4, dr.BGS[0]), (3, dr.BGS[1])):
        picture = np.clip(dr.float_picture(image, ws, C, bg).astype(np.float64), 0.0, 1.0)
        decoded = ds.decode_u8(torch.from_numpy(finish(image, ws, C, bg))).numpy().astype(np.float64)
        bad += int((np.abs(decoded - picture) > 0.5 / 255 + 2.0 ** -20).sum())
    return bad


def blend_disagreements(finish):
    """Values where the C = 4 bytes, decoded and blended over bg by the reference's RGBA expression rgb a + bg (1 - a), land more than one code from the C = 3 byte.
    Why one code is the bound: with e_rgb, e_a the code errors of the stored colour and alpha (each at most half a code), the blend is off by
    e_rgb a + e_a (rgb - bg) (+ e_rgb e_a, a thousandth of a code): under one code unless a AND |rgb - bg| both exceed 0.996 -- and a shift under one code moves the
    rounded code by at most one.  Held on the values a compositor can produce, 0 <= image_c <= a (a sum of w_i c_i with colours in [0, 1]): a colour above its
    alpha is clamped by the straight form and not by the premultiplied one, and the two then differ by design.  Returns (disagreements, values compared)."""
    image, ws = CASES
    a32 = np.fmin(np.fmax(ws, F(0)), F(1))[:, None]
    physical = (image >= 0) & (image <= a32)
    bad = 0
    for bg in dr.BGS:
        four, three = finish(image, ws, 4, bg).astype(np.float64), finish(image, ws, 3, bg).astype(np.int64)
        a = four[:, 3:] / 255.0
        blended = np.rint(255.0 * (four[:, :3] / 255.0 * a + np.asarray(bg, np.float64)[None, :] * (1.0 - a))).astype(np.int64)
        bad += int(((np.abs(blended - three) > 1) & physical).sum())
    return bad, 2 * int(physical.sum())


def test_bytes_are_the_correctly_rounded_ones():
    wrong, excluded, total = exact_disagreements(dr.finish_u8)
    print(f"\nexact check: {total} values, {excluded} within 2^-14 of a tie and excluded ({100.0 * excluded / total:.3f} %), {wrong} wrong")
    assert total > 60000 and wrong == 0
    assert excluded <= EXCLUDED_CAP * total
    assert excluded >= 30          # the half-code edges ARE in the list (and are what the cap is for)


def test_decode_is_within_half_a_code_of_the_float_picture():
    assert decode_disagreements(dr.finish_u8) == 0


def test_rgba_over_the_background_is_within_a_code_of_rgb():
    bad, compared = blend_disagreements(dr.finish_u8)
    assert bad == 0 and compared > 20000


def test_edge_rays_by_hand():
    """The edges' bytes written out: alpha 0 writes (0, 0, 0, 0) whatever the colour; a denormal alpha divides; 1 + 2^-23 and 1.5 clamp to 255; a negative alpha is 0;
    a colour above alpha is 255; RGB over a background keeps the background where alpha is 0."""
    f = dr.finish_u8
    one_up, den = F(1) + F(2.0 ** -23), F(1e-40)
    assert f([[0.3, 0.0, 1.0]], [0.0], 4).tolist() == [[0, 0, 0, 0]]
    assert f([[0.3, 0.2, 0.1]], [-1e-3], 4).tolist() == [[0, 0, 0, 0]]
    assert f([[0.0, den, F(2e-40)]], [den], 4).tolist() == [[0, 255, 255, 0]]
    assert f([[1.0, one_up, 0.25]], [one_up], 4).tolist() == [[255, 255, 64, 255]]
    assert f([[0.2, 0.9, 1.2]], [1.5], 4).tolist() == [[51, 230, 255, 255]]
    assert f([[0.5, 0.41, 0.4]], [0.4], 4).tolist() == [[255, 255, 255, 102]]
    assert f([[0.0, 0.0, 0.0]], [0.0], 3, (0.2, 0.6, 1.0)).tolist() == [[51, 153, 255]]
    assert f([[0.0, 0.0, 0.0]], [-1e-3], 3, (0.2, 0.6, 1.0)).tolist() == [[51, 153, 255]]
    assert f([[0.25, 0.5, 1.0]], [1.5], 3, (0.2, 0.6, 1.0)).tolist() == [[64, 128, 255]]
    # half to even: 255 * (0.5 / 255) and 255 * (2.5 / 255) are exactly 0.5 and 2.5 in float32
    assert F(255) * F(0.5 / 255) == F(0.5) and F(255) * F(2.5 / 255) == F(2.5)
    assert f([[F(0.5 / 255), F(2.5 / 255), 0.0]], [1.0], 4).tolist() == [[0, 2, 0, 255]]


@pytest.mark.parametrize("mutant,check", [("truncate", "exact"), ("premultiplied", "blend"), ("clamp_after_scale", "decode"), ("alpha_unclamped", "exact")])
def test_every_mutant_is_caught(mutant, check):
    """truncation instead of rint; premultiplied instead of straight rgb; the clamp after the scale; alpha not clamped -- each fails the check named beside it (and
    changes bytes of the case list)."""
    finish = lambda image, ws, C, bg: dr.finish_u8(image, ws, C, bg, mutant=mutant)
    image, ws = CASES
    assert any((finish(image, ws, C, dr.BGS[1]) != dr.finish_u8(image, ws, C, dr.BGS[1])).any() for C in (3, 4))
    if check == "exact":
        assert exact_disagreements(finish)[0] > 0
    elif check == "blend":
        assert blend_disagreements(finish)[0] > 0
    else:
        assert decode_disagreements(finish) > 0


def test_every_refusal_word_for_word():
    """rm_finish_u8 checks before it launches: each refusal by its whole message, through the built library, with addresses that are never used; N = 0 is a no-op."""
    from nerf_signature_amd import _native as nv, build
    build.build()
    d = nv._vp(256)

    def refused(message, image=d, ws=d, N=8, C=4, out=d):
        with pytest.raises(ValueError) as e:
            nv.call("rm_finish_u8", image, ws, N, C, 1.0, 1.0, 1.0, out, None)
        assert str(e.value) == f"rm_finish_u8 failed (code 1): rm_finish_u8: {message}"

    for c in (0, 1, 2, 5, 8):
        refused(f"channels={c} is not 3 or 4", C=c)
    refused("channels=5 is not 3 or 4", C=5, N=0)
    for c in (3, 4):
        refused("null pointer", image=None, C=c)
        refused("null pointer", ws=None, C=c)
        refused("null pointer", out=None, C=c)
        nv.call("rm_finish_u8", None, None, 0, c, 1.0, 1.0, 1.0, None, None)      # N = 0: nothing to do, nothing looked at
    assert nv.SIGNATURES["rm_finish_u8"] == [nv._vp, nv._vp, nv._u32, nv._u32, nv._fl, nv._fl, nv._fl, nv._vp, nv._vp]
