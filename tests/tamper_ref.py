"""Host restatement of the model-tampering kernels (include/nerfsig.h section "model tampering", csrc/tamper.hip) and of the verdict's p-value.
Written from the header's text, not from the kernels: numpy float32 bit for bit for prune / quantise / half, float64 for the noise and the statistics.

The noise's unit normal z is the one transcendental part: the device evaluates logf / sqrtf / cosf in fp32, this file in float64 from the same u1, u2 (both
exact 24-bit fractions).  EPS_Z bounds |z_device - z64|.  The local ROCm tree documents no ulp errors for these functions, so it was measured once, on one
MI355X, over the 2^24 draws of (seed 0, tensor 0) against `unit_normal` below (never against the kernel's own output): max |z - z64| = Z_ERR_MEASURED; the
margin for other seeds is four times that."""
import math
from fractions import Fraction

import numpy as np

from draw_ref import draw64, mix64, stream_key, unit24, unit24_open0      # noqa: F401 (mix64: importable from here as before)

MASK64 = (1 << 64) - 1
KINDS = {"prune": 0, "noise": 1, "quantize": 2, "half": 3}

Z_ERR_MEASURED = 1.0941252956975234e-06      # tools/tamper_bench.py --z-error, at element 13 608 692 (z = -1.369); most of it is the fp32 rounding of 6.2831855f * u2
EPS_Z = 4 * Z_ERR_MEASURED


def noise_uniforms(seed, i, n, first=0):
    """(u1 in (0, 1], u2 in [0, 1)) of elements first .. first + n - 1 of tensor i, as float64 (exact: multiples of 2^-24)."""
    h = draw64(stream_key(seed, i), np.arange(first, first + n, dtype=np.uint64))
    return unit24_open0(h >> np.uint64(40)), unit24((h >> np.uint64(8)) & np.uint64(0xFFFFFF))


def unit_normal(seed, i, n, first=0):
    """z64: Box-Muller in float64 from the documented hash.  The device multiplies u2 by the FLOAT 6.28318530717958648f: so does this."""
    u1, u2 = noise_uniforms(seed, i, n, first)
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(float(np.float32(6.28318530717958648)) * u2)


def unit_normal_f32(seed, i, n, first=0):
    """The kernel's own arithmetic in numpy float32 (numpy's logf / sqrtf / cosf: another libm, the same formula)."""
    u1, u2 = noise_uniforms(seed, i, n, first)
    u1, u2 = u1.astype(np.float32), u2.astype(np.float32)
    return np.sqrt(np.float32(-2.0) * np.log(u1)) * np.cos(np.float32(6.28318530717958648) * u2)


def finite_stats(x, biased=False):
    """(min, max, mean, unbiased deviation) of the finite elements of a float32 array, correctly rounded sums (math.fsum); (0, 0, 0, 0) without one, deviation 0 for one."""
    v = np.asarray(x, dtype=np.float32).reshape(-1)
    v = v[np.isfinite(v)].astype(np.float64)
    if v.size == 0:
        return (0.0, 0.0, 0.0, 0.0)
    mean = math.fsum(v.tolist()) / v.size
    ss = math.fsum(((v - mean) ** 2).tolist())      # ((v - mean)^2 in float64: relative error 2^-52 per term, far inside the tests' bound)
    if v.size < 2:
        return (float(v.min()), float(v.max()), mean, 0.0)
    return (float(v.min()), float(v.max()), mean, math.sqrt(ss / (v.size if biased else v.size - 1)))


def stats_bound(x):
    """Worst-case error of (mean, deviation) for ANY summation order in double: a sum of n terms errs by at most (n - 1) 2^-53 sum|terms| (to first order;
    doubled here for the higher orders and the final division / root)."""
    v = np.asarray(x, dtype=np.float32).reshape(-1)
    v = v[np.isfinite(v)].astype(np.float64)
    n = v.size
    if n < 2:
        return 0.0, 0.0
    u = 2.0 ** -53
    e_mean = 2.0 * ((n - 1) * u * float(np.abs(v).sum()) / n + u * abs(float(v.mean())))
    mean = float(v.mean())
    d2 = (v - mean) ** 2
    ss = float(d2.sum())
    # the device's mean is off by at most e_mean: each (x - mean)^2 moves by 2 |x - mean| e_mean + e_mean^2, plus the sum's own error and 3 u per term
    e_ss = 2.0 * ((n - 1) * u * ss + 3 * u * ss + 2.0 * float(np.abs(v - mean).sum()) * e_mean + n * e_mean ** 2)
    std = math.sqrt(ss / (n - 1))
    e_std = (e_ss / (n - 1)) / (2.0 * std) + 4 * u * std if std > 0 else math.sqrt(e_ss / (n - 1))
    return e_mean, e_std


def magnitudes(arrays):
    return np.concatenate([np.asarray(a, dtype=np.float32).reshape(-1).view(np.uint32) & np.uint32(0x7FFFFFFF) for a in arrays])


def abs_kth(arrays, k):
    """(threshold_bits, count_le): the k-th smallest (1-based) magnitude bit pattern over all arrays together, and how many are not above it."""
    m = magnitudes(arrays)
    if not 1 <= k <= m.size:
        raise ValueError(f"k = {k} of {m.size}")
    t = int(np.partition(m, k - 1)[k - 1])
    return t, int((m <= t).sum())


def prune(arrays, threshold_bits, strict=False):
    out = []
    for a in arrays:
        a = np.asarray(a, dtype=np.float32)
        m = a.view(np.uint32) & np.uint32(0x7FFFFFFF)
        out.append(np.where((m < threshold_bits) if strict else (m <= threshold_bits), np.float32(0.0), a))
    return out


def prune_fraction(arrays, p, per_tensor=False, strict=False):
    """Tamper.apply("prune", p): k = round(p total), global threshold.  per_tensor / strict: the mutants."""
    total = sum(np.asarray(a).size for a in arrays)
    if per_tensor:
        return [prune([a], abs_kth([a], max(1, int(round(p * np.asarray(a).size))))[0], strict)[0] if np.asarray(a).size else np.asarray(a, np.float32) for a in arrays]
    k = int(round(p * total))
    if k == 0:
        return [np.asarray(a, dtype=np.float32).copy() for a in arrays]
    return prune(arrays, abs_kth(arrays, k)[0], strict)


def quantize(arrays, bits, levels_plus_one=False, floor=False):
    """Every operation float32, in the header's order.  levels_plus_one / floor: the mutants."""
    out = []
    for a in arrays:
        a = np.asarray(a, dtype=np.float32)
        lo, hi, _, _ = finite_stats(a)
        lo, hi = np.float32(lo), np.float32(hi)
        if a.size == 0 or hi == lo:
            out.append(a.copy())
            continue
        L = np.float32((1 << bits) - 1 + (1 if levels_plus_one else 0))
        step = np.float32(hi - lo) / L
        with np.errstate(invalid="ignore", over="ignore"):
            r = (a - lo) / step
            q = np.minimum(L, np.maximum(np.float32(0.0), np.floor(r) if floor else np.rint(r))).astype(np.float32)
            y = (lo + q * step).astype(np.float32)
        out.append(np.where(np.isfinite(a), y, a))
    return out


def half(arrays):
    with np.errstate(over="ignore"):
        return [np.asarray(a, dtype=np.float32).astype(np.float16).astype(np.float32) for a in arrays]


def noise_scale(strength, std):
    return np.float32(float(strength) * float(std))


def noise64(arrays, strength, seed, biased=False):
    """(x + s z64 in float64, s, z64) per tensor."""
    out = []
    for i, a in enumerate(arrays):
        a = np.asarray(a, dtype=np.float32).reshape(-1)
        s = noise_scale(strength, finite_stats(a, biased)[3])
        z = unit_normal(seed, i, a.size)
        out.append((a.astype(np.float64) + float(s) * z, float(s), z))
    return out


def noise_bound(x, s, z64, eps_z):
    """|y - (x + s z64)| <= s eps_z + 2^-24 (|x| + s |z64|).  The device's y = fl(x + fl(s z)): the error of z (times s), the product's rounding (2^-24 s |z|) and
    the sum's (2^-24 (|x| + s |z|)).  The bound has one 2^-24 s |z| term; the other is at most 2^-24 * 5.77 s = 3.4e-7 s and sits inside the margin of
    eps_z = EPS_Z, three times the measured error (3.3e-6 s)."""
    return s * eps_z + 2.0 ** -24 * (np.abs(np.asarray(x, dtype=np.float64)) + s * np.abs(z64))


def p_value_exact(D, k):
    return Fraction(sum(math.comb(D, j) for j in range(k, D + 1)), 1 << D)
