"""tests/draw_ref.py -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

The host statement of the device's two counter-hash families (csrc/draws.h), in integers.  numpy only; imports nothing of the product.  Every other
reference module of the tests takes its hashes from here; tests/test_draw_ref_cpu.py holds this file to a table of known words.

Every function takes Python ints (any width: reduced modulo 2^64 or 2^32) or numpy integer arrays, and returns a Python int when every argument was a
scalar, a uint64 array otherwise.

The 64-bit family (splitmix64's finaliser): the distortion layer, stage 1's march offsets, the grid refresh, the tamper noise.
    stream_key(seed, k) = mix64(seed ^ 0x9E3779B97F4A7C15 (k + 1))          one sequence per (seed, counter k)
    draw64(key, i)      = mix64(key + 0xD1B54A32D192ED03 (i + 1))           word i of a sequence
The 32-bit family (murmur3's finaliser): the ray samplers' streams 0..5 of a step.
    draw_base(seed, step, stream) = b = mix32(mix32(seed_lo ^ step 0x9e3779b9) + seed_hi), re-keyed for stream > 0 as mix32(b + stream 0x7f4a7c15)
    draw_word(base, i)            = mix32(base ^ (i 0x85ebca6b + 0x6b43a9b5))
A 24-bit word becomes a float on torch.rand's grid: unit24 in [0, 1), unit24_open0 in (0, 1]; both exact in float32 and float64."""
import numpy as np

MASK32 = (1 << 32) - 1
MASK64 = (1 << 64) - 1
_U = np.uint64

# the streams of one step of the 32-bit family
PIXEL_STREAM, RACE_KEY_STREAM, RACE_ROW_STREAM, RACE_COL_STREAM, BACKGROUND_STREAM, ORBIT_STREAM = range(6)


def _u64(v):
    if isinstance(v, (int, np.integer)):
        return np.asarray(int(v) & MASK64, dtype=np.uint64)
    return np.asarray(v).astype(np.uint64)


def _out(v, *args):
    return int(v) if all(isinstance(a, (int, np.integer)) for a in args) else v


def _mix64(v):
    with np.errstate(over="ignore"):
        v = (v ^ (v >> _U(30))) * _U(0xBF58476D1CE4E5B9)
        v = (v ^ (v >> _U(27))) * _U(0x94D049BB133111EB)
        return v ^ (v >> _U(31))


def mix64(v):
    """splitmix64's finaliser, modulo 2^64."""
    return _out(_mix64(_u64(v)), v)


def stream_key(seed, k):
    with np.errstate(over="ignore"):
        return _out(_mix64(_u64(seed) ^ (_U(0x9E3779B97F4A7C15) * (_u64(k) + _U(1)))), seed, k)


def draw64(key, i):
    with np.errstate(over="ignore"):
        return _out(_mix64(_u64(key) + _U(0xD1B54A32D192ED03) * (_u64(i) + _U(1))), key, i)


def _mix32(v):      # on uint64 holding 32-bit values: no product below leaves 64 bits
    v = v & _U(MASK32)
    v = v ^ (v >> _U(16))
    v = (v * _U(0x85EBCA6B)) & _U(MASK32)
    v = v ^ (v >> _U(13))
    v = (v * _U(0xC2B2AE35)) & _U(MASK32)
    return v ^ (v >> _U(16))


def mix32(v):
    """murmur3's finaliser, modulo 2^32."""
    return _out(_mix32(_u64(v)), v)


def draw_base(seed, step, stream):
    """The word of (seed, step) that every draw of sequence `stream` of that step starts from.  `seed` is 64 bits; `step` is read modulo 2^32."""
    lo, hi = _u64(seed) & _U(MASK32), _u64(seed) >> _U(32)
    b = _mix32(_mix32(lo ^ (((_u64(step) & _U(MASK32)) * _U(0x9E3779B9)) & _U(MASK32))) + hi)
    s = _u64(stream)
    return _out(np.where(s == _U(0), b, _mix32(b + s * _U(0x7F4A7C15))), seed, step, stream)


def draw_word(base, index):
    return _out(_mix32(_u64(base) ^ (((_u64(index) & _U(MASK32)) * _U(0x85EBCA6B) + _U(0x6B43A9B5)) & _U(MASK32))), base, index)


def unit24(word24):
    """word24 * 2^-24: [0, 1).  float64 (a Python float for a scalar); exact, and exactly representable in float32."""
    if isinstance(word24, (int, np.integer)):
        return int(word24) * 2.0 ** -24
    return np.asarray(word24).astype(np.float64) * 2.0 ** -24


def unit24_open0(word24):
    """(word24 + 1) * 2^-24: (0, 1]."""
    if isinstance(word24, (int, np.integer)):
        return (int(word24) + 1) * 2.0 ** -24
    return (np.asarray(word24).astype(np.float64) + 1.0) * 2.0 ** -24
