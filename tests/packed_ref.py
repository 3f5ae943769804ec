"""Host restatement of the packed table formats (include/nerfsig.h section "packed released model"), written from the header's text: numpy float32, every
operation rounded on its own, for "f16", "q8" and "q4".  pack -> (bytes, lo, step, non-finite count) per table, unpack -> the decoded float32 array.

    f16  row word: two IEEE halves, feature 0 in bits 0..15 (little endian: the halves in memory order)      decode (float)(_Float16)h
    q8   row word: two 8-bit codes, feature 0 in the low byte                                               decode lo + (float)q * step
    q4   row word: two 4-bit codes, feature 0 in the low nibble                                             decode lo + (float)q * step
    lo = (float)min, hi = (float)max of the finite values, L = 2^b - 1, step = (hi - lo) / L, q = min(L, max(0, rintf((x - lo) / step)));
    a constant table: code 0, step 0; a non-finite value: code 0, counted.

The mutants (swapped nibbles, floor for rint, L = 2^b) are there for the tests to show that each differs from tamper_ref."""
import numpy as np

FORMATS = {"f16": 0, "q8": 1, "q4": 2}
BITS = {"q8": 8, "q4": 4}
ROW_BYTES = {"f16": 4, "q8": 2, "q4": 1}


T = 1 << 19      # NSIG_TABLE_ROWS


# ---- the seeded tables the CPU and the GPU tests share

def tables(bits=8):
    """The seeded tables of the issue, float32 [T, 2] each: uniform +-1e-4 like the hash tables; all +0.0; min and max in the first and the last row; lo = 0,
    hi = L = 2^bits - 1 (step exactly 1) with every other value k + 0.5 on a rintf tie."""
    rng = np.random.RandomState(22)
    uniform = rng.uniform(-1e-4, 1e-4, (T, 2)).astype(np.float32)
    zeros = np.zeros((T, 2), np.float32)
    ends = rng.uniform(-1e-4, 1e-4, (T, 2)).astype(np.float32)
    ends[0, 0], ends[-1, 1] = -3e-4, 5e-4
    L = (1 << bits) - 1
    ties = ((np.arange(2 * T) % L).astype(np.float32) + np.float32(0.5)).reshape(T, 2)
    ties[0, 0], ties[-1, 1] = 0.0, float(L)
    return [uniform, zeros, ends, ties]


def half_table():
    """f16's hard values: round-to-nearest-even ties (1 + (2k+1) 2^-11), half subnormals and the ties between them (multiples of 2^-25), values around and
    above 65504 (65520 is the tie that rounds to infinity), and ordinary hash-table values."""
    rng = np.random.RandomState(23)
    t = rng.uniform(-1e-4, 1e-4, 2 * T).astype(np.float32)
    k = np.arange(4096, dtype=np.float32)
    t[:4096] = 1.0 + (2 * k + 1) * 2.0 ** -11
    t[4096:8192] = k * 2.0 ** -25 * np.where(k % 2 == 0, 1, -1)
    t[8192:8200] = [65504.0, 65519.0, 65520.0, 65536.0, 70000.0, -65520.0, -1e9, 65519.996]
    t[8200:8204] = [2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, 2.0 ** -26]
    return t.reshape(T, 2)


# ---- the restatement

def scalars(a, bits, levels_plus_one=False):
    """(lo, step, L) as float32 of a float32 array."""
    a = np.asarray(a, dtype=np.float32).reshape(-1)
    fin = a[np.isfinite(a)]
    lo = np.float32(fin.min()) if fin.size else np.float32(0.0)
    hi = np.float32(fin.max()) if fin.size else np.float32(0.0)
    L = np.float32((1 << bits) - 1 + (1 if levels_plus_one else 0))
    return lo, np.float32(np.float32(hi - lo) / L), L


def codes(a, bits, floor=False, levels_plus_one=False):
    """(uint8 codes of the array's shape, lo, step, non-finite count)."""
    a = np.asarray(a, dtype=np.float32)
    lo, step, L = scalars(a, bits, levels_plus_one)
    fin = np.isfinite(a)
    if step == 0:
        return np.zeros(a.shape, np.uint8), lo, step, int((~fin).sum())
    with np.errstate(invalid="ignore", over="ignore"):
        r = ((np.where(fin, a, lo) - lo) / step).astype(np.float32)
        q = np.minimum(L, np.maximum(np.float32(0.0), np.floor(r) if floor else np.rint(r)))
    return np.minimum(np.where(fin, q, 0), 255).astype(np.uint8), lo, step, int((~fin).sum())      # (255: only the L = 2^b mutant reaches 256)


def pack(a, fmt, swap_nibbles=False, floor=False, levels_plus_one=False):
    """a: float32 [rows, 2] -> (flat uint8 bytes, lo, step, non-finite count)."""
    a = np.asarray(a, dtype=np.float32).reshape(-1, 2)
    if fmt == "f16":
        with np.errstate(over="ignore"):
            return a.astype("<f2").reshape(-1).view(np.uint8).copy(), np.float32(0.0), np.float32(0.0), 0
    q, lo, step, bad = codes(a, BITS[fmt], floor, levels_plus_one)
    if fmt == "q8":
        return q.reshape(-1).copy(), lo, step, bad
    q = np.minimum(q, 15)                                         # (only the L = 2^b mutant reaches 16; it already differs in step)
    c0, c1 = (q[:, 1], q[:, 0]) if swap_nibbles else (q[:, 0], q[:, 1])
    return (c0 | (c1 << 4)).astype(np.uint8), lo, step, bad


def unpack(b, fmt, lo=0.0, step=0.0):
    """flat uint8 bytes -> float32 [rows, 2]."""
    b = np.asarray(b, dtype=np.uint8).reshape(-1)
    if fmt == "f16":
        return b.view("<f2").astype(np.float32).reshape(-1, 2)
    q = b.reshape(-1, 2) if fmt == "q8" else np.stack([b & 0xF, b >> 4], axis=1)
    lo, step = np.float32(lo), np.float32(step)
    prod = (q.astype(np.float32) * step).astype(np.float32)      # the product, rounded ...
    return (lo + prod).astype(np.float32)                         # ... then the sum, rounded


def round_trip(a, fmt, **mutant):
    b, lo, step, _ = pack(a, fmt, **mutant)
    return unpack(b, fmt, lo, step).reshape(np.asarray(a).shape)
