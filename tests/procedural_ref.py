"""ps_render_u8 restated in numpy from the text of include/nerfsig.h ("procedural scenes"): float32 rays, float64 behind them, every operation on its own and in
the header's order.  tests/test_procedural_cpu.py holds it to an exact check in fractions.Fraction and to closed forms; tests/test_gpu_procedural.py holds the
kernel to it by equality.

MUTANTS names deliberate errors (render(..., mutant=)): a test that cannot tell one of them from the restatement is not testing that rule."""
import math
from fractions import Fraction

import numpy as np

T_MIN = 1e-4
MUTANTS = ("wrong_root", "tie_high", "premultiplied", "checker_round")
f32 = np.float32


def subsample_positions(H, W, S):
    """u [H,W,S,S], v [H,W,S,S] float32, the last two axes (b, a): u = i + (2a+1)/(2S), v = j + (2b+1)/(2S)."""
    i, j = np.arange(W, dtype=f32)[None, :, None, None], np.arange(H, dtype=f32)[:, None, None, None]
    a, b = np.arange(S)[None, None, None, :], np.arange(S)[None, None, :, None]
    off = lambda k: (2 * k + 1).astype(f32) / f32(2 * S)
    z = np.zeros((H, W, S, S), f32)
    return (i + off(a)) + z, (j + off(b)) + z


def pixel_rays(pose, intr, u, v):
    """rg_get_rays' arithmetic at positions (u, v), float32 throughout -> o [3], d [..., 3]."""
    pose = np.asarray(pose, f32)
    fx, fy, cx, cy = (f32(t) for t in intr)
    x, y = (u - cx) / fx, (v - cy) / fy
    nrm = np.sqrt((x * x + y * y) + f32(1.0) * f32(1.0))
    dx, dy, dz = x / nrm, y / nrm, f32(1.0) / nrm
    d = np.stack([(dx * pose[r, 0] + dy * pose[r, 1]) + dz * pose[r, 2] for r in range(3)], axis=-1)
    assert d.dtype == f32
    return pose[:3, 3].copy(), d


def _sphere(q, o, d, mutant):
    c, r = q[4:7].astype(np.float64), np.float64(q[7])
    oc = o - c
    A = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    B = (oc[:, 0] * d[:, 0] + oc[:, 1] * d[:, 1]) + oc[:, 2] * d[:, 2]
    Cq = ((oc[:, 0] * oc[:, 0] + oc[:, 1] * oc[:, 1]) + oc[:, 2] * oc[:, 2]) - r * r
    disc = B * B - A * Cq
    ok = disc >= 0.0
    s = np.sqrt(np.where(ok, disc, 0.0))
    t = (-B - s) / A
    far = (-B + s) / A
    t = far if mutant == "wrong_root" else np.where(t > T_MIN, t, far)
    hit = ok & (t > T_MIN)
    n = ((o + t[:, None] * d) - c) / r
    return hit, t, n, s


def _box(q, o, d):
    N = len(d)
    tn, tf = np.full(N, -np.inf), np.full(N, np.inf)
    an, af = np.zeros(N, np.int64), np.zeros(N, np.int64)
    miss = np.zeros(N, bool)
    with np.errstate(divide="ignore", invalid="ignore"):
        for k in range(3):
            lo, hi = np.float64(q[4 + k]), np.float64(q[7 + k])
            zero = d[:, k] == 0.0
            miss |= zero & ((o[:, k] < lo) | (o[:, k] > hi))
            t0, t1 = (lo - o[:, k]) / d[:, k], (hi - o[:, k]) / d[:, k]
            nr, fr = np.where(d[:, k] > 0.0, t0, t1), np.where(d[:, k] > 0.0, t1, t0)
            up = ~zero & (nr > tn)
            tn, an = np.where(up, nr, tn), np.where(up, k, an)
            dn = ~zero & (fr < tf)
            tf, af = np.where(dn, fr, tf), np.where(dn, k, af)
    hit = ~miss & (tn <= tf) & (tf > T_MIN)
    outside = tn > T_MIN
    t, ax = np.where(outside, tn, tf), np.where(outside, an, af)
    n = np.zeros((N, 3))
    dk = d[np.arange(N), ax]
    n[np.arange(N), ax] = np.where(dk > 0.0, -1.0, 1.0)
    return hit, t, n


def cast(o, d, prims, mutant=None):
    """o [3] or [N,3], d [N,3] float32 -> (win int64 [N], -1 a miss; t [N]; n [N,3]; root [N]: sqrt(disc) of a winning sphere, NaN otherwise)."""
    d = np.asarray(d, f32).reshape(-1, 3).astype(np.float64)
    o = np.broadcast_to(np.asarray(o, f32).astype(np.float64), d.shape)
    N = len(d)
    win, best, normal, root = np.full(N, -1, np.int64), np.full(N, np.inf), np.zeros((N, 3)), np.full(N, np.nan)
    for k, q in enumerate(np.asarray(prims, f32).reshape(-1, 16)):
        if q[0] == 0.0:
            hit, t, n, s = _sphere(q, o, d, mutant)
        else:
            hit, t, n = _box(q, o, d)
            s = np.full(N, np.nan)
        take = hit & ((t <= best) if mutant == "tie_high" else (t < best))
        win, best, root = np.where(take, k, win), np.where(take, t, best), np.where(take, s, root)
        normal = np.where(take[:, None], n, normal)
    return win, best, normal, root


def shade(o, d, prims, light, ambient, win, t, n, mutant=None):
    """colour [N,3] float64 of the hit sub-samples (rows of a miss are 0)."""
    prims = np.asarray(prims, f32).reshape(-1, 16)
    d = np.asarray(d, f32).reshape(-1, 3).astype(np.float64)
    o = np.broadcast_to(np.asarray(o, f32).astype(np.float64), d.shape)
    l = np.asarray(light, f32).astype(np.float64)
    L = l / np.sqrt((l[0] * l[0] + l[1] * l[1]) + l[2] * l[2])
    amb = np.float64(f32(ambient))
    hit = win >= 0
    q = prims[np.where(hit, win, 0)] if len(prims) else np.zeros((len(d), 16), f32)
    p = o + np.where(hit, t, 0.0)[:, None] * d
    f = q[:, 2].astype(np.float64)[:, None]
    cells = np.rint(f * p) if mutant == "checker_round" else np.floor(f * p)
    odd = (cells.astype(np.int64).sum(-1) & 1) != 0
    albedo = np.where(((q[:, 1] != 0.0) & odd)[:, None], q[:, 13:16], q[:, 10:13]).astype(np.float64)
    nl = (n[:, 0] * L[0] + n[:, 1] * L[1]) + n[:, 2] * L[2]
    s = amb + (1.0 - amb) * np.maximum(0.0, nl)
    return np.where(hit[:, None], albedo * s[:, None], 0.0)


def resolve(colour, hit, S, C, bg, mutant=None):
    """colour [H,W,S,S,3], hit [H,W,S,S] -> uint8 [H,W,C]: the header's "Pixel" paragraph."""
    H, W = hit.shape[:2]
    total, hits = np.zeros((H, W, 3)), np.zeros((H, W), np.int64)
    for b in range(S):
        for a in range(S):
            total = np.where(hit[:, :, b, a, None], total + colour[:, :, b, a], total)
            hits = hits + hit[:, :, b, a]
    alpha = hits.astype(np.float64) / np.float64(S * S)
    with np.errstate(divide="ignore", invalid="ignore"):
        rgb = np.where(hits[..., None] > 0, total / (np.float64(S * S) if mutant == "premultiplied" else hits[..., None].astype(np.float64)), 0.0)
    clamp = lambda x: np.minimum(1.0, np.maximum(0.0, x))
    if C == 4:
        return np.concatenate([np.rint(255.0 * clamp(rgb)), np.rint(255.0 * alpha)[..., None]], -1).astype(np.uint8)
    bgd = np.asarray(bg, f32).astype(np.float64)
    return np.rint(255.0 * clamp(rgb * alpha[..., None] + bgd * (1.0 - alpha[..., None]))).astype(np.uint8)


def render(poses, intr, H, W, prims, light, ambient, S=1, C=4, bg=(1.0, 1.0, 1.0), rays=None, mutant=None, details=False):
    """uint8 [P,H,W,C].  rays: (o [P,3], d [P,H*W,3]) to use instead of the restated rays (S = 1 only: rays.get_rays' own).  details: also the winners [P,H,W,S,S]."""
    poses = np.asarray(poses, f32).reshape(-1, 4, 4)
    prims = np.asarray(prims, f32).reshape(-1, 16)
    out, wins = [], []
    for p, pose in enumerate(poses):
        if rays is None:
            u, v = subsample_positions(H, W, S)
            o, d = pixel_rays(pose, intr, u, v)
        else:
            assert S == 1
            o, d = np.asarray(rays[0][p], f32), np.asarray(rays[1][p], f32).reshape(H, W, 1, 1, 3)
        win, t, n, _ = cast(o, d, prims, mutant)
        colour = shade(o, d, prims, light, ambient, win, t, n, mutant)
        out.append(resolve(colour.reshape(H, W, S, S, 3), (win >= 0).reshape(H, W, S, S), S, C, bg, mutant))
        wins.append(win.reshape(H, W, S, S))
    return (np.stack(out), np.stack(wins)) if details else np.stack(out)


# ---- the exact check ----------------------------------------------------------------------------------------------------------------------------------

def _isqrt_bounds(x, bits=160):
    """Rationals lo <= sqrt(x) <= hi with hi - lo = 2^-bits, for a Fraction x >= 0 (lo == hi when the scaled root is an integer)."""
    n = x.numerator * x.denominator << (2 * bits)
    r = math.isqrt(n)
    den = x.denominator << bits
    return Fraction(r, den), Fraction(r if r * r == n else r + 1, den)


def exact_winner(o, d, prims):
    """Hit-or-miss and the winning primitive of ONE float32 ray by the header's rules in exact arithmetic: rationals everywhere, square roots enclosed in
    2^-160 intervals.  -> the index, -1 for a miss; None where the intervals cannot decide (never for the cases the tests use: asserted there)."""
    F = Fraction
    o, d, tmin = [F(float(v)) for v in o], [F(float(v)) for v in d], F(T_MIN)
    found = []          # (t_lo, t_hi, k)
    for k, q in enumerate(np.asarray(prims, f32).reshape(-1, 16)):
        a, b = [F(float(v)) for v in q[4:7]], [F(float(v)) for v in q[7:10]]
        if q[0] == 0.0:
            oc = [o[i] - a[i] for i in range(3)]
            A, B, Cq = sum(x * x for x in d), sum(x * y for x, y in zip(oc, d)), sum(x * x for x in oc) - b[0] * b[0]
            disc = B * B - A * Cq
            if disc < 0:
                continue
            lo, hi = _isqrt_bounds(disc)
            near, far = ((-B - hi) / A, (-B - lo) / A), ((-B + lo) / A, (-B + hi) / A)
            for t in (near, far):
                if t[0] > tmin:
                    found.append((t[0], t[1], k))
                    break
                if t[1] > tmin:
                    return None
        else:
            tn, tf, dead = None, None, False
            for i in range(3):
                if d[i] == 0:
                    dead |= o[i] < a[i] or o[i] > b[i]
                    continue
                t0, t1 = (a[i] - o[i]) / d[i], (b[i] - o[i]) / d[i]
                nr, fr = min(t0, t1), max(t0, t1)
                tn, tf = nr if tn is None else max(tn, nr), fr if tf is None else min(tf, fr)
            if dead or tn is None or tn > tf or not tf > tmin:
                continue
            t = tn if tn > tmin else tf
            found.append((t, t, k))
    if not found:
        return -1
    found.sort(key=lambda e: (e[0], e[2]))
    first = found[0]
    for e in found[1:]:
        if e[0] <= first[1] and not (e[0] == e[1] == first[0] == first[1]):      # overlapping intervals that are not one exact value
            return None
    return first[2]
