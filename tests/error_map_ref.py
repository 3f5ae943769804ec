"""Host mirror of the error-map sampler (csrc/raygen.hip k_sample_rays_weighted): the counter hash in integers (tests/draw_ref.py), the race's keys in float64, the
selection as a sort -- and the statistic both generators are judged by (tests/test_gpu_error_map.py, tests/test_error_map_cpu.py)."""
import functools

import numpy as np

from draw_ref import draw_base, draw_word, mix32, unit24, unit24_open0      # noqa: F401 (random_bg_ref and the tests import the hashes from here)


def pose_of(step, stride, offset, P):
    return (step * stride + offset) % P


def key_uniforms(cells, seed, step):
    """u in (0, 1] of every cell, float64 (exact: 24 bits)."""
    return unit24_open0(draw_word(draw_base(seed, step, 1), np.arange(cells)) >> np.uint64(8))


def keys(weights, seed, step):
    """key = w / -ln(u) for a finite weight > 0, else 0; float64 [cells].  u == 1 gives +inf."""
    w = np.asarray(weights, dtype=np.float64)
    u = key_uniforms(w.shape[0], seed, step)
    valid = np.isfinite(w) & (w > 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        k = np.where(valid, np.where(valid, w, 1.0) / -np.log(u), 0.0)
    return k


def select(key, n):
    """The n cells with the largest keys, equal keys to the lower cell index; returned in ascending cell order."""
    key = np.asarray(key)
    order = np.lexsort((np.arange(key.shape[0]), -key.astype(np.float64)))[:n]
    return np.sort(order).astype(np.int64)


def pixels(cells_drawn, G, H, W, seed, step):
    """Pixel index of ray n (drawn cell n) in the kernel's own float32 arithmetic."""
    n = np.arange(len(cells_drawn))
    f32 = np.float32
    u1 = unit24(draw_word(draw_base(seed, step, 2), n) >> np.uint64(8)).astype(f32)
    u2 = unit24(draw_word(draw_base(seed, step, 3), n) >> np.uint64(8)).astype(f32)
    sx, sy = f32(H) / f32(G), f32(W) / f32(G)
    c = np.asarray(cells_drawn)
    row = np.minimum(H - 1, ((c // G).astype(f32) * sx + u1 * sx).astype(np.int64))
    col = np.minimum(W - 1, ((c % G).astype(f32) * sy + u2 * sy).astype(np.int64))
    return row * W + col


# ---- the distribution check (criterion: the reference's generator against the race)
DIST_G, DIST_N = 128, 4096


def dist_weights():
    """Weight 8 on cells [0, 4096), 0 on [8192, 9216), 1 elsewhere."""
    w = np.ones(DIST_G * DIST_G, np.float32)
    w[:4096] = 8.0
    w[8192:9216] = 0.0
    return w


def dist_statistic(drawn):
    """(fraction of the draw inside [0, 4096), number of zero-weight cells drawn)."""
    drawn = np.asarray(drawn)
    return float((drawn < 4096).mean()), int(((drawn >= 8192) & (drawn < 9216)).sum())


@functools.lru_cache(maxsize=None)
def multinomial_reference(draws=256, seed=0):
    """torch.multinomial(replacement=False) on the CPU: (mean, per-draw standard deviation) of the fraction, zero-weight hits.  Computed once per process."""
    import torch
    g = torch.Generator().manual_seed(seed)
    w = torch.from_numpy(dist_weights())
    stats = [dist_statistic(torch.multinomial(w, DIST_N, replacement=False, generator=g).numpy()) for _ in range(draws)]
    f = np.array([s[0] for s in stats])
    return float(f.mean()), float(f.std(ddof=1)), int(sum(s[1] for s in stats))


def dist_bound(s, n_test=64, n_ref=256):
    return 5.0 * s * (1.0 / n_test + 1.0 / n_ref) ** 0.5
