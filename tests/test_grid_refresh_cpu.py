"""The density-grid refresh entry points (csrc/gridrefresh.hip) without a GPU: tests/grid_refresh_ref.py against the oracle's update_extra_state, the restated
generator alone, every refusal of rg_refresh_begin / draw / points / scatter / finish word for word (each returns before a launch), and the two byte-size
queries against the layout the header states."""
import math
import re

import numpy as np
import pytest
import torch

import closed_form as cf
import grid_refresh_ref as gr
from oracle import field_ref as fr


@pytest.fixture(scope="module")
def native():
    from nerf_signature_amd import build, _native
    build.build()
    return _native


def _refused(native, text, name, *args):
    with pytest.raises(ValueError, match=re.escape(text)):
        native.call(name, *args)


# ---- the reference against the oracle

PALETTE = np.array([-0.5, -0.0, 0.0, 1e-3, 0.3, 0.95, 1.0, 2.5, 40.0], np.float32)


def _oracle_case(iter_density, thresh, seed):
    """One update_extra_state of the oracle on a 16^3 two-cascade grid whose density_fn hands out prescribed values; returns (old grid, tmp, state)."""
    G, C = 16, 2
    rng = np.random.RandomState(seed)
    old = rng.choice(np.array([-1.0, 0.0, 0.2, 1.0, 3.0], np.float32), size=(C, G ** 3)).astype(np.float32)
    ring = torch.zeros(16, 2, dtype=torch.int32)
    ring[:, 0] = torch.from_numpy(rng.randint(0, 5000, 16).astype(np.int32))
    ring[:, 1] = 77
    st = {"density_grid": torch.from_numpy(old.copy()), "density_bitfield": None, "bound": 2, "grid_size": G, "density_scale": 1, "density_thresh": thresh,
          "iter_density": iter_density, "mean_density": 0, "step_counter": ring, "local_step": 5, "mean_count": 0}

    def density(x, message):
        return {"sigma": torch.from_numpy(rng.choice(PALETTE, size=x.shape[0]))}

    with cf.PatchedDraws():
        tmp, _ = fr.update_extra_state(st, density, None, 0.95, 8, rand_like=torch.rand_like, randint=torch.randint)
    return old, tmp.numpy(), st


@pytest.mark.parametrize("iter_density", [3, 16])
@pytest.mark.parametrize("thresh", [0.01, 1e9])
def test_finish_equals_the_oracles_tail(iter_density, thresh):
    """finish() fed the oracle's own tmp grid: grid bit for bit, mean_count, and the bitfield -- at a threshold below the mean exactly; at one above it the level is
    the mean itself, which the oracle sums in float32 (torch.mean) and the reference in float64: no cell may then lie between the two, asserted."""
    old, tmp, st = _oracle_case(iter_density, thresh, seed=iter_density)
    assert (tmp < 0).any() and (tmp == 0).any() and (tmp > 0).any() and np.signbit(tmp[tmp == 0]).any()
    if iter_density >= 16:
        assert (tmp == -1).mean() > 0.2                                            # the partial form leaves cells unprobed
    grid, mean, bits, mean_count = gr.finish(old, tmp, 0.95, thresh, st["step_counter"].numpy(), 5, 5)
    want = st["density_grid"].numpy()
    assert np.array_equal(grid.view(np.uint32), want.reshape(-1).view(np.uint32))
    assert (want != old).mean() > 0.2 and (want[old < 0] == -1).all()
    assert mean == pytest.approx(st["mean_density"], rel=1e-6) and (mean > thresh) == (thresh < 1)
    lo, hi = sorted((float(np.float32(mean)), float(st["mean_density"])))
    assert not ((want >= np.nextafter(np.float32(lo), np.float32(-1))) & (want <= np.nextafter(np.float32(hi), np.float32(np.inf)))).any()
    assert np.array_equal(bits, st["density_bitfield"].numpy())
    assert 0.02 < np.unpackbits(bits).mean() < 0.98
    assert mean_count == st["mean_count"] == int(int(st["step_counter"][:5, 0].sum()) / 5) and mean_count > 0


def test_scatter_keeps_what_the_oracles_mask_keeps():
    """scatter() + finish() on single candidates per cell against the oracle's `valid = (grid >= 0) & (tmp >= 0)`: negative and NaN candidates leave the cell alone,
    both zeros let it decay; repeated cells keep the largest, a NaN among them wins."""
    vals = np.array([-2.0, -0.0, 0.0, 0.5, 3.0, np.inf, np.nan, -np.inf], np.float32)
    fresh = gr.scatter(vals, np.arange(8), 1.0, 16)
    tmp = np.full(16, -1.0, np.float32)
    tmp[:8] = vals
    grid = torch.ones(16)
    with np.errstate(invalid="ignore"):
        valid = torch.from_numpy(tmp >= 0)
    grid[valid] = torch.maximum(grid[valid] * 0.95, torch.from_numpy(tmp)[valid])      # field_ref.py:613-614
    got = gr.finish(np.ones(16, np.float32), fresh, 0.95, 0.5)[0]
    assert np.array_equal(got, grid.numpy()) and got[:8].tolist() == [1.0, np.float32(0.95), np.float32(0.95), np.float32(0.95), 3.0, np.inf, 1.0, 1.0]
    assert np.isnan(fresh[6]) and not np.signbit(fresh[1]) and fresh[1] == 0 and fresh[0] == fresh[7] == -1 and (fresh[8:] == -1).all()
    many = gr.scatter(np.array([0.25, 4.0, -1.0, 1.0, np.nan, 7.0, 0.5], np.float32), np.array([3, 3, 3, 5, 5, 5, 0]), 0.5, 8)
    assert many[3] == 2.0 and np.isnan(many[5]) and many[0] == 0.25 and (many[[1, 2, 4, 6, 7]] == -1).all()


# ---- the restated generator alone (this guards the reference, not the kernel)

def _chi2_sf(x, k):
    """P(chi-square with k degrees of freedom > x): Simpson's rule on the density over [x, x + 400] (the tail beyond is below 1e-80)."""
    def pdf(t):
        return math.exp((k / 2 - 1) * math.log(t) - t / 2 - (k / 2) * math.log(2) - math.lgamma(k / 2))
    n, h = 40000, 400 / 40000
    return (pdf(x) + pdf(x + 400) + sum((4 if i % 2 else 2) * pdf(x + i * h) for i in range(1, n))) * h / 3


def test_generator_is_on_the_24_bit_grid_and_uniform():
    b = gr.draw(gr.stream(5, 16, 1, 2), np.arange(1 << 16, dtype=np.uint64))
    u = gr.u01(b)
    assert u.min() >= 0 and u.max() < 1 and np.array_equal(u * 16777216.0, np.floor(u * 16777216.0))
    assert np.array_equal(u.astype(np.float32).astype(np.float64), u) and np.unique(u).size > 65000
    assert int(gr.mix64(0)) == 0 and int(gr.mix64(1)) == 0x5692161D100B05E5            # splitmix64's finaliser: the published value for 1
    # streams differ in every argument
    keys = {int(gr.stream(*a)) for a in ((5, 16, 1, 2), (6, 16, 1, 2), (5, 17, 1, 2), (5, 16, 2, 2), (5, 16, 1, 1), (5, -1, 1, 2), (5, (1 << 31) - 1, 1, 2))}
    assert len(keys) == 7 and gr.stream(5, -1, 1, 2) == gr.stream(5, (1 << 32) - 1, 1, 2)
    # chi-square of 2^16 uniform cell draws per axis at H = 16: 15 degrees of freedom, bound = the distribution's own upper 1e-6 quantile
    bound = 56.4934
    assert _chi2_sf(bound, 15) == pytest.approx(1e-6, rel=1e-3)
    n = 1 << 16
    for seed, it, cas in ((0, 0, 0), (5, 16, 1), (123456789012345, (1 << 31) - 1, 7)):
        for axis in gr.uniform_cells(n, 16, seed, it, cas):
            counts = np.bincount(axis, minlength=16)
            assert counts.size == 16 and float(((counts - n / 16) ** 2 / (n / 16)).sum()) < bound
    # the keys of the uniform half are those cells; the occupied half indexes flatnonzero in morton order
    grid = np.zeros(16 ** 3, np.float32)
    grid[[7, 4095]] = 1.0                                                              # morton 7 = (1, 1, 1), morton 4095 = (15, 15, 15)
    k = gr.draw_keys(grid, 64, 16, 5, 16, 1)
    x, y, z = gr.uniform_cells(64, 16, 5, 16, 1)
    assert np.array_equal(k[:64], (z * 16 + y) * 16 + x) and set(k[64:].tolist()) == {(1 * 16 + 1) * 16 + 1, 4095}
    assert (gr.draw_keys(np.full(16 ** 3, -1.0, np.float32), 64, 16, 5, 16, 1)[64:] == 0).all()
    assert gr.morton(np.array([1, 15, 3]), np.array([1, 15, 0]), np.array([1, 15, 4])).tolist() == [7, 4095, 1 + 8 + 256]


# ---- refusals: each returns before a launch, with its message

def test_begin_and_scatter_refusals(native):
    d = native._vp(256)
    _refused(native, "rg_refresh_begin: null pointer or no cells", "rg_refresh_begin", None, 8, None)
    _refused(native, "rg_refresh_begin: null pointer or no cells", "rg_refresh_begin", d, 0, None)
    for args in ((None, d, 4, 1.0, d, None), (d, None, 4, 1.0, d, None), (d, d, 4, 1.0, None, None)):
        _refused(native, "rg_refresh_scatter: null pointer", "rg_refresh_scatter", *args)
    native.call("rg_refresh_scatter", d, d, 0, 1.0, d, None)                           # nothing to scatter: no launch, no error


def test_draw_refusals(native):
    d, name = native._vp(256), "rg_refresh_draw"
    ok = [d, d, 64, 16, d, d, 0, d, 0, None]      # keys, ids, N, H, grid_cas, scratch, seed, iter_dev, cas, stream
    for H in (0, 4, 12, 100, 2048):
        _refused(native, f"rg_refresh_draw: grid size {H} must be a power of two in [8,1024]", name, *(ok[:3] + [H] + ok[4:]))
    for i in (0, 1, 4, 5, 7):
        _refused(native, "rg_refresh_draw: null pointer", name, *(ok[:i] + [None] + ok[i + 1:]))
    for N, cas in ((0, 0), (1 << 29, 0), ((1 << 32) - 1, 0), (64, 8)):
        _refused(native, "rg_refresh_draw: N must be in [1, 2^29), cascade < 8", name, *(ok[:2] + [N] + ok[3:8] + [cas, None]))
    _refused(native, "rg_refresh_draw: scratch must be 4-byte, the grid 16-byte aligned", name, *(ok[:4] + [native._vp(264)] + ok[5:]))
    _refused(native, "rg_refresh_draw: scratch must be 4-byte, the grid 16-byte aligned", name, *(ok[:5] + [native._vp(258)] + ok[6:]))


def test_points_refusals(native):
    d, name = native._vp(256), "rg_refresh_points"
    ok = [d, d, 64, 16, 1.0, 0.0625, 0, d, 0, d, d, None]      # keys, ids, n, H, extent, half_cell, seed, iter_dev, cas, xyz, cells, stream
    for H in (4, 24, 2048):
        _refused(native, f"rg_refresh_points: grid size {H} must be a power of two in [8,1024]", name, *(ok[:3] + [H] + ok[4:]))
    for i in (7, 9, 10):
        _refused(native, "rg_refresh_points: null pointer", name, *(ok[:i] + [None] + ok[i + 1:]))
    for i, v in ((2, 0), (4, 0.0), (4, -1.0), (5, 0.0), (8, 8)):
        _refused(native, "rg_refresh_points: n, extent and half_cell must be positive, cascade < 8", name, *(ok[:i] + [v] + ok[i + 1:]))
    together = "rg_refresh_points: keys and ids come together (rg_refresh_draw) or not at all"
    _refused(native, together, name, *([d, None] + ok[2:]))
    _refused(native, together, name, *([None, d] + ok[2:]))
    whole = "rg_refresh_points: without keys the probe is the whole grid (n = H^3)"
    for n in (64, 16 ** 3 - 1, 16 ** 3 + 1):
        _refused(native, whole, name, *([None, None, n] + ok[3:]))


def test_finish_refusals(native):
    d, name = native._vp(256), "rg_refresh_finish"
    # grid, fresh, n_cells, decay, partials, density_thresh, bitfield, mean_density, iter_dev, count_ring, window, step_dev, mean_count, stream
    ok = [d, d, 64, 0.95, d, 0.01, d, d, d, d, 5, d, d, None]
    for i in (0, 1, 4, 6, 7, 8):
        _refused(native, "rg_refresh_finish: null pointer", name, *(ok[:i] + [None] + ok[i + 1:]))
    count = "rg_refresh_finish: the cell count must be a positive multiple of 8, window <= 16"
    for n in (0, 4, 12, 4097):
        _refused(native, count, name, *(ok[:2] + [n] + ok[3:]))
    _refused(native, count, name, *(ok[:10] + [17] + ok[11:]))
    ring = "rg_refresh_finish: a window needs the count ring and somewhere to put the mean"
    for window in (1, 16):
        _refused(native, ring, name, *(ok[:9] + [None, window] + ok[11:]))
        _refused(native, ring, name, *(ok[:10] + [window, d, None, None]))
    aligned = "rg_refresh_finish: grid must be 16-byte, partials 8-byte aligned"
    _refused(native, aligned, name, *([native._vp(264)] + ok[1:]))
    _refused(native, aligned, name, *(ok[:4] + [native._vp(260)] + ok[5:]))


def test_byte_size_queries(native):
    """include/nerfsig.h / gridrefresh.hip: the draw's scratch is, in int32 words, [2N draws | H^2 row bins | H^3 occupancy prefix | ceil(H^3 / 4096) workgroup
    counts | where H^2 <= 16 384: ceil(2N / 8192) histograms of H^2 rows]; the finish's partials one double per 4096 cells."""
    scratch, partials = native.fn("rg_refresh_draw_scratch_bytes"), native.fn("rg_refresh_partials_bytes")
    for H, with_hist in ((8, True), (128, True), (256, False)):
        for N in (1, 4096, 4097):
            words = 2 * N + H * H + H ** 3 + -(-H ** 3 // 4096) + (-(-2 * N // 8192) * H * H if with_hist else 0)
            assert scratch(N, H) == 4 * words
    assert scratch(128 ** 3 // 4, 128) == 4 * (128 ** 3 // 2 + 128 ** 2 + 128 ** 3 + 512 + 128 * 128 ** 2)
    for n, blocks in ((8, 1), (4096, 1), (4104, 2), (2 * 32 ** 3, 16), (2 * 128 ** 3, 1024)):
        assert partials(n) == 8 * blocks
