"""Error-map ray sampling without a GPU: the two entry points are declared, listed and exported; the watermark loop refuses a sampler that draws from a map;
the host mirror of the race (tests/error_map_ref.py) draws like torch.multinomial(replacement=False) and breaks ties the way the kernel is specified to."""
import os
import re
import types

import numpy as np
import pytest

import error_map_ref as em

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rg_sample_rays_weighted", "rg_error_map_update")


def test_entry_points_are_declared_listed_and_exported():
    from nerf_signature_amd import _native, build
    build.build()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nerfsig.h")).read(), flags=re.S)
    for name in SYMBOLS:
        assert re.search(r"^int\s+%s\s*\(" % name, header, flags=re.M), name
        assert name in _native.SIGNATURES
        _native.fn(name)
    # ... with as many arguments in the loader's table as in the header
    for name in SYMBOLS:
        args = re.search(r"^int\s+%s\s*\((.*?)\);" % name, header, flags=re.M | re.S).group(1)
        assert len(args.split(",")) == len(_native.SIGNATURES[name]), name


def test_argument_checks_need_no_gpu():
    from nerf_signature_amd import _native as nv, build
    build.build()
    d = nv._vp(256)
    head = (d, 3, d, 70.0, 70.0, 40.0, 30.0, 60, 80)
    with pytest.raises(ValueError, match="null pointer"):
        nv.call("rg_sample_rays_weighted", *head, 16, None, 1, 0, 0, None, 4, d, d, d, None, None, d, None, None)
    with pytest.raises(ValueError, match="null pointer"):
        nv.call("rg_sample_rays_weighted", *head, 16, None, 1, 0, 0, d, 4, d, d, d, None, None, None, None, None)
    for grid in (0, 129):
        with pytest.raises(ValueError, match="grid .* out of range"):
            nv.call("rg_sample_rays_weighted", *head, 1, None, 1, 0, 0, d, grid, d, d, d, None, None, d, None, None)
    for n in (0, 17):
        with pytest.raises(ValueError, match="N .* out of range"):
            nv.call("rg_sample_rays_weighted", *head, n, None, 1, 0, 0, d, 4, d, d, d, None, None, d, None, None)
    with pytest.raises(ValueError, match="null pointer"):
        nv.call("rg_error_map_update", d, 3, 4, None, d, d, d, 16, None)
    with pytest.raises(ValueError, match="out of range"):
        nv.call("rg_error_map_update", d, 3, 129, d, d, d, d, 16, None)


def test_watermark_loop_refuses_a_map_sampler():
    from nerf_signature_amd.trainer import GraphedWatermarkLoop
    sampler = types.SimpleNamespace(error_map=np.ones((2, 16), np.float32))
    with pytest.raises(ValueError, match="stage 1"):
        GraphedWatermarkLoop(None, None, {}, None, content_sampler=sampler)


def test_mirror_selection_rules():
    # equal keys go to the lower cell; the result is ascending
    key = np.array([0.5, 2.0, 2.0, 0.5, 2.0, 0.0, 0.5])
    assert em.select(key, 2).tolist() == [1, 2] and em.select(key, 4).tolist() == [0, 1, 2, 4] and em.select(key, 7).tolist() == list(range(7))
    # invalid weights have key 0 and fill a draw only behind every valid cell, lowest index first
    w = np.array([0.0, 1.0, np.nan, -2.0, np.inf, 3.0, 0.0, 1e-6], np.float32)
    k = em.keys(w, seed=5, step=3)
    assert (k[[0, 2, 3, 4, 6]] == 0).all() and (k[[1, 5, 7]] > 0).all()
    assert em.select(k, 3).tolist() == [1, 5, 7] and em.select(k, 5).tolist() == [0, 1, 2, 5, 7]
    # the uniforms lie in (0, 1], differ between steps and seeds, and repeat for the same (seed, step)
    u = em.key_uniforms(16384, seed=(7 << 32) | 9, step=11)
    assert u.min() > 0 and u.max() <= 1 and abs(u.mean() - 0.5) < 5 / (12 * 16384) ** 0.5
    assert np.array_equal(u, em.key_uniforms(16384, seed=(7 << 32) | 9, step=11))
    assert not np.array_equal(u, em.key_uniforms(16384, seed=(7 << 32) | 9, step=12)) and not np.array_equal(u, em.key_uniforms(16384, seed=(8 << 32) | 9, step=11))
    # ties are ordinary: an all-ones map has coinciding 24-bit uniforms among its 16 384 cells
    assert len(np.unique(u)) < 16384


def test_mirror_draws_like_torch_multinomial():
    """The statistic of the GPU test on the host: the fraction of a 4096-cell draw that lands in the weight-8 quarter, 64 steps of the race against 256 draws of
    torch.multinomial(replacement=False); no draw touches a zero-weight cell."""
    m, s, zero_hits = em.multinomial_reference()
    assert zero_hits == 0
    w = em.dist_weights()
    stats = [em.dist_statistic(em.select(em.keys(w, seed=1234, step=step), em.DIST_N)) for step in range(64)]
    mean = float(np.mean([f for f, _ in stats]))
    print(f"\nmultinomial: mean {m:.5f}, per-draw sd {s:.5f}; race: mean {mean:.5f}; |difference| {abs(mean - m):.2e} <= bound {em.dist_bound(s):.2e}")
    assert abs(mean - m) <= em.dist_bound(s)
    assert sum(z for _, z in stats) == 0
