"""The stage-1 RGBA step without a GPU: the mirror of the background draw (tests/random_bg_ref.py) is uniform on torch.rand's grid and a sequence of its own; the
three entry points are declared, listed, exported and check their arguments."""
import os
import re

import numpy as np
import pytest

import error_map_ref as em
import random_bg_ref as rb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rg_blend_random_background", "rg_sample_rays_rgba", "rg_sample_rays_weighted_rgba")
SEED = (0x1234 << 32) | 99


def test_mirror_values_lie_on_the_24_bit_grid():
    for step in (0, 7, 2 ** 31 - 1):
        bg = rb.background(4096, SEED, step)
        assert bg.dtype == np.float32 and bg.shape == (4096, 3)
        assert float(bg.min()) >= 0.0 and float(bg.max()) < 1.0
        scaled = bg.astype(np.float64) * (1 << 24)
        assert np.array_equal(scaled, np.round(scaled))
        assert np.array_equal(bg, rb.background(4096, SEED, step))
    assert not np.array_equal(rb.background(64, SEED, 3), rb.background(64, SEED, 4))
    assert not np.array_equal(rb.background(64, SEED, 3), rb.background(64, SEED + (1 << 32), 3))
    # a prefix of a longer draw: ray n's colour does not depend on the batch size
    assert np.array_equal(rb.background(64, SEED, 3), rb.background(65, SEED, 3)[:64])


def test_sequence_4_is_none_of_the_samplers_sequences():
    assert rb.STREAM == 4
    for step in (0, 11):
        bases = [int(em.draw_base(SEED, step, s)) for s in range(5)]
        assert len(set(bases)) == 5
        mine = rb.background(1024, SEED, step)
        for s in range(4):
            other = rb.background(1024, SEED, step, stream=s)
            assert float((mine == other).mean()) < 0.01, s


def test_mirror_blend_is_the_float32_expression():
    import torch
    rng = np.random.RandomState(3)
    rgba = rng.rand(1000, 4).astype(np.float32)
    rgba[:100, 3], rgba[100:200, 3] = 0.0, 1.0
    bg = rb.background(1000, SEED, 5)
    t, b = torch.from_numpy(rgba), torch.from_numpy(bg)
    want = t[..., :3] * t[..., 3:] + b * (1 - t[..., 3:])
    got = rb.blend(rgba, bg)
    assert np.array_equal(got, want.numpy())
    assert np.array_equal(got[:100], bg[:100]) and np.array_equal(got[100:200], rgba[100:200, :3])


def test_draws_are_uniform():
    """3 x 4096 draws a step over 64 steps: n = 262 144 values per channel.  U[0,1): mean 1/2 with variance 1/12, so the sample mean's standard error is
    sqrt(1 / (12 n)); (u - 1/2)^2 has mean 1/12 and variance E(u - 1/2)^4 - 1/144 = 1/80 - 1/144 = 1/180, so the standard error of the mean square about 1/2 is
    sqrt(1 / (180 n)).  Both within 5 standard errors (the 24-bit grid moves either moment by ~2^-24)."""
    u = np.concatenate([rb.background(4096, SEED, step) for step in range(64)]).astype(np.float64)
    n = u.shape[0]
    assert n == 64 * 4096
    se_mean, se_var = (1.0 / (12.0 * n)) ** 0.5, (1.0 / (180.0 * n)) ** 0.5
    for c in range(3):
        mean, var = float(u[:, c].mean()), float(((u[:, c] - 0.5) ** 2).mean())
        print(f"\nchannel {c}: mean {mean:.6f} (|d| {abs(mean - 0.5):.2e} <= {5 * se_mean:.2e}), variance {var:.6f} (|d| {abs(var - 1 / 12):.2e} <= {5 * se_var:.2e})")
        assert abs(mean - 0.5) <= 5 * se_mean
        assert abs(var - 1.0 / 12.0) <= 5 * se_var
    # the channels of one ray are separate words of the sequence
    assert abs(float(np.corrcoef(u[:, 0], u[:, 1])[0, 1])) <= 5 / n ** 0.5


def test_entry_points_are_declared_listed_and_exported():
    from nerf_signature_amd import _native, build
    build.build()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nerfsig.h")).read(), flags=re.S)
    for name in SYMBOLS:
        args = re.search(r"^int\s+%s\s*\((.*?)\);" % name, header, flags=re.M | re.S).group(1)
        assert len(args.split(",")) == len(_native.SIGNATURES[name]), name
        _native.fn(name)
    # one more argument than the 3-channel twin: bg_out
    assert len(_native.SIGNATURES["rg_sample_rays_rgba"]) == len(_native.SIGNATURES["rg_sample_rays"]) + 1
    assert len(_native.SIGNATURES["rg_sample_rays_weighted_rgba"]) == len(_native.SIGNATURES["rg_sample_rays_weighted"]) + 1
    assert _native.fn("nsig_abi_version")() == 1


def test_argument_checks_need_no_gpu():
    from nerf_signature_amd import _native as nv, build
    build.build()
    d, odd = nv._vp(256), nv._vp(264)
    for args in ((None, 16, None, 5, d, d, None), (d, 16, None, 5, None, d, None), (d, 16, None, 5, d, None, None)):
        with pytest.raises(ValueError, match="null pointer"):
            nv.call("rg_blend_random_background", *args)
    with pytest.raises(ValueError, match="16-byte aligned"):
        nv.call("rg_blend_random_background", odd, 16, None, 5, d, d, None)
    nv.call("rg_blend_random_background", None, 0, None, 5, None, None, None)                  # no rays: nothing to do, nothing launched
    head = lambda images: (d, 3, images, 70.0, 70.0, 40.0, 30.0, 60, 80)
    tail = (16, None, 1, 0, 0)
    # the uniform draw: rays_o, rays_d, gt, bg_out, inds_out, pose_out
    with pytest.raises(ValueError, match="rg_sample_rays_rgba: null pointer"):
        nv.call("rg_sample_rays_rgba", *head(d), *tail, d, d, d, None, None, None, None)       # no bg_out
    with pytest.raises(ValueError, match="rg_sample_rays_rgba: null pointer"):
        nv.call("rg_sample_rays_rgba", *head(None), *tail, d, d, None, d, None, None, None)    # no store: there is nothing to blend
    with pytest.raises(ValueError, match="rg_sample_rays_rgba: null pointer"):
        nv.call("rg_sample_rays_rgba", *head(d), *tail, None, d, d, d, None, None, None)
    with pytest.raises(ValueError, match="16-byte aligned"):
        nv.call("rg_sample_rays_rgba", *head(odd), *tail, d, d, d, d, None, None, None)
    # the map draw: error_map, grid, rays_o, rays_d, gt, bg_out, inds_out, pose_out, inds_coarse_out, keys_out
    with pytest.raises(ValueError, match="rg_sample_rays_weighted_rgba: null pointer"):
        nv.call("rg_sample_rays_weighted_rgba", *head(d), *tail, d, 4, d, d, d, None, None, None, d, None, None)
    with pytest.raises(ValueError, match="rg_sample_rays_weighted_rgba: null pointer"):
        nv.call("rg_sample_rays_weighted_rgba", *head(d), *tail, d, 4, d, d, d, d, None, None, None, None, None)
    with pytest.raises(ValueError, match="rg_sample_rays_weighted_rgba: null pointer"):
        nv.call("rg_sample_rays_weighted_rgba", *head(None), *tail, d, 4, d, d, None, d, None, None, d, None, None)
    with pytest.raises(ValueError, match="16-byte aligned"):
        nv.call("rg_sample_rays_weighted_rgba", *head(odd), *tail, d, 4, d, d, d, d, None, None, d, None, None)
    with pytest.raises(ValueError, match="grid .* out of range"):
        nv.call("rg_sample_rays_weighted_rgba", *head(d), *tail, d, 129, d, d, d, d, None, None, d, None, None)
    with pytest.raises(ValueError, match="N .* out of range"):
        nv.call("rg_sample_rays_weighted_rgba", *head(d), 17, None, 1, 0, 0, d, 4, d, d, d, d, None, None, d, None, None)
    # the 3-channel entry points keep their messages
    with pytest.raises(ValueError, match="rg_sample_rays: ground truth requested without an image store"):
        nv.call("rg_sample_rays", *head(None), *tail, d, d, d, None, None, None)
    with pytest.raises(ValueError, match="rg_sample_rays_weighted: null pointer"):
        nv.call("rg_sample_rays_weighted", *head(d), *tail, None, 4, d, d, d, None, None, d, None, None)
