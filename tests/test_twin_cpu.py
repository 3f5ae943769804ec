"""The clean-twin forward and the orbit sampler without a GPU: the library exports them and refuses bad calls before it touches a device, and the float64
mirror of the orbit draw (tests/orbit_ref.py) is what its docstring says -- an unused sequence of the counter hash, uniform angles, blocks.rand_poses' frame."""
import math

import numpy as np
import pytest
import torch

import orbit_ref as orb


@pytest.fixture(scope="module")
def native():
    from nerf_signature_amd import build, _native
    build.build()
    return _native


def test_library_exports_the_two_entry_points(native):
    assert {"field_fwd_twin", "rg_sample_rays_orbit"} <= set(native.verify_exports())
    assert native.fn("nsig_abi_version")() == 1


def test_twin_forward_refuses_missing_outputs_and_unsupported_routes_before_any_launch(native):
    d = native._vp(256)
    tables = (native._vp * 16)(*([256] * 16))
    ok = dict(xyzs=d, dirs=d, M=64, bound=1.0, tables=tables, S=d, packed=d, sigmas=d, rgbs=d, geo=None, masks=None, planes=d, layout=0, sigmas_clean=d, rgbs_clean=d, stream=None)

    def call(**change):
        a = dict(ok, **change)
        native.call("field_fwd_twin", *(a[k] for k in ok))

    for name in ("sigmas", "rgbs", "sigmas_clean", "rgbs_clean", "dirs"):
        with pytest.raises(ValueError, match="null pointer"):
            call(**{name: None})
    with pytest.raises(ValueError, match="fused no-planes route"):
        call(planes=None)
    with pytest.raises(ValueError, match="S is NULL"):
        call(S=None)
    with pytest.raises(ValueError, match="planes_layout"):
        call(layout=7)
    before = native.fn("mlp_get_precision")()
    try:
        native.set_mlp_precision("bf16x3")
        with pytest.raises(ValueError, match="mixed"):       # a mixed plane set carries the fp16 MLP's operands
            call(layout=1)
    finally:
        native.call("mlp_set_precision", before)
    call(M=0)          # nothing to do: no launch, no error


def test_orbit_sampler_refuses_bad_arguments_before_any_launch(native):
    d = native._vp(256)
    ok = dict(fx=100.0, fy=100.0, cx=32.0, cy=32.0, H=64, W=64, N=16, step=None, stride=1, offset=0, seed=5, radius=2.0, t0=1.0, t1=2.0, p0=0.0, p1=6.0,
              rays_o=d, rays_d=d, inds=None, pose=d, stream=None)

    def call(**change):
        a = dict(ok, **change)
        native.call("rg_sample_rays_orbit", *(a[k] for k in ok))

    for name in ("rays_o", "rays_d", "pose"):
        with pytest.raises(ValueError, match="null pointer"):
            call(**{name: None})
    with pytest.raises(ValueError, match="at least 1"):
        call(N=0)
    with pytest.raises(ValueError, match="focal length"):
        call(fx=0.0)
    with pytest.raises(ValueError, match="radius must be positive"):
        call(radius=0.0)
    with pytest.raises(ValueError, match="ordered"):
        call(t0=2.0, t1=1.0)
    with pytest.raises(ValueError, match="strictly inside"):
        call(t0=0.0)
    with pytest.raises(ValueError, match="strictly inside"):
        call(t1=3.2)


def test_python_layers_refuse_what_the_twin_does_not_cover():
    from nerf_signature_amd import fieldops as fo, rays
    x = torch.zeros(4, 3)
    with pytest.raises(ValueError, match="needs a codebook pre-sum"):
        fo.field_forward(x, x, 1.0, [], None, None, twin=True)
    with pytest.raises(NotImplementedError, match="fixed="):
        fo.field_forward(x, x, 1.0, [], x, None, twin=True, fixed=object())
    with pytest.raises(ValueError, match="fused route"):
        fo.field_forward(x, x, 1.0, [], x, None, twin=True, planes=False)
    s = rays.OrbitRaySampler((10.0, 10.0, 4.0, 4.0), 8, 8, 4, 2.0, device="cpu")
    buf = torch.zeros(4, 3)
    for kw in ({"gt": buf}, {"bg": buf}, {"keys_out": buf}):
        with pytest.raises(ValueError, match="no image store"):
            s.sample_into(None, buf, buf, **kw)


def test_sequence_five_is_distinct_from_the_sequences_in_use():
    for seed in (0, 1234, (7 << 32) + 5):
        for step in (0, 7, 2 ** 31 - 1):
            bases = [orb.draw_base(seed, step, s) for s in range(6)]
            assert len(set(bases)) == 6, (seed, step, bases)
            heads = [tuple(orb.draw_word(b, i) for i in range(4)) for b in bases]
            assert all(heads[5] != h for h in heads[:5])
            assert not set(heads[5]) & {w for h in heads[:5] for w in h}


def test_angle_moments_over_4096_steps_are_the_uniforms():
    n, t_range, p_range = 4096, (math.pi / 3, 2 * math.pi / 3), (0.0, 2 * math.pi)
    draws = np.array([orb.angles(99, orb.camera_index(step, 1, 0), t_range, p_range) for step in range(n)], dtype=np.float64)
    for col, (lo, hi) in enumerate((t_range, p_range)):
        x, w = draws[:, col], hi - lo
        assert lo <= x.min() and x.max() < hi + 1e-6
        mean_se = w / math.sqrt(12 * n)
        var, var_se = w * w / 12, math.sqrt((w ** 4 / 80 - (w * w / 12) ** 2) / n)      # fourth central moment of U: w^4 / 80
        assert abs(x.mean() - (lo + hi) / 2) <= 5 * mean_se, (col, x.mean())
        assert abs(x.var() - var) <= 5 * var_se, (col, x.var())
    assert abs(np.corrcoef(draws[:, 0], draws[:, 1])[0, 1]) <= 5 / math.sqrt(n)          # the two angles come from different words
    # another offset is another camera sequence
    other = np.array([orb.angles(99, orb.camera_index(step, 1, 1), t_range, p_range) for step in range(64)])
    shifted = draws[1:65]
    assert np.array_equal(other, shifted)          # (stride 1: offset 1 at step s is camera s + 1)
    assert not np.array_equal(other, draws[:64])


def test_mirror_pose_is_rand_poses_closed_form_orthonormal_and_looks_at_the_origin():
    from nerf_signature_amd import blocks
    rng = np.random.RandomState(3)
    for radius in (1.0, 2.5, 4.0):
        for _ in range(8):
            theta = float(np.float32(rng.uniform(0.2, math.pi - 0.2)))
            phi = float(np.float32(rng.uniform(0.0, 2 * math.pi)))
            mine = orb.pose_from_angles(theta, phi, radius)
            theirs = blocks.rand_poses(1, "cpu", radius=radius, theta_range=(theta, theta), phi_range=(phi, phi))[0].double().numpy()      # rand * 0 + angle: the angle
            assert np.abs(mine - theirs).max() <= orb.pose_bound(radius), (theta, phi, radius)
            R, c = mine[:3, :3], mine[:3, 3]
            assert np.abs(R.T @ R - np.eye(3)).max() < 1e-14 and np.abs(R @ R.T - np.eye(3)).max() < 1e-14      # (the reference's frame: x right, y down, z forward)
            assert abs(np.linalg.norm(c) - radius) < 1e-14 * radius
            assert np.abs(c + radius * R[:, 2]).max() < 1e-14 * radius          # centre + radius * forward = origin: the camera axis passes through it
            assert np.array_equal(mine[3], [0.0, 0.0, 0.0, 1.0])


def test_pose_bound_is_the_documented_ulp_budget():
    assert orb.TRIG_ULP == 1.0
    assert orb.pose_bound(1.0) == (2 * 2.0 ** -23 + 2 * 2.0 ** -24) * (1 + 2.0 ** -20)
    assert orb.pose_bound(4.0) == 4 * orb.pose_bound(1.0) and orb.pose_bound(0.5) == orb.pose_bound(1.0)
