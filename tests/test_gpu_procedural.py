"""ps_render_u8 (csrc/procedural.hip) against its host restatement (tests/procedural_ref.py, itself proven in tests/test_procedural_cpu.py) at the smallest shapes
where each thing can go wrong: the wave tail, a row that is no multiple of anything, one and several views, every sample and channel count, no primitive, one
and sixteen, a camera inside a box and one whose rays have a zero component.  Every comparison is an equality; every device buffer is exactly sized and sits
between guard bytes that must come back untouched; two runs give the same bytes."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import procedural_ref as pr  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GUARD, FILL = 256, 0xA5
SHAPES = [(1, 1), (5, 7), (1, 64), (3, 65), (33, 130)]


class Guarded:
    """A device buffer of exactly n bytes between two runs of guard bytes."""

    def __init__(self, nbytes, data=None):
        self.raw = torch.full((nbytes + 2 * GUARD,), FILL, dtype=torch.uint8, device=DEV)
        self.bytes = self.raw[GUARD:GUARD + nbytes]
        if data is not None:
            self.bytes.copy_(torch.from_numpy(np.ascontiguousarray(data).view(np.uint8).reshape(-1)).to(DEV))

    def intact(self):
        return bool((self.raw[:GUARD] == FILL).all()) and bool((self.raw[GUARD + self.bytes.numel():] == FILL).all())


def primitives(K):
    """K rows: the checker slab first (the 'inside' camera sits in it), then seeded spheres and boxes around the origin, every third one a checker."""
    from nerf_signature_amd import procedural as ps
    rng = np.random.RandomState(16)
    rows = [ps.box((-0.6, -0.5, -0.6), (0.6, -0.2, 0.6), (0.85, 0.82, 0.75), (0.25, 0.3, 0.45), 5.0)]
    for k in range(1, 16):
        c, r, col, colb = rng.uniform(-0.5, 0.5, 3), rng.uniform(0.05, 0.2), rng.uniform(0, 1, 3), rng.uniform(0, 1, 3)
        tex = dict(color_b=colb, frequency=rng.uniform(3, 9)) if k % 3 == 0 else {}
        rows.append(ps.sphere(c, r, col, **tex) if k % 2 else ps.box(c - r, c + r * rng.uniform(0.5, 1.5, 3), col, **tex))
    return rows[:K]


def cameras(P, S):
    """An orbit view, a camera INSIDE the slab and an axis-aligned one (identity rotation: with the intrinsics below one sub-sample has d_0 == 0, one d_1 == 0)."""
    from nerf_signature_amd.synthetic import orbit_pose
    inside, axis = np.eye(4, dtype=np.float32), np.eye(4, dtype=np.float32)
    inside[:3, 3] = (0.1, -0.35, 0.05)
    axis[:3, 3] = (0.0, 0.0, -2.5)
    if P == 3:
        return np.stack([orbit_pose(1.0, 0.4, 2.2), inside, axis])
    return np.stack([axis if S == 1 else inside])


def intrinsics(H, W, S):
    """The principal point ON sub-sample (0, 0) of pixel (min(2, W-1), min(1, H-1)): that ray has x == 0 and y == 0 before the rotation."""
    return (0.9 * max(H, W, 8), 0.8 * max(H, W, 8), min(2, W - 1) + 1 / (2 * S), min(1, H - 1) + 1 / (2 * S))


def device_render(scene, poses, intr, H, W, C, S, bg):
    from nerf_signature_amd import procedural as ps
    P = len(poses)
    gp, out = Guarded(64 * P, poses), Guarded(P * H * W * C)
    img = ps.render(scene, gp.bytes.view(torch.float32).view(P, 4, 4), intr, H, W, C, S, bg, out=out.bytes)
    torch.cuda.synchronize()
    assert gp.intact() and out.intact()
    assert img.data_ptr() == out.bytes.data_ptr() and tuple(img.shape) == (P, H, W, C)
    return img.cpu().numpy()


@pytest.mark.parametrize("K", [0, 1, 16])
@pytest.mark.parametrize("H,W", SHAPES)
def test_kernel_equals_the_restatement(H, W, K):
    from nerf_signature_amd import procedural as ps, rays
    scene = ps.ProceduralScene(primitives(K), light=(0.4, 1.0, 0.5), ambient=0.25)
    bg = (0.2, 0.6, 1.0)
    for S in (1, 2, 4):
        intr = intrinsics(H, W, S)
        for P in (1, 3):
            poses = cameras(P, S)
            for C in (3, 4):
                got = device_render(scene, poses, intr, H, W, C, S, bg)
                want, win = pr.render(poses, intr, H, W, scene.prims, scene.light, scene.ambient, S, C, bg, details=True)
                assert np.array_equal(got, want), (S, P, C, int((got != want).sum()))
                assert np.array_equal(device_render(scene, poses, intr, H, W, C, S, bg), got)          # two runs: the same bytes
                if K == 0:
                    assert (win == -1).all() and (got == (np.rint(255 * np.float64(np.float32(bg))) if C == 3 else 0)).all()
            if P == 3 and K >= 1:          # the cases the cameras are there for do occur
                u, v = pr.subsample_positions(H, W, S)
                d = pr.pixel_rays(poses[2], intr, u, v)[1]
                assert (d[..., 0] == 0).any() and (d[..., 1] == 0).any()
                o = poses[1][:3, 3]
                assert (scene.prims[0, 4:7] < o).all() and (o < scene.prims[0, 7:10]).all() and (win[1] >= 0).all()
        if S == 1:          # fed with rays.get_rays' own rays the restatement gives the kernel's bytes: the kernel's rays ARE rg_get_rays'
            poses = cameras(3, 1)
            r = rays.get_rays(torch.from_numpy(poses).to(DEV), intr, H, W, -1)
            o, d = r["rays_o"][:, 0].cpu().numpy(), r["rays_d"].cpu().numpy()
            for p in range(3):
                u, v = pr.subsample_positions(H, W, 1)
                assert np.array_equal(pr.pixel_rays(poses[p], intr, u, v)[1].reshape(-1, 3).view(np.uint32), d[p].view(np.uint32))
            fed = pr.render(poses, intr, H, W, scene.prims, scene.light, scene.ambient, 1, 4, bg, rays=(o, d))
            assert np.array_equal(device_render(scene, poses, intr, H, W, 4, 1, bg), fed)


def test_plinth_preset_equals_the_restatement():
    """The preset the signing pipeline trains on, at the size of its test: 2 views of 48 x 48, RGBA, S = 2 -- and it has all four primitives and background in view."""
    from nerf_signature_amd import procedural as ps
    scene = ps.SCENES["plinth"]
    poses, intr = ps.orbit_poses(2, 2.2, (0.6, 1.5), seed=0), (58.0, 58.0, 24.0, 24.0)
    got = device_render(scene, poses, intr, 48, 48, 4, 2, None)
    want, win = pr.render(poses, intr, 48, 48, scene.prims, scene.light, scene.ambient, 2, 4, details=True)
    assert np.array_equal(got, want) and {-1, 0, 1} <= set(np.unique(win).tolist())


@pytest.mark.parametrize("channels", [3, 4])
def test_dataset_sampler_draws_the_stores_own_bytes(channels):
    """procedural.dataset(...) is a dataset.Scene: its store equals the restatement's bytes of its own poses, and its sampler hands out those bytes decoded -- RGB
    exactly code / 255; RGBA the straight colour where alpha is 255 and the drawn background where it is 0."""
    from nerf_signature_amd import dataset as ds, procedural as ps
    H, W, n = 20, 28, 512
    scene = ps.SCENES["plinth"]
    store = ps.dataset(scene, 3, H, W, focal=24.0, radius=2.2, seed=3, channels=channels, samples=2, bg=(1.0, 1.0, 1.0), device=DEV)
    assert store.mode == "procedural" and store.files == [] and store.images.dtype == torch.uint8 and tuple(store.images.shape) == (3, H, W, channels)
    assert store.intrinsics == (24.0, 24.0, W / 2, H / 2) and abs(store.radius - 2.2) < 1e-6
    poses = store.poses.cpu().numpy()
    assert np.array_equal(poses, ps.orbit_poses(3, 2.2, (0.6, 1.5), seed=3))
    want = pr.render(poses, store.intrinsics, H, W, scene.prims, scene.light, scene.ambient, 2, channels, (1.0, 1.0, 1.0))
    assert np.array_equal(store.images.cpu().numpy(), want)
    sampler = store.sampler(n, seed=11)
    buf = lambda: torch.empty(n, 3, dtype=torch.float32, device=DEV)
    o, d, gt, bg = buf(), buf(), buf(), (buf() if channels == 4 else None)
    inds, pose = torch.empty(n, dtype=torch.int64, device=DEV), torch.empty(1, dtype=torch.int32, device=DEV)
    for step in (0, 1, 2):
        sampler.sample_into(torch.full((1,), step, dtype=torch.int32, device=DEV), o, d, gt, inds_out=inds, pose_out=pose, bg=bg)
        p = int(pose.item())
        assert p == step % 3
        px = ds.decode_u8(store.images[p].view(H * W, channels)[inds])
        if channels == 3:
            assert torch.equal(gt, px)
        else:
            a = store.images[p].view(H * W, 4)[inds][:, 3]
            assert (a == 255).sum() > 20 and (a == 0).sum() > 20
            assert torch.equal(gt[a == 255], px[a == 255][:, :3]) and torch.equal(gt[a == 0], bg[a == 0])
    view = store.view(1)
    assert torch.equal(view["images"], ds.decode_u8(store.images[1:2])) and view["H"] == H
