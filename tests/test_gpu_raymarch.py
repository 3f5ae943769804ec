"""GPU parity of the ray-marching kernels against the CPU oracle, through the C ABI (ctypes -> libnerfsig.so)."""
import numpy as np
import pytest
import torch

import closed_form as cf
from oracle import field_ref as fr
from oracle import raymarch_ref as orm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rmod():
    from nerf_signature_amd import raymarching
    return raymarching


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _scene(n, bound, seed=0, radius=None):
    grid, bitfield, C = cf.ball_scene(bound=bound)
    pose, intr, inds = cf.orbit_rays(n, seed=seed, radius=radius or (3.2248 if bound == 1.0 else 1.3))
    o, d = fr.get_rays(torch.from_numpy(pose)[None], intr, 400, 400, torch.from_numpy(inds)[None])
    return grid, bitfield, C, o[0].contiguous().numpy(), d[0].contiguous().numpy()


def test_utils_bit_exact(rmod):
    rng = np.random.RandomState(0)
    c = rng.randint(0, 128, size=(10007, 3)).astype(np.int32)
    idx = rmod.morton3D(_cuda(c))
    np.testing.assert_array_equal(idx.cpu().numpy(), orm.morton3D(c))
    np.testing.assert_array_equal(rmod.morton3D_invert(idx).cpu().numpy(), c)
    grid = rng.randn(2, 128 ** 3 // 16).astype(np.float32)
    np.testing.assert_array_equal(rmod.packbits(_cuda(grid), 0.1).cpu().numpy(), orm.packbits(grid, 0.1))
    odd = rng.randn(1, 8 * 37).astype(np.float32)  # byte count not a multiple of 4
    np.testing.assert_array_equal(rmod.packbits(_cuda(odd), 0.0).cpu().numpy(), orm.packbits(odd, 0.0))


@pytest.mark.parametrize("bound", [1.0, 2.0])
def test_near_far_bit_exact(rmod, bound):
    _, _, _, o, d = _scene(4096, bound)
    d[5] = (0, 1, 0)     # axis-parallel ray (infinite reciprocal)
    o[6] = (9, 9, 9)     # misses the box
    aabb = np.array([-bound] * 3 + [bound] * 3, np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        n0, f0 = orm.near_far_from_aabb(o, d, aabb, 0.2)
    n1, f1 = rmod.near_far_from_aabb(_cuda(o), _cuda(d), _cuda(aabb), 0.2)
    np.testing.assert_array_equal(n1.cpu().numpy(), n0)
    np.testing.assert_array_equal(f1.cpu().numpy(), f0)


def test_sph_from_ray(rmod):
    _, _, _, o, d = _scene(1024, 1.0)
    want = orm.sph_from_ray(o * 0.1, d, 4.0)
    got = rmod.sph_from_ray(_cuda(o * 0.1), _cuda(d), 4.0)
    np.testing.assert_allclose(got.cpu().numpy(), want, rtol=0, atol=2e-6)


@pytest.mark.parametrize("bound,dt_gamma,n", [(1.0, 0.0, 4096), (2.0, 0.0, 2048), (2.0, 1 / 128, 2048), (1.0, 0.0, 77), (8.0, 1 / 128, 1024), (16.0, 1 / 256, 1024),
                                              (1.5, 0.0, 1024)])
def test_march_train_counts_and_points_bit_exact(rmod, bound, dt_gamma, n):
    _, bitfield, C, o, d = _scene(n, bound)
    aabb = np.array([-bound] * 3 + [bound] * 3, np.float32)
    nears, fars = orm.near_far_from_aabb(o, d, aabb, 0.2)
    ctr0 = np.zeros(2, np.int32)
    x0, d0, dl0, rays0 = orm.march_rays_train(o, d, bound, bitfield, C, 128, nears, fars, ctr0, -1, False, 128, True, dt_gamma, 1024)
    ctr1 = torch.zeros(2, dtype=torch.int32, device="cuda")
    x1, d1, dl1, rays1 = rmod.march_rays_train(_cuda(o), _cuda(d), bound, _cuda(bitfield), C, 128, _cuda(nears), _cuda(fars), ctr1,
                                               -1, False, 128, True, dt_gamma, 1024)
    np.testing.assert_array_equal(ctr1.cpu().numpy(), ctr0)           # total point count, ray count
    np.testing.assert_array_equal(rays1.cpu().numpy(), rays0)         # (id, offset, count) per ray: bit-exact
    assert ctr0[0] > 0
    np.testing.assert_array_equal(x1.cpu().numpy(), x0)
    np.testing.assert_array_equal(d1.cpu().numpy(), d0)
    np.testing.assert_array_equal(dl1.cpu().numpy(), dl0)


def test_march_train_perturbed_and_bounded(rmod):
    """Fixed noise vector through the C ABI directly (the wrapper draws torch.rand) and the mean_count-bounded mode."""
    from nerf_signature_amd import _native as nv
    _, bitfield, C, o, d = _scene(512, 1.0, seed=3)
    aabb = np.array([-1, -1, -1, 1, 1, 1], np.float32)
    nears, fars = orm.near_far_from_aabb(o, d, aabb, 0.2)
    noises = np.random.RandomState(1).rand(512).astype(np.float32)
    ctr0 = np.zeros(2, np.int32)
    x0, d0, dl0, rays0 = orm.march_rays_train(o, d, 1.0, bitfield, C, 128, nears, fars, ctr0, 3000, True, 128, False, 0.0, 1024, noises=noises)
    M = x0.shape[0]
    assert M == 3072 and ctr0[0] > M      # some rays overflow the bound and are dropped
    ctr1 = torch.zeros(2, dtype=torch.int32, device="cuda")
    to = lambda a: _cuda(a)
    _, _, rays1, write = rmod.march_rays_train_device(to(o), to(d), 1.0, to(bitfield), C, 128, to(nears), to(fars), ctr1, to(noises), 0.0, 1024)
    x1, d1, dl1 = write(M)
    np.testing.assert_array_equal(rays1.cpu().numpy(), rays0)
    np.testing.assert_array_equal(x1.cpu().numpy(), x0)
    np.testing.assert_array_equal(dl1.cpu().numpy(), dl0)


def test_composite_train_fwd_bwd(rmod):
    _, bitfield, C, o, d = _scene(2048, 1.0)
    aabb = np.array([-1, -1, -1, 1, 1, 1], np.float32)
    nears, fars = orm.near_far_from_aabb(o, d, aabb, 0.2)
    x0, d0, dl0, rays0 = orm.march_rays_train(o, d, 1.0, bitfield, C, 128, nears, fars, None, -1, False, 128, True, 0.0, 1024)
    rng = np.random.RandomState(4)
    M = x0.shape[0]
    for scale in (2.0, 300.0):   # thin medium, and opaque enough to hit the T < 1e-4 early exit
        sig = (rng.rand(M) * scale).astype(np.float32)
        rgb = rng.rand(M, 3).astype(np.float32)
        ws0, dep0, img0 = orm.composite_rays_train_forward(sig, rgb, dl0, rays0, 1e-4)
        s1, c1 = _cuda(sig).requires_grad_(True), _cuda(rgb).requires_grad_(True)
        ws1, dep1, img1 = rmod.composite_rays_train(s1, c1, _cuda(dl0), _cuda(rays0), 1e-4)
        np.testing.assert_allclose(ws1.detach().cpu().numpy(), ws0, rtol=0, atol=2e-6)
        np.testing.assert_allclose(dep1.detach().cpu().numpy(), dep0, rtol=0, atol=1e-5)
        np.testing.assert_allclose(img1.detach().cpu().numpy(), img0, rtol=0, atol=2e-6)
        g_ws, g_img = rng.randn(2048).astype(np.float32), rng.randn(2048, 3).astype(np.float32)
        gs0, gc0 = orm.composite_rays_train_backward(g_ws, g_img, sig, rgb, dl0, rays0, ws0, img0, 1e-4)
        torch.autograd.backward([ws1, img1], [_cuda(g_ws), _cuda(g_img)])
        np.testing.assert_allclose(c1.grad.cpu().numpy(), gc0, rtol=0, atol=2e-6)
        np.testing.assert_allclose(s1.grad.cpu().numpy(), gs0, rtol=1e-4, atol=2e-6 * max(1.0, 3.0 / scale))


def test_eval_march_composite_compact(rmod):
    _, bitfield, C, o, d = _scene(1000, 1.0)
    aabb = np.array([-1, -1, -1, 1, 1, 1], np.float32)
    nears, fars = orm.near_far_from_aabb(o, d, aabb, 0.2)
    N = 1000
    sig_of = lambda p: (40.0 * (0.5 + p[:, 0])).astype(np.float32)
    rgb_of = lambda p: np.stack([0.5 + 0.4 * p[:, 1], 0.3 + 0 * p[:, 1], 0.5 - 0.4 * p[:, 2]], -1).astype(np.float32)
    ws0, dep0, img0 = np.zeros(N, np.float32), np.zeros(N, np.float32), np.zeros((N, 3), np.float32)
    alive0, t0 = np.arange(N, dtype=np.int32), nears.copy()
    ws1, dep1, img1 = (torch.zeros(N, device="cuda"), torch.zeros(N, device="cuda"), torch.zeros(N, 3, device="cuda"))
    alive1, t1 = torch.arange(N, dtype=torch.int32, device="cuda"), _cuda(nears).clone()
    bf, oc, dc, nc, fc = _cuda(bitfield), _cuda(o), _cuda(d), _cuda(nears), _cuda(fars)
    step = 0
    while step < 1024 and alive0.shape[0] > 0:
        n_alive = alive0.shape[0]
        n_step = max(min(N // n_alive, 8), 1)
        p0, dd0, dl0 = orm.march_rays(n_alive, n_step, alive0, t0, o, d, 1.0, bitfield, C, 128, nears, fars, 128, False, 0.0, 1024)
        p1, dd1, dl1 = rmod.march_rays(n_alive, n_step, alive1, t1, oc, dc, 1.0, bf, C, 128, nc, fc, 128, False, 0.0, 1024)
        np.testing.assert_array_equal(p1.cpu().numpy(), p0)
        np.testing.assert_array_equal(dl1.cpu().numpy(), dl0)
        orm.composite_rays(n_alive, n_step, alive0, t0, sig_of(p0), rgb_of(p0), dl0, ws0, dep0, img0, 1e-2)
        rmod.composite_rays(n_alive, n_step, alive1, t1, _cuda(sig_of(p0)), _cuda(rgb_of(p0)), dl1, ws1, dep1, img1, 1e-2)
        np.testing.assert_array_equal(alive1.cpu().numpy(), alive0)      # which rays terminated: bit-exact
        alive0 = np.ascontiguousarray(alive0[alive0 >= 0])
        out, n_out = rmod.compact_alive(alive1)
        assert int(n_out.item()) == alive0.shape[0]
        alive1 = out[:alive0.shape[0]].contiguous()
        np.testing.assert_array_equal(alive1.cpu().numpy(), alive0)
        step += n_step
    np.testing.assert_allclose(ws1.cpu().numpy(), ws0, rtol=0, atol=5e-6)
    np.testing.assert_allclose(img1.cpu().numpy(), img0, rtol=0, atol=5e-6)
    np.testing.assert_allclose(dep1.cpu().numpy(), dep0, rtol=0, atol=2e-5)


def test_argument_checks_raise(rmod):
    from nerf_signature_amd import _native as nv
    with pytest.raises(ValueError):
        rmod.march_rays_train(torch.zeros(4, 3, device="cuda"), torch.ones(4, 3, device="cuda"), 1.0, torch.zeros(10, dtype=torch.uint8, device="cuda"),
                              1, 128, torch.zeros(4, device="cuda"), torch.ones(4, device="cuda"), None, -1, False, 128, True, 0.0, 1024)
    with pytest.raises(ValueError):
        nv.call("rm_morton3D", None, 4, None, None)


def test_get_rays_on_device_matches_reference_golden():
    """rg_get_rays vs the reference's own get_rays output (golden G7) and vs the oracle for whole images / batches."""
    import os
    from nerf_signature_amd import rays
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g7_get_rays.npz"))
    poses = torch.from_numpy(g["pose"])[None].cuda()
    torch.manual_seed(0)
    out = rays.get_rays(poses, g["intrinsics"], 400, 400, N=-1)
    assert out["rays_o"].shape == (1, 160000, 3) and torch.equal(out["inds"][0].cpu(), torch.arange(160000))
    np.testing.assert_array_equal(out["rays_o"][0, g["inds"]].cpu().numpy(), g["rays_o"])
    np.testing.assert_allclose(out["rays_d"][0, g["inds"]].cpu().numpy(), g["rays_d"], rtol=0, atol=5e-7)   # 3-term dot product: order/FMA differ by an ulp or two
    sub = rays.get_rays(poses, g["intrinsics"], 400, 400, N=4096)
    assert sub["rays_d"].shape == (1, 4096, 3) and sub["inds"].shape == (1, 4096) and int(sub["inds"].max()) < 160000
    np.testing.assert_array_equal(sub["rays_d"][0].cpu().numpy(), out["rays_d"][0, sub["inds"][0]].cpu().numpy())
    two = torch.cat([poses, poses.roll(1, 2)], 0)
    o0, d0 = fr.get_rays(two.cpu(), g["intrinsics"], 30, 50)
    o1 = rays.get_rays(two, g["intrinsics"], 30, 50)
    np.testing.assert_allclose(o1["rays_d"].cpu().numpy(), d0.numpy(), rtol=0, atol=5e-7)
    np.testing.assert_array_equal(o1["rays_o"].cpu().numpy(), o0.numpy())
    patch = rays.get_rays(poses, g["intrinsics"], 400, 400, N=4096, patch_size=16)
    assert patch["rays_d"].shape == (1, 4096, 3)
    em = torch.rand(1, 128 * 128).cuda()
    coarse = rays.get_rays(poses, g["intrinsics"], 400, 400, N=1024, error_map=em)
    assert coarse["inds_coarse"].shape == (1, 1024) and coarse["rays_d"].shape == (1, 1024, 3)


@pytest.mark.gpu
@pytest.mark.parametrize("capacity_frac", [None, 0.6])
def test_composite_with_fused_tail_matches_separate_launches(capacity_frac):
    """rm_composite_train_finish_fwd/_bwd == composite_rays_train followed by the render tail, values and gradients -- including the
    rows the fused backward zero-fills itself: samples after early termination, rays dropped by a too-small point buffer, padding."""
    import torch
    from nerf_signature_amd import raymarching as rm
    from nerf_signature_amd.renderer import _CompositeFinish, _Finish
    dev = torch.device("cuda")
    _, bitfield, _, o, d = _scene(700, 1.0, seed=2, radius=1.6)
    bits, o, d = _cuda(bitfield), _cuda(o), _cuda(d)
    aabb = torch.tensor([-1., -1, -1, 1, 1, 1], device=dev)
    nears, fars = rm.near_far_from_aabb(o, d, aabb, 0.2)
    counter = torch.zeros(2, dtype=torch.int32, device=dev)
    if capacity_frac is None:
        xyzs, dirs, deltas, rays = rm.march_rays_train(o, d, 1.0, bits, 1, 128, nears, fars, counter, -1, False, 128, True, 0.0, 1024)
    else:
        full = rm.march_rays_train(o, d, 1.0, bits, 1, 128, nears, fars, None, -1, False, 128, True, 0.0, 1024)[0].shape[0]
        xyzs, dirs, deltas, rays = rm.march_rays_train_capacity(o, d, 1.0, bits, 1, 128, nears, fars, counter, rm.padded_point_count(int(full * capacity_frac)))
        assert int(counter[0]) > xyzs.shape[0]                     # some rays did not fit
    M = xyzs.shape[0]
    torch.manual_seed(0)
    sig = (torch.rand(M, device=dev) * 60).requires_grad_(True)     # dense enough for early termination (T < 1e-4) inside rays
    rgb = torch.rand(M, 3, device=dev).requires_grad_(True)
    bg = torch.rand(o.shape[0], 3, device=dev)
    gi, gw = torch.randn(o.shape[0], 3, device=dev), torch.randn(o.shape[0], device=dev)
    ws0, dp0, im0 = rm.composite_rays_train(sig, rgb, deltas, rays, 1e-4)
    im0f, dp0f = _Finish.apply(im0, dp0, ws0, nears, fars, bg)
    g0 = torch.autograd.grad([im0f, ws0], [sig, rgb], [gi, gw])
    junk = torch.full((4 * M + 1024,), float("nan"), device=dev)   # so that recycled allocations do not happen to hold zeros
    del junk
    ws1, dp1, im1 = _CompositeFinish.apply(sig, rgb, deltas, rays, nears, fars, bg, 1e-4)
    g1 = torch.autograd.grad([im1, ws1], [sig, rgb], [gi, gw])
    assert torch.equal(ws0, ws1) and torch.equal(im0f, im1)
    assert torch.equal(torch.nan_to_num(dp0f), torch.nan_to_num(dp1))
    for a, b in zip(g0, g1):
        assert torch.isfinite(b).all()
        np.testing.assert_allclose(b.cpu().numpy(), a.cpu().numpy(), rtol=1e-6, atol=1e-7)
    terminated = (g0[1].abs().sum(dim=1) == 0) & (deltas[:, 0] > 0)
    assert bool(terminated.any())                                   # the early-termination rows were exercised


def test_device_ray_sampler_matches_get_rays():
    """rg_sample_rays: pose (step * stride + offset) mod P from a device counter, uniformly drawn pixels, rays identical to rg_get_rays for
    the same (pose, indices), ground truth = the stored image's pixels; a new step draws new pixels, the same step the same ones."""
    from nerf_signature_amd import rays
    P, H, W, N = 5, 60, 80, 4096
    intr = (70.0, 72.0, W / 2, H / 2)
    poses = torch.stack([torch.from_numpy(cf.orbit_rays(1, seed=0, radius=2.0 + 0.1 * k)[0]) for k in range(P)]).cuda()
    images = torch.rand(P, H * W, 3, device="cuda")
    s = rays.DeviceRaySampler(poses, images, intr, H, W, N, stride=2, offset=1, seed=99)
    ctr = torch.zeros(1, dtype=torch.int32, device="cuda")
    o, d, gt = (torch.empty(1, N, 3, device="cuda") for _ in range(3))
    inds, pose = torch.empty(N, dtype=torch.int64, device="cuda"), torch.empty(1, dtype=torch.int32, device="cuda")
    seen = []
    for step in (0, 1, 2, 7, 7):
        ctr.fill_(step)
        s.sample_into(ctr, o, d, gt, inds, pose)
        k = (step * 2 + 1) % P
        assert int(pose) == k and int(inds.min()) >= 0 and int(inds.max()) < H * W
        want = rays.get_rays(poses[k:k + 1], intr, H, W, N=-1)
        assert torch.equal(o[0], want["rays_o"][0, inds]) and torch.equal(d[0], want["rays_d"][0, inds])
        assert torch.equal(gt[0], images[k][inds])
        seen.append(inds.clone())
    assert torch.equal(seen[3], seen[4]) and not torch.equal(seen[0], seen[1])
    # uniform: every quarter of the image receives its share (4096 draws: +-5 sigma)
    q = torch.bincount((seen[0] * 4 // (H * W)), minlength=4).float()
    assert float((q - N / 4).abs().max()) < 5 * (N * 0.25 * 0.75) ** 0.5
    with pytest.raises(ValueError):
        s.sample_into(ctr, o[:, :10], d, gt)


@pytest.mark.parametrize("bound,dt_gamma,n,perturb", [(1.0, 0.0, 4608, False), (1.0, 0.0, 1, False), (1.0, 0.0, 63, True), (2.0, 0.0, 8704, False),
                                                      (2.0, 1.0 / 128, 4096, True), (1.0, 0.0, 12288, False)])
def test_two_enqueue_march_equals_the_four_enqueue_march(rmod, bound, dt_gamma, n, perturb):
    """The captured step's march -- rm_march_train_count_nf (the walk computes near / far itself) + rm_march_train_scan_write (every
    workgroup scans the counts for itself, offsets in LDS) -- against near_far + count + scan + write: limits, ray table, totals, every
    row and the zero padding bit for bit; a capacity smaller than the total drops the same rays (raymarching.cu:416); and against the C
    oracle's counts."""
    from nerf_signature_amd import _native as nv
    _, bitfield, C, o, d = _scene(n, bound, seed=3)
    oc, dc, bits = _cuda(o), _cuda(d), _cuda(bitfield)
    aabb = torch.tensor([-bound] * 3 + [bound] * 3, device="cuda")
    noises = torch.rand(n, device="cuda") if perturb else None
    nears, fars = rmod.near_far_from_aabb(oc, dc, aabb, 0.2)
    ctr = torch.zeros(2, dtype=torch.int32, device="cuda")
    counts, t_rec, rays, write = rmod.march_rays_train_device(oc, dc, bound, bits, C, 128, nears, fars, ctr, noises, dt_gamma, 1024)
    total = int(ctr[0])
    rays0, total0 = orm.march_counts(o, d, bound, bitfield, C, 128, nears.cpu().numpy(), fars.cpu().numpy(), dt_gamma, 1024,
                                     noises=None if noises is None else noises.cpu().numpy())
    assert total == total0 and np.array_equal(rays[:, 2].cpu().numpy(), rays0[:, 2])
    assert n <= rmod.scan_write_max_rays() == 12288
    for M in (rmod.padded_point_count(total), max(128, (total // 2) // 128 * 128), 0):
        x4, d4, dl4 = write(M) if M else (None, None, None)
        nears2, fars2 = torch.full((n,), -1.0, device="cuda"), torch.full((n,), -1.0, device="cuda")
        ctr2 = torch.full((2,), -5, dtype=torch.int32, device="cuda")
        out = None
        if M:
            out = (torch.full((M, 3), 7.0, device="cuda"), torch.full((M, 3), 7.0, device="cuda"), torch.full((M, 2), 7.0, device="cuda"),
                   torch.full((n, 3), -9, dtype=torch.int32, device="cuda"))
        _, _, rays2, write2 = rmod.march_rays_train_device(oc, dc, bound, bits, C, 128, nears2, fars2, ctr2, noises, dt_gamma, 1024, capacity=M, out=out,
                                                           limits=(aabb, 0.2))
        if M:
            x2, d2, dl2 = write2(M)
            assert torch.equal(x2, x4) and torch.equal(d2, d4) and torch.equal(dl2, dl4)
        else:      # no rows: the launch still leaves the ray table and the totals
            empty = torch.empty(0, 3, device="cuda")
            nv.call("rm_march_train_scan_write", nv.ptr(oc), nv.ptr(dc), float(bound), float(dt_gamma), 1024, n, C, 128, 0, nv.ptr(nears2), nv.ptr(noises),
                    nv.ptr(t_rec), nv.ptr(counts), nv.ptr(rays2), nv.ptr(ctr2), None, None, None, nv.stream())
            del empty
        assert torch.equal(nears2, nears) and torch.equal(fars2, fars)
        assert torch.equal(rays2, rays) and torch.equal(ctr2, ctr)
    with pytest.raises(ValueError, match="outside"):
        nv.call("rm_march_train_scan_write", nv.ptr(oc), nv.ptr(dc), float(bound), float(dt_gamma), 1024, 12289, C, 128, 128, nv.ptr(nears), None,
                nv.ptr(t_rec), nv.ptr(counts), nv.ptr(rays), nv.ptr(ctr), nv.ptr(oc), nv.ptr(oc), nv.ptr(oc), nv.stream())


@pytest.mark.parametrize("n", [1, 4095, 4096, 4097, 20000, 262144])
def test_wide_scan_equals_the_single_workgroup_scan(n):
    """rm_march_train_scan_wide (two launches of 4096-ray workgroups: what a staged full-image render's 262 144-ray march uses) == rm_march_train_scan
    (one workgroup): the (id, offset, count) table and the totals, bit for bit, for ray counts around the workgroup size and at the largest size."""
    from nerf_signature_amd import _native as nv
    rng = np.random.RandomState(n % 1000)
    counts = torch.from_numpy(rng.randint(0, 1025, n).astype(np.int32)).cuda()
    counts[rng.randint(0, n, max(1, n // 7))] = 0                      # rays without samples share their successor's offset
    out = []
    for wide in (False, True):
        rays = torch.full((n, 3), -3, dtype=torch.int32, device="cuda")
        ctr = torch.full((2,), -3, dtype=torch.int32, device="cuda")
        if wide:
            sums = torch.full((int(nv.fn("rm_march_train_scan_blocks")(n)),), -77, dtype=torch.int32, device="cuda")
            nv.call("rm_march_train_scan_wide", nv.ptr(counts), n, nv.ptr(rays), nv.ptr(ctr), nv.ptr(sums), nv.stream())
        else:
            nv.call("rm_march_train_scan", nv.ptr(counts), n, nv.ptr(rays), nv.ptr(ctr), nv.stream())
        out.append((rays, ctr))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    c = counts.cpu().numpy().astype(np.int64)
    r = out[1][0].cpu().numpy().astype(np.int64)
    assert np.array_equal(r[:, 0], np.arange(n)) and np.array_equal(r[:, 2], c) and np.array_equal(r[:, 1], np.concatenate([[0], np.cumsum(c)[:-1]]))
    assert out[1][1].tolist() == [int(c.sum()), n]


# ---- compositing: every entry point against the float64 restatement (tests/composite_ref.py), through the C ABI with hand-built ray tables ----
# The bound is composite_ref.composite_tolerance (derived there; tests/test_composite_cpu.py shows it is reachable and that it kills six mutants).
# Every output buffer starts as NaN, so a row nobody wrote is seen.  Each test prints the largest |kernel - float64| / bound it met.

import composite_ref as cr

_CREF = {}


def _cref(case):
    """float64 forward of a case and the plain backward with its bound, computed once and shared"""
    if case.name not in _CREF:
        a = (case.sigmas, case.rgbs, case.deltas, case.rays, case.T_thresh)
        fwd = cr.train_forward(*a)
        gs, gc = cr.train_backward(case.grad_weights_sum, case.grad_image, *a, fwd=fwd)
        _CREF[case.name] = cr.Bag(a=a, fwd=fwd, gs=gs, gc=gc, tol=cr.composite_tolerance(*a, fwd, case.grad_weights_sum, case.grad_image))
    return _CREF[case.name]


def _nan(*shape):
    return torch.full(shape, float("nan"), device="cuda")


def _dev(case):
    return cr.Bag({k: _cuda(case[k]) for k in ("sigmas", "rgbs", "deltas", "rays", "nears", "fars", "bg", "bg_rays", "gt", "grad_weights_sum", "grad_image")})


def _bits_equal(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


class _Worst(dict):
    def check(self, case, what, got, want, tol, rows=None):
        """got (device) within tol of want on `rows` (default: all)"""
        got = got.cpu().numpy().astype(np.float64)
        if rows is not None:
            got, want, tol = got[rows], want[rows], tol[rows]
        ratio = cr.max_ratio(got, want, tol)
        self[what] = max(self.get(what, 0.0), ratio)
        assert ratio <= 1.0, f"{case.name}: {what} is {ratio:.3g} x its bound"

    def show(self, title):
        print(f"\n{title}: largest |kernel - float64| / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in self.items()))


_SPARE = 2      # output rows behind the table's ids: nobody may write them


def _owned(case):
    """mask over the output rows: the table's ray ids"""
    ids = np.zeros(case.N + _SPARE, bool)
    ids[case.rays[:, 0]] = True
    return ids


def _train_fwd(nv, case, d):
    n_all = case.N + _SPARE
    ws, dep, img = _nan(n_all), _nan(n_all), _nan(n_all, 3)
    nv.call("rm_composite_train_fwd", nv.ptr(d.sigmas), nv.ptr(d.rgbs), nv.ptr(d.deltas), nv.ptr(d.rays), case.M, case.N, float(case.T_thresh),
            nv.ptr(ws), nv.ptr(dep), nv.ptr(img), nv.stream())
    return ws, dep, img


def _check_forward(worst, case, fwd, tol, ws, dep, img):
    own = _owned(case)
    worst.check(case, "weights_sum", ws, fwd.weights_sum, tol.weights_sum, np.flatnonzero(own))
    worst.check(case, "depth", dep, fwd.depth, tol.depth, np.flatnonzero(own))
    worst.check(case, "image", img, fwd.image, tol.image, np.flatnonzero(own))
    for t in (ws, dep, img):
        assert bool(torch.isnan(t[_cuda(~own)]).all()), f"{case.name}: an output of a ray outside the table was written"


def _check_grads(worst, case, live, want_gs, want_gc, tol, gs, gc):
    """live rows within the bound; every other one of the M rows exactly 0.0 (so none is left as the NaN it started as)"""
    worst.check(case, "grad_sigmas", gs, want_gs, tol.grad_sigmas, live)
    worst.check(case, "grad_rgbs", gc, want_gc, tol.grad_rgbs, live)
    dead = _cuda(~live)
    assert bool((gs[dead] == 0).all()) and bool((gc[dead] == 0).all()), f"{case.name}: a row that is not live is not exactly zero"


def test_composite_train_fwd_bwd_against_float64():
    """rm_composite_train_fwd / _bwd on every case: outputs and the gradients of live rows within the bound, every other row exactly 0.0."""
    from nerf_signature_amd import _native as nv
    worst = _Worst()
    for case in cr.cases():
        r, d = _cref(case), _dev(case)
        ws, dep, img = _train_fwd(nv, case, d)
        _check_forward(worst, case, r.fwd, r.tol, ws, dep, img)
        if case.name.startswith("zero"):
            own = _cuda(_owned(case))
            assert bool((ws[own] == 0).all()) and bool((dep[own] == 0).all()) and bool((img[own] == 0).all())
        gs, gc = _nan(case.M), _nan(case.M, 3)
        nv.call("rm_composite_train_bwd", nv.ptr(d.grad_weights_sum), nv.ptr(d.grad_image), nv.ptr(d.sigmas), nv.ptr(d.rgbs), nv.ptr(d.deltas), nv.ptr(d.rays),
                nv.ptr(ws), nv.ptr(img), case.M, case.N, float(case.T_thresh), nv.ptr(gs), nv.ptr(gc), nv.stream())
        _check_grads(worst, case, r.fwd.live, r.gs, r.gc, r.tol, gs, gc)
    worst.show("rm_composite_train_fwd/_bwd")


@pytest.mark.parametrize("bg_stride", [0, 3])
def test_composite_train_finish_fwd_against_float64(bg_stride):
    """The forward with the render tail: the three raw outputs bit-equal to rm_composite_train_fwd's, image_out and depth_out within the bound and
    bit-equal to what rm_finish_fwd makes of rm_composite_train_fwd's outputs."""
    from nerf_signature_amd import _native as nv
    worst = _Worst()
    for case in cr.cases():
        r, d = _cref(case), _dev(case)
        n_all = case.N + _SPARE
        bg = case.bg if bg_stride == 0 else case.bg_rays
        bg_dev = d.bg if bg_stride == 0 else d.bg_rays
        ws0, dep0, img0 = _train_fwd(nv, case, d)
        ws, dep, img, img_out, dep_out = _nan(n_all), _nan(n_all), _nan(n_all, 3), _nan(n_all, 3), _nan(n_all)
        nv.call("rm_composite_train_finish_fwd", nv.ptr(d.sigmas), nv.ptr(d.rgbs), nv.ptr(d.deltas), nv.ptr(d.rays), case.M, case.N, float(case.T_thresh),
                nv.ptr(d.nears), nv.ptr(d.fars), nv.ptr(bg_dev), bg_stride, nv.ptr(ws), nv.ptr(dep), nv.ptr(img),
                nv.ptr(img_out), nv.ptr(dep_out), nv.stream())
        assert _bits_equal(ws, ws0) and _bits_equal(dep, dep0) and _bits_equal(img, img0), case.name
        img_sep, dep_sep = _nan(n_all, 3), _nan(n_all)          # the separate launch: rows 0 .. N-1, which are the table's ids
        nv.call("rm_finish_fwd", nv.ptr(img0), nv.ptr(dep0), nv.ptr(ws0), nv.ptr(d.nears), nv.ptr(d.fars), nv.ptr(bg_dev), bg_stride, case.N,
                nv.ptr(img_sep), nv.ptr(dep_sep), nv.stream())
        rows = _cuda(_owned(case))
        assert _bits_equal(img_out[rows], img_sep[rows]) and _bits_equal(dep_out[rows], dep_sep[rows]), f"{case.name}: fused tail != rm_finish_fwd"
        want_img, want_dep = cr.finish(r.fwd.weights_sum, r.fwd.image, r.fwd.depth, case.nears, case.fars, bg)
        tol = cr.composite_tolerance(*r.a, r.fwd, bg=bg, nears=case.nears, fars=case.fars)
        own = np.flatnonzero(_owned(case))
        worst.check(case, "image_out", img_out, want_img, tol.image_out, own)
        worst.check(case, "depth_out", dep_out, want_dep, tol.depth_out, own)
        assert bool(torch.isnan(img_out[_cuda(~_owned(case))]).all()) and bool(torch.isnan(dep_out[_cuda(~_owned(case))]).all())
        if case.name.startswith("zero"):       # nothing absorbed: exactly the background
            assert torch.equal(img_out[_cuda(own)], _cuda(np.broadcast_to(bg, (case.N, 3))[own]))
    worst.show(f"rm_composite_train_finish_fwd bg_stride={bg_stride}")


@pytest.mark.parametrize("bg_stride", [0, 3])
@pytest.mark.parametrize("with_gws", [True, False])
@pytest.mark.parametrize("in_order", [0, 1])
def test_composite_train_finish_bwd_against_float64(in_order, with_gws, bg_stride):
    """The backward with the tail's adjoint.  rays_in_order = 1 (no memsets: the kernel zero-fills what it does not own) must leave every one of the M rows
    finite, and the rows after termination, of dropped rays and of the padding exactly zero.  All M rows of both gradients are bit-equal to
    rm_composite_train_bwd fed grad_weights_sum (zeros where none is given) + rm_finish_bwd's output, one fp32 addition."""
    from nerf_signature_amd import _native as nv
    worst = _Worst()
    for case in cr.cases():
        if in_order and not case.in_order:
            continue
        r, d = _cref(case), _dev(case)
        bg = case.bg if bg_stride == 0 else case.bg_rays
        bg_dev = d.bg if bg_stride == 0 else d.bg_rays
        ws, dep, img = _train_fwd(nv, case, d)
        gws_in = case.grad_weights_sum if with_gws else None
        gws, gi = cr.finish_backward(case.grad_image, bg, gws_in)
        want_gs, want_gc = cr.train_backward(gws, gi, *r.a, fwd=r.fwd)
        tol = cr.composite_tolerance(*r.a, r.fwd, gws_in, case.grad_image, bg=bg)
        gs, gc = _nan(case.M), _nan(case.M, 3)
        nv.call("rm_composite_train_finish_bwd", nv.ptr(d.grad_weights_sum if with_gws else None), nv.ptr(d.grad_image), nv.ptr(d.sigmas), nv.ptr(d.rgbs),
                nv.ptr(d.deltas), nv.ptr(d.rays), nv.ptr(ws), nv.ptr(img), nv.ptr(bg_dev), bg_stride, case.M, case.N,
                float(case.T_thresh), in_order, nv.ptr(gs), nv.ptr(gc), nv.stream())
        _check_grads(worst, case, r.fwd.live, want_gs, want_gc, tol, gs, gc)
        assert bool(torch.isfinite(gs).all()) and bool(torch.isfinite(gc).all()), case.name
        g_fin = _nan(case.N)                                    # the separate launches: the tail's adjoint, added by torch, then the plain backward
        nv.call("rm_finish_bwd", nv.ptr(d.grad_image), nv.ptr(None), nv.ptr(dep), nv.ptr(d.nears), nv.ptr(d.fars), nv.ptr(bg_dev), bg_stride, case.N,
                nv.ptr(g_fin), nv.ptr(None), nv.stream())
        gws_sep = (d.grad_weights_sum if with_gws else torch.zeros(case.N, device="cuda")) + g_fin
        gs_sep, gc_sep = _nan(case.M), _nan(case.M, 3)
        nv.call("rm_composite_train_bwd", nv.ptr(gws_sep), nv.ptr(d.grad_image), nv.ptr(d.sigmas), nv.ptr(d.rgbs), nv.ptr(d.deltas), nv.ptr(d.rays),
                nv.ptr(ws), nv.ptr(img), case.M, case.N, float(case.T_thresh), nv.ptr(gs_sep), nv.ptr(gc_sep), nv.stream())
        assert _bits_equal(gs, gs_sep) and _bits_equal(gc, gc_sep), f"{case.name}: fused adjoint != rm_finish_bwd + rm_composite_train_bwd"
    worst.show(f"rm_composite_train_finish_bwd rays_in_order={in_order} grad_weights_sum={'given' if with_gws else 'null'} bg_stride={bg_stride}")


def _mse(nv, case, d, bg_stride):
    n_all = case.N + _SPARE
    o = cr.Bag(weights_sum=_nan(n_all), depth=_nan(n_all), image=_nan(n_all, 3), image_out=_nan(n_all, 3), depth_out=_nan(n_all), grad_image=_nan(n_all, 3),
               grad_sigmas=_nan(case.M), grad_rgbs=_nan(case.M, 3))
    nv.call("rm_composite_train_mse", nv.ptr(d.sigmas), nv.ptr(d.rgbs), nv.ptr(d.deltas), nv.ptr(d.rays), case.M, case.N, float(case.T_thresh), nv.ptr(d.nears),
            nv.ptr(d.fars), nv.ptr(d.bg if bg_stride == 0 else d.bg_rays), bg_stride, nv.ptr(d.gt), case.n_values, float(case.grad_scale), nv.ptr(o.weights_sum),
            nv.ptr(o.depth), nv.ptr(o.image), nv.ptr(o.image_out), nv.ptr(o.depth_out), nv.ptr(o.grad_image), nv.ptr(o.grad_sigmas), nv.ptr(o.grad_rgbs), nv.stream())
    return o


def _mse_reference(case, fwd, a, bg):
    """forward -> finish -> seed -> backward, and the bound of the whole chain"""
    img_out, dep_out = cr.finish(fwd.weights_sum, fwd.image, fwd.depth, case.nears, case.fars, bg)
    seed = cr.mse_seed(img_out, case.gt, case.grad_scale, case.n_values)
    gws, gi = cr.finish_backward(seed, bg)
    gs, gc = cr.train_backward(gws, gi, *a, fwd=fwd)
    tol = cr.composite_tolerance(*a, fwd, bg=bg, nears=case.nears, fars=case.fars, gt=case.gt, grad_scale=case.grad_scale, n_values=case.n_values)
    return cr.Bag(image_out=img_out, depth_out=dep_out, grad_image=seed, grad_sigmas=gs, grad_rgbs=gc), tol


def _mse_three_launches(nv, case, d, bg_stride):
    """rm_composite_train_finish_fwd -> the MSE seed -> rm_composite_train_finish_bwd(rays_in_order = 1, no grad_weights_sum): what the one launch replaces"""
    n_all = case.N + _SPARE
    bg_dev = d.bg if bg_stride == 0 else d.bg_rays
    o = cr.Bag(weights_sum=_nan(n_all), depth=_nan(n_all), image=_nan(n_all, 3), image_out=_nan(n_all, 3), depth_out=_nan(n_all), grad_image=_nan(n_all, 3),
               grad_sigmas=_nan(case.M), grad_rgbs=_nan(case.M, 3))
    nv.call("rm_composite_train_finish_fwd", nv.ptr(d.sigmas), nv.ptr(d.rgbs), nv.ptr(d.deltas), nv.ptr(d.rays), case.M, case.N, float(case.T_thresh),
            nv.ptr(d.nears), nv.ptr(d.fars), nv.ptr(bg_dev), bg_stride, nv.ptr(o.weights_sum), nv.ptr(o.depth), nv.ptr(o.image), nv.ptr(o.image_out),
            nv.ptr(o.depth_out), nv.stream())
    if case.n_values == 3 * case.N and np.array_equal(np.sort(case.rays[:, 0]), np.arange(case.N)):     # n_values covers exactly the table's rows: clean_loss's seed
        loss = _nan(1)
        nv.call("clean_loss", nv.ptr(o.image_out), nv.ptr(d.gt), case.n_values, float(case.grad_scale), nv.ptr(loss), nv.ptr(o.grad_image), nv.ptr(None), nv.ptr(None),
                nv.ptr(None), nv.ptr(None), 0, nv.ptr(None), 0, 0, nv.stream())
    else:                                                  # the same product and quotient, then k * (image_out - gt), all in fp32
        k = np.float32(case.grad_scale) * np.float32(2.0) / np.float32(case.n_values)
        ids = _cuda(np.flatnonzero(_owned(case)))
        o.grad_image[ids] = float(k) * (o.image_out[ids] - d.gt[ids])
    nv.call("rm_composite_train_finish_bwd", nv.ptr(None), nv.ptr(o.grad_image), nv.ptr(d.sigmas), nv.ptr(d.rgbs), nv.ptr(d.deltas), nv.ptr(d.rays),
            nv.ptr(o.weights_sum), nv.ptr(o.image), nv.ptr(bg_dev), bg_stride, case.M, case.N, float(case.T_thresh), 1, nv.ptr(o.grad_sigmas), nv.ptr(o.grad_rgbs),
            nv.stream())
    return o


@pytest.mark.parametrize("bg_stride", [0, 3])
def test_composite_train_mse_against_float64(bg_stride):
    """The one-launch kernel of the captured stage-1 loop: every output against the reference chain, and the zero-fill of all rows it does not own.
    Every output is also bit-equal to the three launches it replaces (_mse_three_launches)."""
    from nerf_signature_amd import _native as nv
    worst = _Worst()
    for case in cr.cases():
        if not case.in_order:          # the entry point is defined for ascending gapless tables only
            continue
        r, d = _cref(case), _dev(case)
        bg = case.bg if bg_stride == 0 else case.bg_rays
        want, tol = _mse_reference(case, r.fwd, r.a, bg)
        o = _mse(nv, case, d, bg_stride)
        _check_forward(worst, case, r.fwd, tol, o.weights_sum, o.depth, o.image)
        own = np.flatnonzero(_owned(case))
        for k in ("image_out", "depth_out", "grad_image"):
            worst.check(case, k, o[k], want[k], tol[k], own)
            assert bool(torch.isnan(o[k][_cuda(~_owned(case))]).all())
        _check_grads(worst, case, r.fwd.live, want.grad_sigmas, want.grad_rgbs, tol, o.grad_sigmas, o.grad_rgbs)
        assert bool(torch.isfinite(o.grad_sigmas).all()) and bool(torch.isfinite(o.grad_rgbs).all()), case.name
        sep = _mse_three_launches(nv, case, d, bg_stride)
        for k in o:
            assert _bits_equal(o[k], sep[k]), f"{case.name}: {k} of the one launch != the three launches"
    worst.show(f"rm_composite_train_mse bg_stride={bg_stride}")


def test_composite_non_finite_density_stays_in_its_ray():
    """One -inf and one NaN density in one ray of a workgroup: that ray's sums and the gradients of its live rows are non-finite, its rows behind the
    NaN (not live: a NaN transmittance passes no test) are zero, and the three neighbours are within the bound of the float64 reference."""
    from nerf_signature_amd import _native as nv
    case = cr.poisoned_case()
    r, d = _cref(case), _dev(case)
    bad = case.poison
    off, cnt = int(case.rays[bad, 1]), int(case.rays[bad, 2])
    mine = np.zeros(case.M, bool)
    mine[off:off + cnt] = True
    live_bad, good = r.fwd.live & mine, np.array([i for i in range(case.N) if i != bad])
    assert live_bad.sum() == 6 and not np.isfinite(r.fwd.weights_sum[bad]) and not np.isfinite(r.fwd.image[bad]).any()
    assert not np.isfinite(r.gs[live_bad]).any() and not np.isfinite(r.gc[live_bad]).any()        # the reference says so too
    worst = _Worst()

    def check(ws, img, gs, gc, want_gs, want_gc, tol):
        assert not bool(torch.isfinite(ws[bad])) and not bool(torch.isfinite(img[bad]).any())
        assert not bool(torch.isfinite(gs[_cuda(live_bad)]).any()) and not bool(torch.isfinite(gc[_cuda(live_bad)]).any())
        worst.check(case, "weights_sum", ws, r.fwd.weights_sum, tol.weights_sum, good)
        worst.check(case, "image", img, r.fwd.image, tol.image, good)
        rest = ~mine
        worst.check(case, "grad_sigmas", gs, want_gs, tol.grad_sigmas, r.fwd.live & rest)
        worst.check(case, "grad_rgbs", gc, want_gc, tol.grad_rgbs, r.fwd.live & rest)
        dead = _cuda(~r.fwd.live)
        assert bool((gs[dead] == 0).all()) and bool((gc[dead] == 0).all())

    ws, dep, img = _train_fwd(nv, case, d)
    gs, gc = _nan(case.M), _nan(case.M, 3)
    nv.call("rm_composite_train_bwd", nv.ptr(d.grad_weights_sum), nv.ptr(d.grad_image), nv.ptr(d.sigmas), nv.ptr(d.rgbs), nv.ptr(d.deltas), nv.ptr(d.rays),
            nv.ptr(ws), nv.ptr(img), case.M, case.N, float(case.T_thresh), nv.ptr(gs), nv.ptr(gc), nv.stream())
    check(ws, img, gs, gc, r.gs, r.gc, r.tol)
    want, tol = _mse_reference(case, r.fwd, r.a, case.bg)
    o = _mse(nv, case, d, 0)
    check(o.weights_sum, o.image, o.grad_sigmas, o.grad_rgbs, want.grad_sigmas, want.grad_rgbs, tol)
    worst.check(case, "grad_image", o.grad_image, want.grad_image, tol.grad_image, good)
    assert not bool(torch.isfinite(o.grad_image[bad]).any())
    worst.show("non-finite density, neighbours of the poisoned ray")


def _burst_on_device(nv, n_alive0, first_step, density_scale, eval_form):
    """A whole multi-round evaluation run on the device beside the float64 reference: rays_alive compared after every round (composite_ref.run_burst)."""
    N = cr.BURST_RAYS
    scene = cr.burst_scene()
    t, ws, dep, img = _cuda(scene.rays_t0), _nan(N), _nan(N), _nan(N, 3)       # rays 0 .. n_alive0-1 take part; the others' state must stay NaN
    for x in (ws, dep, img):
        x[:n_alive0] = 0

    def device_round(rd):
        rows = N * rd.n_step                                     # room for every thread of the launch; rows past n_alive * n_step hold deltas = 0
        pad = lambda a: _cuda(np.concatenate([a, np.zeros((rows - len(a),) + a.shape[1:], a.dtype)]))
        alive = _cuda(np.concatenate([rd.rays_alive, np.zeros(N - rd.n_alive, np.int32)]))
        sig, rgb, dl = pad(rd.sigmas), pad(rd.rgbs), pad(rd.deltas)      # held in names: a temporary's memory would be handed to the next one
        if eval_form:
            ctl = _cuda(np.array([rd.n_alive, rd.n_step, rd.n_alive * rd.n_step, 0], np.int32))
            nv.call("rm_eval_composite", nv.ptr(ctl), N, 1e-2, float(density_scale), nv.ptr(alive), nv.ptr(t), nv.ptr(sig), nv.ptr(rgb),
                    nv.ptr(dl), nv.ptr(ws), nv.ptr(dep), nv.ptr(img), nv.stream())
        else:
            nv.call("rm_composite", rd.n_alive, rd.n_step, 1e-2, nv.ptr(alive), nv.ptr(t), nv.ptr(sig), nv.ptr(rgb), nv.ptr(dl),
                    nv.ptr(ws), nv.ptr(dep), nv.ptr(img), nv.stream())
        got = alive.cpu().numpy()
        assert (got[rd.n_alive:] == 0).all()
        return got[:rd.n_alive]
    st, log = cr.run_burst(n_alive0, first_step, 1e-2, density_scale if eval_form else None, fp32=device_round)
    u = np.arange(N) < n_alive0
    np.testing.assert_array_equal(t.cpu().numpy().astype(np.float64), np.where(u, st.t, scene.rays_t0))      # rays_t: exact
    for x in (ws, dep, img):
        assert bool(torch.isnan(x[n_alive0:]).all())
    return [(cr.max_ratio(x.cpu().numpy().astype(np.float64)[u], want[u], tol[u]), k)
            for k, x, want, tol in (("weights_sum", ws, st.ws, st.bound.weights_sum), ("depth", dep, st.d, st.bound.depth), ("image", img, st.im, st.bound.image))], log


@pytest.mark.parametrize("n_alive0", cr.BURST_ALIVE)
def test_composite_burst_against_float64(n_alive0):
    """rm_composite over whole runs: n_step cycles through 1..8, rays end by deltas == 0 (at step 0 and in mid-burst) and by T < T_thresh (on the first and
    on the last step of a burst); rays_alive and rays_t equal the reference's exactly, the accumulators are within the serial chain's bound."""
    from nerf_signature_amd import _native as nv
    ratios, log = _burst_on_device(nv, n_alive0, 1 + n_alive0 % 8, None, False)
    print(f"\nrm_composite n_alive={n_alive0}: largest |kernel - float64| / bound: " + ", ".join(f"{k} {v:.3f}" for v, k in ratios))
    assert all(v <= 1.0 for v, _ in ratios), ratios
    assert log.rounds > 1 and (n_alive0 < 63 or (log.first and log.last and log.zero_first and log.zero_mid and log.steps == set(range(1, 9))))


@pytest.mark.parametrize("density_scale", [1.0, 0.37])
@pytest.mark.parametrize("n_alive0", cr.BURST_ALIVE)
def test_eval_composite_against_float64(n_alive0, density_scale):
    """rm_eval_composite: the same runs with the counts in `ctl` on the device (the launch covers all N threads, ctl[0] < N in every round but the first
    of the full run) and the density scaled inside the kernel."""
    from nerf_signature_amd import _native as nv
    ratios, log = _burst_on_device(nv, n_alive0, 1 + n_alive0 % 8, density_scale, True)
    print(f"\nrm_eval_composite n_alive={n_alive0} density_scale={density_scale}: largest |kernel - float64| / bound: " + ", ".join(f"{k} {v:.3f}" for v, k in ratios))
    assert all(v <= 1.0 for v, _ in ratios), ratios
    assert log.rounds > 1


_COMPACT_SENTINEL = -7


def _compact_fills(n):
    """ray ids in a shuffled order (so that a reordering shows), with -1 for the dead: all alive, all dead, about 40 % dead at seeded random places, only the last alive"""
    rng = np.random.RandomState(1000 + n)
    ids = rng.permutation(n).astype(np.int32)
    dead = np.full(n, -1, np.int32)
    return {"all_alive": ids, "all_dead": dead, "random": np.where(rng.rand(n) < 0.4, -1, ids).astype(np.int32),
            "last_only": np.concatenate([dead[:-1], ids[-1:]])}


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1024, 1025, 2048, 3001])
def test_compaction_pair_against_numpy(n):
    """rm_compact_alive and rm_eval_compact against `alive[alive >= 0]` (order kept) around the wave size and the 1024-element round: entries past the survivor
    count keep the buffer's sentinel, and rm_eval_compact leaves the next round's control words of its kernel's comment -- survivors (0 once
    marched + n_step >= max_steps), clamp(N / alive, 1, 8) (1 when no ray survives), their product, marched + n_step -- or nothing at all when ctl[0] == 0."""
    from nerf_signature_amd import _native as nv
    N, n_step, marched = 4 * n, 3, 10
    for name, alive in _compact_fills(n).items():
        want = alive[alive >= 0]
        k = want.shape[0]
        src = _cuda(alive)

        def check_out(out, count, what):
            got = out.cpu().numpy()
            np.testing.assert_array_equal(got[:count], want[:count], err_msg=f"{what} {name} n={n}")
            np.testing.assert_array_equal(got[count:], np.full(n - count, _COMPACT_SENTINEL, np.int32), err_msg=f"{what} {name} n={n}: past the survivors")

        out = torch.full((n,), _COMPACT_SENTINEL, dtype=torch.int32, device="cuda")
        n_out = torch.full((1,), _COMPACT_SENTINEL, dtype=torch.int32, device="cuda")
        nv.call("rm_compact_alive", nv.ptr(src), n, nv.ptr(out), nv.ptr(n_out), nv.stream())
        assert int(n_out.item()) == k, (name, n)
        check_out(out, k, "rm_compact_alive")

        for max_steps in (1024, marched + n_step):      # not reached; reached by this round
            ctl = _cuda(np.array([n, n_step, n * n_step, marched], np.uint32).view(np.int32))
            out = torch.full((n,), _COMPACT_SENTINEL, dtype=torch.int32, device="cuda")
            nv.call("rm_eval_compact", nv.ptr(ctl), N, max_steps, nv.ptr(src), nv.ptr(out), nv.stream())
            check_out(out, k, "rm_eval_compact")
            survivors = k if marched + n_step < max_steps else 0
            nxt = min(max(N // survivors, 1), 8) if survivors else 1
            assert ctl.cpu().numpy().view(np.uint32).tolist() == [survivors, nxt, survivors * nxt, marched + n_step], (name, n, max_steps)

        idle = [0, n_step, 0, marched]
        ctl = _cuda(np.array(idle, np.uint32).view(np.int32))
        out = torch.full((n,), _COMPACT_SENTINEL, dtype=torch.int32, device="cuda")
        nv.call("rm_eval_compact", nv.ptr(ctl), N, 1024, nv.ptr(src), nv.ptr(out), nv.stream())
        check_out(out, 0, "rm_eval_compact with ctl[0] == 0")
        assert ctl.cpu().numpy().view(np.uint32).tolist() == idle, (name, n)
