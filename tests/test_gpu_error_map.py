"""Error-map ray sampling on the device (rg_sample_rays_weighted, rg_error_map_update; rays.DeviceRaySampler(error_map=), stage1.GraphedCleanLoop): the selection
against a sort of the kernel's own keys, the keys against the float64 mirror, the pixels and rays against get_rays, the distribution against
torch.multinomial(replacement=False), the write-back against the reference's gather / scatter operators, and the captured stage-1 loop with a map against the
same kernel sequence issued eagerly."""
import numpy as np
import pytest
import torch

import closed_form as cf
import error_map_ref as em

pytestmark = pytest.mark.gpu
KW = dict(dt_gamma=0, max_steps=1024)
SEED = (0x1234 << 32) | 99


def _store(P, H, W, focal=None):
    focal = 70.0 * W / 80 if focal is None else focal
    poses = torch.stack([torch.from_numpy(cf.orbit_rays(1, seed=0, radius=3.0 + 0.05 * k)[0]) for k in range(P)]).cuda()
    g = torch.Generator().manual_seed(P * 1000 + H)
    images = torch.rand(P, H * W, 3, generator=g).cuda()
    return poses, images, (focal, focal * 1.03, W / 2, H / 2)


def _maps(kind, P, G, N, p):
    """The map of one selection case; every row but `p` holds other values (they must not matter)."""
    rng = np.random.RandomState(G * 100003 + N)
    cells = G * G
    m = rng.rand(P, cells).astype(np.float32) + 0.5
    if kind == "ones":              # ties: 24-bit uniforms coincide
        row = np.ones(cells, np.float32)
    elif kind == "random":          # weights over 1e-6 .. 1, zeros, one NaN, one negative, one +inf
        row = np.exp(rng.uniform(np.log(1e-6), 0.0, cells)).astype(np.float32)
        bad = rng.permutation(cells)
        n_zero = 1000 if cells > 2000 else 3
        row[bad[:n_zero]] = 0.0
        row[bad[n_zero]], row[bad[n_zero + 1]], row[bad[n_zero + 2]] = np.nan, -0.5, np.inf
    else:                           # fewer than N valid cells
        row = np.zeros(cells, np.float32)
        row[rng.permutation(cells)[:N // 2]] = rng.rand(N // 2).astype(np.float32) + 0.1
        row[rng.randint(cells)] = np.nan if N > 1 else 0.0
    m[p] = row
    return torch.from_numpy(m).cuda()


def _draw(s, step, keys=True):
    N, dev = s.n_rays, s.poses.device
    ctr = torch.full((1,), step, dtype=torch.int32, device=dev)
    o, d, gt = (torch.full((N, 3), float("nan"), device=dev) for _ in range(3))
    inds = torch.full((N,), -1, dtype=torch.int64, device=dev)
    pose = torch.full((1,), -1, dtype=torch.int32, device=dev)
    k = torch.full((s.error_grid ** 2,), float("nan"), device=dev) if keys else None
    s.inds_coarse.fill_(-1)
    s.sample_into(ctr, o, d, gt, inds, pose, keys_out=k)
    return dict(o=o, d=d, gt=gt, inds=inds, pose=int(pose), keys=k, coarse=s.inds_coarse.clone())


def _top_n(keys, n):
    """Sorted top-n by (key descending, index ascending) of float32 keys (compared as the floats they are)."""
    return torch.from_numpy(em.select(keys.cpu().numpy(), n))


@pytest.mark.parametrize("G,N", [(4, 1), (4, 5), (4, 16), (128, 1), (128, 63), (128, 4096), (128, 128 * 128)])
def test_selection_is_exact(G, N):
    """inds_coarse == the sorted top-N by (key descending, cell ascending) of the keys the kernel itself reports."""
    from nerf_signature_amd import rays
    P, H, W, stride, offset = 3, 60, 80, 2, 1
    poses, images, intr = _store(P, H, W)
    cells = G * G
    for kind in ("ones", "random", "few"):
        step = 7
        p = em.pose_of(step, stride, offset, P)
        emap = _maps(kind, P, G, N, p)
        s = rays.DeviceRaySampler(poses, images, intr, H, W, N, stride=stride, offset=offset, seed=SEED, error_map=emap, error_grid=G)
        assert s.error_map is emap
        a = _draw(s, step)
        want = _top_n(a["keys"], N)
        assert torch.equal(a["coarse"].cpu(), want), (kind, G, N)
        assert a["pose"] == p == int(s.pose_word)
        assert len(torch.unique(a["coarse"])) == N and int(a["coarse"].min()) >= 0 and int(a["coarse"].max()) < cells
        row = emap[p].cpu()
        valid = torch.isfinite(row) & (row > 0)
        assert torch.equal(a["keys"].cpu() > 0, valid)                     # invalid weights: key 0
        n_valid = int(valid.sum())
        if n_valid < N:     # every valid cell, then the lowest-index invalid ones
            fill = torch.nonzero(~valid).reshape(-1)[:N - n_valid]
            assert torch.equal(a["coarse"].cpu(), torch.sort(torch.cat([torch.nonzero(valid).reshape(-1), fill])).values), kind
        else:
            assert bool(valid[a["coarse"].cpu()].all()), kind
        if kind == "ones" and cells == 16384:
            assert len(torch.unique(a["keys"])) < cells                    # the tie rule was exercised
        # the same step: the same draw; the rows of the other poses do not matter
        b = _draw(s, step)
        other = emap.clone()
        other[[q for q in range(P) if q != p]] = float("nan")
        s2 = rays.DeviceRaySampler(poses, images, intr, H, W, N, stride=stride, offset=offset, seed=SEED, error_map=other, error_grid=G)
        c = _draw(s2, step)
        for x in (b, c):
            assert torch.equal(x["coarse"], a["coarse"]) and torch.equal(x["inds"], a["inds"]) and torch.equal(x["keys"], a["keys"], )
            assert torch.equal(x["o"], a["o"]) and torch.equal(x["d"], a["d"]) and torch.equal(x["gt"], a["gt"])
        # another step: other keys; another draw wherever a draw has room to differ (16 <= N <= cells / 2 valid cells to choose from)
        step2 = step + P            # (the same pose)
        d = _draw(s, step2)
        assert d["pose"] == p and torch.equal(d["coarse"].cpu(), _top_n(d["keys"], N))
        assert not torch.equal(d["keys"][valid.cuda()], a["keys"][valid.cuda()]) or n_valid == 0
        if 16 <= N <= min(n_valid, cells) // 2:
            assert not torch.equal(d["coarse"], a["coarse"]), kind


@pytest.mark.parametrize("kind", ["ones", "random"])
def test_keys_match_the_float64_mirror(kind):
    """key = w / -ln(u), u = (24 hash bits of (seed, step, cell) + 1) / 2^24: logf and the divide are good to a few ulp; a wrong hash or formula is off by O(1)."""
    from nerf_signature_amd import rays
    P, H, W, G, N = 3, 60, 80, 128, 4096
    poses, images, intr = _store(P, H, W)
    for step in (0, 5):
        p = em.pose_of(step, 1, 2, P)
        emap = _maps(kind, P, G, N, p)
        s = rays.DeviceRaySampler(poses, images, intr, H, W, N, stride=1, offset=2, seed=SEED, error_map=emap, error_grid=G)
        a = _draw(s, step)
        want = em.keys(emap[p].cpu().numpy(), SEED, step)
        got = a["keys"].cpu().numpy().astype(np.float64)
        finite = np.isfinite(want) & (want > 0)
        print(f"\n{kind}, step {step}: worst relative key error {np.max(np.abs(got[finite] - want[finite]) / want[finite]):.2e}")
        np.testing.assert_allclose(got, want, rtol=1e-5, atol=0)
        assert np.array_equal(a["coarse"].cpu().numpy(), em.select(a["keys"].cpu().numpy(), N))


@pytest.mark.parametrize("H,W", [(60, 80), (200, 136)])
def test_pixels_and_rays(H, W):
    """Every drawn pixel lies inside its cell; rays and ground truth are those of get_rays / the image store at the drawn pixels (as
    test_device_ray_sampler_matches_get_rays for the uniform draw)."""
    from nerf_signature_amd import rays
    P, G, N = 5, 128, 4096
    poses, images, intr = _store(P, H, W)
    s = rays.DeviceRaySampler(poses, images, intr, H, W, N, stride=2, offset=1, seed=SEED, error_map=True)
    assert s.error_grid == 128 and tuple(s.error_map.shape) == (P, G * G) and float(s.error_map.min()) == float(s.error_map.max()) == 1.0
    sx, sy = H / G, W / G           # (exact in binary for both shapes)
    for step in (0, 3):
        a = _draw(s, step)
        k = em.pose_of(step, 2, 1, P)
        assert a["pose"] == k
        inds, coarse = a["inds"].cpu(), a["coarse"].cpu()
        assert int(inds.min()) >= 0 and int(inds.max()) < H * W
        row, col, cx, cy = inds // W, inds % W, coarse // G, coarse % G
        assert bool((row >= torch.floor(cx * sx)).all()) and bool((row <= torch.clamp(torch.floor((cx + 1) * sx), max=H - 1)).all())
        assert bool((col >= torch.floor(cy * sy)).all()) and bool((col <= torch.clamp(torch.floor((cy + 1) * sy), max=W - 1)).all())
        assert np.array_equal(inds.numpy(), em.pixels(coarse.numpy(), G, H, W, SEED, step))      # the two sub-cell uniforms of (seed, step, n)
        want = rays.get_rays(poses[k:k + 1], intr, H, W, N=-1)
        assert torch.equal(a["o"], want["rays_o"][0, a["inds"]]) and torch.equal(a["d"], want["rays_d"][0, a["inds"]])
        assert torch.equal(a["gt"], images[k][a["inds"]])
    with pytest.raises(ValueError):
        rays.DeviceRaySampler(poses, images, intr, H, W, N, error_map=torch.ones(P, 100, device="cuda"))
    with pytest.raises(ValueError):
        rays.DeviceRaySampler(poses, images, intr, H, W, 17, error_map=True, error_grid=4)
    with pytest.raises(ValueError):
        rays.DeviceRaySampler(poses, images, intr, H, W, N).update_error_map(a["o"], a["gt"])


def test_distribution_matches_torch_multinomial():
    """The fraction of a 4096-cell draw inside the weight-8 quarter: 64 steps on the device against 256 draws of torch.multinomial(replacement=False) on the CPU,
    |mean_gpu - m| <= 5 s sqrt(1/64 + 1/256); no draw touches a zero-weight cell."""
    from nerf_signature_amd import rays
    P, H, W = 2, 60, 80
    poses, images, intr = _store(P, H, W)
    m, s_ref, zero_hits = em.multinomial_reference()
    assert zero_hits == 0
    emap = torch.rand(P, em.DIST_G ** 2).cuda()
    emap[1] = torch.from_numpy(em.dist_weights()).cuda()
    s = rays.DeviceRaySampler(poses, images, intr, H, W, em.DIST_N, stride=0, offset=1, seed=SEED, error_map=emap, error_grid=em.DIST_G)
    stats = [em.dist_statistic(_draw(s, step, keys=False)["coarse"].cpu().numpy()) for step in range(64)]
    mean = float(np.mean([f for f, _ in stats]))
    print(f"\nmultinomial: mean {m:.5f}, per-draw sd {s_ref:.5f}; device: mean {mean:.5f}; |difference| {abs(mean - m):.2e} <= bound {em.dist_bound(s_ref):.2e}")
    assert abs(mean - m) <= em.dist_bound(s_ref)
    assert sum(z for _, z in stats) == 0


def _clean_model():
    from nerf_signature_amd.stage1 import CleanNeRFNetwork
    m = CleanNeRFNetwork(bound=1.0, cuda_ray=True, density_scale=1, min_near=0.2, density_thresh=10, bg_radius=-1)
    grid, bitfield, _ = cf.ball_scene(bound=1.0)
    with torch.no_grad():
        for l in range(16):
            m.encoder.embeddings[l].weight.copy_(torch.from_numpy(cf.table(l)))
        m.sigma_net.params.copy_(torch.from_numpy(cf.mlp_params(3072, 1337)))
        m.color_net.params.copy_(torch.from_numpy(cf.mlp_params(7168, 1338)))
        m.density_grid.copy_(torch.from_numpy(grid))
        m.density_bitfield.copy_(torch.from_numpy(bitfield))
    return m.cuda().train()


def _adam(m, lr=1e-2):
    return torch.optim.Adam(m.get_params(lr), betas=(0.9, 0.99), eps=1e-15)


def test_write_back_matches_gather_scatter():
    """rg_error_map_update against 0.1 * map.gather(1, inds) + 0.9 * err with scatter_ in torch float32: updated cells within a few ulp (the three squares may be
    summed in another order), everything else untouched, a NaN prediction leaves its cell alone; and CleanLoop(error_map=) -- the reference's operators inside the eager
    loop, fed get_rays(..., error_map=) batches -- against the kernel on the same (index, inds_coarse, pred, gt)."""
    from nerf_signature_amd import _native as nv, rays
    from nerf_signature_amd.stage1 import CleanLoop
    for G, N in ((128, 4096), (4, 5)):
        P, H, W = 3, 60, 80
        poses, images, intr = _store(P, H, W)
        emap = (torch.rand(P, G * G, generator=torch.Generator().manual_seed(G)) + 0.01).cuda()
        s = rays.DeviceRaySampler(poses, images, intr, H, W, N, stride=1, offset=0, seed=SEED, error_map=emap, error_grid=G)
        a = _draw(s, 2)
        before = emap.clone()
        pred = torch.rand(N, 3, device="cuda")
        pred[3, 1] = float("nan")
        s.update_error_map(pred, a["gt"])
        err = ((pred - a["gt"]) ** 2).mean(-1)
        inds = a["coarse"][None]
        want = before.clone()
        row = want[2:3].clone()
        row.scatter_(1, inds, 0.1 * row.gather(1, inds) + 0.9 * err[None])
        row[0, a["coarse"][3]] = before[2, a["coarse"][3]]                  # the NaN ray's cell keeps its value
        want[2] = row[0]
        touched = torch.zeros_like(emap, dtype=torch.bool)
        touched[2, a["coarse"]] = True
        assert torch.equal(emap[~touched], before[~touched])                # other cells, other poses: bit for bit
        assert float(emap[2, a["coarse"][3]]) == float(before[2, a["coarse"][3]])
        np.testing.assert_allclose(emap[touched].cpu().numpy(), want[touched].cpu().numpy(), rtol=5e-7, atol=0)
        assert int((emap[touched] != before[touched]).sum()) >= N - 2
    # the eager loop's torch operators against the kernel
    H = W = 400
    pose, intr, _ = cf.orbit_rays(1, seed=2)
    poses = torch.stack([torch.from_numpy(pose), torch.from_numpy(cf.orbit_rays(1, seed=2, radius=3.0)[0])]).cuda()
    images = torch.rand(2, H * W, 3, generator=torch.Generator().manual_seed(4)).cuda()
    emap = (torch.rand(2, 128 * 128, generator=torch.Generator().manual_seed(5)) + 0.01).cuda()
    start = emap.clone()
    m = _clean_model()
    loop = CleanLoop(m, _adam(m), KW, update_extra_interval=10 ** 9, error_map=emap)
    loop.global_step = 1
    by_kernel = start.clone()
    for k in (1, 0, 1):
        torch.manual_seed(20 + k)
        data = rays.get_rays(poses[k:k + 1], intr, H, W, N=256, error_map=emap[k:k + 1])
        data.update(images=images[k][data["inds"][0]][None], index=[k], perturb=False, force_all_rays=True)
        image, _ = loop.step(data)
        pred, gt = image.detach().reshape(256, 3).contiguous(), data["images"].reshape(256, 3).contiguous()
        nv.call("rg_error_map_update", nv.ptr(by_kernel), 2, 128, nv.ptr(torch.tensor([k], dtype=torch.int32, device="cuda")), nv.ptr(data["inds_coarse"][0].contiguous()),
                nv.ptr(pred), nv.ptr(gt), 256, nv.stream())
        changed = by_kernel != start
        assert torch.equal(changed, emap != start)
        np.testing.assert_allclose(by_kernel.cpu().numpy(), emap.cpu().numpy(), rtol=5e-7, atol=0)
        by_kernel.copy_(emap)       # (the next step starts from one state)
    assert int((emap != start).sum()) > 500


# ---- the captured stage-1 loop with a map
_SCENE = {}


def _ball_views(P=24, H=64, W=64):
    """P orbit views of the ball scene of test_captured_loop_equals_the_eager_loop: the target colour where a pixel's ray meets the ball, the white background elsewhere
    (so that every pixel can be learned)."""
    if not _SCENE:
        from nerf_signature_amd import rays
        focal = 555.56 * W / 400
        poses = torch.stack([torch.from_numpy(cf.orbit_rays(1, seed=0, radius=3.0 + 0.02 * k)[0]) for k in range(P)]).cuda()
        intr = (focal, focal, W / 2, H / 2)
        r = rays.get_rays(poses, intr, H, W, N=-1)
        o, d = r["rays_o"], r["rays_d"]
        b = (o * d).sum(-1)
        hit = b * b - ((o * o).sum(-1) - 0.25) >= 0
        images = torch.where(hit[..., None], torch.tensor([0.2, 0.5, 0.8], device="cuda"), torch.ones(3, device="cuda")).contiguous()
        assert 0.05 < float(hit.float().mean()) < 0.5
        _SCENE.update(poses=poses, images=images, intr=intr, H=H, W=W, P=P)
    return _SCENE


def _map_loop(capture, n_rays=256, grid=32, **kw):
    from nerf_signature_amd import rays
    from nerf_signature_amd.stage1 import GraphedCleanLoop
    v = _ball_views()
    m = _clean_model()
    s = rays.DeviceRaySampler(v["poses"], v["images"], v["intr"], v["H"], v["W"], n_rays, seed=SEED, error_map=True, error_grid=grid)
    torch.manual_seed(11)           # (the first step's march offsets come from torch's generator)
    return m, s, GraphedCleanLoop(m, _adam(m), KW, n_rays=n_rays, sampler=s, update_extra_interval=0, perturb=True, seed=3, capture=capture, **kw)


def test_captured_loop_with_a_map_equals_the_eager_sequence():
    """20 steps of GraphedCleanLoop with a map sampler, captured and issued eagerly: parameters, losses and the error map bit for bit; rows of poses not yet visited
    are still all ones, a visited row differs from ones in exactly the cells its step drew.  Both compositing routes."""
    from nerf_signature_amd import rays
    v = _ball_views()
    got = {}
    for name, capture, kw in (("captured", True, {}), ("eager", False, {}), ("three_launch", True, {"fused_composite": False})):
        m, s, loop = _map_loop(capture, **kw)
        for _ in range(20):
            loop.step()
        torch.cuda.synchronize()
        assert not loop.overflowed() and (len(loop.graph.segments) == 1 or not capture)
        got[name] = ([p.detach().clone() for p in m.trainable()], loop.losses(), s.error_map.clone(), int(loop.step_dev))
        loop.close()
    a = got["captured"]
    for name in ("eager", "three_launch"):
        b = got[name]
        assert a[3] == b[3] == 20 and a[1] == b[1] and len(a[1]) == 20
        for x, y in zip(a[0], b[0]):
            assert torch.equal(x, y), name
        assert torch.equal(a[2], b[2]), name
    emap = a[2]
    assert tuple(emap.shape) == (24, 32 * 32)
    assert bool((emap[20:] == 1).all())                                    # poses 20..23: not visited yet
    probe = rays.DeviceRaySampler(v["poses"], v["images"], v["intr"], v["H"], v["W"], 256, seed=SEED, error_map=True, error_grid=32)
    for step in (0, 7, 19):         # each visited once, from a row of ones: the draw of that step
        drawn = torch.zeros(32 * 32, dtype=torch.bool, device="cuda")
        drawn[_draw(probe, step, keys=False)["coarse"]] = True
        assert torch.equal(emap[step] != 1, drawn), step
        assert bool(torch.isfinite(emap[step]).all()) and float(emap[step].min()) >= 0.1 - 1e-6


def test_captured_loop_with_a_map_trains():
    """200 captured steps drawing from the map: the loss falls, no step overflowed its buffers, every pose's row has been written."""
    m, s, loop = _map_loop(True)
    for _ in range(200):
        loop.step()
    losses = loop.losses()
    first, last = float(np.mean(losses[:50])), float(np.mean(losses[-50:]))
    print(f"\nmean loss of steps 0..49: {first:.4e}, of steps 150..199: {last:.4e}")
    assert len(losses) == 200 and np.isfinite(losses).all()
    assert last < first
    assert not loop.overflowed()
    assert bool((s.error_map != 1).any(dim=1).all()) and bool(torch.isfinite(s.error_map).all())
    loop.close()
