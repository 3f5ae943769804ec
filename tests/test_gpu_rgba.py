"""Stage 1 on RGBA ground truth (the reference's train_step on 4-channel images, nerf/utils.py:491-517: a fresh background colour per pixel, the target blended
against it, the render composited against it): rg_blend_random_background against the integer mirror and against torch's own operators, the two RGBA samplers
against their 3-channel twins and the blend kernel, stage1.train_step / eval_step against the hand-written sequence, the captured loop fed RGBA batches against the
eager loop, the captured loop with an RGBA sampler against the same launches issued eagerly, and a training run in which alpha has to teach opacity."""
import ctypes

import numpy as np
import pytest
import torch

import closed_form as cf
import random_bg_ref as rb
from oracle import field_ref as fr

pytestmark = pytest.mark.gpu
KW = dict(dt_gamma=0, max_steps=1024)
SEED = (0x1234 << 32) | 99          # (above 2^32: both halves of the seed enter the hash)


def _blend(rgba, step, seed=SEED):
    """rg_blend_random_background on rgba [N,4] at `step`: (bg, gt), both pre-filled with NaN."""
    from nerf_signature_amd import _native as nv
    N = rgba.shape[0]
    ctr = torch.full((1,), step, dtype=torch.int32, device="cuda")
    bg, gt = (torch.full((N, 3), float("nan"), device="cuda") for _ in range(2))
    nv.call("rg_blend_random_background", nv.ptr(rgba), N, nv.ptr(ctr), seed, nv.ptr(bg), nv.ptr(gt), nv.stream())
    return bg, gt


@pytest.mark.parametrize("N", [1, 63, 64, 65, 257])
def test_blend_kernel_equals_the_mirror_and_torch(N):
    """bg bit-equal to the mirror; gt bit-equal to rgb * a + bg * (1 - a) written with torch operators on the device (each its own kernel: nothing is contracted) --
    equality, by the operation order.  Alpha is exactly 0, exactly 1 or a random fraction in turn (shifted by the step, so that N = 1 meets all three)."""
    rng = np.random.RandomState(N)
    for k, step in enumerate((0, 7, 2 ** 31 - 1)):
        rgba = rng.rand(N, 4).astype(np.float32)
        kind = (np.arange(N) + k) % 3
        rgba[kind == 0, 3], rgba[kind == 1, 3] = 0.0, 1.0
        t = torch.from_numpy(rgba).cuda()
        bg, gt = _blend(t, step)
        want_bg = rb.background(N, SEED, step)
        assert np.array_equal(bg.cpu().numpy(), want_bg), (N, step)
        want = t[..., :3] * t[..., 3:] + bg * (1 - t[..., 3:])
        assert torch.equal(gt, want), (N, step)
        assert np.array_equal(gt.cpu().numpy(), rb.blend(rgba, want_bg))
        k0, k1 = torch.from_numpy(kind == 0).cuda(), torch.from_numpy(kind == 1).cuda()
        assert torch.equal(gt[k0], bg[k0]) and torch.equal(gt[k1], t[k1][:, :3])
        bg2, gt2 = _blend(t, step)
        assert torch.equal(bg2, bg) and torch.equal(gt2, gt)
    # NULL counter = step 0; another seed, another draw
    from nerf_signature_amd import _native as nv
    bg0, gt0 = (torch.empty(N, 3, device="cuda") for _ in range(2))
    nv.call("rg_blend_random_background", nv.ptr(t), N, None, SEED, nv.ptr(bg0), nv.ptr(gt0), nv.stream())
    assert np.array_equal(bg0.cpu().numpy(), rb.background(N, SEED, 0))
    assert not torch.equal(_blend(t, 0, seed=SEED + 1)[0], bg0)


# ---- the samplers
def _store(P, H, W):
    focal = 70.0 * W / 80
    poses = torch.stack([torch.from_numpy(cf.orbit_rays(1, seed=0, radius=3.0 + 0.05 * k)[0]) for k in range(P)]).cuda()
    g = torch.Generator().manual_seed(P * 1000 + H)
    rgba = torch.rand(P, H * W, 4, generator=g)
    rgba[:, ::5, 3], rgba[:, 1::5, 3] = 0.0, 1.0
    return poses, rgba.cuda(), (focal, focal * 1.03, W / 2, H / 2)


def _draw(s, step):
    N, dev, rgba = s.n_rays, s.poses.device, s.channels == 4
    ctr = torch.full((1,), step, dtype=torch.int32, device=dev)
    o, d, gt, bg = (torch.full((N, 3), float("nan"), device=dev) for _ in range(4))
    inds = torch.full((N,), -1, dtype=torch.int64, device=dev)
    pose = torch.full((1,), -1, dtype=torch.int32, device=dev)
    keys = torch.full((s.error_grid ** 2,), float("nan"), device=dev) if s.error_map is not None else None
    if s.error_map is not None:
        s.inds_coarse.fill_(-1)
    s.sample_into(ctr, o, d, gt, inds, pose, keys_out=keys, **({"bg": bg} if rgba else {}))
    return dict(o=o, d=d, gt=gt, bg=bg, inds=inds, pose=int(pose), keys=keys, coarse=None if s.error_map is None else s.inds_coarse.clone())


@pytest.mark.parametrize("G", [None, 4, 32], ids=["uniform", "map4", "map32"])
@pytest.mark.parametrize("N", [5, 256])
def test_rgba_samplers_draw_like_their_twins_and_blend_like_the_kernel(G, N):
    from nerf_signature_amd import rays
    P, H, W, stride, offset = 3, 60, 80, 2, 1
    poses, rgba, intr = _store(P, H, W)
    if G is not None and N > G * G:     # a draw without replacement cannot take 256 of 16 cells: refused like the 3-channel twin's, then all 16 -- the edge of the selection
        with pytest.raises(ValueError, match="without replacement"):
            rays.DeviceRaySampler(poses, rgba, intr, H, W, N, seed=SEED, error_map=True, error_grid=G)
        N = G * G
    rgb = rgba[..., :3].contiguous()
    kw = dict(stride=stride, offset=offset, seed=SEED)
    if G is not None:
        emap = (torch.rand(P, G * G, generator=torch.Generator().manual_seed(G)) + 0.01).cuda()
        kw.update(error_map=emap, error_grid=G)
    s4, s3 = rays.DeviceRaySampler(poses, rgba, intr, H, W, N, **kw), rays.DeviceRaySampler(poses, rgb, intr, H, W, N, **kw)
    assert (s4.channels, s3.channels) == (4, 3) and tuple(s4.images.shape) == (P, H * W, 4)
    for step in (0, 7):
        a, b = _draw(s4, step), _draw(s3, step)
        assert a["pose"] == b["pose"] == (step * stride + offset) % P
        for key in ("o", "d", "inds") + (("coarse", "keys") if G is not None else ()):
            assert torch.equal(a[key], b[key]), (key, step)
        assert int(a["inds"].min()) >= 0 and int(a["inds"].max()) < H * W
        assert torch.equal(b["gt"], rgb[b["pose"]][b["inds"]])
        bg, gt = _blend(rgba[a["pose"]][a["inds"]].contiguous(), step)
        assert torch.equal(a["bg"], bg) and torch.equal(a["gt"], gt), step
        assert np.array_equal(a["bg"].cpu().numpy(), rb.background(N, SEED, step))
    # the background belongs to an RGBA store, and only to one
    buf = lambda: torch.empty(N, 3, device="cuda")
    with pytest.raises(ValueError, match="bg="):
        s4.sample_into(None, buf(), buf(), buf())
    with pytest.raises(ValueError, match="RGBA store"):
        s3.sample_into(None, buf(), buf(), buf(), bg=buf())
    with pytest.raises(ValueError):
        s4.sample_into(None, buf(), buf(), buf(), bg=torch.empty(N, 4, device="cuda"))
    with pytest.raises(ValueError, match="RGB or RGBA"):
        rays.DeviceRaySampler(poses, torch.rand(P, H * W, 2).cuda(), intr, H, W, N)


# ---- the eager step
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


def _patch_rays(n_side=16, seed=2, lo=184):
    """n_side x n_side pixels through the middle of the ball (test_gpu_stage1.py's patch)."""
    pose, intr, _ = cf.orbit_rays(1, seed=seed)
    rr, cc = np.meshgrid(np.arange(lo, lo + n_side), np.arange(lo, lo + n_side), indexing="ij")
    inds = torch.from_numpy((rr * 400 + cc).reshape(-1).astype(np.int64))
    o, d = fr.get_rays(torch.from_numpy(pose)[None], intr, 400, 400, inds[None])
    return o[0].contiguous().cuda(), d[0].contiguous().cuda()


def _rgba_targets(n=256, seed=6):
    """The patch's colour under a random alpha in (0.75, 1].  Why not U[0,1): the patch's rays cross the middle of the opaque ball (density 100 over a chord of ~1: the
    transmittance behind it is zero), so no render can show them their background, and the term bg * (1 - a) of their target is noise to the fit, with variance
    E(1 - a)^2 / 12 per channel.  For a ~ U[0,1) that is 1/36 = 2.8e-2 -- as large as the squared distance between an untrained colour (~0.5) and the target (0.2, 0.5, 0.8),
    1.5e-2 -- and the 'loss falls below 0.7 of its start' clause taken over from test_captured_loop_equals_the_eager_loop would measure that floor, not the loop; for
    1 - a ~ U[0, 0.25) it is 1/576 = 1.7e-3, a tenth of it.  Every ray still has a fractional alpha, so both sides of the blend are in every loss value and gradient
    that the two loops are compared by (the per-ray background of the compositing weighs in where rays are not opaque: the sampler tests below)."""
    alpha = 1.0 - 0.25 * torch.rand(n, 1, generator=torch.Generator().manual_seed(seed))
    return torch.cat([torch.tensor([0.2, 0.5, 0.8]).view(1, 3).expand(n, 3), alpha], dim=-1).contiguous().cuda()


def test_eager_step_is_the_reference_sequence():
    """stage1.train_step on [1,N,4] images against the same sequence written out: seed, rand_like, blend, render against that background, MSE -- loss and all 18
    gradients equal, data['images'] untouched; data['bg_color'] replaces the draw; eval_step against the white blend and a staged render."""
    from nerf_signature_amd import stage1
    o, d = _patch_rays()
    images = _rgba_targets()[None]
    kept = images.clone()
    m = _clean_model()
    data = {"rays_o": o[None], "rays_d": d[None], "images": images, "perturb": False, "force_all_rays": True}

    def by_hand(bg):
        gt = images[..., :3] * images[..., 3:] + bg * (1 - images[..., 3:])
        out = m.render(o[None], d[None], None, staged=False, bg_color=bg, perturb=False, force_all_rays=True, **KW)
        return out["image"], ((out["image"] - gt) ** 2).mean(-1).mean()

    def grads(loss):
        m.zero_grad(set_to_none=True)
        loss.backward()
        return [p.grad.detach().clone() for p in m.trainable()]

    torch.manual_seed(5)
    image0, loss0 = by_hand(torch.rand_like(images[..., :3]))
    g0 = grads(loss0)
    torch.manual_seed(5)
    image1, loss1 = stage1.train_step(m, data, KW)
    g1 = grads(loss1)
    assert torch.equal(images, kept) and data["images"] is images
    assert len(g0) == len(g1) == 18 and float(loss0) == float(loss1) and torch.equal(image0, image1)
    for a, b in zip(g1, g0):
        assert torch.equal(a, b)
    assert float(sum(g.abs().sum() for g in g1[16:])) > 0
    # the caller's background: that tensor, not a draw
    bg = torch.from_numpy(rb.background(256, SEED, 3)).cuda()[None]
    image2, loss2 = by_hand(bg)
    g2 = grads(loss2)
    torch.manual_seed(5)
    image3, loss3 = stage1.train_step(m, dict(data, bg_color=bg), KW)
    g3 = grads(loss3)
    assert float(loss2) == float(loss3) != float(loss1) and torch.equal(image2, image3)
    for a, b in zip(g3, g2):
        assert torch.equal(a, b)
    # RGB ground truth keeps its white background
    rgb = images[..., :3].contiguous()
    _, loss4 = stage1.train_step(m, dict(data, images=rgb), KW)
    out = m.render(o[None], d[None], None, staged=False, bg_color=1, perturb=False, force_all_rays=True, **KW)
    assert float(loss4) == float(((out["image"] - rgb) ** 2).mean(-1).mean())
    m.zero_grad(set_to_none=True)
    # eval_step: [B,H,W,4] against white, staged, unperturbed
    m.eval()
    view = images.view(1, 16, 16, 4)
    pred, depth, gt, loss = stage1.eval_step(m, {"rays_o": o[None], "rays_d": d[None], "images": view}, KW)
    want_gt = view[..., :3] * view[..., 3:] + 1 * (1 - view[..., 3:])
    with torch.no_grad():
        want = m.render(o[None], d[None], None, staged=True, bg_color=1, perturb=False, **KW)
    assert tuple(pred.shape) == (1, 16, 16, 3) and tuple(depth.shape) == (1, 16, 16) and not loss.requires_grad
    assert torch.equal(gt, want_gt) and torch.equal(pred, want["image"].reshape(1, 16, 16, 3)) and torch.equal(depth, want["depth"].reshape(1, 16, 16))
    assert float(loss) == float(((want["image"].reshape(1, 16, 16, 3) - want_gt) ** 2).mean())
    assert torch.equal(images, kept)
    _, _, gt3, _ = stage1.eval_step(m, {"rays_o": o[None], "rays_d": d[None], "images": view[..., :3].contiguous()}, KW)
    assert torch.equal(gt3, view[..., :3])


# ---- the captured loop, batches handed in
def test_captured_rgba_data_path_equals_the_eager_loop():
    """test_captured_loop_equals_the_eager_loop (test_gpu_stage1.py) on RGBA targets with random alpha: 256 patch rays, 5 steps, perturb=False.  The captured loop draws its
    backgrounds from (seed, step) on the device; the eager loop is handed the mirror's values of the same (seed, step k) as data['bg_color'].  That test's criteria."""
    from nerf_signature_amd.stage1 import CleanLoop, GraphedCleanLoop
    o, d = _patch_rays()
    target = _rgba_targets()
    data = {"rays_o": o[None], "rays_d": d[None], "images": target[None], "perturb": False, "force_all_rays": True}
    m0 = _clean_model()
    eager = CleanLoop(m0, _adam(m0), KW, update_extra_interval=10 ** 9)
    eager.global_step = 1
    l0 = [float(eager.step(dict(data, bg_color=torch.from_numpy(rb.background(256, SEED, k)).cuda()[None]))[1].detach()) for k in range(5)]
    m1 = _clean_model()
    loop = GraphedCleanLoop(m1, _adam(m1), KW, n_rays=256, update_extra_interval=0, perturb=False, rgba=True, seed=SEED)
    assert loop.rgba and tuple(loop.bg.shape) == (256, 3) and loop.bg_stride == 3
    l1 = [float(loop.step(data)) for _ in range(5)]
    print(f"\neager losses {l0}\ncaptured losses {l1}")
    assert len(loop.graph.segments) == 1 and not loop.overflowed()
    assert np.array_equal(loop.bg.cpu().numpy(), rb.background(256, SEED, 4))
    assert np.array_equal(loop.gt.cpu().numpy(), rb.blend(target.cpu().numpy(), rb.background(256, SEED, 4)))
    np.testing.assert_allclose(l1, l0, rtol=2e-4)
    assert l0[-1] < 0.7 * l0[0]
    for i, (a, b) in enumerate(zip(m1.trainable(), m0.trainable())):
        diff = (a - b).detach().abs()
        frac, worst = float((diff > 2e-5).float().mean()), float(diff.max())
        assert (frac < 5e-4 and worst < 3e-2) if i < 16 else worst < 1e-4, (i, frac, worst)
    assert loop.losses() == pytest.approx(l1, rel=1e-6)
    with pytest.raises(ValueError, match="256 x 4"):
        loop.step(dict(data, images=target[None, :, :3].contiguous()))
    loop.close()


# ---- the captured loop with an RGBA sampler
_SCENE = {}


def _rgba_ball_views(P=24, H=64, W=64, radius=0.3):
    """P orbit views (test_gpu_error_map.py's _ball_views) as RGBA: alpha 1 and the target colour where a pixel's ray meets a ball of `radius`, alpha 0 over black
    elsewhere.  The occupancy grid's ball (cf.ball_scene) has radius 0.5: rays through the annulus cross occupied cells while their ground truth is transparent."""
    if not _SCENE:
        from nerf_signature_amd import rays
        focal = 555.56 * W / 400
        intr = (focal, focal, W / 2, H / 2)
        poses = torch.stack([torch.from_numpy(cf.orbit_rays(1, seed=0, radius=3.0 + 0.02 * k)[0]) for k in range(P)]).cuda()
        held = torch.from_numpy(cf.orbit_rays(1, seed=0, radius=3.25)[0]).cuda()[None]

        def hits(ps, r):
            g = rays.get_rays(ps, intr, H, W, N=-1)
            o, d = g["rays_o"], g["rays_d"]
            b = (o * d).sum(-1)
            return o, d, b * b - ((o * o).sum(-1) - r * r) >= 0

        _, _, hit = hits(poses, radius)
        colour = torch.tensor([0.2, 0.5, 0.8, 1.0], device="cuda")
        images = torch.where(hit[..., None], colour, torch.zeros(4, device="cuda")).contiguous()
        assert 0.02 < float(hit.float().mean()) < 0.5
        o, d, inner = hits(held, radius)
        _, _, outer = hits(held, 0.5)
        _SCENE.update(poses=poses, images=images, intr=intr, H=H, W=W, P=P, held_o=o[0], held_d=d[0], held_inner=inner[0], held_annulus=outer[0] & ~inner[0])
    return _SCENE


def _sampler_loop(capture, error_map, n_rays=256, images=None, **kw):
    from nerf_signature_amd import rays
    from nerf_signature_amd.stage1 import GraphedCleanLoop
    v = _rgba_ball_views()
    m = _clean_model()
    s = rays.DeviceRaySampler(v["poses"], v["images"] if images is None else images, v["intr"], v["H"], v["W"], n_rays, seed=SEED, error_map=error_map, error_grid=32)
    torch.manual_seed(11)           # (the first step's march offsets come from torch's generator)
    return m, s, GraphedCleanLoop(m, _adam(m), KW, n_rays=n_rays, sampler=s, update_extra_interval=0, perturb=True, seed=3, capture=capture, **kw)


def _hip_runtime():
    """The HIP runtime this process has loaded (torch's), by the path it was mapped from."""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return ctypes.CDLL(line.split()[-1])
    raise RuntimeError("libamdhip64 is not mapped into this process")


def _graph_nodes(loop):
    """Nodes of one captured step: loop._whole_step captured once more into a graph that keeps its hipGraph_t (never replayed: a capture runs nothing)."""
    loop.prepare()
    g = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        loop._whole_step()
    n = ctypes.c_size_t(0)
    hip = _hip_runtime()
    hip.hipGraphGetNodes.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_size_t)]
    assert hip.hipGraphGetNodes(ctypes.c_void_p(g.raw_cuda_graph()), None, ctypes.byref(n)) == 0
    return int(n.value)


@pytest.mark.parametrize("error_map", [False, True], ids=["uniform", "error_map"])
def test_captured_rgba_sampler_loop_equals_the_eager_sequence(error_map):
    """20 steps of GraphedCleanLoop with an RGBA sampler: captured, the same launches issued eagerly, and the three-launch compositing route -- parameters, losses, the
    error map and the step count bit for bit; one captured segment, no overflow; the loop's backgrounds after the last step are the mirror's of step 19; the ground truth
    is the blend of the pixels drawn against them.  Once (uniform): the captured step has as many graph nodes as the RGB step."""
    got = {}
    for name, capture, kw in (("captured", True, {}), ("eager", False, {}), ("three_launch", True, {"fused_composite": False})):
        m, s, loop = _sampler_loop(capture, error_map, **kw)
        assert loop.rgba and s.channels == 4 and loop.bg_stride == 3 and loop.rgba_px is None
        for _ in range(20):
            loop.step()
        torch.cuda.synchronize()
        assert not loop.overflowed() and (len(loop.graph.segments) == 1 or not capture)
        got[name] = ([p.detach().clone() for p in m.trainable()], loop.losses(), None if s.error_map is None else s.error_map.clone(), int(loop.step_dev),
                     loop.bg.clone(), loop.gt.clone())
        loop.close()
    a = got["captured"]
    for name in ("eager", "three_launch"):
        b = got[name]
        assert a[3] == b[3] == 20 and a[1] == b[1] and len(a[1]) == 20, name
        for x, y in zip(a[0], b[0]):
            assert torch.equal(x, y), name
        assert error_map is False or torch.equal(a[2], b[2]), name
        assert torch.equal(a[4], b[4]) and torch.equal(a[5], b[5]), name
    assert np.isfinite(a[1]).all()
    want_bg = rb.background(256, SEED, 19)
    assert np.array_equal(a[4].cpu().numpy(), want_bg)
    # the last step's target: the drawn pixels under the mirror's backgrounds
    v = _rgba_ball_views()
    from nerf_signature_amd import rays
    probe = rays.DeviceRaySampler(v["poses"], v["images"], v["intr"], v["H"], v["W"], 256, seed=SEED, error_map=error_map, error_grid=32)
    if not error_map:               # (a map's draw of step 19 depends on the map the 19 steps before it wrote)
        drawn = _draw(probe, 19)
        assert torch.equal(drawn["gt"], a[5]) and np.array_equal(a[5].cpu().numpy(), rb.blend(v["images"][19][drawn["inds"]].cpu().numpy(), want_bg))
        # launch count: the blend rides in the sampler's launch
        _, _, rgb_loop = _sampler_loop(True, False, images=v["images"][..., :3].contiguous())
        _, _, rgba_loop = _sampler_loop(True, False)
        assert not rgb_loop.rgba and tuple(rgb_loop.bg.shape) == (3,) and rgb_loop.bg_stride == 0
        n_rgb, n_rgba = _graph_nodes(rgb_loop), _graph_nodes(rgba_loop)
        print(f"\ngraph nodes of one captured step: RGB sampler {n_rgb}, RGBA sampler {n_rgba}")
        assert n_rgb == n_rgba and n_rgb > 5
        rgb_loop.close()
        rgba_loop.close()
    with pytest.raises(ValueError, match="rgba=False"):
        _sampler_loop(False, False, rgba=False)


def _opacity(m, v):
    """Mean weights_sum of the held view's annulus rays and of its alpha = 1 rays: the eval-mode march (unperturbed) of the whole view."""
    from nerf_signature_amd import raymarching
    was_training = m.training
    m.eval()
    with torch.no_grad():
        o, d = v["held_o"].contiguous(), v["held_d"].contiguous()
        nears, fars = raymarching.near_far_from_aabb(o, d, m.aabb_infer, m.min_near)
        ws, _, _ = m._march_and_composite_eval(o, d, None, nears, fars, 0, False, 1024, 1e-4)
    m.train(was_training)
    return float(ws[v["held_annulus"]].mean()), float(ws[v["held_inner"]].mean())


def test_rgba_training_teaches_opacity():
    """200 captured steps on the RGBA ball views (alpha 1 inside radius 0.3; the occupancy grid's ball has radius 0.5 and is never refreshed): the loss falls, no step
    overflows, and the field's opacity along the annulus rays of a held pose -- occupied cells, transparent ground truth: only a random background tells an empty
    pixel from a coloured one -- falls, and ends below the opacity of the alpha = 1 rays.  Directions the loss dictates, not thresholds; the three means are printed."""
    v = _rgba_ball_views()
    assert int(v["held_annulus"].sum()) > 50 and int(v["held_inner"].sum()) > 50
    m, s, loop = _sampler_loop(True, False, n_rays=1024)
    annulus_before, inner_before = _opacity(m, v)
    for _ in range(200):
        loop.step()
    losses = loop.losses()
    first, last = float(np.mean(losses[:50])), float(np.mean(losses[-50:]))
    annulus_after, inner_after = _opacity(m, v)
    print(f"\nmean loss of steps 0..49: {first:.4e}, of steps 150..199: {last:.4e}")
    print(f"mean weights_sum, held pose: annulus before {annulus_before:.4f}, annulus after {annulus_after:.4f}, alpha = 1 rays after {inner_after:.4f} (before {inner_before:.4f})")
    assert len(losses) == 200 and np.isfinite(losses).all()
    assert last < first
    assert not loop.overflowed()
    assert annulus_after < annulus_before
    assert annulus_after < inner_after
    loop.close()
