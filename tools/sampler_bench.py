#!/usr/bin/env python
"""The device-side loader's two draws, alone and inside the captured stage-1 step (DESIGN.md sections 16 and 17).

    python tools/sampler_bench.py [--steps K] [--windows W] [--train-steps T] [--json PATH]

1. rg_sample_rays (uniform pixels), rg_sample_rays_weighted (N = 4096 of a 128 x 128 error map, without replacement) and rg_error_map_update, each as a
   captured chain of 64 launches replayed between two device events: microseconds per launch, launch gap included (what a launch costs at the head of a step).
2. stage1.GraphedCleanLoop on the bench scene's own (sparse) occupancy grid, 4096 rays drawn inside the step, without a grid refresh: the uniform sampler against
   the map sampler, alternating windows of K steps in one process.  The map also moves the rays to where the error is, so the points per step are reported with
   the times: a step that marches more points takes longer for that reason, not for the launch's.
   RGBA rows: the same store with an alpha channel -- rg_sample_rays_rgba / rg_sample_rays_weighted_rgba and rg_blend_random_background
   next to their RGB twins in part 1, the captured step with an RGBA uniform sampler (a background colour per ray, bg_stride 3) in part 2's alternation.
3. PSNR of a few held-out full views after T more steps of each loop (reported side by side, never asserted: the reference calls the option experimental)."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from nerf_signature_amd import _native as nv, blocks, rays, synthetic
from nerf_signature_amd.stage1 import CleanNeRFNetwork, GraphedCleanLoop


def flag(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


steps, windows, train_steps, out_path = flag("--steps", 256), flag("--windows", 5), flag("--train-steps", 2000), flag("--json", "")
dev = torch.device("cuda")
cfg = synthetic.SCENES["hotdog"]
H, W, N, G, P = cfg["H"], cfg["W"], 4096, 128, 16
intr = (cfg["focal"], cfg["focal"], W / 2, H / 2)
KW = dict(dt_gamma=0, max_steps=1024)
prng = np.random.RandomState(77)
mk = lambda n: torch.from_numpy(np.stack([synthetic.orbit_pose(0.6 + 0.9 * prng.rand(), 2 * np.pi * prng.rand(), cfg["radius"]) for _ in range(n)])).to(dev)
poses, test_poses = mk(P), mk(3)


def views(ps):
    """The ball in one colour on white: every pixel can be learned (the field's density is the occupancy grid's ball)."""
    r = rays.get_rays(ps, intr, H, W, N=-1)
    b = (r["rays_o"] * r["rays_d"]).sum(-1)
    hit = b * b - ((r["rays_o"] ** 2).sum(-1) - 0.25) >= 0
    return torch.where(hit[..., None], torch.tensor([0.2, 0.5, 0.8], device=dev), torch.ones(3, device=dev)).contiguous()


images, test_images = views(poses), views(test_poses)
# the same views as RGBA: the ball opaque, everything else transparent (over black: the white of the RGB store is what the step's backgrounds replace)
images_rgba = torch.cat([images, (images != 1).any(-1, keepdim=True).float()], dim=-1)
images_rgba[..., :3] *= images_rgba[..., 3:]
images_rgba = images_rgba.contiguous()


def fresh_model():
    m = CleanNeRFNetwork(bound=cfg["bound"], cuda_ray=True, density_scale=1, min_near=0.2, density_thresh=10, bg_radius=-1)
    with torch.no_grad():
        for l, e in enumerate(m.encoder.embeddings):
            e.weight.copy_(torch.from_numpy(synthetic.table_values(l, 0.5)))
        grid = synthetic.density_grid(cfg["bound"])
        bits, _ = synthetic.pack_bits_np(grid, 10.0)
        m.density_grid.copy_(torch.from_numpy(grid))
        m.density_bitfield.copy_(torch.from_numpy(bits))
    return m.to(dev).train()


def chain_us(fn, launches=64, replays=50):
    """fn() captured `launches` times in a row, replayed `replays` times between two events: microseconds per launch."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(launches):
            fn()
    for _ in range(5):
        g.replay()
    out = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(replays):
            g.replay()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / (replays * launches) * 1e3)
    return float(np.median(out)), out


# ---- 1. the launches alone
ctr = torch.full((1,), 5, dtype=torch.int32, device=dev)
o, d, gt, pred = (torch.empty(N, 3, device=dev) for _ in range(4))
pred.uniform_()
uniform = rays.DeviceRaySampler(poses, images, intr, H, W, N, seed=1000)
weighted = rays.DeviceRaySampler(poses, images, intr, H, W, N, seed=1000, error_map=torch.rand(P, G * G, device=dev) + 0.01, error_grid=G)
ones = rays.DeviceRaySampler(poses, images, intr, H, W, N, seed=1000, error_map=True, error_grid=G)
uniform4 = rays.DeviceRaySampler(poses, images_rgba, intr, H, W, N, seed=1000)
weighted4 = rays.DeviceRaySampler(poses, images_rgba, intr, H, W, N, seed=1000, error_map=weighted.error_map.clone(), error_grid=G)
bg, px = torch.empty(N, 3, device=dev), torch.rand(N, 4, device=dev)
launch = {"rg_sample_rays": chain_us(lambda: uniform.sample_into(ctr, o, d, gt)),
          "rg_sample_rays_rgba": chain_us(lambda: uniform4.sample_into(ctr, o, d, gt, bg=bg)),
          "rg_sample_rays_weighted (random map)": chain_us(lambda: weighted.sample_into(ctr, o, d, gt)),
          "rg_sample_rays_weighted_rgba (random map)": chain_us(lambda: weighted4.sample_into(ctr, o, d, gt, bg=bg)),
          "rg_blend_random_background": chain_us(lambda: nv.call("rg_blend_random_background", nv.ptr(px), N, nv.ptr(ctr), 1000, nv.ptr(bg), nv.ptr(gt), nv.stream())),
          "rg_sample_rays_weighted (map of ones)": chain_us(lambda: ones.sample_into(ctr, o, d, gt)),
          "rg_error_map_update": chain_us(lambda: weighted.update_error_map(pred, gt))}
for k, (us, all_) in launch.items():
    print(f"{k:42s} {us:7.2f} us per launch in a captured chain of 64 ({', '.join('%.2f' % v for v in all_)})")

# ---- 2. the captured stage-1 step on the sparse grid, both samplers, alternating windows
loops = {}
for name, emap, store in (("uniform", False, images), ("rgba", False, images_rgba), ("error_map", True, images)):
    m = fresh_model()
    s = rays.DeviceRaySampler(poses, store, intr, H, W, N, seed=1000, error_map=emap, error_grid=G)
    torch.manual_seed(0)
    loop = GraphedCleanLoop(m, torch.optim.Adam(m.get_params(1e-2), betas=(0.9, 0.99), eps=1e-15), KW, n_rays=N, sampler=s, update_extra_interval=0, perturb=True)
    for _ in range(32):
        loop.step()
    loops[name] = (m, s, loop)
torch.cuda.synchronize()
win = {k: [] for k in loops}
for w in range(windows):
    for name, (m, s, loop) in loops.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            loop.step()
        e1.record()
        torch.cuda.synchronize()
        win[name].append({"ms_per_step": e0.elapsed_time(e1) / steps, "points_per_step": float(loop.count_ring[:, 0].float().mean()), "recaptures": loop.recaptures})
step = {k: {"ms_per_step": float(np.median([x["ms_per_step"] for x in v])), "windows": v} for k, v in win.items()}
for k, v in step.items():
    print(f"stage-1 captured step, sparse grid, {k:9s}: median {v['ms_per_step']:.4f} ms/step over {windows} windows x {steps} steps; per window (ms, points): "
          + ", ".join(f"{x['ms_per_step']:.4f} / {x['points_per_step']:.0f}" for x in v["windows"]))

# ---- 3. held-out PSNR after an equal number of steps
psnr = {}
for name, (m, s, loop) in loops.items():
    if s.channels == 4:      # (trained towards other targets: its held-out PSNR against the white-background views says nothing about the sampler)
        loop.close()
        continue
    for _ in range(train_steps):
        loop.step()
    torch.cuda.synchronize()
    done = loop.global_step
    with torch.no_grad():
        img = blocks.clean_render(m.eval(), test_poses, intr, H, W, KW, max_ray_batch=H * W).reshape(len(test_poses), H * W, 3).clamp_(0, 1)
        mse = ((img - test_images) ** 2).mean(dim=(1, 2))
    psnr[name] = {"steps": done, "psnr_db": [float(-10 * torch.log10(v)) for v in mse], "overflowed": loop.overflowed(), "loss_last": loop.losses(1)[0]}
    print(f"held-out PSNR after {done} steps, {name:9s}: " + ", ".join("%.2f" % v for v in psnr[name]["psnr_db"]) + f" dB (mean {np.mean(psnr[name]['psnr_db']):.2f}); last loss {psnr[name]['loss_last']:.3e}")
    loop.close()
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    json.dump({"rays": N, "grid": G, "poses": P, "image": [H, W], "launch_us": {k: {"median": v[0], "runs": v[1]} for k, v in launch.items()}, "stage1_step": step,
               "heldout_psnr": psnr}, open(out_path, "w"), indent=1)
