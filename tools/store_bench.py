#!/usr/bin/env python
"""The u8 image store against the float store: bytes, the sampler's launch, the captured stage-1 step.

    python tools/store_bench.py [--steps K] [--windows W] [--json PATH]

1. Store bytes of a Blender scene, 100 x 800 x 800 RGBA: float32 against uint8 (arithmetic; the stores below hold 16 poses).
2. rg_sample_rays / _rgba (float store) against rg_sample_rays_u8 over the same pixels as uint8 -- RGB, RGBA, RGBA with a decode table, and the error-map draw --
   at 4096 rays on 800 x 800 images, each as a captured chain of 64 launches replayed between two device events (tools/sampler_bench.py's chain_us): microseconds
   per launch, launch gap included.
3. stage1.GraphedCleanLoop on the bench scene's occupancy grid, 4096 rays drawn inside the step: a u8 store against its float twin (dataset.decode_u8 of the same
   bytes: the two loops draw the same batches and march the same points, bit for bit), RGB and RGBA, alternating windows of K steps in one process.  The bar: the
   median u8 step is no slower than the median float step by more than the float step's own window-to-window spread (max - min) in this run."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from nerf_signature_amd import rays, synthetic
from nerf_signature_amd.dataset import decode_u8
from nerf_signature_amd.stage1 import CleanNeRFNetwork, GraphedCleanLoop


def flag(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


steps, windows, out_path = flag("--steps", 256), flag("--windows", 7), flag("--json", "")
dev = torch.device("cuda")
cfg = synthetic.SCENES["hotdog"]
H, W, N, G, P = cfg["H"], cfg["W"], 4096, 128, 16
intr = (cfg["focal"], cfg["focal"], W / 2, H / 2)
KW = dict(dt_gamma=0, max_steps=1024)
prng = np.random.RandomState(77)
poses = torch.from_numpy(np.stack([synthetic.orbit_pose(0.6 + 0.9 * prng.rand(), 2 * np.pi * prng.rand(), cfg["radius"]) for _ in range(P)])).to(dev)

# ---- 1. bytes
scene_px = 100 * 800 * 800
store_bytes = {"float32 RGBA": scene_px * 16, "uint8 RGBA": scene_px * 4, "float32 RGB": scene_px * 12, "uint8 RGB": scene_px * 3}
for k, v in store_bytes.items():
    print(f"store of 100 x 800 x 800 {k:13s}: {v / 1e6:7.1f} MB")

# the views of tools/sampler_bench.py (the ball in one colour, opaque; everything else transparent), with a soft rim so that alpha takes fractions, as uint8
r = rays.get_rays(poses, intr, H, W, N=-1)
b = (r["rays_o"] * r["rays_d"]).sum(-1)
disc = b * b - ((r["rays_o"] ** 2).sum(-1) - 0.25)
alpha = (disc * 40).clamp(0, 1)
rgba_u8 = (torch.cat([torch.tensor([0.2, 0.5, 0.8], device=dev) * alpha[..., None], alpha[..., None]], dim=-1) * 255).round().to(torch.uint8).contiguous()
rgb_u8 = rgba_u8[..., :3].contiguous()
del r, b, disc, alpha
stores = {"rgb float": decode_u8(rgb_u8), "rgb u8": rgb_u8, "rgba float": decode_u8(rgba_u8), "rgba u8": rgba_u8}


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
    for _ in range(7):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(replays):
            g.replay()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / (replays * launches) * 1e3)
    return float(np.median(out)), out


# ---- 2. the launches alone
ctr = torch.full((1,), 5, dtype=torch.int32, device=dev)
o, d, gt, bg = (torch.empty(N, 3, device=dev) for _ in range(4))
emap = torch.rand(P, G * G, device=dev) + 0.01
table = decode_u8(torch.arange(256, dtype=torch.uint8, device=dev)) ** 2.2
launch = {}
for name, store in stores.items():
    kw = {"bg": bg} if store.shape[-1] == 4 else {}
    s = rays.DeviceRaySampler(poses, store, intr, H, W, N, seed=1000)
    launch[f"uniform, {name}"] = chain_us(lambda: s.sample_into(ctr, o, d, gt, **kw))
    if store.dtype == torch.uint8:
        t = rays.DeviceRaySampler(poses, store, intr, H, W, N, seed=1000, decode=table)
        launch[f"uniform, {name} + decode table"] = chain_us(lambda: t.sample_into(ctr, o, d, gt, **kw))
    m = rays.DeviceRaySampler(poses, store, intr, H, W, N, seed=1000, error_map=emap.clone(), error_grid=G)
    launch[f"error map, {name}"] = chain_us(lambda: m.sample_into(ctr, o, d, gt, **kw))
for k, (us, all_) in launch.items():
    print(f"{k:34s} {us:7.2f} us per launch in a captured chain of 64 ({', '.join('%.2f' % v for v in all_)})")


# ---- 3. the captured stage-1 step, u8 against float, alternating windows
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


loops = {}
for name, store in stores.items():
    m = fresh_model()
    s = rays.DeviceRaySampler(poses, store, intr, H, W, N, seed=1000)
    torch.manual_seed(0)
    loop = GraphedCleanLoop(m, torch.optim.Adam(m.get_params(1e-2), betas=(0.9, 0.99), eps=1e-15), KW, n_rays=N, sampler=s, update_extra_interval=0, perturb=True)
    for _ in range(32):
        loop.step()
    loops[name] = loop
torch.cuda.synchronize()
win = {k: [] for k in loops}
for w in range(windows):
    for name, loop in loops.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            loop.step()
        e1.record()
        torch.cuda.synchronize()
        win[name].append({"ms_per_step": e0.elapsed_time(e1) / steps, "points_per_step": float(loop.count_ring[:, 0].float().mean())})
step = {}
for k, v in win.items():
    ms = [x["ms_per_step"] for x in v]
    step[k] = {"ms_per_step": float(np.median(ms)), "spread_ms": float(max(ms) - min(ms)), "windows": v}
    print(f"stage-1 captured step, {k:10s}: median {step[k]['ms_per_step']:.4f} ms/step, spread {step[k]['spread_ms']:.4f} ms over {windows} windows x {steps} steps; "
          "per window (ms, points): " + ", ".join(f"{x['ms_per_step']:.4f} / {x['points_per_step']:.0f}" for x in v))
verdict = {}
for c in ("rgb", "rgba"):
    f, u = step[f"{c} float"], step[f"{c} u8"]
    verdict[c] = {"u8_minus_float_ms": u["ms_per_step"] - f["ms_per_step"], "float_spread_ms": f["spread_ms"], "within_spread": u["ms_per_step"] - f["ms_per_step"] <= f["spread_ms"]}
    print(f"{c:4s}: u8 - float = {verdict[c]['u8_minus_float_ms'] * 1e3:+.2f} us per step; the float step's spread in this run: {f['spread_ms'] * 1e3:.2f} us -> "
          + ("within it" if verdict[c]["within_spread"] else "SLOWER than the spread"))
    same = all(torch.equal(a, b) for a, b in zip(loops[f"{c} float"].model.trainable(), loops[f"{c} u8"].model.trainable()))
    print(f"{c:4s}: the two loops' parameters after {loops[c + ' u8'].global_step} steps are {'bit-equal' if same else 'DIFFERENT'}")
    verdict[c]["parameters_equal"] = same
for loop in loops.values():
    loop.close()
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    json.dump({"rays": N, "grid": G, "poses": P, "image": [H, W], "store_bytes_100x800x800": store_bytes, "launch_us": {k: {"median": v[0], "runs": v[1]} for k, v in launch.items()},
               "stage1_step": step, "verdict": verdict}, open(out_path, "w"), indent=1)
