#!/usr/bin/env python
"""What the clean twin costs and what it saves.

    python tools/twin_bench.py [--steps K] [--windows W] [--poses P] [--size S] [--json PATH]

1. The captured watermark step at bench size (quality.watermark_stage: scene S0, 4096 content rays) with an OrbitRaySampler and the target rendered inside the
   step, against the same step with a DeviceRaySampler store (poses + pre-rendered clean views: the step as it was), in alternating windows of K steps in one
   process; points per content render beside the times (another camera every step marches another number of points).
2. The pre-pass the online step does without: blocks.clean_render over P poses at S x S (the Blender scenes: 100 views of 800 x 800), wall time and the bytes of
   the image store it fills.
3. field_fwd_twin against field_fwd on the 0.125 M content points of one step, each as a captured chain replayed between two events (launch gap included), in
   every arithmetic / plane layout / loop the twin has."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from nerf_signature_amd import _native as nv, blocks, fieldops as fo, quality, rays, synthetic, trainer
from nerf_signature_amd.optim import CodebookAdam


def flag(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


steps, windows, n_poses, size, out_path = flag("--steps", 256), flag("--windows", 5), flag("--poses", 100), flag("--size", 800), flag("--json", "")
dev = torch.device("cuda")
result = {"device": torch.cuda.get_device_name(0)}

# ---- 1. the captured step, online targets against the store
loops = {}
for name, online in (("store", False), ("orbit_online", True)):
    stage = quality.watermark_stage("hotdog", online_targets=online)
    model, D, kw, H, W, n_rays = stage["model"], stage["D"], stage["render_kwargs"], stage["H"], stage["W"], stage["n_rays"]
    if online:
        sampler = rays.OrbitRaySampler(stage["intr"], H, W, n_rays, stage["radius"], quality.ORBIT_THETA, (0.0, 2 * np.pi), seed=1000, device=dev)
    else:
        sampler = rays.DeviceRaySampler(stage["poses"], stage["clean"], stage["intr"], H, W, n_rays, seed=1000)
    content = {k: torch.empty(1, n_rays, 3, dtype=torch.float32, device=dev) for k in (("rays_o", "rays_d") if online else ("rays_o", "rays_d", "images"))}
    sampler.sample_into(torch.zeros(1, dtype=torch.int32, device=dev), content["rays_o"], content["rays_d"], content.get("images"))
    data = {"watermark": {"rays_o_block": stage["block_o"], "rays_d_block": stage["block_d"]}, "content": content}
    opt = CodebookAdam(model.get_params(quality.README["lr"]), betas=(0.9, 0.99), eps=1e-15, fused=True, capturable=True)
    loop = trainer.GraphedWatermarkLoop(model, opt, kw, data, lambda_w=quality.README["lambda_w"], lambda_i=quality.README["lambda_i"], content_headroom=0.25,
                                        content_sampler=sampler)
    msgs = quality.messages(D, 64)
    loop.prepare(msgs[0])
    for k in range(32):
        loop.step(msgs[k % 63], next_message=msgs[k % 63 + 1])
    loops[name] = (loop, msgs, stage)
torch.cuda.synchronize()
win = {k: [] for k in loops}
for w in range(windows):
    for name, (loop, msgs, _) in loops.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for k in range(steps):
            loop.step(msgs[k % 63], next_message=msgs[k % 63 + 1])
        e1.record()
        torch.cuda.synchronize()
        win[name].append({"ms_per_step": e0.elapsed_time(e1) / steps, "content_points": loop.point_counts()[1], "overflowed": bool(loop.overflowed())})
result["captured_step"] = {k: {"ms_per_step": float(np.median([x["ms_per_step"] for x in v])), "windows": v} for k, v in win.items()}
for k, v in result["captured_step"].items():
    print(f"captured step, {k:13s}: median {v['ms_per_step']:.4f} ms/step over {windows} windows x {steps} steps; per window (ms, content points, overflow): "
          + ", ".join(f"{x['ms_per_step']:.4f} / {x['content_points']} / {int(x['overflowed'])}" for x in v["windows"]))
a, b = result["captured_step"]["store"]["ms_per_step"], result["captured_step"]["orbit_online"]["ms_per_step"]
print(f"online targets / store: {b / a:.4f}")

# ---- 2. the pre-pass
stage = loops["store"][2]
model, cfg = stage["model"], synthetic.SCENES["hotdog"]
for loop, _, _ in loops.values():
    loop.close()
scale = size / cfg["W"]
intr = (cfg["focal"] * scale, cfg["focal"] * scale, size / 2, size / 2)
prng = np.random.RandomState(78)
poses = torch.from_numpy(np.stack([synthetic.orbit_pose(0.6 + 0.9 * prng.rand(), 2 * np.pi * prng.rand(), cfg["radius"]) for _ in range(n_poses)])).to(dev)
with torch.no_grad():
    blocks.clean_render(model, poses[:2], intr, size, size, stage["render_kwargs"])        # (modules loaded, allocator warm)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    store = blocks.clean_render(model, poses, intr, size, size, stage["render_kwargs"])
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
result["prepass"] = {"poses": n_poses, "size": size, "wall_s": wall, "ms_per_view": wall / n_poses * 1e3, "store_bytes": store.numel() * 4}
print(f"clean_render pre-pass: {n_poses} poses at {size} x {size}: {wall:.3f} s ({wall / n_poses * 1e3:.2f} ms per view), image store {store.numel() * 4 / 2 ** 20:.0f} MiB")
del store

# ---- 3. the launch alone
M = 125000
base = [t.detach() for t in model.encoder.tables()]
tables = model.msg_encoder.tables()
S = fo.codebook_presum(fo.select_tables([t.detach() for t in tables], tuple(int(v) for v in quality.messages(stage["D"], 1)[0])))
pts = (torch.rand(M, 3, device=dev) * 2 - 1) * cfg["bound"] * 0.5
dirs = torch.nn.functional.normalize(torch.randn(M, 3, device=dev), dim=-1)
base_ptrs = nv.ptr_array(base)
sig, rgb, sig_c, rgb_c = torch.empty(M, device=dev), torch.empty(M, 3, device=dev), torch.empty(M, device=dev), torch.empty(M, 3, device=dev)
masks = torch.empty((M + 31) // 32 * 32, 6, dtype=torch.int32, device=dev)
ws = torch.empty(int(nv.fn("hg_planes_bytes")(M)), dtype=torch.uint8, device=dev)


def chain_us(fn, launches=32, replays=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(launches):
            fn()
    for _ in range(3):
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
    return float(np.median(out))


prec, pipe = nv.fn("mlp_get_precision")(), nv.fn("mlp_get_pipelined")()
result["launch_us"] = {}
try:
    for arith, half in (("f16", "1"), ("f16", "0"), ("bf16x3", "0")):
        for pipelined in (3, 2):
            os.environ["NERFSIG_HALF_PLANES"] = half
            nv.set_mlp_precision(arith)
            nv.call("mlp_set_pipelined", pipelined)
            packed = model._packed()
            layout = fo.encode_planes(pts, M, cfg["bound"], base_ptrs, S, ws)
            single = chain_us(lambda: nv.call("field_fwd", nv.ptr(pts), nv.ptr(dirs), M, float(cfg["bound"]), base_ptrs, nv.ptr(S), nv.ptr(packed), nv.ptr(sig), nv.ptr(rgb),
                                              None, nv.ptr(masks), nv.ptr(ws), layout, nv.stream()))
            twin = chain_us(lambda: nv.call("field_fwd_twin", nv.ptr(pts), nv.ptr(dirs), M, float(cfg["bound"]), base_ptrs, nv.ptr(S), nv.ptr(packed), nv.ptr(sig),
                                            nv.ptr(rgb), None, nv.ptr(masks), nv.ptr(ws), layout, nv.ptr(sig_c), nv.ptr(rgb_c), nv.stream()))
            key = f"{arith} {'mixed' if layout == fo.PLANES_MIXED else 'f32'} planes, {'pipelined' if pipelined & 1 else 'plain loop'}"
            result["launch_us"][key] = {"field_fwd": single, "field_fwd_twin": twin}
            print(f"{M} points, {key:42s}: field_fwd {single:7.2f} us, field_fwd_twin {twin:7.2f} us ({twin / single:.2f} x)")
finally:
    os.environ.pop("NERFSIG_HALF_PLANES", None)
    nv.call("mlp_set_pipelined", pipe)
    nv.call("mlp_set_precision", prec)
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    json.dump(result, open(out_path, "w"), indent=1)
