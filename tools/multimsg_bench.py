#!/usr/bin/env python
"""What rendering one set of rays under K messages in a single field pass saves.

    python tools/multimsg_bench.py [--messages N] [--batch B] [--repeats R] [--json PATH]

On the bench scene (quality.watermark_stage("hotdog"): the watermark-block rays, D = 32), everything in one process, A and B alternating, medians over R repeats:
(a) quality.test_bitacc over N messages: today's loop (one render per message -- the unchanged sequential path) against message_batch=B, with the block rays
    declared constant (fix_rays) and without; the two must return the same numbers;
(b) one full view, staged=True, under 16 messages against 16 staged renders;
(c) each new launch against its single-message counterpart at the block render's points, as captured chains replayed between two events, K in {1, 2, 4, 8, 16}:
    hg_codebook_presum_multi / hg_codebook_presum_sel, hg_encode_codebook_planes_multi / hg_encode_codebook_plane, field_fwd_multi / field_fwd over planes."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from nerf_signature_amd import _native as nv, fieldops as fo, quality, rays


def flag(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


n_messages, batch, repeats, out_path = flag("--messages", 200), flag("--batch", 16), flag("--repeats", 5), flag("--json", "")
dev = torch.device("cuda")
result = {"device": torch.cuda.get_device_name(0), "messages": n_messages, "batch": batch, "repeats": repeats}
stage = quality.watermark_stage("hotdog", n_poses=1, n_test_poses=1)
model, D, kw, H, W = stage["model"], stage["D"], stage["render_kwargs"], stage["H"], stage["W"]


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


# ---- (a) test_bitacc
result["bitacc"] = {}
for fixed in (False, True):
    if fixed:
        model.fix_rays(stage["block_o"], stage["block_d"], kw["dt_gamma"], kw["max_steps"])
    variants = {"loop": lambda: quality.test_bitacc(stage, n_messages=n_messages), f"batch_{batch}": lambda: quality.test_bitacc(stage, n_messages=n_messages, message_batch=batch)}
    times, numbers = {k: [] for k in variants}, {}
    for r in range(repeats + 1):          # (the first round warms modules and the allocator; not counted)
        for name, fn in variants.items():
            t, numbers[name] = wall(fn)
            if r:
                times[name].append(t)
    key = "fix_rays" if fixed else "marched_per_render"
    a, b = float(np.median(times["loop"])), float(np.median(times[f"batch_{batch}"]))
    result["bitacc"][key] = {"loop_s": a, "batched_s": b, "speedup": a / b, "loop_all_s": times["loop"], "batched_all_s": times[f"batch_{batch}"],
                             "same_numbers": numbers["loop"] == numbers[f"batch_{batch}"], "numbers": numbers["loop"]}
    print(f"(a) test_bitacc, {n_messages} messages, block rays {key:18s}: loop {a * 1e3:8.1f} ms, message_batch={batch} {b * 1e3:8.1f} ms ({a / b:.2f} x); "
          f"same numbers: {numbers['loop'] == numbers[f'batch_{batch}']}; per repeat (ms) loop " + " ".join(f"{t * 1e3:.1f}" for t in times["loop"])
          + " | batched " + " ".join(f"{t * 1e3:.1f}" for t in times[f"batch_{batch}"]))
rec = model.get_marched(stage["block_o"].view(-1, 3), stage["block_d"].view(-1, 3))
M = int(rec.counter[0])
pts, dirs = rec.xyzs[:M].clone(), rec.dirs[:M].clone()
model.drop_marched()

# ---- (b) one staged view under 16 messages
r = rays.get_rays(stage["test_poses"][0:1], stage["intr"], H, W, -1)
gen = torch.Generator(device="cpu").manual_seed(5)
msgs = torch.randint(0, 2, (16, D), generator=gen).float().to(dev)
view_kw = dict(kw, staged=True, bg_color=1, perturb=False, force_all_rays=True, max_ray_batch=4096)
with torch.no_grad():
    variants = {"16_renders": lambda: [model.render(r["rays_o"], r["rays_d"], msgs[k], **view_kw)["image"] for k in range(16)],
                "one_render_16_messages": lambda: model.render(r["rays_o"], r["rays_d"], msgs, **view_kw)["image"]}
    times, images = {k: [] for k in variants}, {}
    for rep in range(repeats + 1):
        for name, fn in variants.items():
            t, images[name] = wall(fn)
            if rep:
                times[name].append(t)
    same = all(torch.equal(images["one_render_16_messages"][k], images["16_renders"][k]) for k in range(16))
a, b = float(np.median(times["16_renders"])), float(np.median(times["one_render_16_messages"]))
result["staged_view"] = {"H": H, "W": W, "sixteen_renders_s": a, "one_render_s": b, "speedup": a / b, "same_images": same, "all_s": times}
print(f"(b) {H} x {W} view, staged: 16 renders {a * 1e3:.1f} ms, one render under 16 messages {b * 1e3:.1f} ms ({a / b:.2f} x); same images: {same}")
del images

# ---- (c) the launches
base = [t.detach() for t in model.encoder.tables()]
tables = [t.detach() for t in model.msg_encoder.tables()]
base_ptrs, table_ptrs = nv.ptr_array(base), nv.ptr_array(tables)
bound = float(model.bound)
packed = model._packed()
S1 = fo.codebook_presum_sel(tables, msgs[0].contiguous())
ws = torch.empty(int(nv.fn("hg_planes_bytes")(M)), dtype=torch.uint8, device=dev)
layout = fo.encode_planes(pts, M, bound, base_ptrs, S1, ws)
sig, rgb = torch.empty(16, M, device=dev), torch.empty(16, M, 3, device=dev)
S_multi = torch.empty(16 * fo.T_ROWS * 2, device=dev)
cplanes = torch.empty(int(nv.fn("hg_multi_planes_bytes")(M, 16)), dtype=torch.uint8, device=dev)


def chain_us(fn, launches=8, replays=10):
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


single = {
    "presum": chain_us(lambda: nv.call("hg_codebook_presum_sel", table_ptrs, nv.ptr(msgs[0]), D, nv.ptr(S1), nv.stream())),
    "gather": chain_us(lambda: nv.call("hg_encode_codebook_plane", nv.ptr(pts), M, bound, nv.ptr(S1), nv.ptr(ws), layout, None, nv.stream())),
    "mlp": chain_us(lambda: nv.call("field_fwd", nv.ptr(pts), nv.ptr(dirs), M, bound, base_ptrs, nv.ptr(S1), nv.ptr(packed), nv.ptr(sig), nv.ptr(rgb), None, None,
                                    nv.ptr(ws), layout, nv.stream())),
}
result["launch_us"] = {"points": M, "layout": "mixed" if layout == fo.PLANES_MIXED else "f32", "single": single, "multi": {}}
print(f"(c) {M} points, D = {D}, {result['launch_us']['layout']} planes; single-message launches: pre-sum {single['presum']:.1f} us, codebook plane {single['gather']:.1f} us, "
      f"field_fwd {single['mlp']:.1f} us")
prev = None
for K in (1, 2, 4, 8, 16):
    mk = msgs[:K].contiguous()
    multi = {
        "presum": chain_us(lambda: nv.call("hg_codebook_presum_multi", table_ptrs, nv.ptr(mk), K, D, nv.ptr(S_multi), nv.stream())),
        "gather": chain_us(lambda: nv.call("hg_encode_codebook_planes_multi", nv.ptr(pts), M, bound, nv.ptr(S_multi), K, nv.ptr(cplanes), nv.stream())),
        "mlp": chain_us(lambda: nv.call("field_fwd_multi", nv.ptr(dirs), M, nv.ptr(packed), nv.ptr(ws), layout, nv.ptr(cplanes), K, nv.ptr(sig), nv.ptr(rgb), nv.stream())),
    }
    multi["per_added_message"] = None if prev is None else {k: (multi[k] - prev[1][k]) / (K - prev[0]) for k in single}
    result["launch_us"]["multi"][K] = multi
    print(f"    K = {K:2d}: " + "; ".join(f"{k} {multi[k]:8.1f} us = {multi[k] / (K * single[k]):.2f} x (K x single)" for k in single)
          + ("" if prev is None else "; per added message " + ", ".join(f"{k} {v:.1f}" for k, v in multi["per_added_message"].items())))
    prev = (K, multi)
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    json.dump(result, open(out_path, "w"), indent=1)
