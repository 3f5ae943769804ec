#!/usr/bin/env python
"""Does the signature survive distillation?  The measurement behind DESIGN.md section 26.

    python tools/distill_bench.py [--size 192] [--views 12,50] [--steps 1024] [--side 0] [--channels 4] [--seed 0] [--reps 20] [--json profiles/distill.json]

Signs the procedural preset that tools/sign_scene.py signs (plinth, 12 + 2 views of --size, focal 1.2 x size, schedule (1536, 1500), message seed 11), runs
quality.distillation_survival over --views x --steps (student views of --side pixels a side; 0: the signed size), and times rm_finish_u8 alone at 4096 rays and at
100 x 800 x 800 rays for both channel counts: device events around each of --reps launches after two warm-up launches, median and all runs.  What survives is
reported, not judged."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from nerf_signature_amd import distill, procedural, quality


def flag(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def time_finish(N, channels, reps, dev):
    image, ws = torch.rand(N, 3, device=dev), torch.rand(N, device=dev)
    image *= ws[:, None]
    out = torch.empty(N * channels, dtype=torch.uint8, device=dev)
    run = lambda: distill.finish_u8(image, ws, channels, out=out)
    for _ in range(2):
        run()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    traffic = N * (16 + channels)
    return {"rays": N, "channels": channels, "median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "runs_ms": [round(x, 5) for x in ms],
            "bytes_moved": traffic, "gb_per_s_at_median": traffic / statistics.median(ms) / 1e6}


def main():
    dev = torch.device("cuda")
    size, seed, reps, channels, side = flag("--size", 192), flag("--seed", 0), flag("--reps", 20), flag("--channels", 4), flag("--side", 0)
    views = tuple(int(v) for v in flag("--views", "12,50").split(","))
    steps = tuple(int(v) for v in flag("--steps", "1024").split(","))
    focal, radius = 1.2 * size, 2.2
    preset = procedural.SCENES["plinth"]
    train = procedural.dataset(preset, 12, size, size, focal, radius, seed=0, device=dev)
    held = procedural.dataset(preset, 2, size, size, focal, radius, seed=1, device=dev)
    message = quality.messages(32, 1, seed=11)[0]
    t0 = time.perf_counter()
    signed = quality.sign_scene(train, message, bound=1.0, stage1_steps=1536, stage2_steps=1500, seed=seed, held_out=held, rows=16, cols=16)
    torch.cuda.synchronize()
    sign_s = time.perf_counter() - t0
    rec = signed["record"]
    print(f"signed: stage 1 {rec['stage1']['psnr_db']:.2f} dB, bit accuracy {rec['stage2']['test_bitacc']:.4f}, verify {rec['verify']['matches']} of {rec['D']}")
    t0 = time.perf_counter()
    survival = quality.distillation_survival(signed, message, views=views, steps=steps, H=side or None, W=side or None, channels=channels, seed=seed)
    torch.cuda.synchronize()
    survival["wall_s"] = time.perf_counter() - t0
    survival["field"] = {k: v for k, v in survival["field"].items() if k != "bits"}
    print(f"released field: {survival['field']['matches']} of {rec['D']} bits (p = {survival['field']['p_value']:.3g})")
    for c in survival["cells"]:
        print(f"student of {c['views']} views, {c['steps']} steps: {c['matches']} of {rec['D']} bits (p = {c['p_value']:.3g}), {c['psnr_db']:.2f} dB / SSIM {c['ssim']:.3f} "
              f"against the teacher (a constant picture: {c['constant_psnr_db']:.2f} dB), {c['ms_per_step']:.3f} ms per step")
    del signed
    torch.cuda.empty_cache()
    kernel = []
    for N in (4096, 100 * 800 * 800):
        for C in (4, 3):
            k = time_finish(N, C, reps, dev)
            kernel.append(k)
            print(f"rm_finish_u8, {N} rays, C = {C}: median {k['median_ms'] * 1e3:.2f} us of {reps} ({k['min_ms'] * 1e3:.2f} .. {k['max_ms'] * 1e3:.2f}), "
                  f"{k['gb_per_s_at_median']:.0f} GB/s")
    args = [a for i, a in enumerate(sys.argv[1:], 1) if a != "--json" and sys.argv[i - 1] != "--json"]      # (where the file went changes no number)
    bench = {"what": "measured on one MI355X, one process", "command": "python tools/distill_bench.py " + " ".join(args), "device": torch.cuda.get_device_name(0),
             "signed": {"size": size, "stage1": rec["stage1"], "stage2": rec["stage2"], "verify": {k: v for k, v in rec["verify"].items() if k != "bits"}, "wall_s": sign_s},
             "student_side": side or size, "channels": channels, "distillation_survival": survival, "rm_finish_u8": kernel}
    path = flag("--json", os.path.join(ROOT, "profiles", "distill.json"))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(bench, f, indent=1)
    print("written:", path)


if __name__ == "__main__":
    main()
