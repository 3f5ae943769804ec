#!/usr/bin/env python
"""What tampering a released model costs, and what survives it.

    python tools/tamper_bench.py [--reps R] [--sweep] [--z-error] [--json PATH]

Default: on the released model's tensor list (16 base tables, the signature table, both MLP vectors: 17 836 032 floats) of scene S0, per kind the time of
select / statistics + apply (tamper.Tamper.apply, from the pristine copy into the live tensors) next to the torch statement of the same attack (kthvalue over
the concatenated magnitudes -- torch.quantile refuses this many elements -- / std + randn_like / min, max, round / .half().float(), each with the copy back into
the live tensors), and one whole sweep point (apply + verify + the held-out view's PSNR).  Events around R repetitions after a warm-up, median.
--sweep:   trains the stage with the README schedule and runs quality.model_robustness for the four messages of quality.messages and two noise seeds: the table
           of bit accuracy and PSNR per grid point.
--z-error: max |z - z64| of the device's unit normal over the 2^24 draws of (seed 0, tensor 0) against tests/tamper_ref.py's float64 restatement (the figure
           behind tamper_ref.EPS_Z)."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

from nerf_signature_amd import metrics, quality, rays, release as rel, tamper


def flag(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


reps, out_path = flag("--reps", 20), flag("--json", "")
dev = torch.device("cuda")
result = {"device": torch.cuda.get_device_name(0), "what": "measured on one MI355X, one session"}


def timed(fn, reps=reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms)


if "--z-error" in sys.argv:
    import tamper_ref as tr
    n = 1 << 24
    x = torch.zeros(n, dtype=torch.float32, device=dev)
    unit = torch.tensor([[0.0, 0.0, 0.0, 1.0]], dtype=torch.float64, device=dev)      # deviation 1, strength 1: y = 0 + 1 z
    tamper.apply([x], [x], "noise", strength=1.0, stats=unit, seed=0)
    z = x.cpu().numpy().astype(np.float64)
    err = np.abs(z - tr.unit_normal(0, 0, n))
    at = int(err.argmax())
    result["z_error"] = {"draws": n, "max_abs_error": float(err.max()), "at_element": at, "z_there": float(z[at]), "max_abs_z": float(np.abs(z).max()),
                         "mean": float(z.mean()), "variance": float(z.var())}
    print(json.dumps(result["z_error"]))

elif "--sweep" in sys.argv:
    stage = quality.watermark_stage()
    rec = quality.train(stage, mode="graphed", log_every=0)
    msgs = [m.to(dev) for m in quality.messages(stage["D"], 4)]
    runs = [quality.model_robustness(stage, m, seeds=(0, 1)) for m in msgs]
    table = []
    for kind, strength in quality.MODEL_ATTACKS:
        recs = [r[p] for r in runs for p in r if p[:2] == (kind, strength)]
        finite = [r["psnr"] for r in recs if np.isfinite(r["psnr"])]
        table.append({"kind": kind, "strength": strength, "n": len(recs), "bit_accuracy_mean": float(np.mean([r["bit_accuracy"] for r in recs])),
                      "matches_min": min(r["matches"] for r in recs), "psnr_db_mean": float(np.mean(finite)) if finite else float("inf"),
                      "bit_equal_renders": len(recs) - len(finite)})
        print(json.dumps(table[-1]))
    clean = [rel.verify(rel.release(stage["model"], m), rel.SignatureKey.from_block_rays(m, stage["model"].msg_decoder, stage["block_o"], stage["block_d"], stage["render_kwargs"]))
             for m in msgs]
    result["sweep"] = {"scene": stage["scene"], "train_steps": rec["steps"], "messages": len(msgs), "noise_seeds": [0, 1], "untampered_matches": [c["matches"] for c in clean],
                       "table": table}

else:
    stage = quality.watermark_stage()
    msg = quality.messages(stage["D"], 1)[0].to(dev)
    with torch.no_grad():
        released = rel.release(stage["model"], msg, copy=True)
        key = rel.SignatureKey.from_block_rays(msg, stage["model"].msg_decoder, stage["block_o"], stage["block_d"], stage["render_kwargs"])
        tm = released.tamper()
        live, pristine = released.tampered_tensors(), tm.pristine
        result["floats"] = tm.total

        def torch_prune(p=0.5):
            mags = torch.cat([t.reshape(-1).abs() for t in pristine])
            thr = torch.kthvalue(mags, int(round(p * mags.numel()))).values
            for t, src in zip(live, pristine):
                t.copy_(torch.where(src.abs() <= thr, torch.zeros_like(src), src))

        def torch_noise(s=0.1):
            for t, src in zip(live, pristine):
                t.copy_(src + (s * src.std()) * torch.randn_like(src))

        def torch_quantize(b=8):
            L = float((1 << b) - 1)
            for t, src in zip(live, pristine):
                lo, hi = src.min(), src.max()
                step = (hi - lo) / L
                t.copy_(lo + torch.clamp(torch.round((src - lo) / step), 0, L) * step)

        def torch_half():
            for t, src in zip(live, pristine):
                t.copy_(src.half().float())

        def torch_restore():
            for t, src in zip(live, pristine):
                t.copy_(src)

        rows = {}
        for name, ours, theirs in (("prune 0.5", lambda: tm.apply("prune", 0.5), torch_prune), ("noise 0.1", lambda: tm.apply("noise", 0.1, seed=1), torch_noise),
                                   ("quantize 8", lambda: tm.apply("quantize", 8), torch_quantize), ("half", lambda: tm.apply("half"), torch_half),
                                   ("restore", tm.restore, torch_restore)):
            rows[name] = {"kernels_ms": timed(ours)}
            try:
                rows[name]["torch_ms"] = timed(theirs, reps=max(3, reps // 4), warm=1)
            except RuntimeError as e:      # (an operator that refuses the size is a result too)
                rows[name]["torch_error"] = str(e).splitlines()[0][:160]
            print(name, json.dumps(rows[name]))
        tm._stats_valid = False
        rows["statistics alone"] = {"kernels_ms": timed(lambda: tm.launch.stats(out=tm._stats))}
        rows["select alone"] = {"kernels_ms": timed(lambda: tm.launch.abs_kth(tm.total // 2, out=tm._threshold))}
        try:
            torch.quantile(torch.cat([t.reshape(-1).abs() for t in pristine]), 0.5)
        except RuntimeError as e:
            rows["torch.quantile"] = {"torch_error": str(e).splitlines()[0][:160]}
        r = rays.get_rays(stage["test_poses"][:1], stage["intr"], stage["H"], stage["W"], -1)
        H, W = stage["H"], stage["W"]
        full = lambda: released.render(r["rays_o"], r["rays_d"], staged=True, bg_color=1, perturb=False, force_all_rays=True, **stage["render_kwargs"])["image"].reshape(1, H, W, 3).clamp(0, 1)
        tm.restore()
        truth = full()

        def point():
            tm.apply("noise", 0.1, seed=2)
            v = rel.verify(released, key)
            return v["matches"], float(metrics.psnr(full(), truth))

        rows["sweep point (noise 0.1: apply + verify + view PSNR)"] = {"wall_ms": timed(point, reps=max(3, reps // 4), warm=1)}
        rows["verify alone (4608 key rays + decoder + host read)"] = {"wall_ms": timed(lambda: rel.verify(released, key), reps=max(3, reps // 4), warm=1)}
        print(json.dumps(rows, indent=1))
        result["launch_times"] = rows

if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
