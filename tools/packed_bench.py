#!/usr/bin/env python
"""The packed released model on one MI355X: what each format costs and keeps, and whether gathering from smaller tables is faster.

    python tools/packed_bench.py [--repeats 9] [--encoder-reps 200] [--out profiles/packed_bench.json]

One process, one session: quality.watermark_stage() trained with the README schedule (about a second), released under one message, then
  report    quality.packed_report -- per format and for the fp32 release (the yardstick, timed the same way in the same process): checkpoint bytes, verify's
            verdict, PSNR of held-out view 0 against the fp32 release, milliseconds per staged full-view render (median of --repeats, every timing kept);
  encoder   the encoder launch ALONE on the bench workload's block-render points (the 1.29 M samples of the watermark blocks), in both plane layouts:
            hg_encode_planes / hg_encode_planes_mixed over the fp32 tables against hg_encode_planes_packed over each format.  The variants ALTERNATE inside every
            round (fp32, f16, q8, q4, fp32, ...), --encoder-reps launches each per round between device events, five rounds after one warm-up round: the median
            round and the spread (min .. max) of every variant are reported, so a difference can be read against the run-to-run noise of the same session."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

ROUNDS = 5


def encoder_launches(stage, released, packed, reps):
    """{layout: {variant: {"us_median", "us_min", "us_max", "us_rounds"}}} of the encoder launch alone, M points of the block render."""
    from nerf_signature_amd import _native as nv, fieldops as fo, raymarching as rm
    model, kw = stage["model"], stage["render_kwargs"]
    o, d = stage["block_o"].reshape(-1, 3).contiguous(), stage["block_d"].reshape(-1, 3).contiguous()
    nears, fars = rm.near_far_from_aabb(o, d, model.aabb_train, model.min_near)
    xyzs = rm.march_rays_train(o, d, model.bound, model.density_bitfield, model.cascade, model.grid_size, nears, fars, None, -1, False, 128, True,
                               kw["dt_gamma"], kw["max_steps"])[0]
    M, bound = xyzs.shape[0], float(model.bound)
    planes = torch.empty(int(nv.fn("hg_planes_bytes")(M)), dtype=torch.uint8, device=xyzs.device)
    base, S = nv.ptr_array(released.encoder.tables()), released.signature.weight
    out = {"points": M}
    for layout, name in ((fo.PLANES_F32, "f32_planes"), (fo.PLANES_MIXED, "mixed_planes")):
        if layout == fo.PLANES_MIXED and nv.fn("mlp_get_precision")() != 1:
            continue
        if layout == fo.PLANES_MIXED:
            fp32 = lambda: nv.call("hg_encode_planes_mixed", nv.ptr(xyzs), M, None, bound, base, nv.ptr(S), nv.ptr(planes), nv.stream())
        else:
            fp32 = lambda: nv.call("hg_encode_planes", nv.ptr(xyzs), M, bound, base, nv.ptr(S), nv.ptr(planes), nv.stream())
        variants = {"fp32": fp32}
        for fmt, m in packed.items():
            ptrs = fo.packed_ptrs(m.encoder.codes(), m.signature.codes, fmt)
            variants[fmt] = (lambda ptrs=ptrs, fmt=fmt, m=m: nv.call("hg_encode_planes_packed", nv.ptr(xyzs), M, None, bound, ptrs, fo.PACK_FORMATS[fmt],
                                                                     nv.ptr(m.table_params), nv.ptr(planes), layout, nv.stream()))
        rounds = {k: [] for k in variants}
        for rnd in range(ROUNDS + 1):
            for k, launch in variants.items():
                launch()                                  # (the variant's tables into the caches before its window: steady state of a loop that renders with it)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(reps):
                    launch()
                b.record()
                torch.cuda.synchronize()
                if rnd:                                   # (round 0: warm-up)
                    rounds[k].append(a.elapsed_time(b) / reps * 1e3)
        out[name] = {k: {"us_median": float(np.median(v)), "us_min": min(v), "us_max": max(v), "us_rounds": [round(x, 2) for x in v]} for k, v in rounds.items()}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9, help="timed full-view renders per model")
    ap.add_argument("--encoder-reps", type=int, default=200, help="encoder launches per variant and round")
    ap.add_argument("--formats", nargs="+", default=["f16", "q8", "q4"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "packed_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("packed_bench needs a GPU")
    from nerf_signature_amd import quality, release as rel
    stage = quality.watermark_stage()
    quality.train(stage, mode="graphed", log_every=0)
    message = quality.messages(stage["D"], 1)[0].to(stage["device"])
    rec = {"device": torch.cuda.get_device_name(0), "scene": stage["scene"], "view": [stage["H"], stage["W"]], "repeats": a.repeats, "encoder_reps": a.encoder_reps}
    rec["report"] = quality.packed_report(stage, message, formats=tuple(a.formats), repeats=a.repeats)
    for name, r in rec["report"].items():
        print(f"{name:5s} {r['bytes'] / 2 ** 20:8.2f} MiB  matches {r['verify']['matches']:2d}/{stage['D']}  psnr {r['psnr']:7.2f} dB  render {r['render_ms']:.3f} ms "
              f"({min(r['render_ms_all']):.3f} .. {max(r['render_ms_all']):.3f})", flush=True)
    with torch.no_grad():
        released = rel.release(stage["model"], message)
        rec["encoder"] = encoder_launches(stage, released, {f: rel.pack(released, f) for f in a.formats}, a.encoder_reps)
    for name in ("f32_planes", "mixed_planes"):
        for k, v in rec["encoder"].get(name, {}).items():
            print(f"encoder {name:12s} {k:5s} {v['us_median']:7.1f} us ({v['us_min']:.1f} .. {v['us_max']:.1f}), M = {rec['encoder']['points']}", flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
