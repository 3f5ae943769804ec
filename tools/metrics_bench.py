#!/usr/bin/env python
"""Image metrics timing and accuracy on one MI355X: PSNR + SSIM of one view at 400 x 400, 800 x 800 and 756 x 1008 (B = 1, C = 3).

    python tools/metrics_bench.py [--out profiles/metrics_bench.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/metrics_bench.py --kernels-only --sizes 756x1008
    python tools/metrics_bench.py --stats DIR --sizes 756x1008 [--out ...]   # add that size's kernel times from DIR's *_kernel_stats.csv

Per size: (a) ImageMetrics.update (both entry points, four launches, plus the handful of scalar torch ops that accumulate on the device);
the two entry points alone (im_range_sse, im_ssim: kernel + finish launch each, buffers allocated once); (b) the reference-shaped route on the
same GPU -- permute to NCHW, the literal torch-operator sequence of tests/ssim_ref.py in fp32, .item(), plus PSNRMeter.update's copy to the
host -- which is what a user gets today with torchmetrics installed; (c) ten views through quality.test_image_metrics (one host read) against
ten through (b).  Times are device events around windows of `--reps` calls, `--windows` windows each: median, and the spread over the windows.
Bytes a pass must move, from shapes: 2 images x B H W C x 4 B (the halo re-reads of the SSIM tiles hit the caches and are not counted).
Accuracy: E32 / M32 (the literal fp32 sequence against fp64 on the CPU, tests/test_gpu_metrics.py) and the kernels' largest errors over the same
test images.
"""
import argparse
import csv
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_PEAK = 8.0e12          # bytes/s, MI355X HBM3E spec
SIZES = [(400, 400), (800, 800), (756, 1008)]
KERNELS = ("k_im_range", "k_im_range_finish", "k_im_ssim", "k_im_ssim_finish")


def windows(fn, reps, n_windows):
    """ms per call of fn(): device events around `reps` calls, `n_windows` times -> {median, min, max}."""
    per_call = []
    for _ in range(n_windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        per_call.append(a.elapsed_time(b) / reps)
    return {"median_ms": float(np.median(per_call)), "min_ms": float(min(per_call)), "max_ms": float(max(per_call))}


def view(size, dev, seed=0):
    import ssim_ref
    return tuple(x.to(dev) for x in ssim_ref.images("wm", size, seed=seed))


def reference_shaped(pred, truth, psnr_meter):
    """What the reference's two meters do per view, on this GPU: SSIMMeter's permute + torchmetrics' operator sequence + a host read of the
    value, and PSNRMeter's host copies + numpy."""
    import ssim_ref
    v = ssim_ref.ssim_literal(pred, truth, dtype=torch.float32)[0].item()
    psnr_meter.update(pred, truth)
    return v


def entry_points(pred, truth):
    """The two C entry points with every buffer allocated once -> (range call, ssim call)."""
    from nerf_signature_amd import _native as nv
    B, H, W, C = pred.shape
    dev = pred.device
    s1 = torch.empty(int(nv.fn("im_range_scratch_bytes")(B, H * W * C)), dtype=torch.uint8, device=dev)
    s2 = torch.empty(int(nv.fn("im_ssim_scratch_bytes")(B, H, W, C)), dtype=torch.uint8, device=dev)
    extrema, sse, out = torch.empty(4, device=dev), torch.empty(B, dtype=torch.float64, device=dev), torch.empty(B, dtype=torch.float64, device=dev)
    rng = lambda: nv.call("im_range_sse", nv.ptr(pred), nv.ptr(truth), B, H * W * C, nv.ptr(s1), nv.ptr(extrema), nv.ptr(sse), nv.stream())
    ssim = lambda: nv.call("im_ssim", nv.ptr(pred), nv.ptr(truth), B, H, W, C, nv.ptr(extrema), 0.0, nv.ptr(s2), nv.ptr(out), None, nv.stream())
    return rng, ssim


def accuracy():
    import test_gpu_metrics as T
    e32, m32 = T._bars()
    worst_mean = worst_map = 0.0
    for case in T.CASES:
        mean, per_image, smap = T._gpu(case)
        mean64, per64, map64 = T._fp64(case)
        worst_mean = max(worst_mean, abs(float(mean - mean64)), float((per_image - per64).abs().max()))
        worst_map = max(worst_map, float((smap.double() - map64).abs().max()))
    return {"E32_literal_fp32_mean_error": e32, "M32_literal_fp32_map_error": m32, "bar_mean": 2 * e32, "bar_map": m32,
            "gpu_largest_mean_error": worst_mean, "gpu_largest_map_error": worst_map, "cases": list(T.CASES)}


def run(sizes, reps, n_windows):
    from nerf_signature_amd import metrics, quality
    from nerf_signature_amd.trainer import PSNRMeter
    dev = torch.device("cuda:0")
    rec = {"device": torch.cuda.get_device_name(0), "reps_per_window": reps, "windows": n_windows, "accuracy": accuracy(), "runs": []}
    print(json.dumps(rec["accuracy"]), flush=True)
    for size in sizes:
        pred, truth = view(size, dev)
        meter, host_meter = metrics.ImageMetrics(dev), PSNRMeter()
        rng, ssim = entry_points(pred, truth)
        a_fn, b_fn = (lambda: meter.update(pred, truth)), (lambda: reference_shaped(pred, truth, host_meter))
        for fn in (a_fn, b_fn, rng, ssim):        # warm-up: code objects, allocator, convolution algorithm
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        a1, b1 = windows(a_fn, reps, n_windows), windows(b_fn, max(1, reps // 10), n_windows)     # alternating: a b a b
        a2, b2 = windows(a_fn, reps, n_windows), windows(b_fn, max(1, reps // 10), n_windows)
        t_rng, t_ssim = windows(rng, reps, n_windows), windows(ssim, reps, n_windows)
        ten = [view(size, dev, seed=i) for i in range(10)]
        stage = {"device": dev}
        quality.test_image_metrics(stage, views=ten)
        c_ours = windows(lambda: quality.test_image_metrics(stage, views=ten), max(1, reps // 10), n_windows)
        c_ref = windows(lambda: [reference_shaped(p, t, host_meter) for p, t in ten], max(1, reps // 50), n_windows)
        pass_bytes = 2 * pred.numel() * 4
        per_pass = lambda t: {**t, "bytes": pass_bytes, "bytes_per_s": pass_bytes / (t["median_ms"] * 1e-3),
                              "share_of_hbm_peak": pass_bytes / (t["median_ms"] * 1e-3) / HBM_PEAK, "hbm_floor_us": pass_bytes / HBM_PEAK * 1e6}
        run_rec = {"H": size[0], "W": size[1], "B": 1, "C": 3,
                   "a_image_metrics_update": [a1, a2], "b_reference_shaped_route": [b1, b2],
                   "a_not_slower_than_b": max(a1["median_ms"], a2["median_ms"]) <= min(b1["median_ms"], b2["median_ms"]),
                   "im_range_sse_two_launches": per_pass(t_rng), "im_ssim_two_launches": per_pass(t_ssim),
                   "c_ten_views_test_image_metrics": c_ours, "c_ten_views_reference_shaped": c_ref}
        rec["runs"].append(run_rec)
        print(json.dumps(run_rec), flush=True)
    return rec


def kernels_only(sizes, reps):
    """What the profiled run executes: the two entry points, reps times per size."""
    dev = torch.device("cuda:0")
    for size in sizes:
        rng, ssim = entry_points(*view(size, dev))
        for _ in range(reps):
            rng()
            ssim()
        torch.cuda.synchronize()


def add_stats(d, pass_bytes):
    """Calls and times of the metric kernels from the *_kernel_stats.csv of a --kernels-only run under rocprofv3 (one size per run); for the two
    kernels that stream the images, the pass's bytes over the mean time."""
    f = sorted(glob.glob(os.path.join(d, "**", "*_kernel_stats.csv"), recursive=True))[-1]
    out = {}
    for r in csv.DictReader(open(f)):
        for k in KERNELS:
            if k + "<" in r["Name"] or k + "(" in r["Name"]:
                rec = {"calls": int(r["Calls"]), "avg_us": float(r["AverageNs"]) / 1e3, "min_us": float(r["MinNs"]) / 1e3, "max_us": float(r["MaxNs"]) / 1e3}
                if "finish" not in k:
                    rec.update(bytes=pass_bytes, bytes_per_s=pass_bytes / (rec["avg_us"] * 1e-6), share_of_hbm_peak=pass_bytes / (rec["avg_us"] * 1e-6) / HBM_PEAK)
                out[r["Name"].split("(")[0]] = rec
    out["stats_file"] = os.path.relpath(f, ROOT)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "metrics_bench.json"))
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--sizes", nargs="+", default=[f"{h}x{w}" for h, w in SIZES], help="HxW ...")
    ap.add_argument("--stats", help="directory of a rocprofv3 --kernel-trace --stats run of --kernels-only with one size: --sizes HxW")
    a = ap.parse_args()
    sizes = [tuple(int(v) for v in s.split("x")) for s in a.sizes]
    if a.stats:
        rec = json.load(open(a.out))
        if len(sizes) != 1:
            sys.exit("--stats: give the one size the profiled run used")
        run_rec = next(r for r in rec["runs"] if (r["H"], r["W"]) == sizes[0])
        run_rec["kernels"] = add_stats(a.stats, 2 * run_rec["B"] * run_rec["H"] * run_rec["W"] * run_rec["C"] * 4)
        print(json.dumps(run_rec["kernels"]))
    else:
        if not torch.cuda.is_available():
            sys.exit("metrics_bench needs a GPU")
        if a.kernels_only:
            kernels_only(sizes, a.reps)
            return
        rec = run(sizes, a.reps, a.windows)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
