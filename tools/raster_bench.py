#!/usr/bin/env python
"""What rasterising an exported mesh costs, and whether a signature survives the export.

    python tools/raster_bench.py [--reps R] [--resolution 256] [--threshold median|DENSITY] [--survival] [--steps N] [--json PATH]

Default: the mesh of scene S0's model (opaque density head, cut to its occupancy grid as quality.mesh_survival cuts it; untrained: training moves no geometry) at `--resolution`^3 and `--threshold` (default: the median density of the occupied nodes -- the random density head has no surface of its own, and save_mesh's 10 cuts
only scattered blobs out of it), cleaned, seen from the key pose at 400 x 400 and at
800 x 800 (the intrinsics scaled with the image): per size the time of rs_project, rs_raster and rs_shade alone (events around R repetitions after a warm-up, median; each
launch on the state the previous one left), of the whole raster.render_mesh (wall clock: it ends in a host read), the share of triangles on the large route, and --
for context only -- the field's own staged render of the same view in the same session.
--survival: trains the stage with the README schedule (--steps N for a shorter one) and runs quality.mesh_survival for the first message of quality.messages: the
            table of bit accuracy, p-value, PSNR and SSIM per (resolution, colouring)."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from nerf_signature_amd import mesh, quality, raster, rays, release as rel


def flag(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


reps, out_path, R, steps, thr = flag("--reps", 20), flag("--json", ""), flag("--resolution", 256), flag("--steps", 0), flag("--threshold", "median")
thr = thr if thr == "median" else float(thr)
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


def wall(fn, reps=reps, warm=3):
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms)


stage = quality.watermark_stage(opaque=True) if "--survival" in sys.argv else quality.watermark_stage(n_poses=1, n_test_poses=1, opaque=True)      # (timing needs no training views)
msg = quality.messages(stage["D"], 1)[0].to(dev)

if "--survival" in sys.argv:
    rec = quality.train(stage, mode="graphed", log_every=0, **({"steps": steps} if steps else {}))
    t0 = time.perf_counter()
    out = quality.mesh_survival(stage, msg, threshold=thr)
    result["survival"] = {"scene": stage["scene"], "train_steps": rec["steps"], "seconds": time.perf_counter() - t0,
                          "field": {k: out["field"][k] for k in ("matches", "bit_accuracy", "p_value")}, "cells": out["cells"]}
    print(json.dumps(result["survival"]["field"]))
    for c in out["cells"]:
        print(json.dumps(c))
else:
    with torch.no_grad():
        model = stage["model"]
        key = quality.stage_key(stage, msg)
        lo, hi = model.aabb_infer[:3], model.aabb_infer[3:]
        u = mesh.lattice(model, lo, hi, R, msg)
        occ = mesh.occupied(model, lo, hi, R)
        level = float(u[occ].median()) if thr == "median" else thr
        q = torch.quantile(u[occ][:1 << 22].double(), torch.tensor([0.1, 0.5, 0.9, 0.99], dtype=torch.float64, device=dev)).tolist()
        u = torch.where(occ, u, torch.full_like(u, -1.0))
        v, t, n = mesh.marching_cubes(u, level, normals=True, scale=mesh.lattice_scale(lo, hi, R))
        rgb = mesh.vertex_colors(model, mesh.world_vertices(v, lo, hi, R), n, msg)
        v, t, rgb = mesh.clean(v, t, 8, attributes=(rgb,))
        verts, rgb = mesh.world_vertices(v, lo, hi, R).float().contiguous(), rgb.contiguous()
        V, T = int(verts.shape[0]), int(t.shape[0])
        result["mesh"] = {"resolution": R, "threshold": level, "occupied_density_quantiles_10_50_90_99": q, "V": V, "T": T}
        print(json.dumps(result["mesh"]))
        released = rel.release(model, msg, copy=True)
        rows = {}
        for scale in (1, 2):
            H, W = stage["H"] * scale, stage["W"] * scale
            intr = tuple(float(x) * scale for x in key.intrinsics)
            args = raster.check_inputs(verts, t, rgb, key.poses[0], intr, H, W, 1.0, 0.05)
            a_v, a_t, a_c, a_pose, a_bg, _, _ = args
            sc = raster.RasterScratch(V, T, H, W, dev)
            image, depth, winner = torch.empty(H, W, 3, device=dev), torch.empty(H, W, device=dev), torch.empty(H, W, dtype=torch.int32, device=dev)
            go = lambda only=None: raster.launch(a_v, a_t, a_c, a_pose, intr, H, W, a_bg, 0.05, sc, image, depth, winner, only=only)
            go()
            status = sc.status.tolist()
            row = {"large_route_triangles": status[3], "large_route_share": status[3] / max(T, 1), "culled": status[1:3], "covered_pixels": int((winner >= 0).sum())}

            def raster_only():      # rs_raster needs the z-buffer rs_project resets: time the pair and subtract the projection
                go("project")
                go("raster")

            row["rs_project_ms"] = timed(lambda: go("project"))
            row["rs_project_plus_raster_ms"] = timed(raster_only)
            row["rs_raster_ms"] = row["rs_project_plus_raster_ms"] - row["rs_project_ms"]
            row["rs_shade_ms"] = timed(lambda: go("shade"))
            row["three_launches_ms"] = timed(go)
            row["render_mesh_wall_ms"] = wall(lambda: raster.render_mesh(verts, t, rgb, key.poses[0], intr, H, W, scratch=sc))
            r = rays.get_rays(torch.from_numpy(key.poses).to(dev), intr, H, W, -1)
            row["field_render_wall_ms"] = wall(lambda: released.render(r["rays_o"], r["rays_d"], staged=True, bg_color=1, perturb=False, force_all_rays=True,
                                                                         **stage["render_kwargs"])["image"], reps=max(3, reps // 4), warm=1)
            rows[f"{H}x{W}"] = row
            print(f"{H}x{W}", json.dumps(row))
        result["views"] = rows

if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
