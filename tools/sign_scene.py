#!/usr/bin/env python
"""A scene to a released, signed, verified model: quality.sign_scene from the command line.

    python tools/sign_scene.py --procedural plinth [--size 192] [--views 12] [--focal 230] [--radius 2.2]
    python tools/sign_scene.py --scene DIR [--downscale 2] [--scale 0.33] [--bound 1.0]
        [--message 0110... | --message-seed 11] [--bits 32] [--stage1-steps N] [--stage2-steps N] [--grid 16] [--seed 0] [--out DIR]
        [--bench [--survival] [--resolutions 128,256] [--json profiles/sign_scene.json]]

--scene reads split "train" through dataset.load_scene and, where the directory has one, split "val" as the held-out views; --procedural renders the preset's
train and held-out views on the GPU (procedural.dataset, seeds 0 and 1).  Written to --out (default: sign_scene_out): released.pth (release.ReleasedModel.save), key/
(release.SignatureKey.save: key_poses.npy, block coordinates, decoder) and report.json (sign_scene's record).
--bench adds, to --json: ps_render_u8 at 100 x 800 x 800 RGBA for S = 1, 2, 4 (device events around each of `--reps` launches after a warm-up; median and all
runs), the wall time of every phase of the pipeline and, with --survival, quality.mesh_survival of the TRAINED stage at threshold 10 and at "median" -- the open
question of DESIGN.md section 24.  What survives is reported, not judged."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from nerf_signature_amd import dataset, procedural, quality


def flag(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def main():
    dev = torch.device("cuda")
    directory, preset = flag("--scene", ""), flag("--procedural", "")
    if bool(directory) == bool(preset):
        raise SystemExit("sign_scene: give --scene DIR or --procedural NAME (one of them)")
    size, views, focal, radius = flag("--size", 192), flag("--views", 12), flag("--focal", 0.0), flag("--radius", 2.2)
    bits, seed, grid, out_dir = flag("--bits", 32), flag("--seed", 0), flag("--grid", 16), flag("--out", "sign_scene_out")
    s1, s2 = flag("--stage1-steps", 1536), flag("--stage2-steps", 1500)      # the plinth's schedule; a photographed scene wants the reference's
    text = flag("--message", "")
    message = torch.tensor([float(c) for c in text]) if text else quality.messages(bits, 1, seed=flag("--message-seed", 11))[0]
    if text and set(text) - {"0", "1"}:
        raise SystemExit("sign_scene: --message is a string of 0s and 1s")
    t0 = time.perf_counter()
    if preset:
        if preset not in procedural.SCENES:
            raise SystemExit(f"sign_scene: the presets are {sorted(procedural.SCENES)}")
        focal = focal or 1.2 * size
        scene = procedural.dataset(procedural.SCENES[preset], views, size, size, focal, radius, seed=0, device=dev)
        held = procedural.dataset(procedural.SCENES[preset], 2, size, size, focal, radius, seed=1, device=dev)
        source = {"procedural": preset, "size": size, "views": views, "focal": focal, "radius": radius}
    else:
        kw = dict(scale=flag("--scale", 0.33), downscale=flag("--downscale", 1), device=dev)
        scene = dataset.load_scene(directory, "train", **kw)
        held = dataset.load_scene(directory, "val", **kw) if os.path.exists(os.path.join(directory, "transforms_val.json")) else None
        if held is not None and held.poses.shape[0] > 4:
            held = dataset.Scene(held.poses[:4], held.images[:4], held.intrinsics, held.H, held.W, held.radius, held.mode, held.files[:4])
        source = {"scene": os.path.abspath(directory), **{k: v for k, v in kw.items() if k != "device"}}
    torch.cuda.synchronize()
    load_s = time.perf_counter() - t0
    os.makedirs(out_dir, exist_ok=True)
    result = quality.sign_scene(scene, message, bound=flag("--bound", 1.0), stage1_steps=s1, stage2_steps=s2, seed=seed, workdir=out_dir, held_out=held, rows=grid, cols=grid)
    record = dict(result["record"], source=source, message="".join(str(int(b)) for b in message.tolist()), seed=seed, device=torch.cuda.get_device_name(0))
    record["phases_s"] = {"load_or_render_scene_s": load_s, **record["phases_s"]}
    result["released"].save(os.path.join(out_dir, "released.pth"))
    result["key"].save(os.path.join(out_dir, "key"))
    with open(os.path.join(out_dir, "report.json"), "w") as f:
        json.dump(record, f, indent=1)
    one, two, v = record["stage1"], record["stage2"], record["verify"]
    print(f"stage 1: {one['steps']} steps, held-out PSNR {one['psnr_db']:.2f} dB (a constant picture: {one['constant_psnr_db']:.2f} dB), SSIM {one['ssim']:.3f}, "
          f"{one['ms_per_step']:.3f} ms/step, {one['samples_per_ray']:.1f} samples per ray")
    print(f"stage 2: {two['steps']} steps, {two['ms_per_step']:.3f} ms/step, bit accuracy {two['bit_acc_before_training']:.3f} -> {two['test_bitacc']:.4f}, "
          f"watermarked against clean {two['psnr_db']:.2f} dB")
    print(f"verify: {v['matches']} of {record['D']} bits, p = {v['p_value']:.3g}; written to {out_dir}")
    if "--bench" not in sys.argv:
        return
    args = [a for i, a in enumerate(sys.argv[1:], 1) if a not in ("--out", "--json") and sys.argv[i - 1] not in ("--out", "--json")]      # (where the files went changes no number)
    bench = {"what": "measured on one MI355X, one process", "command": "python tools/sign_scene.py " + " ".join(args), "pipeline": record}
    reps = flag("--reps", 10)
    poses = torch.from_numpy(procedural.orbit_poses(100, 4.0, quality.ORBIT_THETA, seed=0)).to(dev)
    big = procedural.SCENES[preset or "plinth"]
    out = torch.empty(100 * 800 * 800 * 4, dtype=torch.uint8, device=dev)
    bench["ps_render_u8_100x800x800_rgba_ms"] = {}
    for S in (1, 2, 4):
        run = lambda: procedural.render(big, poses, (1111.0, 1111.0, 400.0, 400.0), 800, 800, 4, S, out=out)
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
        bench["ps_render_u8_100x800x800_rgba_ms"][f"S={S}"] = {"median": statistics.median(ms), "runs": [round(x, 4) for x in ms]}
        print(f"ps_render_u8, 100 x 800 x 800 RGBA, S = {S}: median {statistics.median(ms):.3f} ms of {reps} ({min(ms):.3f} .. {max(ms):.3f})")
    del out
    if "--survival" in sys.argv:
        resolutions = tuple(int(r) for r in flag("--resolutions", "128,256").split(","))
        bench["mesh_survival"] = {}
        for threshold in (10, "median"):
            t0 = time.perf_counter()
            got = quality.mesh_survival(result["stage"], message.to(dev), resolutions=resolutions, threshold=threshold)
            got["field"] = {k: v for k, v in got["field"].items() if k != "bits"}
            got["wall_s"] = time.perf_counter() - t0
            bench["mesh_survival"][f"threshold={threshold}"] = got
            for c in got["cells"]:
                print(f"mesh at {c['resolution']}^3, threshold {c['threshold']:.3g}, colours '{c['colors']}': {c['T']} triangles, {c['matches']} of {record['D']} bits "
                      f"(p = {c['p_value']:.3g}), PSNR {c['psnr_db']:.2f} dB against the field's view")
    path = flag("--json", os.path.join(ROOT, "profiles", "sign_scene.json"))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(bench, f, indent=1)
    print("written:", path)


if __name__ == "__main__":
    main()
