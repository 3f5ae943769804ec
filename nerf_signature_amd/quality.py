"""Does the path LEARN a watermark?  The reference's whole run, on the synthetic stand-in of its data: `--iters` steps of the loop body
(/root/reference/nerf/utils_wtmk_disen.py:1164-1181) with the README's hyper-parameters (README.md:45: --iters 1000 --lambda_w 0.005
--lambda_i 1.0, lr 1e-2 decayed by 0.1 ** min(it / iters, 1), main_nerf_wtmk.py:110-116), then `test_bitacc` (:935-1030: random messages,
block render -> decoder -> BIT_ACC) and `test_image` (:816-933: staged full views with a random message against the clean views, PSNRMeter).

  watermark_stage(...)   the stage's inputs as bench.py builds them (scene S0, clean views of `n_poses` orbit poses, block rays), with the
                         codebook at the reference's initialisation U(-1e-4, 1e-4) (hash_encoding_wtmk_bit.py:69)
  train(stage, ...)      the steps, driven by the captured loop exactly as bench.py configures it ("graphed"), by the eager loop
                         the reference's Trainer shape gets ("eager"), with the block rays declared constant ("fixed"), or through a
                         world-size-1 RCCL group with every collective of the multi-rank step issued and the codebook optimiser in its
                         sharded form ("rccl1"); every mode draws the same content batches (rg_sample_rays) and the same messages
  test_bitacc / test_image   the two evaluation loops; test_image_metrics: test_image with PSNR and SSIM taken on the device

Used by tests/test_gpu_convergence.py, bench.py's `quality` block and tools/converge.py."""
import time

import numpy as np
import torch

from . import blocks, rays, synthetic, trainer
from .distortion import DistortionLayer
from .fieldops import message_chunks
from .metrics import ImageMetrics
from .trainer import BIT_ACC, PSNRMeter

README = dict(iters=1000, lambda_w=0.005, lambda_i=1.0, lr=1e-2)       # README.md:45 + main_nerf_wtmk.py:21


ORBIT_THETA = (0.6, 1.5)      # the polar range the stage's stored poses are drawn from (bench.py's): online targets draw their cameras from the same


def watermark_stage(scene="hotdog", device="cuda", n_poses=8, n_test_poses=10, codebook_scale=1e-4, n_rays=4096, seed=0, online_targets=False, opaque=False):
    """opaque: the density head scaled so that the ball is a solid (synthetic.init_model(opaque=True)): a scene with a surface, which a mesh can stand for
    (mesh_survival); the default is the translucent ball every other measurement uses.  online_targets: no clean-render pre-pass and no image store -- `poses` / `clean` are None, train() draws a new orbit camera every step
    (rays.OrbitRaySampler) and the step renders its own target (the content render's clean twin); the held-out views' clean images are rendered when
    test_views asks for them."""
    from .network import NeRFNetwork
    dev = torch.device(device)
    cfg = synthetic.SCENES[scene]
    D, H, W = cfg["message_dim"], cfg["H"], cfg["W"]
    intr = (cfg["focal"], cfg["focal"], W / 2, H / 2)
    torch.manual_seed(seed)
    model = NeRFNetwork(bound=cfg["bound"], cuda_ray=True, density_scale=1, min_near=0.2, density_thresh=10, bg_radius=-1, message_dim=D, n_views=1)
    synthetic.init_model(model, scene, codebook_scale=codebook_scale, opaque=opaque)
    model.to(dev).train()
    kw = dict(dt_gamma=cfg["dt_gamma"], max_steps=1024)
    bo, bd = synthetic.block_rays(scene, dev)
    prng = np.random.RandomState(77)          # (bench.py's poses)
    mk = lambda n: torch.from_numpy(np.stack([synthetic.orbit_pose(0.6 + 0.9 * prng.rand(), 2 * np.pi * prng.rand(), cfg["radius"]) for _ in range(n)])).to(dev)
    poses, test_poses = mk(n_poses), mk(n_test_poses)
    if online_targets:
        return dict(model=model, scene=scene, device=dev, D=D, H=H, W=W, intr=intr, render_kwargs=kw, block_o=bo, block_d=bd, poses=None, clean=None,
                    test_poses=test_poses, clean_test=None, n_rays=n_rays, radius=cfg["radius"])
    with torch.no_grad():     # "ground truth" = the clean model's render of the same pose (provider_wtmk.py:408-416)
        clean = blocks.clean_render(model, poses, intr, H, W, kw, max_ray_batch=H * W).reshape(n_poses, H * W, 3).clamp_(0, 1).contiguous()
        clean_test = blocks.clean_render(model, test_poses, intr, H, W, kw, max_ray_batch=H * W).reshape(n_test_poses, H, W, 3).clamp_(0, 1).contiguous()
    return dict(model=model, scene=scene, device=dev, D=D, H=H, W=W, intr=intr, render_kwargs=kw, block_o=bo, block_d=bd, poses=poses, clean=clean,
                test_poses=test_poses, clean_test=clean_test, n_rays=n_rays)


def messages(D, n, seed=1234):
    """The per-step draws of utils_wtmk_disen.py:1165 from one seeded host stream (the same sequence in every mode and on every rank)."""
    rng = np.random.RandomState(seed)
    return [torch.from_numpy(rng.randint(0, 2, D).astype(np.float32)) for _ in range(n)]


def lr_lambda(iters):
    return lambda it: 0.1 ** min(it / iters, 1)       # main_nerf_wtmk.py:115


def snapshot(stage, optimizer, lr=README["lr"]):
    """The trainable state of a run on the host -- codebook, decoder, Adam moments and step counts -- in a form `train(..., resume=)` loads into
    a fresh stage under ANY mode (the captured loop keeps its learning rate and step counts in device tensors: normalised here)."""
    model = stage["model"]
    sd = optimizer.state_dict()
    groups = [{k: (lr if k == "lr" else v) for k, v in g.items() if k != "initial_lr"} for g in sd["param_groups"]]
    state = {k: {n: (v.detach().to("cpu", copy=True) if torch.is_tensor(v) else v) for n, v in st.items()} for k, st in sd["state"].items()}
    params = {k: v.detach().to("cpu", copy=True) for k, v in model.state_dict().items() if k.startswith(("msg_encoder.", "msg_decoder."))}
    return {"params": params, "optimizer": {"state": state, "param_groups": groups}}


def train(stage, steps=None, mode="graphed", lambda_w=README["lambda_w"], lambda_i=README["lambda_i"], lr=README["lr"], iters=None, distortion="none",
          msg_seed=1234, sampler_seed=1000, log_every=100, check_every=250, start=0, resume=None):
    """Runs `steps` training steps on stage['model'] in place.  Returns a record: losses sampled every `log_every` steps (host reads happen
    only there and at the capacity checks every `check_every` steps), wall time, capacity overflow, per-table Adam step counts.
    start / resume: continue a run at step `start` (messages, content batches and learning rate of steps start .. start+steps-1) from a
    `snapshot` taken there."""
    from .optim import CodebookAdam
    steps = README["iters"] if steps is None else steps
    iters = start + steps if iters is None else iters
    model, dev, D, kw = stage["model"], stage["device"], stage["D"], stage["render_kwargs"]
    H, W, n_rays = stage["H"], stage["W"], stage["n_rays"]
    msgs = messages(D, start + steps + 1, msg_seed)[start:]
    from . import dp as _dp
    world, rank = _dp.world_size(), _dp.rank()          # data-parallel: every rank draws its own content batches (pose k * world + rank, own pixel stream)
    online = stage["clean"] is None      # watermark_stage(online_targets=True): cameras drawn per step, the target rendered inside the step
    if online:
        sampler = rays.OrbitRaySampler(stage["intr"], H, W, n_rays, stage["radius"], ORBIT_THETA, (0.0, 2 * np.pi), stride=world, offset=rank, seed=sampler_seed + rank,
                                       device=dev)
    else:
        sampler = rays.DeviceRaySampler(stage["poses"], stage["clean"], stage["intr"], H, W, n_rays, stride=world, offset=rank, seed=sampler_seed + rank)
    content = {k: torch.empty(1, n_rays, 3, dtype=torch.float32, device=dev) for k in (("rays_o", "rays_d") if online else ("rays_o", "rays_d", "images"))}
    counter = torch.full((1,), start, dtype=torch.int32, device=dev)
    sampler.sample_into(counter, content["rays_o"], content["rays_d"], content.get("images"))
    data = {"watermark": {"rays_o_block": stage["block_o"], "rays_d_block": stage["block_d"]}, "content": content}
    extra = {} if distortion == "none" else {"distortion": distortion}
    graphed = mode in ("graphed", "fixed", "rccl1")
    if mode == "rccl1":
        from . import dp
        if not dp.exchange_active():
            raise RuntimeError("mode 'rccl1' needs the world-size-1 RCCL group: NERFSIG_FORCE_EXCHANGE=1 RANK=0 WORLD_SIZE=1 NERFSIG_SHARD_OPTIMIZER=1 + dp.init_from_env()")
    optimizer = CodebookAdam(model.get_params(lr), betas=(0.9, 0.99), eps=1e-15, **({"fused": True, "capturable": True} if graphed else {}))
    if resume is not None:
        missing, unexpected = model.load_state_dict(resume["params"], strict=False)
        if unexpected:
            raise ValueError(f"resume: unexpected keys {unexpected}")
        optimizer.load_state_dict(resume["optimizer"])
    schedule = lr_lambda(iters)
    shifted = (lambda it: schedule(it + start)) if (schedule is not None and start) else schedule
    if graphed:
        loop = trainer.GraphedWatermarkLoop(model, optimizer, kw, data, lambda_w=lambda_w, lambda_i=lambda_i, lr_lambda=schedule, content_headroom=0.25,
                                            content_sampler=sampler, fixed_blocks=True if mode == "fixed" else None, **extra)
        if start:
            loop.resume_at(start)
        one = lambda k: loop.step(msgs[k], next_message=msgs[k + 1])
    elif mode == "eager":
        sched = None if shifted is None else torch.optim.lr_scheduler.LambdaLR(optimizer, shifted)
        loop = trainer.WatermarkLoop(model, optimizer, kw, lambda_w=lambda_w, lambda_i=lambda_i, lr_scheduler=sched, side_stream=torch.cuda.Stream(), **extra)

        def one(k):
            counter.fill_(start + k + 1)  # the captured loop's opening kernel counts the replay before the step draws its batch
            sampler.sample_into(counter, content["rays_o"], content["rays_d"], content.get("images"))
            used_lr[0] = float(optimizer.param_groups[0]["lr"])
            return loop.step(data, msgs[k])
    else:
        raise ValueError(f"mode {mode!r}: graphed | eager | fixed | rccl1")
    log, recaptures, overflow = [], 0, False
    used_lr = [None]       # the learning rate the LAST step ran with
    torch.cuda.synchronize()
    t_prep = time.perf_counter()
    if graphed:          # sizing march, warm-up steps (restored afterwards), capture: set-up, timed apart from the steps
        loop.prepare(msgs[0])
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    t_prep = t0 - t_prep
    for k in range(steps):
        out = one(k)
        if log_every and (k % log_every == 0 or k == steps - 1):
            log.append((k, float(out[3].detach()), float(out[4].detach())))
        if graphed and check_every and k % check_every == check_every - 1 and k != steps - 1:
            if loop.ensure_capacity():      # a replay dropped rays that did not fit: buffers re-sized, step re-captured (the dropped rays stay dropped)
                recaptures += 1
                overflow = True
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    if graphed:
        overflow = overflow or bool(loop.overflowed())
        loop.close()
    tables = model.msg_encoder.tables()
    counts = [float(optimizer.state[t]["step"]) if len(optimizer.state[t]) else 0.0 for t in tables]
    return dict(mode=mode, steps=steps, wall_s=wall, prepare_s=t_prep, ms_per_step=wall / steps * 1e3, log=log, overflowed=bool(overflow), recaptures=recaptures,
                adam_steps=counts, optimizer=optimizer, last_lr=float(optimizer.param_groups[0]["lr"]) if used_lr[0] is None else used_lr[0], loss_image=log[-1][1] if log else None,
                loss_watermark=log[-1][2] if log else None)


@torch.no_grad()
def state_checksums(stage):
    """Integer checksums of everything the watermark stage trains -- the 2D codebook tables and the decoder's parameters and buffers: the sum of each tensor's
    bit patterns (int64, wrapping).  Two runs leave the same list iff (up to a 2^-64 collision) they left the same bits; no 256 MB read-back."""
    model = stage["model"]
    named = [(f"msg_encoder.{i}", t) for i, t in enumerate(model.msg_encoder.tables())] + [(f"msg_decoder.{k}", v) for k, v in model.msg_decoder.state_dict().items()]
    out = []
    for name, t in named:
        t = t.detach().contiguous()
        bits = t.view(torch.int32) if t.dtype == torch.float32 else t.to(torch.int64)
        w = torch.arange(1, bits.numel() + 1, dtype=torch.int64, device=bits.device).view(bits.shape)      # (position-weighted: a permutation of the values changes the sum)
        out.append((name, int((bits.to(torch.int64) * w).sum().item())))
    return out


@torch.no_grad()
def trained_tensors(stage):
    """Copies (on the device: 256 MiB of tables at D = 32) of everything the watermark stage trains, by name -- for an element-wise comparison of two runs."""
    model = stage["model"]
    named = [(f"msg_encoder.{i}", t) for i, t in enumerate(model.msg_encoder.tables())] + [(f"msg_decoder.{k}", v) for k, v in model.msg_decoder.state_dict().items()]
    return [(name, t.detach().clone()) for name, t in named]


@torch.no_grad()
def test_bitacc(stage, n_messages=200, seed=4321, distortion="none", message_batch=None):
    """Trainer.test_bitacc (utils_wtmk_disen.py:935-1030): per item a random message, eval_step(render_whole=False) on the watermark blocks
    (the model stays in whatever mode it is in -- the reference never calls model.eval() here, :951), BIT_ACC over the items.
    message_batch: None -- one render per message, as the reference; an integer -- the same messages (same generator, same order) rendered that many at a
    time by trainer.eval_blocks_multi (one march and base encode per batch; distortion and decoder per message in the same order): the same numbers.
    Returns (mean bit accuracy, mean wrong bits per message, worst message's wrong bits)."""
    model, D, dev = stage["model"], stage["D"], stage["device"]
    acc = BIT_ACC()
    gen = torch.Generator(device="cpu").manual_seed(seed)
    wm = {"rays_o_block": stage["block_o"], "rays_d_block": stage["block_d"]}
    wrong = []
    layer = None if distortion in (None, "none") else DistortionLayer(distortion, seed)
    if message_batch is not None:
        for a, b in message_chunks(n_messages, message_batch):
            messages = torch.stack([torch.randint(0, 2, (D,), generator=gen).float() for _ in range(a, b)]).to(dev)
            _, decoded = trainer.eval_blocks_multi(model, wm, messages, stage["render_kwargs"], distortion=layer)
            for k in range(b - a):
                acc.update(decoded[k].permute(1, 0), messages[k].unsqueeze(0))
                wrong.append(round((1.0 - acc.instant_V) * D))
        return float(acc.measure()), float(np.mean(wrong)), int(np.max(wrong))
    for _ in range(n_messages):
        message = torch.randint(0, 2, (D,), generator=gen).float().to(dev)
        _, _, _, decoded, _, _, _ = trainer.eval_step(model, wm, message, stage["render_kwargs"], render_whole=False, distortion=layer)
        acc.update(decoded.permute(1, 0), message.unsqueeze(0))
        wrong.append(round((1.0 - acc.instant_V) * D))
    return float(acc.measure()), float(np.mean(wrong)), int(np.max(wrong))


test_bitacc.__test__ = False


def robustness(stage, kinds=("none", "noise", "brightness", "blurring", "rotation", "scaling"), n_messages=200, seed=4321, message_batch=None):
    """{kind: bit accuracy} of the stage's model with the evaluated blocks under each distortion in turn (test_bitacc with the same messages and the same
    evaluation seed for every kind): what a model trained against one kind, a mixed set or none keeps under each attack."""
    return {kind: test_bitacc(stage, n_messages, seed, distortion=kind, message_batch=message_batch)[0] for kind in kinds}


MODEL_ATTACKS = (tuple(("prune", p) for p in (0.1, 0.3, 0.5, 0.7, 0.9)) + tuple(("noise", s) for s in (0.01, 0.03, 0.1, 0.3, 1.0))
                 + tuple(("quantize", b) for b in (16, 8, 6, 4)) + (("half", 0),))


@torch.no_grad()
def model_robustness(stage, message, attacks=MODEL_ATTACKS, seeds=(0,), view=0):
    """What survives an attack on the released WEIGHTS (robustness() above attacks the rendered image): stage['model'] is released under `message`
    (release.release, a copy), the key is built from the stage's block rays, and for every (kind, strength) of `attacks` -- noise once per seed of `seeds`,
    the other kinds are deterministic: seed 0 -- the 16 base tables, the signature table and both MLP vectors are tampered from their pristine copy
    (tamper.Tamper), the key is verified (release.verify) and held-out view `view` is rendered and compared with the untampered release's (metrics.psnr:
    an attack that destroys the picture is not an attack on the watermark; +inf where the render is bit-equal).
    -> {(kind, strength, seed): {"bit_accuracy", "matches", "p_value", "psnr"}}.  The stage's model is left untouched."""
    from . import metrics, release as rel
    model, dev, H, W = stage["model"], stage["device"], stage["H"], stage["W"]
    released = rel.release(model, message, copy=True)
    key = rel.SignatureKey.from_block_rays(message, model.msg_decoder, stage["block_o"], stage["block_d"], stage["render_kwargs"])
    r = rays.get_rays(stage["test_poses"][view:view + 1], stage["intr"], H, W, -1)
    full = lambda: released.render(r["rays_o"], r["rays_d"], staged=True, bg_color=1, perturb=False, force_all_rays=True, **stage["render_kwargs"])["image"] \
        .reshape(1, H, W, 3).clamp(0, 1)
    truth = full()
    tamper = released.tamper()
    out = {}
    for kind, strength in attacks:
        for seed in (seeds if kind == "noise" else (0,)):
            tamper.apply(kind, strength, seed=seed)
            v = rel.verify(released, key)
            out[(kind, strength, seed)] = {"bit_accuracy": v["bit_accuracy"], "matches": v["matches"], "p_value": v["p_value"], "psnr": float(metrics.psnr(full(), truth))}
    tamper.restore()
    return out


def _timed_ms(fn, warmup=2, repeats=5):
    """[ms] of `repeats` runs of fn() after `warmup` untimed ones, each between device synchronisations (wall clock around a drained queue)."""
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


@torch.no_grad()
def packed_report(stage, message, formats=("f16", "q8", "q4"), view=0, repeats=5, directory=None):
    """What the packed forms of stage['model'] released under `message` cost and keep (release.pack).  Per format, and under "fp32" for the
    fp32 release measured the same way in the same process (the yardstick):
      "bytes"             the saved checkpoint's size (written to `directory`, a temporary one by default, and removed)
      "verify"            release.verify's dict against the key of the stage's block rays (whether q4 keeps every bit is REPORTED here, asserted nowhere)
      "psnr"              held-out view `view` against the fp32 release's render of it (metrics.psnr; +inf where bit-equal: the "fp32" entry)
      "render_ms"         median milliseconds of one staged full-view render; "render_ms_all": the `repeats` timings behind it (the spread)"""
    import os
    import tempfile
    from . import metrics, release as rel
    model, H, W = stage["model"], stage["H"], stage["W"]
    released = rel.release(model, message)
    key = rel.SignatureKey.from_block_rays(message, model.msg_decoder, stage["block_o"], stage["block_d"], stage["render_kwargs"])
    r = rays.get_rays(stage["test_poses"][view:view + 1], stage["intr"], H, W, -1)
    full = lambda m: m.render(r["rays_o"], r["rays_d"], staged=True, bg_color=1, perturb=False, force_all_rays=True, **stage["render_kwargs"])["image"] \
        .reshape(1, H, W, 3).clamp(0, 1)
    truth = full(released)
    out = {}
    with tempfile.TemporaryDirectory(dir=directory) as tmp:
        for name in ("fp32", *formats):
            m = released if name == "fp32" else rel.pack(released, name)
            path = m.save(os.path.join(tmp, f"{name}.pth"))
            times = _timed_ms(lambda: full(m), repeats=repeats)
            out[name] = {"bytes": os.path.getsize(path), "verify": rel.verify(m, key), "psnr": float(metrics.psnr(full(m), truth)),
                         "render_ms": float(np.median(times)), "render_ms_all": [round(t, 3) for t in times]}
            os.remove(path)
    return out


def stage_key(stage, message):
    """The pose-and-blocks SignatureKey of a synthetic stage: synthetic.block_rays' pose (orbit_pose(1.1, 0.7, radius)) and the rectangles of its blocks in the scene's
    rows x cols grid, with the stage's decoder; a scene's stage (scene_stage) names its own pose and rectangles in "key_pose" / "block_coordinates".  Its rays are rebuilt on the device (rg_get_rays); they must equal the stage's block rays bit for bit -- the model was
    trained on those -- and a key whose rays differ is refused here."""
    from . import release as rel
    if stage.get("key_pose") is not None and stage.get("block_coordinates") is not None:      # a scene's stage (scene_stage) carries its own key view and blocks
        pose, coordinates = stage["key_pose"], stage["block_coordinates"]
    else:
        pose, coordinates = synthetic.block_pose(stage["scene"]), synthetic.block_coordinates(stage["scene"])
    key = rel.SignatureKey(message, stage["model"].msg_decoder.state_dict(), stage["intr"], stage["H"], stage["W"], np.asarray(pose, np.float32)[None], coordinates,
                           stage["render_kwargs"])
    o, d = key.block_rays(stage["device"])
    if not (torch.equal(o, stage["block_o"]) and torch.equal(d, stage["block_d"])):
        raise RuntimeError("stage_key: the key's block rays differ from the stage's (max |difference| of the directions: "
                           f"{float((d - stage['block_d']).abs().max()):.3g})")
    return key


@torch.no_grad()
def mesh_survival(stage, message, resolutions=(128, 256, 384), colors=("normal", "view"), min_triangles=8, threshold=10, near=0.05, quantize=True, occupancy=True):
    """Does the signature survive the export to a coloured mesh?  stage['model'] under `message` is turned into a mesh exactly as mesh.save_mesh does it -- mesh.lattice
    over aabb_infer at each of `resolutions`, marching cubes at `threshold` (a density, or "median": the median density of the lattice's occupied nodes) with normals, vertex colours, mesh.clean(min_triangles) -- and the mesh alone is
    verified against the stage's key (raster.verify_mesh: the key view rasterised, release.verify on its blocks).  colors: "normal" = the colour head seen against
    the normal (save_mesh's), "view" = seen from the key camera (raster.view_directions: the best case for the signature).  quantize: colours go through the PLY's
    bytes (mesh.quantize_colors) first; positions through float32.  occupancy: the lattice is cut to the cells the model's occupancy grid marks (mesh.occupied; density
    -1 elsewhere) -- a render never evaluates the field outside them, and the synthetic stage's geometry IS that grid: its random density head fills the whole box, and
    without the cut the mesh is a cube of noise around the ball the renders show.  The stage wants a surface: watermark_stage(opaque=True).  The mesh's key view is also compared with the field's own render of that view (the released
    model's, staged, white background; metrics.ImageMetrics).
    -> {"field": release.verify's record of the released FIELD (the yardstick), "cells": [one dict per (resolution, colouring): "resolution", "colors", "threshold", "V", "T",
        "matches", "bit_accuracy", "p_value", "psnr_db", "ssim", "culled": (near, guard)]}.  What survives is REPORTED here and asserted nowhere."""
    from . import mesh, raster, release as rel
    model, dev, H, W = stage["model"], stage["device"], stage["H"], stage["W"]
    key = stage_key(stage, message)
    pose = torch.from_numpy(key.poses[0]).to(dev)
    released = rel.release(model, message, copy=True)
    r = rays.get_rays(pose[None], stage["intr"], H, W, -1)
    truth = released.render(r["rays_o"], r["rays_d"], staged=True, bg_color=1, perturb=False, force_all_rays=True, **stage["render_kwargs"])["image"] \
        .reshape(1, H, W, 3).clamp(0, 1)
    out = {"field": rel.verify(released, key), "cells": []}
    bmin, bmax = model.aabb_infer[:3], model.aabb_infer[3:]
    for R in resolutions:
        u = mesh.lattice(model, bmin, bmax, R, message)
        occ = mesh.occupied(model, bmin, bmax, R) if occupancy else None
        thr = float(threshold) if threshold != "median" else float((u[occ] if occupancy else u.reshape(-1)).median())
        if occupancy:
            u = torch.where(occ, u, torch.full_like(u, -1.0))
        v, t, n = mesh.marching_cubes(u, thr, normals=True, scale=mesh.lattice_scale(bmin, bmax, R))
        del u
        world = mesh.world_vertices(v, bmin, bmax, R)
        for how in colors:
            if how not in ("normal", "view"):
                raise ValueError(f"mesh_survival: colouring '{how}' is neither 'normal' nor 'view'")
            rgb = mesh.vertex_colors(model, world, n, message, directions=raster.view_directions(world, pose) if how == "view" else None)
            if quantize:
                rgb = mesh.quantize_colors(rgb).float() / 255.0
            cv, ct, crgb = mesh.clean(v, t, min_triangles, attributes=(rgb,))
            cw = mesh.world_vertices(cv, bmin, bmax, R).float().contiguous()
            record, view = raster.verify_mesh(cw, ct, crgb.contiguous(), key, near=near, details=True)
            meter = ImageMetrics(dev)
            meter.update(view["image"].reshape(1, H, W, 3).clamp(0, 1), truth)
            m = meter.measure()
            out["cells"].append({"resolution": int(R), "colors": how, "threshold": thr, "V": int(cv.shape[0]), "T": int(ct.shape[0]), "matches": record["matches"],
                                 "bit_accuracy": record["bit_accuracy"], "p_value": record["p_value"], "psnr_db": m["psnr_db"], "ssim": m["ssim"],
                                 "culled": view["culled"]})
    return out


def test_views(stage, seed=9876, max_ray_batch=4096):
    """Trainer.test_image's loop (:816-933) as a generator of (pred, truth) [1, H, W, 3]: per test view a random message and
    eval_step(render_whole=True) -- the full view staged in max_ray_batch chunks -- beside the clean view."""
    model, D, dev, H, W = stage["model"], stage["D"], stage["device"], stage["H"], stage["W"]
    gen = torch.Generator(device="cpu").manual_seed(seed)
    for b in range(stage["test_poses"].shape[0]):
        with torch.no_grad():
            message = torch.randint(0, 2, (D,), generator=gen).float().to(dev)
            r = rays.get_rays(stage["test_poses"][b:b + 1], stage["intr"], H, W, -1)
            if stage["clean_test"] is None:      # (online targets: no pre-pass rendered the held-out views either)
                stage["clean_test"] = blocks.clean_render(model, stage["test_poses"], stage["intr"], H, W, stage["render_kwargs"], max_ray_batch=H * W) \
                    .reshape(-1, H, W, 3).clamp_(0, 1).contiguous()
            data = {"rays_o": r["rays_o"], "rays_d": r["rays_d"], "images": stage["clean_test"][b:b + 1], "H": H, "W": W}
            pred, _, gt, _, _, _, _ = trainer.eval_step(model, data, message, dict(stage["render_kwargs"], max_ray_batch=max_ray_batch), render_whole=True)
        yield pred, gt


def test_image(stage, seed=9876, max_ray_batch=4096):
    """Trainer.test_image (:816-933): the views of `test_views` against the clean views; PSNRMeter over the views.  Returns the mean PSNR in dB."""
    meter = PSNRMeter()
    for pred, gt in test_views(stage, seed, max_ray_batch):
        meter.update(pred, gt)
    return float(meter.measure())


def test_image_metrics(stage, seed=9876, max_ray_batch=4096, views=None, psnr_meter=None):
    """The same loop with PSNR and SSIM taken on the device (metrics.ImageMetrics) and one host read at the end -> {"psnr_db", "ssim"}, each the mean
    over the views.  views: (pred, truth) pairs to measure instead of rendering `test_views`; psnr_meter: a PSNRMeter fed the same views (its host copies)."""
    meter = ImageMetrics(stage["device"])
    for pred, gt in (test_views(stage, seed, max_ray_batch) if views is None else views):
        meter.update(pred, gt)
        if psnr_meter is not None:
            psnr_meter.update(pred, gt)
    m = meter.measure()
    return {"psnr_db": m["psnr_db"], "ssim": m["ssim"]}


test_views.__test__ = test_image.__test__ = test_image_metrics.__test__ = False


@torch.no_grad()
def scene_stage(model, scene, D=32, rows=16, cols=16, key_view=0, n_test=2, n_rays=4096, render_kwargs=None, test_poses=None):
    """watermark_stage for a model that was TRAINED on `scene` (a dataset.Scene: loaded from a directory, or procedural.dataset's): the same dict, built the way the
    reference's loader builds it.  Clean store: blocks.clean_render of the scene's poses (provider_wtmk.py:408-421).  Key: pose `key_view` and the D blocks of the
    rows x cols grid that blocks.process_image keeps of its clean render (the ones JPEG compresses worst); block_o / block_d: blocks.block_rays over rays.get_rays of
    that pose.  test_poses: the held-out cameras (default: the scene's first n_test).  Beside watermark_stage's fields: key_pose [4,4] float32 (numpy),
    block_coordinates int64 [D,4] (numpy) -- what stage_key builds the key from -- and scene=None."""
    dev = scene.poses.device
    H, W, intr = scene.H, scene.W, tuple(float(v) for v in scene.intrinsics)
    kw = dict(dt_gamma=0.0, max_steps=1024) if render_kwargs is None else dict(render_kwargs)
    poses = scene.poses.float().contiguous()
    test_poses = poses[:n_test].clone() if test_poses is None else test_poses.to(dev).float().contiguous()
    model.train()
    clean = blocks.clean_render(model, poses, intr, H, W, kw, max_ray_batch=H * W).reshape(poses.shape[0], H * W, 3).clamp_(0, 1).contiguous()
    clean_test = blocks.clean_render(model, test_poses, intr, H, W, kw, max_ray_batch=H * W).reshape(test_poses.shape[0], H, W, 3).clamp_(0, 1).contiguous()
    coordinates, bh, bw = blocks.process_image(clean[key_view].reshape(1, H, W, 3), rows, cols, D)
    if coordinates.shape[0] != D:
        raise ValueError(f"scene_stage: a {rows} x {cols} grid has {rows * cols} blocks, fewer than the {D} bits of the message")
    r = rays.get_rays(poses[key_view:key_view + 1], intr, H, W, -1)
    bo, bd = blocks.block_rays(r["rays_o"].reshape(1, H, W, 3), r["rays_d"].reshape(1, H, W, 3), coordinates)
    return dict(model=model, scene=None, device=dev, D=D, H=H, W=W, intr=intr, render_kwargs=kw, block_o=bo, block_d=bd, poses=poses, clean=clean,
                test_poses=test_poses, clean_test=clean_test, n_rays=n_rays, key_pose=poses[key_view].cpu().numpy(),
                block_coordinates=coordinates.cpu().numpy().astype(np.int64))


def _constant_image_psnr(truth):
    """PSNR [dB] of the best constant-colour picture of these views: the per-channel mean of `truth` [B,H,W,3] (values in [0, 1]) against it."""
    mean = truth.mean(dim=(0, 1, 2), keepdim=True)
    return float(-10.0 * torch.log10(((truth - mean) ** 2).mean()))


def train_clean_field(scene, bound=1.0, steps=1024, n_rays=4096, lr=README["lr"], ema_decay=0.95, seed=0, render_kwargs=None, lap=None):
    """The stage-1 recipe, once, for sign_scene and distill.distill: torch.manual_seed(seed), a fresh stage1.CleanNeRFNetwork of `bound`, mark_untrained_grid over the
    scene's cameras, Adam with betas (0.9, 0.99), stage1.GraphedCleanLoop over scene.sampler(n_rays, seed) with the grid refreshed on the device every 16 steps, the
    learning rate decayed over `steps` and the moving average of the weights on; `steps` steps with an overflow poll every 256.  lap: called as lap("capture") after
    the first step (set-up, sizing march and capture) and lap("train") after the last -- the caller's stopwatch, which synchronises.
    -> (model, loop, record): the loop is left OPEN (the caller evaluates or checkpoints under loop.ema_weights() and closes it); record: steps, samples_per_ray (the
    march's mean over the last 16 steps), overflowed."""
    from . import stage1
    dev = scene.poses.device
    kw = dict(dt_gamma=0.0, max_steps=1024) if render_kwargs is None else dict(render_kwargs)
    lap = (lambda name: None) if lap is None else lap
    torch.manual_seed(seed)
    clean = stage1.CleanNeRFNetwork(bound=bound, cuda_ray=True, density_scale=1, min_near=0.2, density_thresh=10, bg_radius=-1).to(dev).train()
    clean.mark_untrained_grid(scene.poses, scene.intrinsics)
    optimizer = torch.optim.Adam(clean.get_params(lr), betas=(0.9, 0.99), eps=1e-15)
    loop = stage1.GraphedCleanLoop(clean, optimizer, kw, n_rays=n_rays, sampler=scene.sampler(n_rays, seed=seed), update_extra_interval=16, lr_lambda=lr_lambda(steps),
                                   headroom=1.0, seed=seed, device_refresh=True, ema_decay=ema_decay)
    loop.step()
    lap("capture")
    overflow = False
    for k in range(1, steps):
        loop.step()
        if k % 256 == 255:
            overflow = overflow or loop.overflowed()
    overflow = overflow or loop.overflowed()
    lap("train")
    samples_per_ray = float(loop.count_ring[:min(16, steps), 0].float().mean()) / n_rays
    return clean, loop, {"steps": steps, "samples_per_ray": samples_per_ray, "overflowed": bool(overflow)}


def sign_scene(scene, message, bound=1.0, stage1_steps=1024, stage2_steps=README["iters"], ema_decay=0.95, seed=0, workdir=None, held_out=None, rows=16, cols=16,
               key_view=0, n_rays=4096, lr=README["lr"], n_messages=50):
    """From a dataset.Scene to a released, signed, verified model -- both stages in one run:
      stage 1   a fresh stage1.CleanNeRFNetwork, mark_untrained_grid over the scene's cameras, stage1.GraphedCleanLoop over scene.sampler(n_rays) (RGBA when the
                store is: a random background per ray), the grid refreshed on the device every 16 steps, the moving average of the weights on;
      handover  under ema_weights(): checkpoint.save_checkpoint to <workdir>/stage1.pth (workdir=None: a temporary directory, removed), and the held-out views
                (held_out: a dataset.Scene with the same intrinsics; None: the scene's first two training views, record["held_out"] False) scored;
      stage 2   a fresh watermark NeRFNetwork of D = len(message) bits, checkpoint.load_checkpoint(model_only=True), mark_untrained_grid, scene_stage,
                train(stage, stage2_steps), release.release under `message`, stage_key (poses and blocks), release.verify.
    -> {"released", "key", "stage", "record", "clean"}; clean: {"model": the stage-1 model (its trained weights), "ema": copies of what was checkpointed, in the order
    of model.trainable(), "missing" / "unexpected": load_checkpoint's}.  record: stage1 {psnr_db, ssim, constant_psnr_db, steps, ms_per_step, samples_per_ray (the
    march's mean over the last 16 steps: the grid stage 2 marches), overflowed, recaptures}, stage2 {steps, ms_per_step, bit_acc_before_training, test_bitacc,
    psnr_db / ssim of the watermarked against the clean held-out views, overflowed}, verify, phases_s (wall seconds of each phase), overflowed (either loop)."""
    import os
    import tempfile
    from . import checkpoint, release as rel, stage1
    from .network import NeRFNetwork
    dev = scene.poses.device
    message = torch.as_tensor(message).detach().float().reshape(-1)
    D = int(message.numel())
    kw = dict(dt_gamma=0.0, max_steps=1024)
    phases, t0 = {}, time.perf_counter()

    def lap(name):
        nonlocal t0
        torch.cuda.synchronize()
        now = time.perf_counter()
        phases[name], t0 = now - t0, now

    # ---- stage 1
    clean, loop, rec1 = train_clean_field(scene, bound, stage1_steps, n_rays, lr, ema_decay, seed, kw, lap=lambda name: lap(f"stage1_{name}_s"))
    overflow1, samples_per_ray = rec1["overflowed"], rec1["samples_per_ray"]
    views = scene if held_out is None else held_out
    n_views = min(2, views.poses.shape[0]) if held_out is None else views.poses.shape[0]
    with tempfile.TemporaryDirectory() as tmp, loop.ema_weights():
        path = checkpoint.save_checkpoint(os.path.join(tmp if workdir is None else workdir, "stage1.pth"), clean)
        ema = [p.detach().clone() for p in clean.trainable()]
        meter, truths = ImageMetrics(dev), []
        clean.eval()      # as the reference's evaluate (nerf/utils.py:874): a model left in training mode marches a view with the training march, bounded by the mean
        for i in range(n_views):      # sample count of the last steps, and drops the rays that do not fit -- whole bands of a full view come out as background
            pred, _, gt, _ = stage1.eval_step(clean, views.view(i), kw)
            meter.update(pred.clamp(0, 1), gt)
            truths.append(gt)
        clean.train()
        m1 = meter.measure()
        lap("handover_s")
        # ---- stage 2
        torch.manual_seed(seed)
        model = NeRFNetwork(bound=bound, cuda_ray=True, density_scale=1, min_near=0.2, density_thresh=10, bg_radius=-1, message_dim=D, n_views=1)
        missing, unexpected, _ = checkpoint.load_checkpoint(path, model, model_only=True, map_location="cpu")
    loop.close()
    model.to(dev).train()
    model.mark_untrained_grid(scene.poses, scene.intrinsics)
    stage = scene_stage(model, scene, D=D, rows=rows, cols=cols, key_view=key_view, n_rays=n_rays, render_kwargs=kw, test_poses=views.poses[:n_views])
    lap("stage2_prepass_s")
    before = test_bitacc(stage, n_messages)[0]
    rec = train(stage, stage2_steps)
    lap("stage2_train_s")
    after = test_bitacc(stage, n_messages)
    marked = test_image_metrics(stage)
    released = rel.release(model, message.to(dev), copy=True)
    key = stage_key(stage, message)
    verdict = rel.verify(released, key)
    lap("evaluate_release_verify_s")
    record = {"stage1": {"steps": stage1_steps, "psnr_db": m1["psnr_db"], "ssim": m1["ssim"], "constant_psnr_db": _constant_image_psnr(torch.cat(truths, dim=0)),
                         "views": n_views, "held_out": held_out is not None, "ms_per_step": phases["stage1_train_s"] / max(stage1_steps - 1, 1) * 1e3,
                         "samples_per_ray": samples_per_ray, "overflowed": bool(overflow1), "recaptures": loop.recaptures},
              "stage2": {"steps": rec["steps"], "ms_per_step": rec["ms_per_step"], "capture_s": rec["prepare_s"], "bit_acc_before_training": before, "test_bitacc": after[0],
                         "wrong_bits_mean": after[1], "wrong_bits_worst_message": after[2], "psnr_db": marked["psnr_db"], "ssim": marked["ssim"],
                         "overflowed": bool(rec["overflowed"]), "recaptures": rec["recaptures"], "loss_image": rec["loss_image"], "loss_watermark": rec["loss_watermark"]},
              "verify": verdict, "phases_s": phases, "overflowed": bool(overflow1 or rec["overflowed"]), "D": D, "image": [scene.H, scene.W],
              "train_views": int(scene.poses.shape[0]), "blocks": [rows, cols]}
    return {"released": released, "key": key, "stage": stage, "record": record,
            "clean": {"model": clean, "ema": ema, "missing": missing, "unexpected": unexpected}}


def distillation_survival(stage_or_signed, message, views=(12, 50), steps=(1024,), H=None, W=None, channels=4, seed=0):
    """Does the signature survive distillation?  The pirate never touches the released weights: they render pictures from the released model and train a field of their
    own on them (distill.distill).  stage_or_signed: a stage (watermark_stage's / scene_stage's dict) or sign_scene's result.  The stage's model is released under
    `message` (a copy), the key is stage_key's, and release.verify of the released FIELD is the yardstick.  Then, per (views, steps) cell: `views` orbit cameras
    (distill.orbit_cameras at the mean distance of the stage's own cameras, seed `seed`; the key pose is not among them) of H x W pixels (default: the stage's; another
    size scales the intrinsics) -> distill -> release.verify(distill.student_render(student), key).
    -> {"field": the verdict on the released field, "cells": [one dict per cell: "views", "steps", "matches", "bit_accuracy", "p_value", "psnr_db" and "ssim" (the
        student against the teacher's renders of two held-out cameras), "ms_per_step", "constant_psnr_db", "overflowed", "store_bytes"]}.
    What survives is REPORTED here and asserted nowhere, as in mesh_survival."""
    from . import distill as dst, release as rel
    stage = stage_or_signed["stage"] if "stage" in stage_or_signed else stage_or_signed
    model, dev, kw = stage["model"], stage["device"], stage["render_kwargs"]
    message = torch.as_tensor(message).detach().float().reshape(-1)
    released = rel.release(model, message.to(dev), copy=True)
    key = stage_key(stage, message)
    out = {"field": rel.verify(released, key), "cells": []}
    H0, W0 = stage["H"], stage["W"]
    H, W = (H0 if H is None else int(H)), (W0 if W is None else int(W))
    fx, fy, cx, cy = stage["intr"]
    intr = (fx * W / W0, fy * H / H0, cx * W / W0, cy * H / H0)
    if stage.get("poses") is not None:
        radius = float(stage["poses"][:, :3, 3].double().norm(dim=-1).mean())
    else:
        radius = float(stage["radius"])
    for n_views in views:
        for n_steps in steps:
            got = dst.distill(released, dst.orbit_cameras(n_views, radius, seed), intr, H, W, steps=int(n_steps), channels=channels, bound=model.bound,
                              n_rays=stage["n_rays"], seed=seed, render_kwargs=kw)
            v, r = rel.verify(dst.student_render(got["student"], kw), key), got["record"]
            out["cells"].append({"views": int(n_views), "steps": int(n_steps), "matches": v["matches"], "bit_accuracy": v["bit_accuracy"], "p_value": v["p_value"],
                                 "psnr_db": r["psnr_db"], "ssim": r["ssim"], "ms_per_step": r["ms_per_step"], "constant_psnr_db": r["constant_psnr_db"],
                                 "overflowed": r["overflowed"], "store_bytes": r["store_bytes"]})
            del got
    return out


LAST_STAGE = None      # (tools/converge.py's two-rank run compares the ranks' final models)


def run(mode="graphed", steps=None, scene="hotdog", n_messages=200, online_targets=False, **train_kw):
    """watermark_stage + train + both evaluations -> the `quality` record of bench.py.  online_targets: see watermark_stage."""
    global LAST_STAGE
    stage = LAST_STAGE = watermark_stage(scene, online_targets=online_targets)
    before = test_bitacc(stage, min(n_messages, 50))[0]
    rec = train(stage, steps, mode, **train_kw)
    t0 = time.perf_counter()
    acc, wrong_mean, wrong_max = test_bitacc(stage, n_messages)
    distorted = None
    if train_kw.get("distortion", "none") != "none":      # the reference's eval_step distorts the evaluated blocks too (utils_wtmk_disen.py:666)
        distorted = test_bitacc(stage, n_messages, distortion=train_kw["distortion"])[0]
    host_psnr = PSNRMeter()        # the record's PSNR stays the reference meter's; SSIM comes from the same renders
    ssim = test_image_metrics(stage, psnr_meter=host_psnr)["ssim"]
    psnr = float(host_psnr.measure())
    torch.cuda.synchronize()
    sel = [c for c in rec["adam_steps"]]
    return {"mode": mode, "online_targets": bool(online_targets), "steps": rec["steps"], "bit_acc": acc, "wrong_bits_mean": wrong_mean, "wrong_bits_worst_message": wrong_max, "psnr_db": psnr, "ssim": ssim,
            **({} if distorted is None else {"bit_acc_distorted_blocks": distorted}),
            "wall_s": rec["wall_s"], "capture_s": rec["prepare_s"], "train_ms_per_step": rec["ms_per_step"], "eval_wall_s": time.perf_counter() - t0, "bit_acc_before_training": before,
            "n_messages": n_messages, "n_test_views": int(stage["test_poses"].shape[0]), "overflowed": rec["overflowed"], "recaptures": rec["recaptures"],
            "adam_steps_total": sum(sel), "adam_steps_min_max": [min(sel), max(sel)], "loss_image": rec["loss_image"], "loss_watermark": rec["loss_watermark"],
            "loss_log": [(k, round(a, 8), round(b, 5)) for k, a, b in rec["log"]],
            "hyper_parameters": {"lambda_w": train_kw.get("lambda_w", README["lambda_w"]), "lambda_i": train_kw.get("lambda_i", README["lambda_i"]),
                                 "lr": train_kw.get("lr", README["lr"]), "lr_schedule": "0.1 ** min(it / iters, 1)", "iters": train_kw.get("iters") or rec["steps"],
                                 "codebook_init": "U(-1e-4, 1e-4)", "decoder_init": "torch default (random)", "distortion": train_kw.get("distortion", "none")},
            "what": "scene S0 (random frozen field), README.md:45 hyper-parameters; bit accuracy over random messages as Trainer.test_bitacc, PSNR of the "
                    "watermarked full views against the clean views as Trainer.test_image"}
