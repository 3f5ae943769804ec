"""Distillation (model extraction): a fresh field trained on nothing but pictures rendered from a released model.

    cameras = orbit_cameras(50, radius=2.2, seed=3)                                  # the pirate's cameras, not the dataset's
    scene = teacher_dataset(released, cameras, intrinsics, H, W, channels=4)         # a dataset.Scene: the teacher's views as store bytes (rm_finish_u8)
    out = distill(released, cameras, intrinsics, H, W, steps=1024)                   # {"student", "scene", "record"}
    release.verify(student_render(out["student"]), key)                              # what the signer then finds in the copy

The attacker holds the released model and nothing else: no key, no decoder, no training data.  The teacher is only rendered (eval march, no gradients), the student
is a fresh stage1.CleanNeRFNetwork trained by the stage-1 recipe of quality.sign_scene (quality.train_clean_field), the verdict is release.verify's.  The teacher's
float pictures never exist as a whole: each view's compositor outputs go through rm_finish_u8 (csrc/composite.hip) straight into its slice of one uint8 [P,H,W,C]
store, the form the device samplers draw from."""
import time

import numpy as np
import torch

from . import _native as nv
from . import dataset as ds
from . import rays

RENDER_KWARGS = dict(dt_gamma=0.0, max_steps=1024)
HELD_OUT_SEED = 7919      # the default held-out cameras: orbit_cameras(2, radius, HELD_OUT_SEED + seed)


def orbit_cameras(n, radius, seed, theta=None):
    """n seeded orbit poses at `radius` -> float32 [n,4,4] (numpy): procedural.orbit_poses with the polar range of the stage's own cameras (quality.ORBIT_THETA) unless
    `theta` = (lo, hi) says otherwise.  The key pose is among them only if the caller puts it there."""
    from . import procedural, quality
    return procedural.orbit_poses(int(n), float(radius), quality.ORBIT_THETA if theta is None else tuple(theta), seed)


def finish_u8(image, weights_sum, channels=4, bg=(1.0, 1.0, 1.0), out=None):
    """rm_finish_u8: a compositor's image [N,3] (premultiplied: rendered against background 0) and weights_sum [N] -> uint8 [N,channels] store bytes, straight alpha
    for channels=4, over `bg` for channels=3 (include/nerfsig.h has the arithmetic).  out: a contiguous uint8 tensor of N*channels bytes to write into (any view of
    a store)."""
    image, weights_sum = image.detach(), weights_sum.detach()
    if not (image.is_cuda and image.dtype == torch.float32 and weights_sum.is_cuda and weights_sum.dtype == torch.float32):
        raise ValueError("finish_u8: image and weights_sum must be float32 tensors on the GPU (there is no CPU path)")
    N, C = int(weights_sum.numel()), int(channels)
    if image.numel() != 3 * N:
        raise ValueError(f"finish_u8: image has {image.numel()} values for {N} rays (3 per ray)")
    bg = tuple(float(v) for v in bg)
    if len(bg) != 3:
        raise ValueError("finish_u8: bg takes three numbers")
    if out is None:
        out = torch.empty((N, C), dtype=torch.uint8, device=image.device)
    elif not (out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous() and out.numel() == N * C):
        raise ValueError(f"finish_u8: out must be a contiguous uint8 tensor of {N * C} bytes on the GPU")
    nv.call("rm_finish_u8", nv.ptr(image.contiguous()), nv.ptr(weights_sum.contiguous()), N, C, bg[0], bg[1], bg[2], nv.ptr(out), nv.stream())
    return out


def _device_of(model):
    for t in model.parameters():
        return t.device
    for t in model.buffers():
        return t.device
    raise ValueError("the model holds no tensor to take a device from")


@torch.no_grad()
def teacher_view(render, rays_o, rays_d, render_kwargs=None, max_ray_batch=None):
    """The one render call teacher_dataset makes per view: staged, background 0, unperturbed, every ray, the model in eval() (its mode is restored) ->
    {"image" [1,N,3]: the raw premultiplied sum, "weights_sum" [1,N], "depth"}."""
    kw = dict(RENDER_KWARGS if render_kwargs is None else render_kwargs)
    was_training = render.training
    render.eval()
    try:
        out = render.render(rays_o, rays_d, staged=True, max_ray_batch=int(rays_o.shape[1] if max_ray_batch is None else max_ray_batch), bg_color=0, perturb=False,
                            force_all_rays=True, return_weights_sum=True, **kw)
    finally:
        render.train(was_training)
    if "weights_sum" not in out:
        raise TypeError("teacher_dataset: the model's render(..., return_weights_sum=True) returned no 'weights_sum' (renderer.NeRFRenderer's does)")
    return out


@torch.no_grad()
def teacher_dataset(render, poses, intrinsics, H, W, channels=4, bg=(1.0, 1.0, 1.0), render_kwargs=None, max_ray_batch=None):
    """The views of `poses` [P,4,4] as a model renders them, as a dataset.Scene over one preallocated uint8 [P,H,W,channels] store: per pose rays.get_rays, teacher_view,
    rm_finish_u8 into the pose's slice -- no float copy of the store exists at any time.  render: a release.ReleasedModel, a PackedReleasedModel or any
    renderer.NeRFRenderer.  channels=4 stores straight colour and the render's own alpha (weights_sum), channels=3 the view over `bg`.  max_ray_batch: rays per
    staged chunk (default: the whole view).  The Scene has the poses, the intrinsics, radius = the mean camera distance as load_scene forms it, mode "blender" and
    no files: sampler(), view(i) and procedural.write_scene take it as they take a loaded scene."""
    dev = _device_of(render)
    if dev.type != "cuda":
        raise ValueError("teacher_dataset: the model must be on the GPU (there is no CPU path)")
    P_host = torch.as_tensor(np.asarray(poses.detach().cpu() if torch.is_tensor(poses) else poses, dtype=np.float32)).reshape(-1, 4, 4)
    P, H, W, C = int(P_host.shape[0]), int(H), int(W), int(channels)
    if P < 1 or H < 1 or W < 1:
        raise ValueError(f"teacher_dataset: {P} views of {H} x {W} pixels")
    if C not in (3, 4):
        raise ValueError(f"teacher_dataset: channels={C} is not 3 or 4")
    intrinsics = tuple(float(v) for v in intrinsics)
    centres = P_host[:, :3, 3].double()
    radius = sum(float(v) for v in (centres * centres).sum(-1).sqrt()) / P
    poses_dev = P_host.to(dev).contiguous()
    store = torch.empty((P, H, W, C), dtype=torch.uint8, device=dev)
    for p in range(P):
        r = rays.get_rays(poses_dev[p:p + 1], intrinsics, H, W, -1)
        out = teacher_view(render, r["rays_o"], r["rays_d"], render_kwargs, max_ray_batch)
        finish_u8(out["image"], out["weights_sum"], C, bg, out=store[p])
    return ds.Scene(poses_dev, store, intrinsics, H, W, radius, "blender", [])


@torch.no_grad()
def _white_view(model, rays_o, rays_d, render_kwargs):
    """[.., 3] of the rays against white: staged, unperturbed, the model in eval() (its mode is restored)."""
    o, d = rays_o.reshape(1, -1, 3), rays_d.reshape(1, -1, 3)
    was_training = model.training
    model.eval()
    try:
        out = model.render(o, d, staged=True, max_ray_batch=min(int(o.shape[1]), 1 << 18), bg_color=1, perturb=False, force_all_rays=True, **render_kwargs)
    finally:
        model.train(was_training)
    return out["image"].reshape(*rays_o.shape[:-1], 3)


def student_render(student, render_kwargs=None):
    """The (rays_o, rays_d) -> image closure release.verify takes for a suspect model: the student's staged render against white in eval() mode."""
    kw = dict(RENDER_KWARGS if render_kwargs is None else render_kwargs)
    return lambda rays_o, rays_d: _white_view(student, rays_o, rays_d, kw)


def distill(teacher, poses, intrinsics, H, W, *, steps=1024, channels=4, bound=1.0, n_rays=4096, seed=0, ema_decay=0.95, lr=None, held_out_poses=None,
            render_kwargs=None):
    """The attack: teacher_dataset of `poses`, then a fresh stage1.CleanNeRFNetwork trained on that store by quality.train_clean_field -- the stage-1 recipe of
    quality.sign_scene, nothing added -- for `steps` steps.  -> {"student": under its EMA weights (ema_decay=None: the trained ones) and in eval(), "scene": the
    teacher's store, "record"}.  record: steps, ms_per_step, samples_per_ray, overflowed, recaptures, psnr_db / ssim of the student against the TEACHER's own renders
    of held_out_poses (metrics.ImageMetrics, both against white; default: orbit_cameras(2, the poses' mean distance, HELD_OUT_SEED + seed), re-drawn should one
    coincide with a training pose), constant_psnr_db (the best constant picture of those renders), store_bytes, views, phases_s."""
    from . import quality
    from .metrics import ImageMetrics
    kw = dict(RENDER_KWARGS if render_kwargs is None else render_kwargs)
    lr = quality.README["lr"] if lr is None else lr
    phases, t0 = {}, time.perf_counter()

    def lap(name):
        nonlocal t0
        torch.cuda.synchronize()
        now = time.perf_counter()
        phases[f"{name}_s"], t0 = now - t0, now

    scene = teacher_dataset(teacher, poses, intrinsics, H, W, channels, render_kwargs=kw)
    lap("teacher_views")
    student, loop, rec = quality.train_clean_field(scene, bound, steps, n_rays, lr, ema_decay, seed, kw, lap=lap)
    if loop.ema_parameters() is not None:
        with torch.no_grad():
            for p, s in zip(student.trainable(), loop.ema_parameters()):
                p.copy_(s)
    recaptures = loop.recaptures
    loop.close()
    student.eval()
    dev = scene.poses.device
    if held_out_poses is None:
        train, s = scene.poses.cpu().numpy(), HELD_OUT_SEED + seed
        held = orbit_cameras(2, scene.radius, s)
        while any(np.array_equal(h, t) for h in held for t in train):
            s += 1
            held = orbit_cameras(2, scene.radius, s)
    else:
        held = np.asarray(held_out_poses.detach().cpu() if torch.is_tensor(held_out_poses) else held_out_poses, dtype=np.float32).reshape(-1, 4, 4)
    held = torch.from_numpy(np.ascontiguousarray(held)).to(dev)
    meter, truths = ImageMetrics(dev), []
    for i in range(held.shape[0]):
        r = rays.get_rays(held[i:i + 1], scene.intrinsics, scene.H, scene.W, -1)
        truth = _white_view(teacher, r["rays_o"], r["rays_d"], kw).reshape(1, scene.H, scene.W, 3).clamp(0, 1)
        pred = _white_view(student, r["rays_o"], r["rays_d"], kw).reshape(1, scene.H, scene.W, 3).clamp(0, 1)
        meter.update(pred, truth)
        truths.append(truth)
    m = meter.measure()
    lap("evaluate")
    record = {"steps": rec["steps"], "ms_per_step": phases["train_s"] / max(steps - 1, 1) * 1e3, "samples_per_ray": rec["samples_per_ray"],
              "overflowed": rec["overflowed"], "recaptures": recaptures, "psnr_db": m["psnr_db"], "ssim": m["ssim"],
              "constant_psnr_db": quality._constant_image_psnr(torch.cat(truths, dim=0)), "held_out_views": int(held.shape[0]),
              "store_bytes": int(scene.images.numel()), "views": int(scene.poses.shape[0]), "image": [scene.H, scene.W], "channels": int(channels), "phases_s": phases}
    return {"student": student, "scene": scene, "record": record}
