"""Analytic scenes whose pictures are known exactly: spheres and axis-aligned boxes, Lambert shading, a checker texture, ray-cast on the GPU straight into the
uint8 [P,H,W,C] store that dataset.Scene and the device samplers use (csrc/procedural.hip; include/nerfsig.h, "procedural scenes").

    scene = SCENES["plinth"]
    images = render(scene, poses, intrinsics, H, W, channels=4, samples=2)       # uint8 [P,H,W,4] on the poses' device
    store = dataset(scene, 12, 192, 192, focal=230.0, radius=2.2)                # a dataset.Scene: store.sampler(...), store.view(i)
    write_scene(store, "out/plinth")                                            # a Blender-layout directory that dataset.load_scene(path, scale=1, offset=(0, 0, 0)) reads back

There is no dataset in the build or test environment and nothing can be fetched; this is the ground truth stage 1 can be trained to (quality.sign_scene).  The
picture is a single-valued function of its arguments (tests/procedural_ref.py restates it from the header and tests compare by equality)."""
import json
import math
import os

import numpy as np
import torch

from . import _native as nv

MAX_PRIMS, PRIM_WORDS, MAX_SIDE = 16, 16, 4096
SPHERE, BOX = 0, 1
FLAT, CHECKER = 0, 1


def sphere(centre, radius, color, color_b=None, frequency=0.0):
    """One row of the primitive table: a sphere; with color_b a checker of cell size 1 / frequency between the two colours."""
    return _row(SPHERE, centre, (radius, 0.0, 0.0), color, color_b, frequency)


def box(lo, hi, color, color_b=None, frequency=0.0):
    """One row of the primitive table: the axis-aligned box [lo, hi]."""
    return _row(BOX, lo, hi, color, color_b, frequency)


def _row(kind, a, b, color, color_b, frequency):
    texture = FLAT if color_b is None else CHECKER
    return [float(kind), float(texture), float(frequency), 0.0, *(float(v) for v in a), *(float(v) for v in b), *(float(v) for v in color),
            *(float(v) for v in (color if color_b is None else color_b))]


class ProceduralScene:
    """primitives: up to 16 rows of 16 numbers (sphere() / box(); the header's layout), light: the direction towards the light, ambient in [0, 1].  Refuses what
    ps_render_u8 refuses, by the same rules, before anything reaches the device."""

    def __init__(self, primitives, light=(0.4, 1.0, 0.5), ambient=0.25):
        prims = np.asarray(primitives, dtype=np.float64).reshape(-1, PRIM_WORDS) if len(primitives) else np.zeros((0, PRIM_WORDS))
        if prims.shape[0] > MAX_PRIMS:
            raise ValueError(f"ProceduralScene: {prims.shape[0]} primitives; at most {MAX_PRIMS}")
        prims = prims.astype(np.float32)
        if not np.isfinite(prims).all():
            raise ValueError("ProceduralScene: every parameter of a primitive must be finite")
        for k, q in enumerate(prims):
            if q[0] not in (SPHERE, BOX) or q[1] not in (FLAT, CHECKER):
                raise ValueError(f"ProceduralScene: primitive {k}: kind {q[0]:g} / texture {q[1]:g} (kinds 0 sphere, 1 box; textures 0 flat, 1 checker)")
            if q[0] == SPHERE and not q[7] > 0:
                raise ValueError(f"ProceduralScene: primitive {k}: radius {q[7]:g} is not > 0")
            if q[0] == BOX and not (q[4:7] <= q[7:10]).all():
                raise ValueError(f"ProceduralScene: primitive {k}: box lo > hi")
        light = np.asarray(light, dtype=np.float32).reshape(3)
        if not np.isfinite(light).all() or not light.any():
            raise ValueError("ProceduralScene: the light must be a finite vector other than zero")
        if not 0.0 <= float(ambient) <= 1.0:
            raise ValueError(f"ProceduralScene: ambient={ambient!r} outside [0, 1]")
        self.prims, self.light, self.ambient = np.ascontiguousarray(prims), light, float(np.float32(ambient))


# +y is up (synthetic.orbit_pose's world); everything lies inside bound 1
SCENES = {
    "plinth": ProceduralScene([
        box((-0.6, -0.5, -0.6), (0.6, -0.2, 0.6), (0.85, 0.82, 0.75), (0.25, 0.3, 0.45), frequency=5.0),        # the checker slab under the origin
        sphere((0.0, 0.1, 0.0), 0.3, (0.9, 0.35, 0.2), (0.95, 0.85, 0.3), frequency=8.0),                          # resting on it
        sphere((0.36, -0.08, 0.3), 0.12, (0.2, 0.65, 0.4)),                                                        # a smaller one, off-centre
        box((-0.5, -0.2, -0.45), (-0.25, 0.05, -0.2), (0.3, 0.4, 0.85)),                                           # a small flat-coloured box
    ]),
}


@torch.no_grad()
def render(scene, poses, intrinsics, H, W, channels=4, samples=2, bg=None, out=None):
    """uint8 [P,H,W,channels] on the poses' device (ps_render_u8).  poses: float32 [P,4,4] on the GPU; bg: the colour behind the scene for channels=3 (default
    white); out: a uint8 buffer of exactly P*H*W*channels bytes to write into."""
    if not (torch.is_tensor(poses) and poses.is_cuda and poses.dtype == torch.float32 and poses.dim() == 3 and tuple(poses.shape[1:]) == (4, 4)):
        raise ValueError("procedural.render: poses must be a float32 tensor [P,4,4] on the GPU (there is no CPU path)")
    poses = poses.contiguous()
    P, H, W, C, S = int(poses.shape[0]), int(H), int(W), int(channels), int(samples)
    fx, fy, cx, cy = (float(v) for v in intrinsics)
    bg = (1.0, 1.0, 1.0) if bg is None else tuple(float(v) for v in bg)
    if len(bg) != 3:
        raise ValueError("procedural.render: bg takes three numbers")
    if out is None:
        out = torch.empty((P, H, W, C) if P * H * W * C > 0 else (0,), dtype=torch.uint8, device=poses.device)
    elif not (out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous() and out.numel() == P * H * W * C):
        raise ValueError(f"procedural.render: out must be a contiguous uint8 tensor of {P * H * W * C} bytes on the GPU")
    K = int(scene.prims.shape[0])
    table = scene.prims.ctypes.data_as(nv._vp) if K else None
    nv.call("ps_render_u8", nv.ptr(poses), P, fx, fy, cx, cy, H, W, table, K, float(scene.light[0]), float(scene.light[1]), float(scene.light[2]), scene.ambient,
            S, C, bg[0], bg[1], bg[2], nv.ptr(out), nv.stream())
    return out.view(P, H, W, C)


def orbit_poses(n, radius, theta, seed):
    """n poses of synthetic.orbit_pose under one seeded RandomState: polar angle uniform in `theta`, azimuth in [0, 2 pi) -> float32 [n,4,4] (numpy)."""
    from . import synthetic
    rng = np.random.RandomState(seed)
    return np.stack([synthetic.orbit_pose(theta[0] + (theta[1] - theta[0]) * rng.rand(), 2 * math.pi * rng.rand(), radius) for _ in range(n)]).astype(np.float32)


def dataset(scene, n_poses, H, W, focal, radius, theta=None, seed=0, channels=4, samples=2, bg=None, device="cuda"):
    """A dataset.Scene of `n_poses` seeded orbit views of `scene`: mode "procedural", files [], radius the mean camera distance as load_scene forms it."""
    from . import dataset as ds, quality
    theta = quality.ORBIT_THETA if theta is None else theta
    poses = torch.from_numpy(orbit_poses(n_poses, radius, theta, seed))
    intrinsics = (float(focal), float(focal), W / 2, H / 2)
    centres = poses[:, :3, 3].double()
    mean_radius = sum(float(v) for v in (centres * centres).sum(-1).sqrt()) / len(centres)
    poses = poses.to(device)
    images = render(scene, poses, intrinsics, H, W, channels, samples, bg)
    return ds.Scene(poses, images, intrinsics, int(H), int(W), mean_radius, "procedural", [])


def file_matrix(pose):
    """The transform_matrix whose dataset.ngp_pose(., scale=1, offset=(0, 0, 0)) is `pose`: ngp_pose's row permutation and sign flips undone."""
    pose = np.asarray(pose, dtype=np.float32)
    m = np.zeros((4, 4), dtype=np.float32)
    for r, src in enumerate((1, 2, 0)):
        m[src, 0], m[src, 1], m[src, 2], m[src, 3] = pose[r, 0], -pose[r, 1], -pose[r, 2], pose[r, 3]
    m[3, 3] = 1.0
    return m


def write_scene(scene_store, path, split="train"):
    """Writes a dataset.Scene as a Blender-layout directory: transforms_<split>.json (camera_angle_x, and the exact fl_x / fl_y / cx / cy / h / w beside it) and
    one PNG per view under <split>/, through PIL.  dataset.load_scene(path, split, scale=1, offset=(0, 0, 0)) gives back the same bytes and poses: a float32
    survives JSON's decimal form, and ngp_pose with scale 1 and offset 0 only permutes and negates."""
    from PIL import Image
    images, poses = scene_store.images.cpu().numpy(), scene_store.poses.cpu().numpy()
    P, H, W, C = images.shape
    fx, fy, cx, cy = scene_store.intrinsics
    os.makedirs(os.path.join(path, split), exist_ok=True)
    frames = []
    for p in range(P):
        name = f"r_{p:03d}"
        Image.fromarray(images[p], mode="RGBA" if C == 4 else "RGB").save(os.path.join(path, split, name + ".png"))
        frames.append({"file_path": f"./{split}/{name}", "transform_matrix": [[float(v) for v in row] for row in file_matrix(poses[p])]})
    transform = {"camera_angle_x": 2.0 * math.atan(W / (2.0 * fx)), "fl_x": fx, "fl_y": fy, "cx": cx, "cy": cy, "h": H, "w": W, "frames": frames}
    out = os.path.join(path, f"transforms_{split}.json")
    with open(out, "w") as f:
        json.dump(transform, f, indent=1)
    return out
