"""The scene loader restated in numpy (nerf_signature_amd/dataset.py load_scene; the reference's NeRFDataset.__init__, nerf/provider.py:114-274), the tiny scene
directories the tests write, and what one draw of a sampler over a loaded scene must hand out.  Written apart from the loader: loops over pixels and matrix entries
where the loader uses array operations."""
import json
import math
import os

import numpy as np

import orbit_ref
import random_bg_ref as rb


# ---- scenes on disk
def frame_matrix(k):
    """A camera-to-world matrix with no zero entry in its upper 3 x 4 (so every sign and row of the permutation shows)."""
    rng = np.random.RandomState(100 + k)
    m = rng.uniform(0.1, 1.0, (4, 4)) * np.where(rng.rand(4, 4) < 0.5, -1.0, 1.0)
    m[3] = [0, 0, 0, 1]
    return m.tolist()


def frame_image(k, h, w, C):
    """uint8 [h, w, C]: random codes."""
    return np.random.RandomState(7 * k + C).randint(0, 256, (h, w, C)).astype(np.uint8)


def write_scene(root, mode, C=3, h=5, w=7, frames=3, size_keys=True, focal=None, centre=False, missing=(), suffix=True, splits=("train", "val", "test"), ext=".png"):
    """A scene directory under `root` (created).  mode 'colmap': transforms.json with `frames` frames; 'blender': transforms_<split>.json for every split, `frames`
    frames each (frame numbers run on across the splits).  focal: dict of the focal keys to write (default camera_angle_x = 0.8).  size_keys: write h / w.
    centre: write cx / cy.  missing: frame numbers whose image file is not written.  suffix=False: a blender scene's file_path entries carry no '.png' (the suffix
    rule adds it); a colmap scene's always do.  Returns {frame number: image}."""
    from PIL import Image
    os.makedirs(os.path.join(root, "images"), exist_ok=True)
    head = dict({"camera_angle_x": 0.8} if focal is None else focal)
    if size_keys:
        head.update(h=h, w=w)
    if centre:
        head.update(cx=w / 2 + 0.25, cy=h / 2 - 0.5)
    written, k = {}, 0
    for name in (("transforms.json",) if mode == "colmap" else tuple(f"transforms_{s}.json" for s in splits)):
        entries = []
        for _ in range(frames):
            stem = f"images/r_{k}"
            if k not in missing:
                img = frame_image(k, h, w, C)
                Image.fromarray(img, "RGB" if C == 3 else "RGBA").save(os.path.join(root, stem + ext))
                written[k] = img
            entries.append({"file_path": stem + (ext if (suffix or mode == "colmap") else ""), "transform_matrix": frame_matrix(k)})
            k += 1
        with open(os.path.join(root, name), "w") as f:
            json.dump(dict(head, frames=entries), f)
    return written


# ---- the loader, restated
def ngp_pose(m, scale, offset):
    """provider.py:19-27 entry by entry; the translation in Python floats (float64), rounded once."""
    m = np.array(m, dtype=np.float32)
    out = np.zeros((4, 4), dtype=np.float32)
    for row, src in ((0, 1), (1, 2), (2, 0)):
        out[row, 0] = m[src, 0]
        out[row, 1] = -m[src, 1]
        out[row, 2] = -m[src, 2]
        out[row, 3] = np.float32(float(m[src, 3]) * scale + offset[row])
    out[3] = [0, 0, 0, 1]
    return out


def box_mean(img, f):
    """Integer box mean pixel by pixel: (sum + f*f//2) // (f*f)."""
    H, W, C = img.shape[0] // f, img.shape[1] // f, img.shape[2]
    out = np.zeros((H, W, C), dtype=np.uint8)
    for r in range(H):
        for c in range(W):
            for ch in range(C):
                s = sum(int(img[r * f + i, c * f + j, ch]) for i in range(f) for j in range(f))
                out[r, c, ch] = (s + (f * f) // 2) // (f * f)
    return out


def expected(root, split="train", scale=0.33, offset=(0, 0, 0), downscale=1):
    """dict(poses, images, intrinsics, H, W, radius, mode, files) of a scene written by write_scene."""
    from PIL import Image
    mode = "colmap" if os.path.exists(os.path.join(root, "transforms.json")) else "blender"
    load = lambda name: json.load(open(os.path.join(root, name)))
    if mode == "colmap":
        t = load("transforms.json")
        frames = {"train": t["frames"][1:], "val": t["frames"][:1]}.get(split, t["frames"])
    else:
        names = {"trainval": ["transforms_train.json", "transforms_val.json"], "all": sorted(n for n in os.listdir(root) if n.endswith(".json"))}.get(split, [f"transforms_{split}.json"])
        t = load(names[0])
        frames = [fr for n in names for fr in load(n)["frames"]]
    poses, images, files = [], [], []
    H = W = None
    if "h" in t and "w" in t:
        H, W = int(t["h"]) // downscale, int(t["w"]) // downscale
    for fr in frames:
        p = os.path.join(root, fr["file_path"])
        if mode == "blender" and "." not in os.path.basename(p):
            p += ".png"
        if not os.path.exists(p):
            continue
        img = np.array(Image.open(p))
        if H is None:
            H, W = img.shape[0] // downscale, img.shape[1] // downscale
        images.append(box_mean(img, downscale))
        poses.append(ngp_pose(fr["transform_matrix"], scale, offset))
        files.append(p)
    poses = np.stack(poses)
    if "fl_x" in t or "fl_y" in t:
        fx, fy = t.get("fl_x", t.get("fl_y")) / downscale, t.get("fl_y", t.get("fl_x")) / downscale
    else:
        fx = W / (2 * np.tan(t["camera_angle_x"] / 2)) if "camera_angle_x" in t else None
        fy = H / (2 * np.tan(t["camera_angle_y"] / 2)) if "camera_angle_y" in t else None
        fx, fy = (fy if fx is None else fx), (fx if fy is None else fy)
    cx, cy = (t["cx"] / downscale if "cx" in t else W / 2), (t["cy"] / downscale if "cy" in t else H / 2)
    total = 0.0
    for q in poses:             # the mean camera distance in float64, one camera after the other
        total += math.sqrt(float(q[0, 3]) ** 2 + float(q[1, 3]) ** 2 + float(q[2, 3]) ** 2)
    return dict(poses=poses, images=np.stack(images), intrinsics=(fx, fy, cx, cy), H=H, W=W, radius=total / len(poses), mode=mode, files=files)


# ---- one uniform draw over a loaded scene
def expected_draw(scene, seed, step, n, stride=1, offset=0):
    """(pose number, inds int64 [n], gt float32 [n,3], bg float32 [n,3] or None) of the uniform sampler over expected()'s scene: pixel indices from the counter hash
    (orbit_ref.pixel_indices), the decode code / 255 in float32, an RGBA pixel blended against the step's backgrounds (random_bg_ref)."""
    P, H, W = scene["images"].shape[0], scene["H"], scene["W"]
    p = (step * stride + offset) % P
    inds = orbit_ref.pixel_indices(seed, step, n, H, W)
    px = scene["images"][p].reshape(H * W, -1)[inds].astype(np.float32) / np.float32(255)
    if px.shape[-1] == 3:
        return p, inds, px, None
    bg = rb.background(n, seed, step)
    return p, inds, rb.blend(px, bg), bg
