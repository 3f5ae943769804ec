"""A scene directory (transforms*.json + image files) as a device store: poses float32 [P,4,4] and the images as the files hold them, uint8 [P,H,W,C].

    scene = load_scene("data/nerf_synthetic/lego", split="train", downscale=2)
    sampler = scene.sampler(4096, seed=0)                      # rays.DeviceRaySampler over the u8 store: stage1.GraphedCleanLoop(sampler=)
    stage1.eval_step(model, scene.view(0), render_kwargs)

Restated from reading the reference's loader (nerf/provider.py:19-27 nerf_matrix_to_ngp, :114-274 NeRFDataset.__init__); what differs, and why:
  * The reference decodes every image to float32 (:221, image.astype(np.float32) / 255): 16 bytes per RGBA pixel on the device against the file's 4.  Here the bytes
    stay bytes; the sampler's kernel does that same IEEE division on the pixels a step draws (rg_sample_rays_u8), so no ground-truth bit changes.
  * Images are read with PIL (cv2 is not a dependency).  They must be 8-bit RGB or RGBA, all with one channel count; any other PIL mode is refused by name.
  * downscale is an integer >= 1 and an image must measure exactly (H * downscale, W * downscale): every output channel is the integer box mean
    (sum + f*f//2) // (f*f) of its f x f block.  That is cv2's INTER_AREA at an integer ratio (:219) up to the rounding of exact ties (cv2 rounds a float mean,
    half to even; this rounds half up) -- never checked against cv2 itself, which this project does not depend on.  The fractional-ratio resize is not offered.
  * nerf_matrix_to_ngp's translation, pose[i, 3] * scale + offset[k], is formed in float64 and rounded once to float32: what NumPy 1.x (the reference's) computes
    for a float32 scalar times a Python float.
  * radius, the mean camera distance (:231, poses[:, :3, 3].norm(dim=-1).mean(0) in float32), is formed in float64 from the float32 poses, one camera after the
    other: within float32 rounding of the reference's value, and the same on every torch build (a float32 mean's summation order is torch's to choose).
  * split "all" of a blender scene reads every *.json in sorted order (the reference: in glob's order, which the file system decides).
  * A colmap scene's split "test" (a slerp between two randomly chosen poses, :166-182) is not offered."""
import glob
import json
import os

import numpy as np
import torch

from . import rays


def ngp_pose(matrix, scale=0.33, offset=(0, 0, 0)):
    """nerf_matrix_to_ngp (provider.py:19-27): rows (1, 2, 0) of the file's matrix, the y and z columns negated, the translation scaled and shifted."""
    m = np.array(matrix, dtype=np.float32)
    out = np.zeros((4, 4), dtype=np.float32)
    for r, src in enumerate((1, 2, 0)):
        out[r, 0], out[r, 1], out[r, 2] = m[src, 0], -m[src, 1], -m[src, 2]
        out[r, 3] = np.float32(float(m[src, 3]) * float(scale) + float(offset[r]))
    out[3, 3] = 1.0
    return out


def box_downscale(image, f):
    """uint8 [H*f, W*f, C] -> uint8 [H, W, C]: the mean of every f x f block, (sum + f*f//2) // (f*f), in integers."""
    if f == 1:
        return image
    Hf, Wf, C = image.shape
    s = image.reshape(Hf // f, f, Wf // f, f, C).astype(np.uint32).sum(axis=(1, 3))
    return ((s + (f * f) // 2) // (f * f)).astype(np.uint8)


def _read_image(path):
    from PIL import Image
    with Image.open(path) as im:
        if im.mode not in ("RGB", "RGBA"):
            raise ValueError(f"load_scene: {path} has PIL mode '{im.mode}'; images must be 8-bit RGB or RGBA")
        return np.array(im, dtype=np.uint8)


def _read_transforms(path, mode, split):
    def one(name):
        with open(os.path.join(path, name)) as f:
            return json.load(f)

    if split not in ("train", "val", "test", "trainval", "all"):
        raise ValueError(f"load_scene: the splits are train, val, test, trainval and all, not '{split}'")
    if mode == "colmap":
        return one("transforms.json")
    if split == "all":          # provider.py:128-137
        transform = None
        for p in sorted(glob.glob(os.path.join(path, "*.json"))):
            t = one(os.path.basename(p))
            if transform is None:
                transform = t
            else:
                transform["frames"].extend(t["frames"])
        return transform
    if split == "trainval":     # :139-144
        transform = one("transforms_train.json")
        transform["frames"].extend(one("transforms_val.json")["frames"])
        return transform
    return one(f"transforms_{split}.json")


def decode_u8(images):
    """uint8 codes -> float32 code / 255 in IEEE division, on the tensor's device: the reference's loader (provider.py:221, numpy on the host).  NOT images.float() / 255
    on the GPU: there torch divides by a Python scalar by multiplying with its reciprocal, and 126 of the 256 codes come out one ulp off (measured on an MI355X;
    on the CPU the same expression is exact).  A tensor divisor takes the division kernel."""
    return images.float() / torch.full((), 255.0, dtype=torch.float32, device=images.device)


class Scene:
    """What load_scene read.  poses float32 [P,4,4] and images uint8 [P,H,W,C] (C 3 or 4) on `device`; intrinsics (fl_x, fl_y, cx, cy) as Python floats; radius: the
    mean camera distance (provider.py:231); mode 'colmap' | 'blender'; files: the image paths, in store order."""

    def __init__(self, poses, images, intrinsics, H, W, radius, mode, files):
        self.poses, self.images, self.intrinsics, self.H, self.W, self.radius, self.mode, self.files = poses, images, intrinsics, H, W, radius, mode, files

    def sampler(self, n_rays, seed=0, error_map=False, stride=1, offset=0, decode=None):
        """The rays.DeviceRaySampler over the u8 store (decode=: see linear_decode)."""
        if self.images is None:
            raise ValueError("Scene.sampler: this scene holds no images")
        return rays.DeviceRaySampler(self.poses, self.images, self.intrinsics, self.H, self.W, n_rays, stride=stride, offset=offset, seed=seed, error_map=error_map,
                                     decode=decode)

    def view(self, i):
        """View i as the dict stage1.eval_step takes: all H*W rays of pose i (rays.get_rays) and the image decoded as the reference's loader does (decode_u8)."""
        if self.images is None:
            raise ValueError("Scene.view: this scene holds no images")
        r = rays.get_rays(self.poses[i:i + 1], self.intrinsics, self.H, self.W, N=-1)
        return {"rays_o": r["rays_o"], "rays_d": r["rays_d"], "images": decode_u8(self.images[i:i + 1]), "H": self.H, "W": self.W}

    def linear_decode(self):
        """The sRGB -> linear table for DeviceRaySampler(decode=): the reference's srgb_to_linear (nerf/utils.py:49-50, applied per step at :496) on the 256 values a
        decoded colour channel can take (decode_u8 of the 256 codes), once."""
        from .trainer import srgb_to_linear
        return srgb_to_linear(decode_u8(torch.arange(256, dtype=torch.uint8, device=self.poses.device))).contiguous()


def load_scene(path, split="train", scale=0.33, offset=(0, 0, 0), downscale=1, device="cuda"):
    """Read split `split` of the scene directory `path` (see the module doc string) -> Scene."""
    if not (isinstance(downscale, int) and not isinstance(downscale, bool) and downscale >= 1):
        raise ValueError(f"load_scene: downscale must be an integer >= 1, not {downscale!r}")
    if os.path.exists(os.path.join(path, "transforms.json")):              # provider.py:114-120
        mode = "colmap"
    elif os.path.exists(os.path.join(path, "transforms_train.json")):
        mode = "blender"
    else:
        raise NotImplementedError(f"[NeRFDataset] Cannot find transforms*.json under {path}")
    if mode == "colmap" and split == "test":
        raise NotImplementedError("load_scene: split 'test' of a colmap scene (poses interpolated between two randomly chosen frames) is not offered")
    transform = _read_transforms(path, mode, split)
    H = W = None
    if "h" in transform and "w" in transform:                              # :154-159
        H, W = int(transform["h"]) // downscale, int(transform["w"]) // downscale
    frames = transform["frames"]
    if mode == "colmap":                                                   # :186-191
        frames = frames[1:] if split == "train" else frames[:1] if split == "val" else frames
    poses, images, files, channels = [], [], [], None
    for f in frames:
        f_path = os.path.join(path, f["file_path"])
        if mode == "blender" and "." not in os.path.basename(f_path):      # :197-198
            f_path += ".png"
        if not os.path.exists(f_path):                                     # :201-202
            continue
        image = _read_image(f_path)
        if H is None or W is None:                                         # :208-210
            H, W = image.shape[0] // downscale, image.shape[1] // downscale
        if channels is None:
            channels = image.shape[-1]
        if image.shape[-1] != channels:
            raise ValueError(f"load_scene: {f_path} has {image.shape[-1]} channels, the images before it {channels}")
        if image.shape[0] != H * downscale or image.shape[1] != W * downscale:
            raise ValueError(f"load_scene: {f_path} is {image.shape[0]} x {image.shape[1]}, not {H * downscale} x {W * downscale} "
                             f"(H x W = {H} x {W} times downscale = {downscale}; a fractional resize is not offered)")
        poses.append(ngp_pose(f["transform_matrix"], scale, offset))
        images.append(box_downscale(image, downscale))
        files.append(f_path)
    if not poses:
        raise ValueError(f"load_scene: none of the {len(frames)} frames of split '{split}' under {path} has an image file")
    poses = torch.from_numpy(np.stack(poses, axis=0))
    images = torch.from_numpy(np.ascontiguousarray(np.stack(images, axis=0)))
    centres = poses[:, :3, 3].double()                                     # :231, in float64 (see the module doc string)
    radius = sum(float(v) for v in (centres * centres).sum(-1).sqrt()) / len(centres)
    if "fl_x" in transform or "fl_y" in transform:                         # :259-269
        fl_x = (transform["fl_x"] if "fl_x" in transform else transform["fl_y"]) / downscale
        fl_y = (transform["fl_y"] if "fl_y" in transform else transform["fl_x"]) / downscale
    elif "camera_angle_x" in transform or "camera_angle_y" in transform:
        fl_x = W / (2 * np.tan(transform["camera_angle_x"] / 2)) if "camera_angle_x" in transform else None
        fl_y = H / (2 * np.tan(transform["camera_angle_y"] / 2)) if "camera_angle_y" in transform else None
        fl_x, fl_y = (fl_y if fl_x is None else fl_x), (fl_x if fl_y is None else fl_y)
    else:
        raise RuntimeError("Failed to load focal length, please check the transforms.json!")
    cx = (transform["cx"] / downscale) if "cx" in transform else (W / 2)    # :271-272
    cy = (transform["cy"] / downscale) if "cy" in transform else (H / 2)
    intrinsics = tuple(float(v) for v in (fl_x, fl_y, cx, cy))
    return Scene(poses.to(device), images.to(device), intrinsics, H, W, radius, mode, files)
