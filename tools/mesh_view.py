#!/usr/bin/env python
"""Look at an exported mesh: render a PLY written by mesh.save_mesh / mesh.write_ply from one camera and write a PNG.

    python tools/mesh_view.py MESH.ply OUT.png [--pose POSE.npy | --orbit THETA PHI RADIUS] [--size H W] [--intrinsics FX FY CX CY] [--near 0.05] [--bg 1.0]

--pose: a camera-to-world [4,4] (or [1,4,4], e.g. a key's pose file) as .npy; --orbit: a camera on a sphere about the origin looking at it (synthetic.orbit_pose;
default 1.1 0.7 3.2248, the synthetic scene's key view).  Default size 400 x 400, default intrinsics those of scene S0 scaled to the size.  A mesh without
colours is drawn with its normals as colours (n / 2 + 0.5), one without either in grey.  Prints the counts of triangles culled at the near plane and guard band."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from PIL import Image

from nerf_signature_amd import mesh, raster, synthetic


def values(name, n, default):
    if name not in sys.argv:
        return default
    i = sys.argv.index(name)
    return [float(x) for x in sys.argv[i + 1:i + 1 + n]]


if len(sys.argv) < 3 or sys.argv[1].startswith("--"):
    sys.exit(__doc__)
src, dst = sys.argv[1], sys.argv[2]
H, W = (int(x) for x in values("--size", 2, [400, 400]))
cfg = synthetic.SCENES["hotdog"]
intr = values("--intrinsics", 4, [cfg["focal"] * W / cfg["W"], cfg["focal"] * H / cfg["H"], W / 2, H / 2])
if "--pose" in sys.argv:
    pose = np.load(sys.argv[sys.argv.index("--pose") + 1]).astype(np.float32).reshape(-1, 4, 4)[0]
else:
    pose = synthetic.orbit_pose(*values("--orbit", 3, [1.1, 0.7, cfg["radius"]]))
near, bg = values("--near", 1, [0.05])[0], values("--bg", 1, [1.0])[0]

m = mesh.read_ply(src)
dev = torch.device("cuda")
V = len(m["vertices"])
if m["colors"] is not None:
    colors = m["colors"].astype(np.float32) / np.float32(255)
elif m["normals"] is not None:
    colors = m["normals"] * np.float32(0.5) + np.float32(0.5)
else:
    colors = np.full((V, 3), 0.6, np.float32)
out = raster.render_mesh(torch.from_numpy(m["vertices"].astype(np.float32)).to(dev), torch.from_numpy(m["triangles"]).to(dev), torch.from_numpy(colors).to(dev),
                         pose, intr, H, W, bg_color=bg, near=near)
img = mesh.quantize_colors(out["image"]).cpu().numpy()
d = os.path.dirname(os.path.abspath(dst))
os.makedirs(d, exist_ok=True)
Image.fromarray(img, "RGB").save(dst)
print(f"{src}: {V} vertices, {len(m['triangles'])} triangles -> {dst} ({H} x {W}); culled at the near plane {out['culled'][0]}, at the guard band {out['culled'][1]}; "
      f"{int((out['triangle'] >= 0).sum())} pixels covered")
