"""Rendering an exported mesh on the GPU, and verifying a signature through it (csrc/raster.hip; include/nerfsig.h, "mesh rasteriser").

    render_mesh(vertices, triangles, colors, pose, intrinsics, H, W, bg_color=1.0, near=0.05)   -> {"image", "depth", "triangle", "culled": (near, guard)}
    key_blocks(image, key)                                       the [D, bh, bw, 3] rectangles of key.blocks out of an [H, W, 3] view
    verify_mesh(vertices, triangles, colors, key, near=0.05)     release.verify's record of the mesh seen from the key pose
    view_directions(vertices_world, pose)                        normalize(vertex - camera centre) [V, 3]: mesh.vertex_colors(..., directions=) as the camera sees the field

The attack this measures needs one call of this project's own API: export the signed model to a coloured mesh (mesh.save_mesh) and throw the field away.
The rasteriser's answer is unique -- integer coverage on 8 sub-pixel bits, float64 depth, a 64-bit (depth, triangle) minimum per pixel -- so tests compare it
with tests/raster_ref.py by equality."""
import torch

from . import _native as nv
from . import mesh as _mesh

MAX_SIDE = 4096              # rs_*: 1 <= H, W <= 4096
STATUS_BYTES = 256           # the scratch's status block; words: first bad triangle, near-plane culls, guard-band culls, large-route triangles
RS_OK = 0xFFFFFFFF


def _align(n):
    return (n + 255) & ~255


class RasterScratch:
    """rs_project / rs_raster / rs_shade's scratch for meshes of up to V vertices and T triangles at H x W, reusable across views.  Views into it, valid after a
    render with exactly these sizes: status (int64 [4]), records (int32 [V, 4]: x, y, the bits of iz, flag) and zbuf (int64 [H, W]: -1 or depth bits << 32 | id)."""

    def __init__(self, V, T, H, W, device="cuda"):
        n = int(nv.fn("rs_scratch_bytes")(int(V), int(T), int(H), int(W)))
        if n == 0:
            raise ValueError(f"RasterScratch: V={V}, T={T}, {H} x {W} out of range (V, T below 2^31; 1 <= H, W <= {MAX_SIDE})")
        self.V, self.T, self.H, self.W = int(V), int(T), int(H), int(W)
        self.buf = torch.empty(n, dtype=torch.uint8, device=device)

    def fits(self, V, T, H, W, device):
        return (self.V, self.T, self.H, self.W) == (V, T, H, W) and self.buf.device == device

    @property
    def status(self):
        return self.buf[:16].view(torch.int32).to(torch.int64) & RS_OK

    @property
    def records(self):
        return self.buf[STATUS_BYTES:STATUS_BYTES + 16 * self.V].view(torch.int32).view(self.V, 4)

    @property
    def zbuf(self):
        o = STATUS_BYTES + _align(16 * self.V)
        return self.buf[o:o + 8 * self.H * self.W].view(torch.int64).view(self.H, self.W)


def _device_f32(t, shape_last, who, what):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ValueError(f"{who}: the {what} must be a tensor on the GPU (there is no CPU path)")
    if t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != shape_last:
        raise ValueError(f"{who}: the {what} must be float32 [V,{shape_last}], got {t.dtype} {tuple(t.shape)}")
    return t.contiguous()


def launch(vertices, triangles, colors, pose, intrinsics, H, W, bg, near, scratch, image, depth, winner, only=None):
    """The three entry points on checked arguments (render_mesh's core; tools/raster_bench.py times them one by one through `only`)."""
    V, T = int(vertices.shape[0]), int(triangles.shape[0])
    fx, fy, cx, cy = (float(v) for v in intrinsics)
    s, st = nv.ptr(scratch.buf), nv.stream()
    tp = nv.ptr(triangles) if T else None
    if only in (None, "project"):
        nv.call("rs_project", nv.ptr(vertices) if V else None, V, nv.ptr(pose), fx, fy, cx, cy, float(near), H, W, s, st)
    if only in (None, "raster"):
        nv.call("rs_raster", tp, T, V, H, W, s, st)
    if only in (None, "shade"):
        nv.call("rs_shade", tp, T, V, nv.ptr(colors) if V else None, nv.ptr(bg), H, W, s, nv.ptr(image), nv.ptr(depth), nv.ptr(winner), st)


def check_inputs(vertices, triangles, colors, pose, intrinsics, H, W, bg_color, near, who="render_mesh"):
    """-> (vertices, triangles, colors, pose [4,4] fp32, bg [3] fp32, H, W) on the vertices' device, or ValueError."""
    vertices = _device_f32(vertices, 3, who, "vertices")
    triangles = _mesh._check_triangles(triangles, who)
    colors = _device_f32(colors, 3, who, "colors")
    dev = vertices.device
    if colors.shape[0] != vertices.shape[0] or colors.device != dev or triangles.device != dev:
        raise ValueError(f"{who}: {vertices.shape[0]} vertices with {colors.shape[0]} colors, or tensors on different devices")
    H, W = int(H), int(W)
    if not (1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE):
        raise ValueError(f"{who}: image of {H} x {W} pixels is out of range (1 .. {MAX_SIDE} each way)")
    if vertices.shape[0] >= _mesh.MAX_ELEMENTS or triangles.shape[0] >= _mesh.MAX_ELEMENTS:
        raise ValueError(f"{who}: V={vertices.shape[0]}, T={triangles.shape[0]} out of range (each below 2^31)")
    pose = torch.as_tensor(pose).to(dev, torch.float32).reshape(4, 4).contiguous()
    if len(tuple(intrinsics)) != 4:
        raise ValueError(f"{who}: the intrinsics are (fx, fy, cx, cy)")
    bg = torch.as_tensor(bg_color, dtype=torch.float32).to(dev).reshape(-1)
    if bg.numel() not in (1, 3):
        raise ValueError(f"{who}: bg_color is one value or three, got {bg.numel()}")
    return vertices, triangles, colors, pose, bg.expand(3).contiguous(), H, W


def render_mesh(vertices, triangles, colors, pose, intrinsics, H, W, bg_color=1.0, near=0.05, scratch=None):
    """The mesh seen from `pose` (camera-to-world [4,4], get_rays' conventions) with pinhole `intrinsics` (fx, fy, cx, cy) at H x W.
    vertices float32 [V,3] world positions, triangles int32 [T,3], colors float32 [V,3]: device tensors.  ->
      "image" float32 [H,W,3] perspective-correct vertex colours, bg_color where nothing was drawn (nothing is clamped); "depth" float32 [H,W] camera z, +inf
      where nothing was drawn; "triangle" int32 [H,W] the winner's index or -1 -- all on the device; "culled": (near, guard) = how many triangles were skipped
      for a vertex nearer than `near` (there is no near-plane clipping: they leave holes) and for a vertex outside the guard band of 16384 pixels.
    Both windings are drawn.  Of equal depths the lower triangle index wins, so the result does not depend on arrival order.  One host read (the status block,
    after the launches); a triangle with an id outside [0, V) raises ValueError.  V = 0 or T = 0: all background.  scratch: a RasterScratch of these sizes to reuse."""
    vertices, triangles, colors, pose, bg, H, W = check_inputs(vertices, triangles, colors, pose, intrinsics, H, W, bg_color, near)
    V, T, dev = int(vertices.shape[0]), int(triangles.shape[0]), vertices.device
    with torch.cuda.device(dev):
        if scratch is None:
            scratch = RasterScratch(V, T, H, W, dev)
        elif not scratch.fits(V, T, H, W, dev):
            raise ValueError("render_mesh: the scratch was sized for another mesh, image or device")
        image = torch.empty(H, W, 3, dtype=torch.float32, device=dev)
        depth = torch.empty(H, W, dtype=torch.float32, device=dev)
        winner = torch.empty(H, W, dtype=torch.int32, device=dev)
        launch(vertices, triangles, colors, pose, intrinsics, H, W, bg, near, scratch, image, depth, winner)
        bad, n_near, n_guard, _ = scratch.status.tolist()               # the one host read
    if bad != RS_OK:
        raise ValueError(f"render_mesh: triangle {bad} has a vertex id outside [0, {V})")
    return {"image": image, "depth": depth, "triangle": winner, "culled": (n_near, n_guard)}


def key_blocks(image, key):
    """[D, bh, bw, 3]: the rectangles (row0, col0, row1, col1) of key.blocks out of the view image [H, W, 3], in the key's order (blocks.block_rays' slicing)."""
    if key.blocks is None:
        raise ValueError("key_blocks: the key has no block coordinates (it was built from ready block rays)")
    if image.dim() != 3 or tuple(image.shape[:2]) != (key.H, key.W):
        raise ValueError(f"key_blocks: expected the key view [{key.H}, {key.W}, 3], got {tuple(image.shape)}")
    return torch.stack([image[r0:r1, c0:c1] for r0, c0, r1, c1 in key.blocks.tolist()]).contiguous()


def _key_view(key, who):
    if key.poses is None or key.blocks is None:
        raise ValueError(f"{who}: the key needs its pose and block coordinates; one built from ready block rays (from_block_rays) has no view to render")
    if key.poses.shape[0] != 1:
        raise NotImplementedError("block rays of more than one key pose: the reference reshapes the key view to [1, H, W, 3] (provider_wtmk.py:465)")
    return key.poses[0], key.intrinsics, key.H, key.W


@torch.no_grad()
def verify_mesh(vertices, triangles, colors, key, near=0.05, scratch=None, details=False):
    """release.verify's record for a MESH: the key pose rendered at key.H x key.W over the key's background (white), its blocks cut out and handed to
    release.verify as the render -- clamp, normalisation, decoder and p-value are verify's own.  details=True: -> (record, render_mesh's dict)."""
    from . import release as rel
    pose, intr, H, W = _key_view(key, "verify_mesh")
    view = render_mesh(vertices, triangles, colors, pose, intr, H, W, bg_color=float(key.render_kwargs["bg_color"]), near=near, scratch=scratch)
    blocks = key_blocks(view["image"], key)
    record = rel.verify(lambda o, d: blocks, key)
    return (record, view) if details else record


def view_directions(vertices_world, pose):
    """float32 [V,3] on the vertices' device: the unit vector from the camera centre of `pose` to every vertex -- the direction under which that camera's ray
    meets the field there."""
    x = torch.as_tensor(vertices_world)
    c = torch.as_tensor(pose).to(x.device, torch.float32).reshape(4, 4)[:3, 3]
    d = x.to(torch.float32).reshape(-1, 3) - c
    return (d / torch.norm(d, dim=-1, keepdim=True)).contiguous()
