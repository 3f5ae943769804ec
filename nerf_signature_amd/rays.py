"""get_rays on the device: the step just before the render path.

Mirror of get_rays in /root/reference/nerf/utils_wtmk_disen.py:59-143 (same arguments, same result dict: 'rays_o',
'rays_d' [B,N,3], 'inds' [B,N], and 'inds_coarse' with an error map).  Index selection keeps the reference's torch
calls (randint / multinomial / patch offsets, now on the device the poses live on); the ray arithmetic -- the
reference's [B, H*W] meshgrid, gathers and ~15 elementwise ops -- is one kernel (rg_get_rays)."""
import torch

from . import _native as nv


@torch.no_grad()
def get_rays(poses, intrinsics, H, W, N=-1, error_map=None, patch_size=1):
    device = poses.device
    if not poses.is_cuda:
        raise ValueError("get_rays: poses must be on the GPU")
    B = poses.shape[0]
    fx, fy, cx, cy = (float(v) for v in intrinsics)
    results = {}
    if N > 0:
        N = min(N, H * W)
        if patch_size > 1:      # utils_wtmk_disen.py:85-102
            num_patch = N // (patch_size ** 2)
            inds_x = torch.randint(0, H - patch_size, size=[num_patch], device=device)
            inds_y = torch.randint(0, W - patch_size, size=[num_patch], device=device)
            inds = torch.stack([inds_x, inds_y], dim=-1)
            pi, pj = torch.meshgrid(torch.arange(patch_size, device=device), torch.arange(patch_size, device=device), indexing="ij")
            offsets = torch.stack([pi.reshape(-1), pj.reshape(-1)], dim=-1)
            inds = (inds.unsqueeze(1) + offsets.unsqueeze(0)).view(-1, 2)
            inds = inds[:, 0] * W + inds[:, 1]
            inds = inds.expand([B, inds.shape[0]])
        elif error_map is None:  # :104-106
            inds = torch.randint(0, H * W, size=[N], device=device).expand([B, N])
        else:                    # :108-119
            inds_coarse = torch.multinomial(error_map.to(device), N, replacement=False)
            inds_x, inds_y = inds_coarse // 128, inds_coarse % 128
            sx, sy = H / 128, W / 128
            inds_x = (inds_x * sx + torch.rand(B, N, device=device) * sx).long().clamp(max=H - 1)
            inds_y = (inds_y * sy + torch.rand(B, N, device=device) * sy).long().clamp(max=W - 1)
            inds = inds_x * W + inds_y
            results["inds_coarse"] = inds_coarse
        inds = inds.contiguous().long()
        n = inds.shape[1]
        ind_ptr = nv.ptr(inds)
    else:
        n = H * W
        inds = torch.arange(H * W, device=device).expand([B, H * W])
        ind_ptr = None
    results["inds"] = inds
    P = poses.contiguous().float()
    rays_o = torch.empty(B, n, 3, dtype=torch.float32, device=device)
    rays_d = torch.empty(B, n, 3, dtype=torch.float32, device=device)
    nv.call("rg_get_rays", nv.ptr(P), fx, fy, cx, cy, int(H), int(W), ind_ptr, B, n, nv.ptr(rays_o), nv.ptr(rays_d), nv.stream())
    results["rays_o"] = rays_o
    results["rays_d"] = rays_d
    return results


class DeviceRaySampler:
    """The loader step of the training loop on the device (rg_sample_rays): a store of poses [P,4,4] and (optionally) their images
    [P,H*W,3] resident in HBM; every call writes one batch -- pose (step * stride + offset) mod P, N uniformly drawn pixels, their rays
    and ground-truth colours -- into caller-owned buffers, with `step` read from a device counter.  Nothing in the call depends on a
    host value, so trainer.GraphedWatermarkLoop captures it at the head of its step (`content_sampler=`): the per-step hand-over of
    rays costs one 5 us launch inside the graph instead of a randint, a ray kernel, a gather and three copies between two replays.
    error_map=: the pixels are drawn from a per-image map of recent errors instead (see __init__).
    RGBA images [P,H*W,4] (the Blender scenes): `channels` is 4, and every draw also writes one random background colour per ray (`bg`) and hands out the
    ground truth blended against it, gt = rgb * a + bg * (1 - a) (the reference's stage-1 train_step, nerf/utils.py:498-507) -- in the same launch
    (rg_sample_rays_rgba / rg_sample_rays_weighted_rgba).
    A torch.uint8 store [P,H,W,C] or [P,H*W,C] -- the bytes of the image files, a quarter of the float store -- is kept as it is and decoded on the drawn pixels
    only (rg_sample_rays_u8 / rg_sample_rays_weighted_u8): code / 255 in IEEE division, the reference's loader (nerf/provider.py:221, numpy on the host), so every
    draw has the bits of the draw from that loader's float store.  (On the GPU torch's `images.float() / 255` is NOT that store: a Python-scalar divisor becomes a
    multiplication by 1/255, other bits for 126 of the 256 codes; dataset.decode_u8 divides by a tensor.)  decode= (u8 stores only): a float32 [256] table on the
    store's device that replaces code / 255 for the colour channels (alpha stays code / 255) -- a colour space costs nothing per step: build it once with the
    reference's own torch expression on dataset.decode_u8 of the 256 codes (Scene.linear_decode)."""

    def __init__(self, poses, images, intrinsics, H, W, n_rays, stride=1, offset=0, seed=0, error_map=False, error_grid=128, decode=None):
        """error_map: the reference's --error_map loader (nerf/provider.py:234-238,300-321; nerf/utils.py:105-114,534-556) on the device.  True allocates a
        map of ones [P, error_grid^2]; a tensor of that shape is taken as given (and updated in place).  With a map, sample_into draws n_rays cells of the
        pose's row without replacement in proportion to their weight and one pixel inside each (rg_sample_rays_weighted), and update_error_map(pred, gt)
        writes 0.1 * old + 0.9 * error back into the drawn cells (rg_error_map_update).  torch.multinomial raises when fewer than n_rays cells have a positive
        weight; here the lowest-index invalid cells fill the draw: nothing inside a captured step may fault."""
        if not poses.is_cuda:
            raise ValueError("DeviceRaySampler: poses must be on the GPU")
        self.poses = poses.contiguous().float()
        if images is not None and images.shape[-1] not in (3, 4):
            raise ValueError(f"DeviceRaySampler: images must be RGB or RGBA, not {images.shape[-1]} channels")
        self.channels = 3 if images is None else int(images.shape[-1])
        if images is not None and images.dtype != torch.uint8 and not images.is_floating_point():
            raise ValueError(f"DeviceRaySampler: images must be a float or a uint8 tensor, not {images.dtype}")
        self.u8 = images is not None and images.dtype == torch.uint8
        if self.u8:       # kept as stored: .float() would sample the codes as 0...255
            self.images = images.contiguous().view(self.poses.shape[0], H * W, self.channels)
            if self.channels == 4 and self.images.data_ptr() % 4:
                raise ValueError("DeviceRaySampler: an RGBA uint8 store is read one 4-byte pixel at a time: its address must be 4-byte aligned")
        else:
            self.images = None if images is None else images.contiguous().float().view(self.poses.shape[0], H * W, self.channels)
        if decode is not None:
            if not self.u8:
                raise ValueError("DeviceRaySampler: decode= belongs to a uint8 store (this one holds " + ("no images)" if images is None else "floats)"))
            if not (torch.is_tensor(decode) and decode.dtype == torch.float32 and tuple(decode.shape) == (256,) and decode.device == self.images.device):
                raise ValueError(f"DeviceRaySampler: decode must be a float32 tensor [256] on {self.images.device}")
            decode = decode.contiguous()
        self.decode = decode
        self.intr = tuple(float(v) for v in intrinsics)
        self.H, self.W, self.n_rays, self.stride, self.offset, self.seed = int(H), int(W), int(n_rays), int(stride), int(offset), int(seed)
        self.error_map, self.error_grid = None, int(error_grid)
        if error_map is not False and error_map is not None:
            G, P = self.error_grid, self.poses.shape[0]
            if not 1 <= G <= 128:
                raise ValueError("DeviceRaySampler: error_grid must lie in 1..128")
            if not 1 <= self.n_rays <= G * G:
                raise ValueError(f"DeviceRaySampler: a draw without replacement takes at most error_grid^2 = {G * G} rays, not {self.n_rays}")
            if error_map is True:
                error_map = torch.ones(P, G * G, dtype=torch.float32, device=self.poses.device)      # provider.py:236
            elif not (torch.is_tensor(error_map) and error_map.device == self.poses.device and error_map.dtype == torch.float32
                      and tuple(error_map.shape) == (P, G * G) and error_map.is_contiguous()):
                raise ValueError(f"DeviceRaySampler: error_map must be a contiguous float32 tensor [{P}, {G * G}] on {self.poses.device}")
            self.error_map = error_map
            self.inds_coarse = torch.zeros(self.n_rays, dtype=torch.int64, device=self.poses.device)      # the cells of the last draw, ascending
            self.pose_word = torch.zeros(1, dtype=torch.int32, device=self.poses.device)                  # ... and its pose

    @torch.no_grad()
    def sample_into(self, step_counter, rays_o, rays_d, gt=None, inds_out=None, pose_out=None, keys_out=None, bg=None):
        """step_counter: int32 device tensor [1] (or None = step 0).  rays_o / rays_d / gt: float32 buffers of n_rays * 3 elements.
        keys_out (map only): float32 [error_grid^2], every cell's key of the race.  bg (an RGBA store only, and required there): float32 buffer of
        n_rays * 3 elements for the rays' background colours; gt is then the blend against them."""
        if self.channels == 4 and bg is None:
            raise ValueError("DeviceRaySampler: an RGBA store draws a background colour per ray: pass bg=")
        if self.channels != 4 and bg is not None:
            raise ValueError("DeviceRaySampler: bg= belongs to an RGBA store (this one holds RGB)")
        rgba = ("_rgba", (nv.ptr(bg),)) if self.channels == 4 else ("", ())
        store = (nv.ptr(self.images),)
        if self.u8:       # one entry point for both channel counts: bg_out is NULL for RGB
            rgba, store = ("_u8", (nv.ptr(bg),)), (nv.ptr(self.images), self.channels, nv.ptr(self.decode))
        for t in (rays_o, rays_d, gt, bg):
            if t is not None and (t.numel() != self.n_rays * 3 or t.dtype != torch.float32):
                raise ValueError(f"DeviceRaySampler: buffers must hold {self.n_rays} x 3 float32 values")
        if gt is not None and self.images is None:
            raise ValueError("DeviceRaySampler: no image store to take the ground truth from")
        fx, fy, cx, cy = self.intr
        if self.error_map is not None:
            if keys_out is not None and (keys_out.numel() != self.error_grid ** 2 or keys_out.dtype != torch.float32):
                raise ValueError(f"DeviceRaySampler: keys_out must hold {self.error_grid ** 2} float32 values")
            nv.call("rg_sample_rays_weighted" + rgba[0], nv.ptr(self.poses), self.poses.shape[0], *store, fx, fy, cx, cy, self.H, self.W, self.n_rays,
                    nv.ptr(step_counter), self.stride, self.offset, self.seed, nv.ptr(self.error_map), self.error_grid, nv.ptr(rays_o), nv.ptr(rays_d), nv.ptr(gt),
                    *rgba[1], nv.ptr(inds_out), nv.ptr(self.pose_word), nv.ptr(self.inds_coarse), nv.ptr(keys_out), nv.stream())
            if pose_out is not None:
                pose_out.copy_(self.pose_word)
            return
        if keys_out is not None:
            raise ValueError("DeviceRaySampler: keys_out belongs to the error-map draw")
        nv.call("rg_sample_rays" + rgba[0], nv.ptr(self.poses), self.poses.shape[0], *store, fx, fy, cx, cy, self.H, self.W, self.n_rays,
                nv.ptr(step_counter), self.stride, self.offset, self.seed, nv.ptr(rays_o), nv.ptr(rays_d), nv.ptr(gt), *rgba[1], nv.ptr(inds_out), nv.ptr(pose_out),
                nv.stream())

    @torch.no_grad()
    def update_error_map(self, pred, gt):
        """Behind the step's loss: the cells of the last draw take 0.1 * old + 0.9 * mean((pred - gt)^2 over the channels) (utils.py:549-553).  pred / gt:
        float32 buffers of n_rays * 3 elements, in the order sample_into wrote the rays.  No host value: capturable."""
        if self.error_map is None:
            raise ValueError("DeviceRaySampler: this sampler draws uniformly (error_map=False)")
        for t in (pred, gt):
            if t.numel() != self.n_rays * 3 or t.dtype != torch.float32:
                raise ValueError(f"DeviceRaySampler: buffers must hold {self.n_rays} x 3 float32 values")
        nv.call("rg_error_map_update", nv.ptr(self.error_map), self.poses.shape[0], self.error_grid, nv.ptr(self.pose_word), nv.ptr(self.inds_coarse),
                nv.ptr(pred), nv.ptr(gt), self.n_rays, nv.stream())


class OrbitRaySampler:
    """DeviceRaySampler without a store (rg_sample_rays_orbit): every call DRAWS its camera -- one orbit pose looking at the origin, blocks.rand_poses' closed
    form with theta ~ U[theta_range], phi ~ U[phi_range] at `radius`, from the counter hash of (seed, step * stride + offset) -- then n_rays uniform pixels and
    their rays, in one launch with `step` read from a device counter: capturable, like the store samplers.  There are no images to take a ground truth from:
    a training step fed by this sampler renders its own target (trainer.train_step without content["images"]: the clean twin of the content render), so
    the watermark stage needs a checkpoint, intrinsics and a camera radius -- no dataset, and every step sees a new pose.  The last pose drawn is kept in
    `pose` [4,4] (device)."""

    def __init__(self, intrinsics, H, W, n_rays, radius, theta_range=(1.0471975511965976, 2.0943951023931953), phi_range=(0.0, 6.283185307179586), stride=1, offset=0,
                 seed=0, device="cuda"):
        self.intr = tuple(float(v) for v in intrinsics)
        self.H, self.W, self.n_rays, self.stride, self.offset, self.seed = int(H), int(W), int(n_rays), int(stride), int(offset), int(seed)
        self.radius = float(radius)
        self.theta_range, self.phi_range = (float(theta_range[0]), float(theta_range[1])), (float(phi_range[0]), float(phi_range[1]))
        if self.n_rays < 1:
            raise ValueError("OrbitRaySampler: n_rays must be at least 1")
        self.images, self.error_map, self.channels = None, None, 3
        self.pose = torch.zeros(4, 4, dtype=torch.float32, device=device)

    @torch.no_grad()
    def sample_into(self, step_counter, rays_o, rays_d, gt=None, inds_out=None, pose_out=None, keys_out=None, bg=None):
        """step_counter: int32 device tensor [1] (or None = step 0).  rays_o / rays_d: float32 buffers of n_rays * 3 elements.  pose_out: float32 [4,4] that
        receives the drawn pose (default: self.pose).  gt / keys_out / bg belong to samplers with a store and are refused."""
        if gt is not None or keys_out is not None or bg is not None:
            raise ValueError("OrbitRaySampler: no image store to take a ground truth (gt=), race keys (keys_out=) or backgrounds (bg=) from; the step renders its "
                             "own target (trainer.train_step without content[\"images\"])")
        for t in (rays_o, rays_d):
            if t.numel() != self.n_rays * 3 or t.dtype != torch.float32:
                raise ValueError(f"OrbitRaySampler: buffers must hold {self.n_rays} x 3 float32 values")
        if inds_out is not None and (inds_out.numel() != self.n_rays or inds_out.dtype != torch.int64):
            raise ValueError(f"OrbitRaySampler: inds_out must hold {self.n_rays} int64 values")
        pose = self.pose if pose_out is None else pose_out
        if pose.numel() != 16 or pose.dtype != torch.float32:
            raise ValueError("OrbitRaySampler: pose_out must hold 4 x 4 float32 values")
        fx, fy, cx, cy = self.intr
        nv.call("rg_sample_rays_orbit", fx, fy, cx, cy, self.H, self.W, self.n_rays, nv.ptr(step_counter), self.stride, self.offset, self.seed, self.radius,
                *self.theta_range, *self.phi_range, nv.ptr(rays_o), nv.ptr(rays_d), nv.ptr(inds_out), nv.ptr(pose), nv.stream())
