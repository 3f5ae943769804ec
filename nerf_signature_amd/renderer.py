"""NeRFRenderer: the host-side mirror of /root/reference/nerf/renderer_wtmk.py:61-575 on top of libnerfsig.

Same constructor, buffers (`density_grid`, `density_bitfield`, `step_counter`, `aabb_train`, `aabb_infer`),
attributes and methods (`render`, `run_cuda`, `run`, `mark_untrained_grid`, `update_extra_state`,
`reset_extra_state`) as the reference class, so the reference's Trainer / provider / CLI drive it unchanged.
`render` accepts and ignores arbitrary extra keyword arguments: the reference splats its whole argparse
namespace into it (nerf/utils_wtmk_disen.py:590,616)."""
import math
import os

import numpy as np
import torch
import torch.nn as nn

from . import _native as nv
from . import raymarching


def is_multi_message(message):
    """A [K, D] tensor of K messages (render's multi-message form) as opposed to one message [D] or None."""
    return torch.is_tensor(message) and message.dim() == 2


def custom_meshgrid(*args):
    return torch.meshgrid(*args, indexing="ij")


def sample_pdf(bins, weights, n_samples, det=False):
    """Importance re-sampling of depths: `n_samples` quantiles of the piecewise-constant density `weights` [B, T-1] over the
    intervals between `bins` [B, T], by inverting its CDF (what renderer_wtmk.py:12-47 computes; same 1e-5 floors, and in the
    random mode the same single host-side torch.rand draw of B x n_samples numbers, so seeded runs consume the generator alike).
    det: the midpoints of n_samples equal quantile intervals instead of random quantiles.  Returns [B, n_samples]."""
    B, T = bins.shape
    mass = weights + 1e-5
    cdf = torch.zeros(B, T, dtype=mass.dtype, device=mass.device)
    torch.cumsum(mass / mass.sum(-1, keepdim=True), -1, out=cdf[:, 1:])
    if det:
        q = ((torch.arange(n_samples, dtype=mass.dtype) + 0.5) / n_samples).to(mass.device).expand(B, n_samples)
    else:
        q = torch.rand(B, n_samples).to(mass.device)
    q = q.contiguous()
    hi = torch.searchsorted(cdf, q, right=True)          # first knot whose CDF exceeds the quantile
    lo = (hi - 1).clamp_(min=0)
    hi = hi.clamp_(max=T - 1)
    c_lo, c_hi = torch.take_along_dim(cdf, lo, -1), torch.take_along_dim(cdf, hi, -1)
    z_lo, z_hi = torch.take_along_dim(bins, lo, -1), torch.take_along_dim(bins, hi, -1)
    span = c_hi - c_lo
    span = torch.where(span < 1e-5, torch.ones_like(span), span)       # an (almost) empty interval: keep its left end
    return z_lo + (q - c_lo) / span * (z_hi - z_lo)


_BG_CONST = {}


def _background_tensor(bg_color, image):
    """bg_color as a [3] or [N,3] float32 device tensor (constants are cached: no fill kernel per call), or None if it is
    something rm_finish does not take (then the stock operators broadcast it)."""
    if isinstance(bg_color, (int, float)):
        key = (image.device, float(bg_color))
        if key not in _BG_CONST:
            _BG_CONST[key] = torch.full((3,), float(bg_color), dtype=torch.float32, device=image.device)
        return _BG_CONST[key]
    if torch.is_tensor(bg_color) and bg_color.dtype == torch.float32 and bg_color.device == image.device and not bg_color.requires_grad:
        if bg_color.numel() == 3:
            return bg_color.reshape(3).contiguous()
        if bg_color.numel() == image.numel():
            return bg_color.reshape(-1, 3).contiguous()
    return None


class _Finish(torch.autograd.Function):
    """rm_finish_fwd / rm_finish_bwd: image + (1 - weights_sum) * bg and clamp(depth - near, 0) / (far - near)."""

    @staticmethod
    def forward(ctx, image, depth, weights_sum, nears, fars, bg):
        image, depth, weights_sum = image.contiguous(), depth.contiguous(), weights_sum.contiguous()
        N = depth.numel()
        image_out, depth_out = torch.empty_like(image), torch.empty_like(depth)
        stride = 0 if bg.numel() == 3 else 3
        nv.call("rm_finish_fwd", nv.ptr(image), nv.ptr(depth), nv.ptr(weights_sum), nv.ptr(nears), nv.ptr(fars), nv.ptr(bg), stride, N,
                nv.ptr(image_out), nv.ptr(depth_out), nv.stream())
        ctx.save_for_backward(depth, nears, fars, bg)
        ctx.set_materialize_grads(False)
        return image_out, depth_out

    @staticmethod
    def backward(ctx, g_image, g_depth):
        depth, nears, fars, bg = ctx.saved_tensors
        N = depth.numel()
        if g_image is not None:
            g_image = g_image.contiguous()
        g_ws = torch.empty_like(depth)
        g_depth_in = torch.empty_like(depth) if g_depth is not None else None
        nv.call("rm_finish_bwd", nv.ptr(g_image), nv.ptr(g_depth.contiguous() if g_depth is not None else None), nv.ptr(depth), nv.ptr(nears),
                nv.ptr(fars), nv.ptr(bg), 0 if bg.numel() == 3 else 3, N, nv.ptr(g_ws), nv.ptr(g_depth_in), nv.stream())
        return g_image, g_depth_in, g_ws, None, None, None


class _CompositeFinish(torch.autograd.Function):
    """composite_rays_train + the render tail in one launch each way (rm_composite_train_finish_fwd/_bwd).  `rays` must come from
    this package's marcher (ascending, gapless offsets): the backward relies on it to zero-fill unwritten rows itself."""

    @staticmethod
    def forward(ctx, sigmas, rgbs, deltas, rays, nears, fars, bg, T_thresh):
        sigmas, rgbs, deltas = sigmas.contiguous(), rgbs.contiguous(), deltas.contiguous()
        M, N = sigmas.shape[0], rays.shape[0]
        dev = sigmas.device
        weights_sum, depth, image = (torch.empty(N, dtype=torch.float32, device=dev), torch.empty(N, dtype=torch.float32, device=dev),
                                     torch.empty(N, 3, dtype=torch.float32, device=dev))
        image_out, depth_out = torch.empty_like(image), torch.empty_like(depth)
        stride = 0 if bg.numel() == 3 else 3
        nv.call("rm_composite_train_finish_fwd", nv.ptr(sigmas), nv.ptr(rgbs), nv.ptr(deltas), nv.ptr(rays), M, N, float(T_thresh), nv.ptr(nears),
                nv.ptr(fars), nv.ptr(bg), stride, nv.ptr(weights_sum), nv.ptr(depth), nv.ptr(image), nv.ptr(image_out), nv.ptr(depth_out), nv.stream())
        ctx.save_for_backward(sigmas, rgbs, deltas, rays, weights_sum, image, bg)
        ctx.dims = (M, N, float(T_thresh), stride)
        ctx.set_materialize_grads(False)
        return weights_sum, depth_out, image_out      # (depth stays differentiable as in the reference; its gradient is ignored below, raymarching.py:275)

    @staticmethod
    def backward(ctx, g_ws, g_depth, g_image):
        sigmas, rgbs, deltas, rays, weights_sum, image, bg = ctx.saved_tensors
        M, N, T_thresh, stride = ctx.dims
        g_image = torch.zeros_like(image) if g_image is None else g_image.contiguous()
        grad_sigmas, grad_rgbs = torch.empty_like(sigmas), torch.empty_like(rgbs)
        nv.call("rm_composite_train_finish_bwd", nv.ptr(None if g_ws is None else g_ws.contiguous()), nv.ptr(g_image), nv.ptr(sigmas), nv.ptr(rgbs),
                nv.ptr(deltas), nv.ptr(rays), nv.ptr(weights_sum), nv.ptr(image), nv.ptr(bg), stride, M, N, T_thresh, 1, nv.ptr(grad_sigmas),
                nv.ptr(grad_rgbs), nv.stream())
        return grad_sigmas, grad_rgbs, None, None, None, None, None, None


class NeRFRenderer(nn.Module):
    def __init__(self, bound=1, cuda_ray=False, density_scale=1, min_near=0.2, density_thresh=0.01, bg_radius=-1):
        super().__init__()
        self.bound = bound
        self.cascade = 1 + math.ceil(math.log2(bound))
        self.grid_size = 128
        self.density_scale = density_scale
        self.min_near = min_near
        self.density_thresh = density_thresh
        self.bg_radius = bg_radius
        aabb_train = torch.FloatTensor([-bound, -bound, -bound, bound, bound, bound])
        self.register_buffer("aabb_train", aabb_train)
        self.register_buffer("aabb_infer", aabb_train.clone())
        self.cuda_ray = cuda_ray
        if cuda_ray:
            self.register_buffer("density_grid", torch.zeros([self.cascade, self.grid_size ** 3]))
            self.register_buffer("density_bitfield", torch.zeros(self.cascade * self.grid_size ** 3 // 8, dtype=torch.uint8))
            self.mean_density = 0
            self.iter_density = 0
            self.register_buffer("step_counter", torch.zeros(16, 2, dtype=torch.int32))
            self.mean_count = 0
            self.local_step = 0
        self._grid_epoch = 0      # bumped by everything that rewrites the occupancy grid (see grid_key)
        # the training march's host state (plain attributes: none of it belongs in a state_dict)
        self.point_capacity = None      # {ray count: sample rows} set by a captured loop: the no-host-sync march (capacity_for)
        self.point_headroom = ()        # the ray counts among them whose rows were sized with headroom: their backward stops at the march's device count (rows_for)
        self._marched = {}              # _rays_key -> raymarching.MarchRecord of samples marched ahead of their render (march_ahead, fix_rays)
        self._premarched = None         # the MarchRecord of premarch(), for the next render only
        self._keep_rays, self._last_rays = False, None      # _render_staged_fused: leave the last march's ray table in _last_rays

    # mean_density / mean_count (renderer_wtmk.py:523,536): plain host numbers, as in the reference -- except behind a device-side refresh
    # (gridrefresh.DeviceGridRefresh), which leaves them in device memory: they are then read back when somebody asks, not every 16 steps.
    def _host_number(self, name, convert):
        src = self.__dict__.get(f"_{name}_dev")
        if src is not None:
            self.__dict__[f"_{name}"] = convert(src.item())
            self.__dict__[f"_{name}_dev"] = None
        return self.__dict__.get(f"_{name}", 0)

    @property
    def mean_density(self):
        return self._host_number("mean_density", float)

    @mean_density.setter
    def mean_density(self, value):
        self.__dict__["_mean_density"], self.__dict__["_mean_density_dev"] = value, None

    @property
    def mean_count(self):
        return self._host_number("mean_count", int)

    @mean_count.setter
    def mean_count(self, value):
        self.__dict__["_mean_count"], self.__dict__["_mean_count_dev"] = value, None

    def grid_key(self):
        """Identity of the occupancy grid the marcher reads: address and version of the bitfield AND an explicit epoch.  The version alone
        misses writes through a raw pointer (packbits re-packs the bitfield in place); samples kept across steps (fix_rays, the captured
        loop's fixed blocks) compare this key."""
        return (self.density_bitfield.data_ptr(), self.density_bitfield._version, self._grid_epoch)

    def _load_from_state_dict(self, *args, **kwargs):
        super()._load_from_state_dict(*args, **kwargs)
        self._grid_epoch = getattr(self, "_grid_epoch", 0) + 1      # a checkpoint may have brought another grid

    def forward(self, x, d):
        raise NotImplementedError()

    def density(self, x):
        raise NotImplementedError()

    def color(self, x, d, mask=None, **kwargs):
        raise NotImplementedError()

    def reset_extra_state(self):
        if not self.cuda_ray:
            return
        self.density_grid.zero_()
        self.mean_density = 0
        self.iter_density = 0
        self.step_counter.zero_()
        self.mean_count = 0
        self.local_step = 0
        self._grid_epoch += 1

    # ------------------------------------------------------------------ shared pieces

    def _flatten_rays(self, rays_o, rays_d):
        return rays_o.shape[:-1], rays_o.contiguous().view(-1, 3), rays_d.contiguous().view(-1, 3)

    def _background(self, bg_color):
        if self.bg_radius > 0:
            raise NotImplementedError("background model (bg_radius > 0) is asserted off on this path (main_nerf_wtmk.py:86)")
        return 1 if bg_color is None else bg_color

    @staticmethod
    def _finish(prefix, image, depth, weights_sum, bg_color, nears, fars):
        """Background mix and depth normalisation shared by both branches (renderer_wtmk.py:316-319,369-372);
        depth is NaN for rays that miss the box (near == far == FLT_MAX), as in the reference.  One kernel each way on the GPU."""
        if image.is_cuda and image.dtype == torch.float32:
            bg = _background_tensor(bg_color, image)
            if bg is not None:
                image, depth = _Finish.apply(image, depth, weights_sum, nears, fars, bg)
                return image.view(*prefix, 3), depth.view(*prefix)
        image = image + (1 - weights_sum).unsqueeze(-1) * bg_color
        depth = torch.clamp(depth - nears, min=0) / (fars - nears)
        return image.view(*prefix, 3), depth.view(*prefix)

    # ------------------------------------------------------------------ uniform-sample path (renderer_wtmk.py:125-253)

    def run(self, rays_o, rays_d, message, num_steps=128, upsample_steps=128, bg_color=None, perturb=False, **kwargs):
        """num_steps samples per ray, uniformly in [near, far]; with upsample_steps > 0 that many more drawn from the first pass's weights
        (sample_pdf: evenly spaced quantiles in eval mode, random ones in training mode) and merged in depth order; density everywhere,
        colour only where the compositing weight exceeds 1e-4 (renderer_wtmk.py:125-253).
        As in the reference the re-sampled points are evaluated WITHOUT the message (renderer_wtmk.py:187 calls density(new_xyzs) with its
        default message=None): they see the clean field, and no gradient reaches the codebook through them."""
        bg_color = self._background(bg_color)
        prefix, o, d = self._flatten_rays(rays_o, rays_d)
        N, T = o.shape[0], num_steps
        aabb = self.aabb_train if self.training else self.aabb_infer
        nears, fars = (t.unsqueeze(-1) for t in raymarching.near_far_from_aabb(o, d, aabb, self.min_near))
        span = fars - nears
        z = nears + span * torch.linspace(0.0, 1.0, T, device=o.device).unsqueeze(0).expand(N, T)
        spacing = span / T
        if perturb:
            z = z + (torch.rand(z.shape, device=o.device) - 0.5) * spacing
        pts = torch.min(torch.max(o.unsqueeze(-2) + d.unsqueeze(-2) * z.unsqueeze(-1), aabb[:3]), aabb[3:])
        differentiable = torch.is_grad_enabled() and message is not None and any(p.requires_grad for p in self.parameters())
        dirs_of = lambda p: d.view(-1, 1, 3).expand_as(p).reshape(-1, 3).contiguous()
        if differentiable:
            # Training through this path (the reference trains through density() + masked color() when --cuda_ray is off): one joint,
            # differentiable field pass over all samples, colour zeroed where the reference does not evaluate it.  Same values -- a
            # masked-out sample's colour is 0 there too -- and the same gradient: the mask is a constant of the backward pass in both.
            sigma_all, rgb_all = self(pts.reshape(-1, 3), dirs_of(pts), message)
            sigma, rgb_all = sigma_all.view(N, T), rgb_all.view(N, T, 3)
            geo = None
        else:
            field = self.density(pts.reshape(-1, 3), message=message)
            sigma, geo = field["sigma"].view(N, T), field["geo_feat"].view(N, T, -1)
            rgb_all = None
        if upsample_steps > 0:
            with torch.no_grad():
                step0 = torch.cat([z[..., 1:] - z[..., :-1], spacing * torch.ones_like(z[..., :1])], dim=-1)
                alpha0 = 1 - torch.exp(-step0 * self.density_scale * sigma.detach())
                w0 = alpha0 * torch.cumprod(torch.cat([torch.ones_like(alpha0[..., :1]), 1 - alpha0 + 1e-15], dim=-1), dim=-1)[..., :-1]
                z_mid = z[..., :-1] + 0.5 * step0[..., :-1]
                new_z = sample_pdf(z_mid, w0[:, 1:-1], upsample_steps, det=not self.training).detach()
                new_pts = torch.min(torch.max(o.unsqueeze(-2) + d.unsqueeze(-2) * new_z.unsqueeze(-1), aabb[:3]), aabb[3:])
            t = upsample_steps
            if differentiable:
                # no message: the clean field (renderer_wtmk.py:187).  Evaluated with gradients enabled like the reference's call; in this network
                # every parameter such a pass reads is frozen (network_wtmk_tcnn.py:90-95), so autograd records nothing for it
                s_new, c_new = self(new_pts.reshape(-1, 3), dirs_of(new_pts), None)
                new_sigma, new_rgb = s_new.view(N, t), c_new.view(N, t, 3)
            else:
                nf = self.density(new_pts.reshape(-1, 3))
                new_sigma, new_geo = nf["sigma"].view(N, t), nf["geo_feat"].view(N, t, -1)
            z, order = torch.sort(torch.cat([z, new_z], dim=1), dim=1)
            gather = lambda a, b: torch.gather(torch.cat([a, b], dim=1), 1, order.unsqueeze(-1).expand(-1, -1, a.shape[-1]) if a.dim() == 3 else order)
            pts = gather(pts, new_pts)
            sigma = gather(sigma, new_sigma)
            if differentiable:
                rgb_all = gather(rgb_all, new_rgb)
            else:
                geo = gather(geo, new_geo)
            T = T + t
        step = torch.cat([z[..., 1:] - z[..., :-1], spacing * torch.ones_like(z[..., :1])], dim=-1)
        alpha = 1 - torch.exp(-step * self.density_scale * sigma)
        transmittance = torch.cumprod(torch.cat([torch.ones_like(alpha[..., :1]), 1 - alpha + 1e-15], dim=-1), dim=-1)[..., :-1]
        weights = alpha * transmittance
        if differentiable:
            rgbs = rgb_all * (weights > 1e-4).unsqueeze(-1)
        else:
            rgbs = self.color(pts.reshape(-1, 3), dirs_of(pts), mask=(weights > 1e-4).reshape(-1), geo_feat=geo.reshape(N * T, -1)).view(N, T, 3)
        weights_sum = weights.sum(dim=-1)
        depth = torch.sum(weights * ((z - nears) / span).clamp(0, 1), dim=-1)
        image = torch.sum(weights.unsqueeze(-1) * rgbs, dim=-2) + (1 - weights_sum).unsqueeze(-1) * bg_color
        return {"depth": depth.view(*prefix), "image": image.view(*prefix, 3), "weights_sum": weights_sum}

    # ------------------------------------------------------------------ occupancy-grid path (renderer_wtmk.py:256-377)

    # ------------------------------------------------------------------ samples marched ahead of their step

    @staticmethod
    def _rays_key(o, d):
        return (o.data_ptr(), o._version, d.data_ptr(), d._version, o.shape[0])

    def capacity_for(self, n_rays):
        """Sample rows a captured loop has reserved for renders of this many rays (`point_capacity`), or None."""
        return self.point_capacity.get(n_rays) if self.point_capacity else None

    def rows_for(self, n_rays, counter):
        """The march's device counter as the row count of the field backward, for renders whose reserved rows carry headroom (`point_headroom`); else None."""
        return counter if self.point_capacity and n_rays in self.point_headroom else None

    def march_ahead(self, rays_o, rays_d, dt_gamma=0, max_steps=1024, perturb=False, capacity=None, noises=None):
        """March the training samples of these rays now, for a render issued later with the same (unmodified) ray tensors.

        The march needs the rays and the occupancy grid only -- nothing a training step updates -- so a loop that knows its next
        rays runs it beside the optimiser of the current step (an HBM stream that leaves the ALUs idle) instead of at the head of
        the next one.  Needs `point_capacity` (the no-host-sync march); a repeated call for the same tensors re-marches into the
        same buffers.  run_cuda picks the samples up by the tensors' addresses and versions; any in-place change of the rays after
        the call makes it march again as usual.  noises: the per-ray start offsets [N] drawn by the caller (instead of torch.rand under perturb=True:
        a captured loop that keeps its own counter-based draws, stage1.GraphedCleanLoop)."""
        # (the walk while the current step is in flight and offsets + samples at its end, as two calls: measured, slower)
        prefix, o, d = self._flatten_rays(rays_o, rays_d)
        if capacity is None:      # (an explicit capacity: NeRFNetwork.fix_rays sizing its own buffers)
            capacity = self.capacity_for(o.shape[0])
        if capacity is None or not o.is_cuda:
            raise RuntimeError("march_ahead needs point_capacity for this ray count (see trainer.GraphedWatermarkLoop.prepare) and CUDA rays")
        rec = self.find_marched(o, d, capacity) or raymarching.MarchRecord.allocate(o, d, capacity, max_steps)
        if rec.max_steps != int(max_steps):
            raise ValueError("march_ahead: max_steps changed for rays that were marched before")
        geom = (self.bound, dt_gamma, max_steps, self.cascade, self.grid_size)
        rec.noises = noises if noises is not None else (torch.rand(o.shape[0], dtype=torch.float32, device=o.device) if perturb else None)
        raymarching.enqueue_train_walk(o, d, self.density_bitfield, geom, rec.noises, rec.nears, rec.fars, rec.counts, rec.t_rec,
                                       limits=(self.aabb_train, self.min_near))
        raymarching.enqueue_train_samples(o, d, geom, rec.noises, rec.nears, rec.t_rec, rec.counts, rec.rays, rec.counter, (rec.xyzs, rec.dirs, rec.deltas))
        self.keep_marched(rec, o, d)
        return rec

    # the cache of marched samples: records keyed by their ray tensors' addresses and versions (_rays_key)
    def find_marched(self, o, d, capacity=None, fixed=False):
        """The record marched from these tensors whatever their versions (and of this capacity / with kept points, if asked), or None."""
        return next((r for r in self._marched.values() if r.matches(o, d, capacity) and (r.fixed is not None or not fixed)), None)

    def get_marched(self, o, d):
        """The record of exactly these tensors, unmodified since their march, or None."""
        return self._marched.get(self._rays_key(o, d)) if self._marched else None

    def keep_marched(self, rec, o, d):
        """(Re-)enter a record under the current versions of its tensors."""
        self.forget_marched(rec)
        rec.key = self._rays_key(o, d)
        self._marched[rec.key] = rec

    def forget_marched(self, rec):
        self._marched = {k: r for k, r in self._marched.items() if r is not rec}

    def marched_records(self):
        return list(self._marched.values())

    def drop_marched(self):
        self._marched = {}

    def premarch(self, rays_o, rays_d, dt_gamma=0, max_steps=1024):
        """The exact (synchronising) training march of these rays NOW, for the next training render of the same two tensor OBJECTS, unmodified, with the
        same arguments (perturb=False, force_all_rays=True) -- the launches and the host read of the sample count that render would issue, moved in
        front of whatever the caller enqueues in between.  An eager step whose content rays are known before its block render (trainer.train_step)
        calls this first: the read-back then waits for the march alone instead of for the block render and the decoder queued in front of it.
        The samples are used once; anything that does not match (other tensors, an in-place change, another grid) marches again as usual."""
        prefix, o, d = self._flatten_rays(rays_o, rays_d)
        nears, fars = raymarching.near_far_from_aabb(o, d, self.aabb_train, self.min_near)
        counter = self.step_counter[self.local_step % 16]
        self.local_step += 1
        counter.zero_()
        xyzs, dirs, deltas, rays = raymarching.march_rays_train(o, d, self.bound, self.density_bitfield, self.cascade, self.grid_size, nears, fars, counter,
                                                               self.mean_count, False, 128, True, dt_gamma, max_steps)
        self._premarched = raymarching.MarchRecord(o, d, xyzs, dirs, deltas, rays, nears, fars).made_for(rays_o, rays_d, float(dt_gamma), int(max_steps), self.grid_key())

    def run_cuda(self, rays_o, rays_d, message, dt_gamma=0, bg_color=None, perturb=False, force_all_rays=False, max_steps=1024,
                 T_thresh=1e-4, clean_twin=False, return_weights_sum=False, **kwargs):
        """return_weights_sum: results["weights_sum"] [N] in eval() mode too (the training path always carries it): what a caller that writes the render's own
        alpha needs (distill.teacher_dataset).  clean_twin (training path, with a message): results["clean_image"] is the image of the SAME samples through the field without the message -- the clean
        field comes out of the watermarked render's own MLP launch (field_fwd_twin) and goes through the same compositing forward and render tail, with the same
        deltas, rays and background; no gradient flows through it.  Bit for bit the "image" of this call with message=None."""
        if clean_twin and not self.training:
            raise NotImplementedError("clean_twin: the eval loop terminates rays per field (a ray leaves the alive list when ITS transmittance falls under T_thresh), "
                                      "so a watermarked and a clean image would not share samples; the twin exists on the training path (model.train())")
        if clean_twin and message is None:
            raise ValueError("clean_twin needs a message: without one \"image\" is the clean image")
        multi = is_multi_message(message)
        if multi:
            self._check_multi_messages(message, clean_twin)
        bg_color = self._background(bg_color)
        prefix, o, d = self._flatten_rays(rays_o, rays_d)
        plain = self.training and force_all_rays and not perturb      # (the render that march_ahead and premarch march for)
        marched = self.get_marched(o, d) if plain else None
        if marched is None and self._premarched is not None:
            pre, self._premarched = self._premarched, None      # (for the next render only)
            if plain and self.point_capacity is None and pre.valid_for(rays_o, rays_d, float(dt_gamma), int(max_steps), self.grid_key()):
                marched = pre                                  # (marched a moment ago for exactly this call: premarch)
        if marched is not None and marched.fixed is not None and not torch.cuda.is_current_stream_capturing() and marched.grid_key != self.grid_key():
            marched = self.fix_rays(o, d, *marched.fixed_args)      # rays declared constant, but the grid they were marched through changed
        march_limits = marched is None and self.training and self.capacity_for(o.shape[0]) is not None and force_all_rays and o.is_cuda and o.dtype == torch.float32
        if marched is not None:
            nears, fars = marched.nears, marched.fars
        elif march_limits:       # the capacity march (a captured step) fills them itself: raymarching.enqueue_train_walk
            nears, fars = torch.empty(o.shape[0], dtype=torch.float32, device=o.device), torch.empty(o.shape[0], dtype=torch.float32, device=o.device)
        else:
            nears, fars = raymarching.near_far_from_aabb(o, d, self.aabb_train if self.training else self.aabb_infer, self.min_near)
        if self.training:
            bg = _background_tensor(bg_color, o) if o.is_cuda else None
            out = self._march_and_composite_train(o, d, message, nears, fars, dt_gamma, perturb, force_all_rays, max_steps, T_thresh, finish=bg,
                                                  marched=marched, limits=(self.aabb_train, self.min_near) if march_limits else None, clean_twin=clean_twin)
            weights_sum, depth, image = out[:3]
            if multi:      # [K, N], [K, N], [K, N, 3]: one march, K composited images
                K = message.shape[0]
                if bg is None:
                    tails = [self._finish((o.shape[0],), image[k], depth[k], weights_sum[k], bg_color, nears, fars) for k in range(K)]
                    image, depth = torch.stack([t[0] for t in tails]), torch.stack([t[1] for t in tails])
                return {"depth": depth.view(K, *prefix), "image": image.view(K, *prefix, 3), "weights_sum": weights_sum}
            clean = None
            if clean_twin:
                clean = out[3][2] if bg is not None else self._finish(prefix, out[3][2], out[3][1], out[3][0], bg_color, nears, fars)[0]
                clean = {"clean_image": clean.view(*prefix, 3)}
            if bg is not None:   # the tail was done by the compositing launch
                return {"depth": depth.view(*prefix), "image": image.view(*prefix, 3), "weights_sum": weights_sum, **(clean or {})}
        else:
            weights_sum, depth, image = self._march_and_composite_eval(o, d, message, nears, fars, dt_gamma, perturb, max_steps, T_thresh)
        image, depth = self._finish(prefix, image, depth, weights_sum, bg_color, nears, fars)
        results = {"depth": depth, "image": image}
        if self.training or return_weights_sum:
            results["weights_sum"] = weights_sum
        if self.training:
            results.update(clean or {})
        return results

    def _march_and_composite_train(self, o, d, message, nears, fars, dt_gamma, perturb, force_all_rays, max_steps, T_thresh, finish=None,
                                   marched=None, limits=None, clean_twin=False):
        """All samples of all rays at once, then one differentiable composite (renderer_wtmk.py:280-321)."""
        if marched is not None:      # the samples were marched ahead of this step (march_ahead)
            rows_dev = self.rows_for(o.shape[0], marched.counter) if marched.fixed is None else None
            return self._field_and_composite(marched.xyzs, marched.dirs, marched.deltas, marched.rays, message, nears, fars, finish, T_thresh, marched.fixed,
                                             clean_twin, rows_dev=rows_dev)
        counter = self.step_counter[self.local_step % 16]  # ring of the last 16 (points, rays) totals
        self.local_step += 1
        capacity = self.capacity_for(o.shape[0])
        rows_dev = None
        if capacity is not None and force_all_rays:
            rows_dev = self.rows_for(o.shape[0], counter)
            # no host round trip: buffers sized by a known bound on the padded point count (see march_rays_train_capacity); its scan kernel writes
            # both entries of `counter` itself (no zero-fill: one launch less in the captured step)
            xyzs, dirs, deltas, rays = raymarching.march_rays_train_capacity(o, d, self.bound, self.density_bitfield, self.cascade,
                                                                            self.grid_size, nears, fars, counter, capacity, perturb,
                                                                            dt_gamma, max_steps, limits=limits)
        else:
            counter.zero_()
            xyzs, dirs, deltas, rays = raymarching.march_rays_train(o, d, self.bound, self.density_bitfield, self.cascade, self.grid_size,
                                                                   nears, fars, counter, self.mean_count, perturb, 128, force_all_rays,
                                                                   dt_gamma, max_steps)
        self._last_rays = rays if self._keep_rays else None      # (render's fused staging reads the per-ray counts)
        return self._field_and_composite(xyzs, dirs, deltas, rays, message, nears, fars, finish, T_thresh, clean_twin=clean_twin, rows_dev=rows_dev)

    def _field_and_composite(self, xyzs, dirs, deltas, rays, message, nears, fars, finish, T_thresh, fixed=None, clean_twin=False, rows_dev=None):
        # fixed: rays declared constant (NeRFNetwork.fix_rays) -- base planes and scatter plan are kept beside the samples
        # clean_twin: a fourth result, the (weights_sum, depth, image) of the clean field at the same samples -- the same compositing launch once more, no gradient
        # rows_dev: the march's device counter when the sample buffers carry headroom (rows_for): the field's backward pass stops at the rows that hold samples
        rows = {} if rows_dev is None else {"rows_dev": rows_dev}
        if is_multi_message(message):
            # K messages: the field pass shares everything but the codebook level (forward_multi_chunks: base planes once, at most NSIG_MULTI_MAX_MESSAGES messages
            # per launch); slice k then goes through the compositing launch and render tail of the single render -- stacked (weights_sum [K,N], depth [K,N], image [K,N,3])
            outs = []
            for sigmas, rgbs in self.forward_multi_chunks(xyzs, dirs, message, fixed=fixed):
                for k in range(sigmas.shape[0]):
                    s = sigmas[k] if self.density_scale == 1 else self.density_scale * sigmas[k]
                    if finish is not None:
                        outs.append(_CompositeFinish.apply(s, rgbs[k], deltas, rays, nears, fars, finish, T_thresh))
                    else:
                        outs.append(raymarching.composite_rays_train(s, rgbs[k], deltas, rays, T_thresh))
            return tuple(torch.stack([o[i] for o in outs]) for i in range(3))
        if clean_twin:
            if fixed is not None:
                raise NotImplementedError("clean_twin for rays declared constant (fix_rays): their kept plane set is not read by the twin launch")
            sigmas, rgbs, sigmas_clean, rgbs_clean = self(xyzs, dirs, message, twin=True, **rows)
        else:
            sigmas, rgbs = self(xyzs, dirs, message, **rows) if fixed is None else self(xyzs, dirs, message, fixed=fixed)
        sigmas = sigmas if self.density_scale == 1 else self.density_scale * sigmas
        composite = ((lambda s, c: _CompositeFinish.apply(s, c, deltas, rays, nears, fars, finish, T_thresh)) if finish is not None
                     else (lambda s, c: raymarching.composite_rays_train(s, c, deltas, rays, T_thresh)))
        out = composite(sigmas, rgbs)
        if clean_twin:
            with torch.no_grad():
                out = tuple(out) + (tuple(composite(sigmas_clean if self.density_scale == 1 else self.density_scale * sigmas_clean, rgbs_clean)),)
        return out

    def _march_and_composite_eval(self, o, d, message, nears, fars, dt_gamma, perturb, max_steps, T_thresh):
        """Bursts of 1..8 samples over the still-alive rays (renderer_wtmk.py:323-367).

        Default (CUDA rays): the loop's control lives on the device (_eval_loop_on_device) -- no per-round read-back.  NERFSIG_EVAL_LOOP=host keeps
        the round-by-round form: the alive list compacted on the device, the survivor count read back every round."""
        if o.is_cuda and o.shape[0] > 0 and os.environ.get("NERFSIG_EVAL_LOOP", "device") != "host" and hasattr(self, "_eval_field_rows"):
            return self._eval_loop_on_device(o, d, message, nears, fars, dt_gamma, perturb, max_steps, T_thresh)
        N, device = o.shape[0], o.device
        weights_sum = torch.zeros(N, dtype=torch.float32, device=device)
        depth = torch.zeros(N, dtype=torch.float32, device=device)
        image = torch.zeros(N, 3, dtype=torch.float32, device=device)
        rays_alive = torch.arange(N, dtype=torch.int32, device=device)
        rays_t = nears.clone()
        n_alive, step = N, 0
        while step < max_steps and n_alive > 0:
            n_step = max(min(N // n_alive, 8), 1)
            xyzs, dirs, deltas = raymarching.march_rays(n_alive, n_step, rays_alive, rays_t, o, d, self.bound, self.density_bitfield,
                                                        self.cascade, self.grid_size, nears, fars, 128, perturb if step == 0 else False,
                                                        dt_gamma, max_steps)
            sigmas, rgbs = self(xyzs, dirs, message)
            raymarching.composite_rays(n_alive, n_step, rays_alive, rays_t, self.density_scale * sigmas, rgbs, deltas, weights_sum, depth,
                                       image, T_thresh)
            compacted, n_out = raymarching.compact_alive(rays_alive[:n_alive])
            n_alive = int(n_out.item())
            rays_alive = compacted[:n_alive]
            step += n_step
        return weights_sum, depth, image

    def _eval_loop_on_device(self, o, d, message, nears, fars, dt_gamma, perturb, max_steps, T_thresh, check_every=8, trace=None):
        """The same bursts, alive lists and images as the host-driven loop (tests/test_gpu_raymarch.py), with n_alive / n_step / the sample count kept in
        a device control block (rm_eval_*): every round's launches are sized for the worst case (n_alive * n_step <= N) and early-out on the
        device counts, the field pass evaluates exactly `rows` rows (field_fwd_rows), and the host reads the survivor count back once every
        `check_every` rounds -- only to stop enqueueing.  At most max_steps rounds (a round marches at least one sample).
        trace: a list that receives (n_alive, n_step, alive ids) per round (tests: costs a read-back per round)."""
        N, device = o.shape[0], o.device
        f32 = dict(dtype=torch.float32, device=device)
        weights_sum, depth, image = torch.zeros(N, **f32), torch.zeros(N, **f32), torch.zeros(N, 3, **f32)
        alive = [torch.empty(N, dtype=torch.int32, device=device), torch.empty(N, dtype=torch.int32, device=device)]
        ctl = torch.empty(4, dtype=torch.int32, device=device)
        rays_t = nears.clone()
        xyzs, dirs, deltas = torch.empty(N, 3, **f32), torch.empty(N, 3, **f32), torch.empty(N, 2, **f32)
        sigmas, rgbs = torch.empty(N, **f32), torch.empty(N, 3, **f32)
        nv.call("rm_eval_begin", N, nv.ptr(ctl), nv.ptr(alive[0]), nv.stream())
        field = self._eval_field_rows(N, message)          # (tables selected, pre-sum computed, buffers for N rows: once per render)
        noises = torch.rand(N, **f32) if perturb else None
        geom = (float(self.bound), float(dt_gamma), int(max_steps), int(self.cascade), int(self.grid_size))
        cur = 0
        for rnd in range(int(max_steps)):
            if trace is not None:
                c = ctl.tolist()
                trace.append((c[0], c[1], alive[cur][:c[0]].clone()))
            nv.call("rm_eval_march", nv.ptr(ctl), N, nv.ptr(alive[cur]), nv.ptr(rays_t), nv.ptr(o), nv.ptr(d), *geom, nv.ptr(self.density_bitfield),
                    nv.ptr(fars), nv.ptr(xyzs), nv.ptr(dirs), nv.ptr(deltas), nv.ptr(noises) if rnd == 0 else None, nv.stream())
            field(xyzs, dirs, ctl[2:3], sigmas, rgbs)
            nv.call("rm_eval_composite", nv.ptr(ctl), N, float(T_thresh), float(self.density_scale), nv.ptr(alive[cur]), nv.ptr(rays_t), nv.ptr(sigmas),
                    nv.ptr(rgbs), nv.ptr(deltas), nv.ptr(weights_sum), nv.ptr(depth), nv.ptr(image), nv.stream())
            nv.call("rm_eval_compact", nv.ptr(ctl), N, int(max_steps), nv.ptr(alive[cur]), nv.ptr(alive[1 - cur]), nv.stream())
            cur = 1 - cur
            if (rnd % check_every == check_every - 1 or trace is not None) and int(ctl[0]) == 0:
                break
        return weights_sum, depth, image

    # ------------------------------------------------------------------ density-grid maintenance

    def _grid_blocks(self, S):
        """All grid cells in S^3 blocks: yields (integer coords [n,3], morton index [n]) on the grid's device; coords.block_dims = (nx, ny, nz), z fastest.
        The blocks never change: built once per (S, grid size, device) and kept (42 MB at 128^3) -- a refresh otherwise spends six launches on them."""
        dev = self.density_bitfield.device
        key = (int(S), int(self.grid_size), str(dev))
        cache = self.__dict__.setdefault("_grid_block_cache", {})
        if key not in cache:
            blocks = []
            axis = torch.arange(self.grid_size, dtype=torch.int32, device=dev).split(S)
            for xs in axis:
                for ys in axis:
                    for zs in axis:
                        coords = torch.stack(custom_meshgrid(xs, ys, zs), dim=-1).reshape(-1, 3)
                        coords.block_dims = (len(xs), len(ys), len(zs))
                        coords.centres = {}
                        blocks.append((coords, raymarching.morton3D(coords).long()))
            cache.clear()      # (one geometry at a time)
            cache[key] = blocks
        yield from cache[key]

    def _cascade_extent(self, cas):
        extent = min(2 ** cas, self.bound)
        return extent, extent / self.grid_size  # (half-width of the cascade, half a cell)

    def _cell_centres(self, coords, cas, jitter):
        """World position of grid cells of cascade `cas` (optionally jittered inside the cell)."""
        extent, half_cell = self._cascade_extent(cas)
        kept = getattr(coords, "centres", None)      # (a cached block of _grid_blocks: its un-jittered centres are constants too -- five launches per refresh)
        if kept is not None and (cas, float(extent)) in kept:
            pts = kept[(cas, float(extent))]
        else:
            pts = (2 * coords.float() / (self.grid_size - 1) - 1) * (extent - half_cell)
            if kept is not None:
                kept[(cas, float(extent))] = pts
        if jitter:
            pts = pts + (torch.rand_like(pts) * 2 - 1) * half_cell      # (the reference's `+=`: the same sum, the kept centres left alone)
        return pts

    @torch.no_grad()
    def mark_untrained_grid(self, poses, intrinsic, S=64):
        """Cells that no training camera sees get density -1 (renderer_wtmk.py:380-442)."""
        if not self.cuda_ray:
            return
        if isinstance(poses, np.ndarray):
            poses = torch.from_numpy(poses)
        fx, fy, cx, cy = intrinsic
        seen = torch.zeros_like(self.density_grid)
        poses = poses.to(seen.device)
        for coords, indices in self._grid_blocks(S):
            for cas in range(self.cascade):
                _, half_cell = self._cascade_extent(cas)
                world = self._cell_centres(coords, cas, jitter=False).unsqueeze(0)
                for head in range(0, poses.shape[0], S):
                    batch = poses[head:head + S]
                    cam = (world - batch[:, :3, 3].unsqueeze(1)) @ batch[:, :3, :3]  # world -> camera, [S,n,3]
                    in_front = cam[:, :, 2] > 0
                    in_x = torch.abs(cam[:, :, 0]) < cx / fx * cam[:, :, 2] + half_cell * 2
                    in_y = torch.abs(cam[:, :, 1]) < cy / fy * cam[:, :, 2] + half_cell * 2
                    seen[cas, indices] += (in_front & in_x & in_y).sum(0).reshape(-1)
        self.density_grid[seen == 0] = -1
        self._grid_epoch += 1
        print(f"[mark untrained grid] {(seen == 0).sum()} from {self.grid_size ** 3 * self.cascade}")

    PROBE_SORT_MIN = 1 << 16      # points from which a scattered probe is sorted before the density query

    def _probe_density(self, coords, cas, message):
        pts = self._cell_centres(coords, cas, jitter=True)
        dims = getattr(coords, "block_dims", None)
        if dims is not None and pts.is_cuda:
            # A whole block of the grid, z fastest (the order the reference draws its jitter in, renderer_wtmk.py:470-486): queried x FASTEST instead.  The reference's
            # hash takes x un-multiplied (hash_encoding.py:16), so points that follow each other in x land in the same or the next 128-byte line of a table on almost
            # every level, where z-neighbours hit 64 unrelated lines per gather instruction (the 2 M-point encoder launch: LABNOTES section 17).  Every point's density
            # is independent of its neighbours: the same bits, in the old order again below.
            nx, ny, nz = dims
            q = pts.view(nx, ny, nz, 3).permute(2, 1, 0, 3).reshape(-1, 3).contiguous()
            sigma = self.density(q, message)["sigma"].reshape(nz, ny, nx).permute(2, 1, 0).reshape(-1)
            return sigma.detach() * self.density_scale
        if pts.is_cuda and pts.shape[0] >= self.PROBE_SORT_MIN:
            # scattered cells (the partial refresh: a random quarter of the grid + as many occupied cells): the same locality from a sort of the QUERY on (y, z, x)
            c = coords.long()
            order = torch.argsort((c[:, 1] * self.grid_size + c[:, 2]) * self.grid_size + c[:, 0])
            sigma = torch.empty(pts.shape[0], dtype=torch.float32, device=pts.device)
            sigma[order] = self.density(pts[order], message)["sigma"].reshape(-1).detach()
            return sigma * self.density_scale
        return self.density(pts, message)["sigma"].reshape(-1).detach() * self.density_scale

    @torch.no_grad()
    def update_extra_state(self, message=None, decay=0.95, S=128):
        """EMA update of the density grid, re-pack of the bitfield, mean sample count (renderer_wtmk.py:445-538):
        the first 16 calls probe every cell, later calls a random quarter plus as many occupied cells."""
        if not self.cuda_ray:
            return
        dev = self.density_bitfield.device
        fresh = -torch.ones_like(self.density_grid)
        if self.iter_density == 0 and dev.type == "cuda":
            # the scattered probe of the 17th refresh on sorts its query: load that operator's kernels now (tens of ms the first time), not in the middle of the
            # training loop.  No random numbers drawn, nothing of the model touched.
            torch.argsort(torch.arange(self.PROBE_SORT_MIN, dtype=torch.int64, device=dev).flip(0))
        if self.iter_density < 16:
            for coords, indices in self._grid_blocks(S):
                for cas in range(self.cascade):
                    fresh[cas, indices] = self._probe_density(coords, cas, message)
        else:
            n = self.grid_size ** 3 // 4
            for cas in range(self.cascade):
                rand_coords = torch.randint(0, self.grid_size, (n, 3), device=dev)
                rand_idx = raymarching.morton3D(rand_coords).long()
                occupied = torch.nonzero(self.density_grid[cas] > 0).squeeze(-1)
                occ_idx = occupied[torch.randint(0, occupied.shape[0], [n], dtype=torch.long, device=dev)]
                occ_coords = raymarching.morton3D_invert(occ_idx)
                indices = torch.cat([rand_idx, occ_idx], dim=0)
                fresh[cas, indices] = self._probe_density(torch.cat([rand_coords, occ_coords], dim=0), cas, message)
        both = (self.density_grid >= 0) & (fresh >= 0)
        # (the reference's masked assignment, renderer_wtmk.py:521-522, as a select: the same values without the nonzero() and host read of boolean indexing)
        self.density_grid.copy_(torch.where(both, torch.maximum(self.density_grid * decay, fresh), self.density_grid))
        self.mean_density = torch.mean(self.density_grid.clamp(min=0)).item()
        self.iter_density += 1
        self.density_bitfield = raymarching.packbits(self.density_grid, min(self.mean_density, self.density_thresh), self.density_bitfield)
        self._grid_epoch += 1
        steps = min(16, self.local_step)
        if steps > 0:
            self.mean_count = int(self.step_counter[:steps, 0].sum().item() / steps)
        self.local_step = 0

    # ------------------------------------------------------------------ entry point (renderer_wtmk.py:541-575)

    # rays per launch sequence of the fused staged render: 64 of the reference's 4096-ray chunks (1 GiB of march scratch)
    STAGED_SUPER_RAYS = 1 << 18

    def _render_staged_fused(self, rays_o, rays_d, message, max_ray_batch, **kwargs):
        """render(staged=True) without gradients on the occupancy-grid training path (what the reference's test_image / test_bitacc and
        the clean-render pre-pass run, utils_wtmk_disen.py:832, provider_wtmk.py:415): the reference walks the image in max_ray_batch
        chunks because its march zero-fills 134 MB per 4096 rays and reads a count back per chunk; every ray's samples and colour are
        independent of the chunking (ray-id ordered march), so here up to 64 chunks go through ONE march / encode / MLP / composite
        sequence with ONE count read-back.  The visible side effects of the per-chunk calls -- `local_step` and the 16-row `step_counter`
        ring of (points, rays) per call (renderer_wtmk.py:282-284) -- are reproduced from the per-ray counts."""
        B, N = rays_o.shape[:2]
        device = rays_o.device
        lead = (message.shape[0],) if is_multi_message(message) else ()      # K messages: [K, B, N(, 3)], every super-chunk marched once for all of them
        depth = torch.empty(lead + (B, N), device=device)
        image = torch.empty(lead + (B, N, 3), device=device)
        self._keep_rays = True
        try:
            for b in range(B):
                for head in range(0, N, self.STAGED_SUPER_RAYS):
                    tail = min(head + self.STAGED_SUPER_RAYS, N)
                    first_call = self.local_step
                    out = self.run_cuda(rays_o[b:b + 1, head:tail], rays_d[b:b + 1, head:tail], message, **kwargs)
                    depth[..., b:b + 1, head:tail] = out["depth"]
                    image[..., b:b + 1, head:tail, :] = out["image"]
                    counts = self._last_rays[:, 2].long()                                   # ray-id order
                    bounds = list(range(0, tail - head, max_ray_batch)) + [tail - head]
                    csum = torch.cat([counts.new_zeros(1), torch.cumsum(counts, 0)])
                    idx = torch.tensor(bounds, device=device)
                    totals = (csum[idx[1:]] - csum[idx[:-1]]).to(torch.int32)
                    n_calls = len(bounds) - 1
                    for k in range(max(0, n_calls - 16), n_calls):                         # the ring rows the per-chunk calls would have left
                        row = (first_call + k) % 16
                        self.step_counter[row, 0] = totals[k]
                        self.step_counter[row, 1] = bounds[k + 1] - bounds[k]
                    self.local_step = first_call + n_calls
        finally:
            self._keep_rays = False
            self._last_rays = None
        return {"depth": depth, "image": image}

    def _check_multi_messages(self, messages, clean_twin=False):
        """What a render under K messages [K, D] supports: the occupancy-grid training-mode path without gradients (what test_bitacc / test_image run)."""
        D = getattr(self, "message_dim", None)
        if D is not None and messages.shape[1] != D:
            raise ValueError(f"messages are [K, {messages.shape[1]}], the network was built with message_dim={D}")
        if not hasattr(self, "forward_multi_chunks"):
            raise NotImplementedError("a render under K messages needs a field with forward_multi_chunks (NeRFNetwork)")
        if not self.cuda_ray:
            raise NotImplementedError("K messages on the uniform-sample `run` path: it re-samples depths from each field's own weights, so the messages would not "
                                      "share samples; the multi-message render exists on the occupancy-grid path (cuda_ray=True)")
        if not self.training:
            raise NotImplementedError("K messages in model.eval(): the eval loop terminates rays per field (a ray leaves the alive list when ITS transmittance falls "
                                      "under T_thresh), so the messages would not share samples; render in model.train() mode under torch.no_grad()")
        if clean_twin:
            raise NotImplementedError("clean_twin together with K messages: the twin launch evaluates one message and the clean field (render the clean image once, "
                                      "with message=None)")
        if torch.is_grad_enabled():
            raise RuntimeError("a render under K messages is inference only (forward, no gradients): call it under torch.no_grad()")

    def render(self, rays_o, rays_d, message=None, staged=False, max_ray_batch=4096, **kwargs):
        """message: None, one message [D], or K messages [K, D] (K >= 1; training-mode kernels under torch.no_grad()): one march and one base-level encode for all K,
        the codebook level and the MLP chain per message -> image [K, *prefix, 3], depth [K, *prefix] (unstaged also weights_sum [K, N]); image[k] has the bits of
        render(..., message[k])."""
        if is_multi_message(message):
            if not self.cuda_ray or kwargs.get("clean_twin"):      # (what run_cuda -- which checks every call it gets -- would not see, or not see first)
                self._check_multi_messages(message, kwargs.get("clean_twin", False))
            message = message.detach().to(device=rays_o.device, dtype=torch.float32).contiguous()      # (a host tensor: copied once, here; nothing is read back)
        if kwargs.get("clean_twin") and (staged or not self.cuda_ray):
            raise NotImplementedError("clean_twin exists on the unstaged occupancy-grid training path only (cuda_ray=True, staged=False): the uniform-sample path "
                                      "re-samples depths from the field's own weights, so the two images would not share samples, and a staged render assembles "
                                      "\"image\" and \"depth\" chunk by chunk and carries nothing else")
        _run = self.run_cuda if self.cuda_ray else self.run
        B, N = rays_o.shape[:2]
        device = rays_o.device
        if (staged and self.cuda_ray and self.training and not torch.is_grad_enabled() and rays_o.is_cuda and N > max_ray_batch
                and kwargs.get("force_all_rays", False) and not kwargs.get("perturb", False) and self.point_capacity is None and not kwargs.get("return_weights_sum")
                and os.environ.get("NERFSIG_STAGED_FUSED", "1") != "0"):
            return self._render_staged_fused(rays_o, rays_d, message, max_ray_batch, **kwargs)
        if staged:
            lead = (message.shape[0],) if is_multi_message(message) else ()
            depth = torch.empty(lead + (B, N), device=device)
            image = torch.empty(lead + (B, N, 3), device=device)
            alpha = torch.empty(B, N, device=device) if kwargs.get("return_weights_sum") else None      # (asked for: the staged result carries it too)
            if alpha is not None and lead:
                raise NotImplementedError("return_weights_sum on a staged render under K messages")
            for b in range(B):
                head = 0
                while head < N:
                    tail = min(head + max_ray_batch, N)
                    results_ = _run(rays_o[b:b + 1, head:tail], rays_d[b:b + 1, head:tail], message, **kwargs)
                    depth[..., b:b + 1, head:tail] = results_["depth"]
                    image[..., b:b + 1, head:tail, :] = results_["image"]
                    if alpha is not None:
                        alpha[b, head:tail] = results_["weights_sum"].reshape(-1)
                    head += max_ray_batch
            results = {"depth": depth, "image": image, **({} if alpha is None else {"weights_sum": alpha})}
        else:
            if getattr(self, "auto_fix_rays", False):
                self._maybe_fix_rays(rays_o, rays_d, **kwargs)
            results = _run(rays_o, rays_d, message, **kwargs)
        return results

    def _maybe_fix_rays(self, rays_o, rays_d, dt_gamma=0, max_steps=1024, perturb=False, force_all_rays=False, **kwargs):
        """auto_fix_rays (the drop-in modules switch it on): a training render that is handed the SAME two ray tensors (same objects, unmodified) a second
        time -- the watermark-block rays, which the reference's dataset builds once (provider_wtmk.py:442-494) and passes every step -- declares them
        constant by itself (NeRFNetwork.fix_rays: samples marched once, base-level planes and scatter plan kept; bit-identical renders), which
        INTEGRATION.md section 5 otherwise asks the user to do with one call.  Identity is by object (weak references), never by address alone: the
        content rays are fresh tensors every step and the allocator reuses their addresses."""
        if not (self.cuda_ray and self.training and force_all_rays and not perturb and rays_o.is_cuda and torch.is_grad_enabled()
                and self.point_capacity is None and hasattr(self, "fix_rays") and not torch.cuda.is_current_stream_capturing()):
            return
        import weakref
        seen = self.__dict__.setdefault("_ray_sightings", {})
        key, ver = id(rays_o), (rays_o._version, rays_d._version, rays_o.data_ptr(), rays_d.data_ptr(), float(dt_gamma), int(max_steps))
        rec = seen.get(key)
        if rec is not None and rec[0]() is rays_o and rec[1]() is rays_d and rec[2] == ver:
            if not rec[3]:
                self.fix_rays(rays_o, rays_d, dt_gamma, max_steps)
                rec[3] = True
            seen[key] = seen.pop(key)          # most recently used last
            return
        seen[key] = [weakref.ref(rays_o), weakref.ref(rays_d), ver, False]
        while len(seen) > 4:
            seen.pop(next(iter(seen)))
