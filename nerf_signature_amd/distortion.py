"""The distortion layer of the training step: Trainer.distortion_layer of /root/reference/nerf/utils_wtmk_disen.py:551-577, applied to the
clamped block renders in front of the decoder (:594), selected by `--distortion` (main_nerf_wtmk.py:75).

    noise       x + n,  n ~ N(0, 0.1) per element (`torch.normal(0, sqrt(0.1), size)`)
    brightness  torchvision ColorJitter(brightness=0.5): ONE factor f ~ U[0.5, 1.5] per call, clamp(f * x, 0, 1)
    blurring    torchvision GaussianBlur(kernel_size=3, sigma=(0.01, 0.5)): ONE sigma ~ U[0.01, 0.5] per call, separable taps
                exp(-0.5 (d / sigma)^2), d in {-1, 0, 1}, normalised; reflect padding
    rotation    torchvision RandomRotation((-30, 30)) per image: nearest-neighbour resampling about the centre, zero fill
    scaling     per image [3, H, W]: F.interpolate(scale_factor=sf ~ U[0.75, 1.25], mode='linear') -- 1-d, along W only

noise / brightness / blurring run inside the fused decoder's first layer (dec_forward_train: no launch of their own) or, for decoder
shapes the fused chain does not implement, as wm_distort_fwd / _bwd; rotation / scaling change the sampling geometry and are one small
launch in front of the decoder and one behind its backward (wm_distort_geom_fwd / _bwd).  The random draws live in device buffers so that a
captured step (trainer.GraphedWatermarkLoop) refreshes them itself from a counter-based generator (wm_distort_draw, keyed by the replay
count); the eager loop draws like the reference's libraries do, from torch's generators.  The scaling factor decides the decoder's input
WIDTH (floor(W * sf)), i.e. a tensor shape: it is always drawn by the host.
torchvision is not installed here: rotation restates its documented resampling and is pinned by nothing."""
import math

import torch
import torch.nn.functional as F

from . import _native as nv

KINDS = {"none": 0, "noise": 1, "brightness": 2, "blurring": 3, "rotation": 4, "scaling": 5}
NAMES = {v: k for k, v in KINDS.items()}
# The mixed layer (a set of kinds, one of them drawn per step): the native code 6 and the words of its parameter block (include/nerfsig.h)
MIXED = 6
SELECTOR, BRIGHTNESS, SIGMA, SCALING, ROTATION = 0, 1, 2, 3, 4
_WORDS = {2: slice(BRIGHTNESS, BRIGHTNESS + 1), 3: slice(SIGMA, SIGMA + 1), 4: slice(ROTATION, None), 5: slice(SCALING, SCALING + 1)}      # kind -> its words of the block


def parse_kinds(distortion):
    """The members of a mixed set, in kind order: from a tuple / list of names, "a+b+c", or "mixed" (all five).  "none" is a legal member (an undistorted step)."""
    names = list(distortion) if isinstance(distortion, (tuple, list)) else (["noise", "brightness", "blurring", "rotation", "scaling"] if distortion == "mixed" else str(distortion).split("+"))
    for n in names:
        if n not in KINDS:
            raise ValueError(f"distortion {distortion!r}: {n!r} is none of none, noise, rotation, scaling, blurring, brightness")
    if not names or len(set(names)) != len(names):
        raise ValueError(f"distortion {distortion!r}: a mixed set names at least one kind, each once")
    return tuple(sorted(names, key=KINDS.get))


class _Distort(torch.autograd.Function):
    """D(clamp(img)) for the native kinds on [B, H, W, C] (img = the unclamped render)."""

    @staticmethod
    def forward(ctx, img, kind, param, noise):
        img = img.contiguous().float()
        B, H, W, C = img.shape
        out = torch.empty_like(img)
        nv.call("wm_distort_fwd", nv.ptr(img), B, H, W, C, kind, nv.ptr(param), nv.ptr(noise), nv.ptr(out), nv.stream())
        ctx.save_for_backward(img, param, noise)
        ctx.kind = kind
        return out

    @staticmethod
    def backward(ctx, g):
        img, param, noise = ctx.saved_tensors
        B, H, W, C = img.shape
        gx = torch.empty_like(img)
        nv.call("wm_distort_bwd", nv.ptr(g.contiguous().float()), nv.ptr(img), B, H, W, C, ctx.kind, nv.ptr(param), nv.ptr(noise), nv.ptr(gx), nv.stream())
        return gx, None, None, None


class _DistortGeometry(torch.autograd.Function):
    """rotation / scaling of clamp(img) for [B, H, W, C] (img = the unclamped render) -> (distorted [B, H, W_out, C], clamp(img))."""

    @staticmethod
    def forward(ctx, img, kind, param, out_width):
        img = img.contiguous().float()
        B, H, W, C = img.shape
        out = torch.empty(B, H, out_width, C, dtype=torch.float32, device=img.device)
        clamped = torch.empty_like(img)
        nv.call("wm_distort_geom_fwd", nv.ptr(img), B, H, W, C, kind, nv.ptr(param), out_width, nv.ptr(out), nv.ptr(clamped), nv.stream())
        ctx.save_for_backward(img, param)
        ctx.kind, ctx.out_width = kind, out_width
        ctx.mark_non_differentiable(clamped)
        ctx.set_materialize_grads(False)
        return out, clamped

    @staticmethod
    def backward(ctx, g, _=None):
        if g is None:
            return None, None, None, None
        img, param = ctx.saved_tensors
        B, H, W, C = img.shape
        gx = torch.empty_like(img)
        nv.call("wm_distort_geom_bwd", nv.ptr(g.contiguous().float()), nv.ptr(img), B, H, W, C, ctx.kind, nv.ptr(param), ctx.out_width, nv.ptr(gx), nv.stream())
        return gx, None, None, None


_M64 = (1 << 64) - 1


def _mix64(z):
    """splitmix64's finaliser"""
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def _draw_key(seed, step):
    return _mix64((int(seed) ^ (0x9E3779B97F4A7C15 * (int(step) + 1))) & _M64)


def host_uniform(seed, step, lo, hi):
    """One U[lo, hi) draw as a pure function of (seed, step) -- splitmix64's finaliser, the generator the device-side draws use -- for the one parameter a
    captured loop needs on the HOST (the scaling factor: it decides which captured shape a step replays); the same on every rank."""
    u = (_mix64(_draw_key(seed, step) ^ _M64) >> 40) / 16777216.0
    return lo + (hi - lo) * u


def kinds_mask(kinds):
    """The bit mask of a set of kinds (names or codes): bit k = kind k."""
    return sum(1 << (KINDS[k] if isinstance(k, str) else int(k)) for k in set(kinds))


def host_selector(seed, step, mask):
    """Which kind of the set `mask` (bit k = kind k) the mixed layer trains against at (seed, step): the host's statement of wm_distort_draw(6)'s selector --
    the (floor(u n))-th of the n members in kind order, u a 24-bit word of a sequence of its own under the step's key.  A captured loop whose set holds
    scaling asks it which captured width to replay; the same on every rank."""
    mask = int(mask)
    if mask <= 0 or mask >> 6:
        raise ValueError(f"host_selector: the mask {mask:#x} is empty or holds bits beyond the kinds 0..5")
    members = [k for k in range(6) if (mask >> k) & 1]
    return members[((_mix64(_draw_key(seed, step) ^ 0xC2B2AE3D27D4EB4F) >> 40) * len(members)) >> 24]


def scaled_width(W, sf):
    """F.interpolate's output size for scale_factor = sf: floor(W * sf) in double precision, at least one column."""
    return max(1, int(math.floor(float(W) * float(sf))))


class DistortionLayer:
    """distortion: one of none | noise | brightness | blurring | rotation | scaling -- or a SET of them (a tuple / list of names, "a+b+c", "mixed" = all five; "none"
    may be a member): every step then draws one kind of the set uniformly and that kind's parameter as the single-kind layer does (no composition).  A single
    kind is the set of itself: `kinds` has one member, `selected` is that kind for ever and `param` is its parameter.  A mixed set's kind is a word in device
    memory (the native code 6: one captured step serves every kind), `param` is the native parameter block (selector word, every kind's parameter at its own word)
    and `selected` is the step's kind where the host knows it (draw, set_mixed, select_on_host) and None where only the device does (a captured step).

    draw(shape, device)              the eager loop's per-step draws: torch's generators, the calls the reference's libraries make (from generators of
                                     the layer's own, seeded with `seed`)
    draw_on_device(step_counter)     the captured loop's: wm_distort_draw from (seed, replay count) -- no host value involved
    param / noise                    the device buffers the decoder reads (static addresses: a captured graph holds them)
    out_width(W)                     the decoder's input width for this step's draw (scaling: floor(W * sf); W otherwise)
    __call__(pred_rgb)               the layer on the CLAMPED blocks [B, H, W, 3] as stand-alone operators (rotation, scaling, and the
                                     other kinds when the decoder's fused first layer is not available)"""

    def __init__(self, distortion="none", seed=0):
        self.mixed = isinstance(distortion, (tuple, list)) or (isinstance(distortion, str) and (distortion == "mixed" or "+" in distortion))
        if self.mixed:
            self.kinds = parse_kinds(distortion)
            self.name = distortion if isinstance(distortion, str) else "+".join(self.kinds)
        elif distortion not in KINDS:
            raise ValueError(f"distortion {distortion!r}: choose from none, noise, rotation, scaling, blurring, brightness (main_nerf_wtmk.py:75)")
        else:
            self.kinds, self.name = (distortion,), distortion
        self.seed, self.mask = int(seed), kinds_mask(self.kinds)
        self.kind = MIXED if self.mixed else KINDS[distortion]
        self.selected = None if self.mixed else self.kind
        self.param = self.noise = None
        self.factor = 1.0             # scaling: this step's factor as the host knows it (it decides a shape)
        # generators of the layer's own, seeded alike on every rank: the decoder is replicated in a data-parallel run (it sees the all-gathered
        # blocks), so every rank has to distort them the same way
        self._host_gen = torch.Generator(device="cpu").manual_seed(self.seed)
        self._dev_gen = None

    @property
    def native(self):
        return self.kind > 0

    @property
    def fused(self):
        """applied inside the fused decoder's first layer (dec_forward_train: the codes 1..3, and 6, which reads the step's kind on the device) -- except in a step
        the HOST knows to be a scaling step (another decoder width, hence another capture): there the decoder runs plain, behind the resampling launch."""
        return self.kind in (1, 2, 3, MIXED) and self.selected != 5

    @property
    def geometric(self):
        """a resampling kernel of its own in front of the decoder (wm_distort_geom_fwd): the scaling launch in a scaling step, else the rotation launch whenever
        the set holds rotation -- always enqueued, an exact copy at the (1, 0) an unselected rotation keeps."""
        return self.selected == 5 or "rotation" in self.kinds

    @property
    def code(self):
        """the native `distortion` argument: a single kind's own code (never a one-member 6: code 6 always goes through the scratch image and its extra launch);
        a mixed set: 6, the set's mask and the block's image count in one word"""
        return self.kind if not self.mixed else MIXED | self.mask << 8 | ((self.param.numel() - ROTATION) // 2) << 16

    @property
    def needs_grad_scratch(self):
        """the fused decoder's image gradient goes through a scratch image and the layer's adjoint launch (dec_backward_train: the blur, and every mixed set)"""
        return self.kind in (3, MIXED)

    @property
    def geom_kind(self):
        """which resampling the launch in front of the decoder is (4 | 5)"""
        return 5 if self.selected == 5 else 4

    @property
    def geom_param(self):
        """the device parameter that launch reads"""
        return self.word(self.geom_kind)

    def word(self, kind):
        """the device words that hold `kind`'s parameter: `param` itself, or the kind's slice of a mixed set's block; None for a kind without one"""
        if kind not in _WORDS:
            return None
        return self.param[_WORDS[kind]] if self.mixed else self.param

    def out_width(self, W):
        return scaled_width(W, self.factor) if self.selected == 5 else int(W)

    def widths(self, W):
        """{decoder input width: a scaling factor that gives it} over the factor's range [0.75, 1.25): the shapes a captured loop has to hold"""
        return {scaled_width(W, f): f for f in (0.75 + 0.5 * i / 4096.0 for i in range(4096))}

    def _buffers(self, shape, device):
        n_images = int(shape[0])
        n = ROTATION + 2 * n_images if self.mixed else (2 * n_images if self.kind == 4 else 1)       # rotation: (cos, sin) per image
        if self.mixed and n_images >= 65536:
            raise ValueError("the mixed layer's native code carries the image count in 16 bits")
        if self.param is None or self.param.device != device or self.param.numel() != n:
            self.param = torch.zeros(n, dtype=torch.float32, device=device)
            if self.mixed:
                self.param[ROTATION::2] = 1.0       # an unselected rotation: (cos, sin) = (1, 0); selector word 0: "none" until the first draw
        if "noise" in self.kinds and (self.noise is None or tuple(self.noise.shape) != tuple(shape) or self.noise.device != device):
            self.noise = torch.zeros(tuple(shape), dtype=torch.float32, device=device)

    def _set(self, kind, value=None, noise=None):
        """This step's kind and its parameter, from host values (tests, tools, the eager draw): the kind's word(s) and, in a mixed set's block, the selector word and
        every rotation pair at (1, 0) unless rotation is the kind.  value: the brightness factor / the sigma / the scaling factor / one angle (radians) per image;
        noise: a tensor copied into the noise buffer.  The buffers must exist (draw, draw_on_device or _buffers has sized them)."""
        if kind not in self.kinds:
            raise ValueError(f"{kind!r} is no member of {self.name!r}")
        code = KINDS[kind]
        if code >= 2 and value is None:
            raise ValueError(f"{kind} needs its parameter")
        # writes only: nothing is read back from the device, so an eager loop's per-step draw does not wait for it
        if self.mixed:
            self.param[SELECTOR:SELECTOR + 1].view(torch.int32).fill_(code)
        if code == 4:
            if 2 * len(value) != self.word(4).numel():
                raise ValueError(f"rotation takes one angle per image ({self.word(4).numel() // 2})")
            self.word(4).copy_(torch.tensor([[math.cos(a), math.sin(a)] for a in value], dtype=torch.float32).reshape(-1))
        elif self.mixed:
            self.word(4).copy_(torch.tensor([1.0, 0.0]).repeat(self.word(4).numel() // 2))
        if code == 5:
            self.factor = float(value)
            self.word(5).fill_(self.factor)
        elif code in (2, 3):
            self.word(code).fill_(float(value))
        if noise is not None:
            self.noise.copy_(noise)
        self.selected = code

    def set_mixed(self, kind, factor=None, sigma=None, radians=None, scaling=None, noise=None):
        """this step's kind of a set and its parameter by name (_set)"""
        self._set(kind, {"brightness": factor, "blurring": sigma, "rotation": radians, "scaling": scaling}.get(kind), noise)

    def set_rotation(self, radians):
        """this step's angles, one per image (host values -> the device buffer the kernels read)"""
        self._set("rotation", radians)

    def set_scaling(self, sf):
        self._set("scaling", sf)

    def select_on_host(self, step):
        """The kind the device draws at `step` (host_selector) -- and, for scaling, its factor (host_uniform) -- as host values: what decides which captured
        shape a loop replays, and what out_width / fused / geometric answer afterwards.  Returns the kind's code."""
        self.selected = host_selector(self.seed, step, self.mask)
        if self.selected == 5:
            self.factor = host_uniform(self.seed, step, 0.75, 1.25)
        return self.selected

    def _draw_kind(self, kind, shape, device):
        """one kind's draw as the reference's libraries make it, from the layer's generators"""
        gen = self._host_gen
        if kind == "noise":           # utils_wtmk_disen.py:555: torch.normal(0, sqrt(0.1), size=pred_rgb.shape, device=pred_rgb.device)
            if self._dev_gen is None or self._dev_gen.device != device:
                self._dev_gen = torch.Generator(device=device).manual_seed(self.seed)
            self._set(kind)
            torch.normal(0.0, math.sqrt(0.1), size=tuple(shape), generator=self._dev_gen, device=device, out=self.noise)
        elif kind == "brightness":    # ColorJitter.get_params: float(torch.empty(1).uniform_(lo, hi)) on the host
            self._set(kind, float(torch.empty(1).uniform_(0.5, 1.5, generator=gen)))
        elif kind == "blurring":      # GaussianBlur.get_params: torch.empty(1).uniform_(sigma_min, sigma_max).item()
            self._set(kind, float(torch.empty(1).uniform_(0.01, 0.5, generator=gen)))
        elif kind == "rotation":      # RandomRotation.get_params, once per image (utils_wtmk_disen.py:560): float(torch.empty(1).uniform_(-30, 30))
            self._set(kind, [math.radians(float(torch.empty(1).uniform_(-30.0, 30.0, generator=gen))) for _ in range(int(shape[0]))])
        elif kind == "scaling":       # utils_wtmk_disen.py:563: sf = torch.empty(1).uniform_(0.75, 1.25).item(), ONE factor per call
            self._set(kind, torch.empty(1).uniform_(0.75, 1.25, generator=gen).item())
        else:
            self._set(kind)

    def draw(self, shape, device):
        """The eager loops' draw: a mixed set picks its kind with one torch.randint from the layer's host generator (a single kind draws none), then the kind's own draw."""
        if not self.native:
            return
        self._buffers(shape, device)
        pick = int(torch.randint(len(self.kinds), (1,), generator=self._host_gen)) if self.mixed else 0
        self._draw_kind(self.kinds[pick], shape, device)

    def draw_on_device(self, step_counter, shape, device):
        """The captured loop's draws: a pure function of (seed, *step_counter) computed on the device -- a mixed set's selector, then the selected kind's parameter
        (a scaling step's factor too: the word host_uniform gives the host).  A lone scaling factor is a host value (it selects the captured shape):
        trainer.GraphedWatermarkLoop sets it through host_uniform / set_scaling."""
        if self.kind == 5:
            raise NotImplementedError("the scaling factor decides the decoder's input width: it is drawn by the host (host_uniform, set_scaling)")
        self._buffers(shape, device)
        n = self.noise.numel() if self.noise is not None else (int(shape[0]) if self.kind == 4 else 0)
        nv.call("wm_distort_draw", self.code, self.seed, nv.ptr(step_counter), n, nv.ptr(self.param), nv.ptr(self.noise), nv.stream())

    def __call__(self, pred_rgb, raw=None):
        """pred_rgb: clamped blocks [B, H, W, 3].  raw: the unclamped render (native kinds back-propagate through the clamp themselves)."""
        if self.name == "none":
            return pred_rgb
        if not pred_rgb.is_cuda:      # the selected kind's stock operators (the host knows the kind: draw / set_mixed / select_on_host)
            name = NAMES[self.selected]
            return pred_rgb if name == "none" else reference_ops(pred_rgb, name, self.factor if name == "scaling" else self.word(self.selected), self.noise)
        x = pred_rgb if raw is None else raw
        if self.geometric:
            x = _DistortGeometry.apply(x, self.geom_kind, self.geom_param, self.out_width(pred_rgb.shape[2]))[0]
        return _Distort.apply(x, self.code, self.param, self.noise) if self.fused else x


def gaussian_kernel(sigma, dtype=torch.float32, device="cpu"):
    d = torch.tensor([-1.0, 0.0, 1.0], dtype=dtype, device=device)
    k = torch.exp(-0.5 * (d / sigma) ** 2)
    k = k / k.sum()
    return k[:, None] * k[None, :]


def reference_ops(pred_rgb, name, param=None, noise=None):
    """The layer on the CLAMPED blocks [B, H, W, C] as stock operators with the draws passed in (CPU / differentiable; what the kernels are tested
    against).  param: brightness factor / blur sigma (one element), rotation: (cos, sin) per image [2 B], scaling: the factor (a Python float)."""
    if name == "noise":
        return pred_rgb + noise
    if name == "brightness":
        return torch.clamp(pred_rgb * param.reshape(()), 0, 1)
    x = pred_rgb.permute(0, 3, 1, 2)
    if name == "rotation":
        cs = param.detach().reshape(-1, 2).cpu()
        return torch.stack([rotate_nearest(img, float(cs[i, 0]), float(cs[i, 1])) for i, img in enumerate(x)]).permute(0, 2, 3, 1)
    if name == "scaling":         # utils_wtmk_disen.py:565: every image [3, H, W] is a batch of 3 one-dimensional signals with H channels: resized along W only
        return torch.stack([F.interpolate(img, scale_factor=float(param), mode="linear") for img in x]).permute(0, 2, 3, 1)
    C = x.shape[1]
    k = gaussian_kernel(float(param), x.dtype, x.device).expand(C, 1, 3, 3)
    y = F.conv2d(F.pad(x, (1, 1, 1, 1), mode="reflect"), k, groups=C)
    return y.permute(0, 2, 3, 1)


def rotate_nearest(img, cos, sin):
    """[C, H, W] rotated counter-clockwise about its centre by the angle with the given (float32-representable) cosine and sine, same size,
    nearest-neighbour sampling (round half to even), zeros outside: the source of every output pixel centre (x, y measured from the image
    centre) is  x' = cos * x - sin * y,  y' = sin * x + cos * y  -- float32, every product and sum rounded on its own, as the kernel computes it."""
    C, H, W = img.shape
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32, device=img.device) - (H - 1) / 2,
                            torch.arange(W, dtype=torch.float32, device=img.device) - (W - 1) / 2, indexing="ij")
    sx = cos * xs - sin * ys + (W - 1) / 2
    sy = sin * xs + cos * ys + (H - 1) / 2
    ix, iy = torch.round(sx).long(), torch.round(sy).long()
    inside = (ix >= 0) & (ix < W) & (iy >= 0) & (iy < H)
    flat = img.reshape(C, H * W)
    out = flat[:, (iy.clamp(0, H - 1) * W + ix.clamp(0, W - 1)).reshape(-1)].reshape(C, H, W)
    return out * inside.to(img.dtype)
