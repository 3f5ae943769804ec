"""The released model, the key and the verdict: what a signer hands out, what the signer keeps, and how a suspect model is tested.

After the watermark stage a model carries the whole codebook -- 2 D tables of 4 MiB -- and every render needs a message.  The field sees the codebook only as
the pre-sum S = sum_i table[2 i + bit_i] (network._presum), ONE [T, 2] table, so the model that carries one signature is

    release(model, message) -> ReleasedModel     the 16 base tables, S as `signature.weight`, the two MLP vectors, the grid buffers: 17 * 2^20 + 10 240 floats
                                                 at any D; no `msg_encoder.*`, no `msg_decoder.*`; render() takes no message and has the bits of
                                                 model.render(..., message) (same field launches, which take S already)
    SignatureKey                                 the secret: key pose(s) and block coordinates (the reference's --keyposes_dir / --keyblocks_dir files,
                                                 provider_wtmk.py:451,453,475,477, interchangeable with ours), intrinsics, render keywords, message, decoder
    verify(render, key) -> dict                  bits, matches, bit_accuracy and the exact p-value of that many matches under a fair coin
    pack(released, format) -> PackedReleasedModel   the same model with its 17 tables stored as fp16 pairs, 8-bit or 4-bit codes ("f16" | "q8" | "q4": 34, 17 or 8.5 MiB
                                                 of tables instead of 68) and rendered from that storage; its bits are those of the fp32 release whose tables went
                                                 through Tamper.apply("half" | "quantize", 8 | 4)

A released checkpoint uses the clean checkpoint's key names plus `signature.weight`: loaded with
checkpoint.load_checkpoint(path, clean_network, model_only=True) it gives the CLEAN model (strict=False reports `signature.weight` as unexpected and
ignores it) -- a loader that does not know about signatures renders the unsigned scene."""
import math
import os

import numpy as np
import torch
import torch.nn as nn

from . import fieldops as fo
from .renderer import NeRFRenderer, is_multi_message

SIGNATURE_KEY = "signature.weight"


class _Table(nn.Module):
    def __init__(self, weight):
        super().__init__()
        self.weight = nn.Parameter(weight, requires_grad=False)


class _TableList(nn.Module):
    def __init__(self, weights):
        super().__init__()
        self.embeddings = nn.ModuleList([_Table(w) for w in weights])

    def tables(self):
        return [m._parameters["weight"] for m in self.embeddings._modules.values()]


class _Params(nn.Module):
    def __init__(self, params):
        super().__init__()
        self.params = nn.Parameter(params, requires_grad=False)


_SCALARS = ("bound", "density_scale", "min_near", "density_thresh", "bg_radius")


class ReleasedModel(NeRFRenderer):
    """A signed field without its codebook (see the module's doc string).  Inference only: the occupancy-grid path (`run_cuda`) in training mode under
    torch.no_grad() (what test_bitacc / test_image run), in eval() mode (the burst loop), unstaged or staged.

    The packed MLP weights and any kept ray samples are caches of tensors that tamper.Tamper rewrites through raw pointers (no version counter moves):
    invalidate() drops them all; Tamper calls it after every write (tampered_tensors / tamper())."""

    def __init__(self, base_tables, signature, sigma_params, color_params, scalars, buffers=None, mean_count=0, mean_density=0):
        super().__init__(bound=scalars["bound"], cuda_ray=True, density_scale=scalars["density_scale"], min_near=scalars["min_near"],
                         density_thresh=scalars["density_thresh"], bg_radius=scalars["bg_radius"])
        if len(base_tables) != 16:
            raise ValueError(f"a released model has the 16 base tables, got {len(base_tables)}")
        for i, t in enumerate([*base_tables, signature]):
            fo._check_table(t, f"table {i}" if i < 16 else SIGNATURE_KEY)
        self.encoder = _TableList(base_tables)
        self.signature = _Table(signature)
        self.sigma_net = _Params(sigma_params)
        self.encoder_dir = _Params(torch.zeros(0, dtype=torch.float32, device=sigma_params.device))
        self.color_net = _Params(color_params)
        for name, value in (buffers or {}).items():
            setattr(self, name, value)                # (registered by NeRFRenderer: assigning a tensor replaces the buffer)
        self.mean_count, self.mean_density = mean_count, mean_density
        self._packed_cache = None

    # ------------------------------------------------------------------ caches

    def invalidate(self):
        """Drop every cache of the tensors tampering rewrites: the packed MLP weight image and the ray samples kept across renders."""
        self._packed_cache = None
        self._premarched = None
        self.drop_marched()

    def _packed(self):
        sp, cp = self.sigma_net.params, self.color_net.params
        key = (sp.data_ptr(), sp._version, cp.data_ptr(), cp._version)
        if self._packed_cache is None or self._packed_cache[0] != key:
            self._packed_cache = (key, fo.pack_weights(sp, cp))
        return self._packed_cache[1]

    def tampered_tensors(self):
        """What an attacker sees and quality.model_robustness tampers: the 16 base tables, the signature table, both MLP vectors (17 836 032 floats)."""
        return [*self.encoder.tables(), self.signature.weight, self.sigma_net.params, self.color_net.params]

    def tamper(self):
        """tamper.Tamper over tampered_tensors() that invalidates this model's caches after every write."""
        from .tamper import Tamper
        return Tamper(self.tampered_tensors(), on_write=self.invalidate)

    # ------------------------------------------------------------------ the field (the existing launches, which take S)

    def forward(self, x, d, message=None, fixed=None, twin=False):
        if twin:
            raise NotImplementedError("clean_twin on a released model: it holds no clean field apart from the signed one (render the source model)")
        return fo.field_apply(x, d, self.bound, self._packed(), self.encoder.tables(), (), self.signature.weight, None, fixed, False)

    def _eval_field_rows(self, capacity, message):
        return fo.field_rows_runner(capacity, self.bound, self.encoder.tables(), self.signature.weight, self._packed())

    def run(self, *args, **kwargs):
        raise NotImplementedError("a released model on the uniform-sample `run` path (cuda_ray=False): its re-sampled points are evaluated without the message "
                                  "(renderer_wtmk.py:187), which needs the clean field a released model does not hold; it renders on the occupancy-grid path")

    def render(self, rays_o, rays_d, staged=False, max_ray_batch=4096, **kwargs):
        """{"image", "depth"(, "weights_sum")} with the bits of the source model's render(rays_o, rays_d, message, ...).  Takes no message."""
        if "message" in kwargs or torch.is_tensor(staged) or staged not in (False, True):
            raise TypeError("ReleasedModel.render takes no message: the model carries one signature (release(model, message))")
        if kwargs.get("clean_twin"):
            raise NotImplementedError("clean_twin on a released model: it holds no clean field apart from the signed one (render the source model)")
        if torch.is_grad_enabled():
            raise RuntimeError("a released model is inference only (forward, no gradients): call render under torch.no_grad()")
        return super().render(rays_o, rays_d, None, staged=staged, max_ray_batch=max_ray_batch, **kwargs)

    # ------------------------------------------------------------------ checkpoint

    def save(self, path):
        """One torch.save'd dict in the reference's checkpoint shape ('model' = state_dict(), 'mean_count', 'mean_density') plus 'release': the constructor's scalars."""
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        torch.save({"model": {k: v.detach().cpu() for k, v in self.state_dict().items()}, "mean_count": self.mean_count, "mean_density": self.mean_density,
                    "release": {k: getattr(self, k) for k in _SCALARS}}, path)
        return path

    @classmethod
    def load(cls, path_or_dict, device=None):
        ckpt = torch.load(path_or_dict, map_location="cpu", weights_only=False) if isinstance(path_or_dict, (str, os.PathLike)) else path_or_dict
        sd = ckpt["model"]
        if SIGNATURE_CODES_KEY in sd or "format" in ckpt.get("release", {}):
            raise ValueError("this is a packed released model: load it with PackedReleasedModel.load (and unpack() it for fp32 tables)")
        if SIGNATURE_KEY not in sd:
            raise ValueError(f"not a released model: the checkpoint has no '{SIGNATURE_KEY}'")
        to = (lambda t: t.to(device)) if device is not None else (lambda t: t)
        base = [to(sd[f"encoder.embeddings.{i}.weight"].float()) for i in range(16)]
        model = cls(base, to(sd[SIGNATURE_KEY].float()), to(sd["sigma_net.params"].float()), to(sd["color_net.params"].float()), ckpt["release"],
                    mean_count=ckpt.get("mean_count", 0), mean_density=ckpt.get("mean_density", 0))
        if device is not None:
            model.to(device)
        missing, unexpected = model.load_state_dict({k: to(v) for k, v in sd.items()}, strict=False)
        if unexpected:
            raise ValueError(f"released checkpoint with unexpected keys {list(unexpected)}")
        return model.train()


def _sharded(model):
    from .network import _data_parallel
    return _data_parallel() or getattr(model, "codebook_shard", None) is not None or getattr(model, "_codebook_stale", False)


def signature_table(model, message):
    """S = sum_i table[2 i + bit_i] of `message` as a table of its own: the existing pre-sum launch (hg_codebook_presum, the one model.render's own pre-sum
    runs) into a fresh buffer.  A CPU model (format conversion, the CPU tests) is summed by torch in the same order."""
    bits = fo.message_bits(message)
    if len(bits) != model.message_dim:
        raise ValueError(f"message has {len(bits)} bits, the network was built with message_dim={model.message_dim}")
    selected = fo.select_tables(model.msg_encoder.tables(), bits)
    if selected[0].is_cuda:
        with torch.no_grad():
            return fo.codebook_presum(selected)
    S = selected[0].detach().clone()
    for t in selected[1:]:
        S += t.detach()
    return S


def release(model, message, copy=False):
    """The released form of `model` under `message` [D] (see ReleasedModel).  copy=False: base tables, MLP vectors and grid buffers are the source model's own
    tensors (tampering the release then tampers the source); copy=True: clones.  The signature table and the step-counter ring are always the release's own."""
    if is_multi_message(message):
        raise NotImplementedError("release under K messages [K, D]: a released model carries ONE signature (call release once per message)")
    if not getattr(model, "cuda_ray", False):
        raise NotImplementedError("release of a model on the uniform-sample `run` path (cuda_ray=False): its re-sampled points are evaluated without the message "
                                  "(renderer_wtmk.py:187), which needs the clean field a released model does not hold; build the model with cuda_ray=True")
    if _sharded(model):
        raise NotImplementedError("release under data-parallel table sharding: this rank holds current values only for the tables of its own bits, and the "
                                  "signature sums all of them (gather the codebook and release on one rank)")
    if message is None:
        raise ValueError("release needs a message: without one the model is the clean one")
    take = (lambda t: t.detach().clone()) if copy else (lambda t: t.detach())
    buffers = {"aabb_train": take(model.aabb_train), "aabb_infer": take(model.aabb_infer), "density_grid": take(model.density_grid),
               "density_bitfield": take(model.density_bitfield), "step_counter": model.step_counter.detach().clone()}
    out = ReleasedModel([take(t) for t in model.encoder.tables()], signature_table(model, message), take(model.sigma_net.params), take(model.color_net.params),
                        {k: getattr(model, k) for k in _SCALARS}, buffers, mean_count=model.mean_count, mean_density=model.mean_density)
    out.iter_density, out.local_step = model.iter_density, model.local_step
    out.train(model.training)
    return out


# ---------------------------------------------------------------------------------------------------- the packed form

SIGNATURE_CODES_KEY, TABLE_PARAMS_KEY = "signature.codes", "table_params"


class _Codes(nn.Module):
    def __init__(self, codes):
        super().__init__()
        self.register_buffer("codes", codes)


class _CodesList(nn.Module):
    def __init__(self, codes):
        super().__init__()
        self.embeddings = nn.ModuleList([_Codes(c) for c in codes])

    def codes(self):
        return [m._buffers["codes"] for m in self.embeddings._modules.values()]


class PackedReleasedModel(NeRFRenderer):
    """A released model whose 17 tables are stored as fp16 pairs ("f16"), 8-bit ("q8") or 4-bit ("q4") codes (include/nerfsig.h "packed released model";
    DESIGN.md section 22) and gathered from in that form: 34, 17 or 8.5 MiB of tables instead of 68.  Every table is one flat uint8 tensor
    (`encoder.embeddings.{i}.codes`, `signature.codes`); `table_params` [17, 2] holds each table's (lo, step) (zeros for f16); the MLP vectors stay fp32.
    render() has ReleasedModel.render's contract and the bits of the fp32 release whose 17 tables went through Tamper.apply("half") / ("quantize", 8) /
    ("quantize", 4): the decode restores exactly those floats.  Always the two-launch route (packed encoder, MLP over the plane set) -- the header guarantees
    the fused small-batch route gives the same bits.  Inference only; the fp32 density grid is not carried (the render path reads the bitfield): the model keeps
    the constructor's zero grid and refuses to refresh it."""

    def __init__(self, base_codes, signature_codes, table_params, format, sigma_params, color_params, scalars, buffers=None, mean_count=0, mean_density=0):
        super().__init__(bound=scalars["bound"], cuda_ray=True, density_scale=scalars["density_scale"], min_near=scalars["min_near"],
                         density_thresh=scalars["density_thresh"], bg_radius=scalars["bg_radius"])
        self.format = fo.pack_format(format)
        if len(base_codes) != 16:
            raise ValueError(f"a packed released model has the 16 base tables, got {len(base_codes)}")
        for i, c in enumerate([*base_codes, signature_codes]):
            fo._check_codes(c, self.format, f"codes {i}" if i < 16 else SIGNATURE_CODES_KEY)
        if table_params.dtype != torch.float32 or tuple(table_params.shape) != (17, 2):
            raise ValueError(f"{TABLE_PARAMS_KEY}: expected a float32 [17, 2] tensor, got {table_params.dtype} {tuple(table_params.shape)}")
        grid = self._buffers.pop("density_grid")                       # not part of the checkpoint: kept as a plain zero buffer
        self.register_buffer("density_grid", grid, persistent=False)
        self.encoder = _CodesList(base_codes)
        self.signature = _Codes(signature_codes)
        self.register_buffer(TABLE_PARAMS_KEY, table_params.contiguous())
        self.sigma_net = _Params(sigma_params)
        self.color_net = _Params(color_params)
        for name, value in (buffers or {}).items():
            setattr(self, name, value)
        self.mean_count, self.mean_density = mean_count, mean_density
        self._packed_cache = None

    def _packed(self):
        sp, cp = self.sigma_net.params, self.color_net.params
        key = (sp.data_ptr(), sp._version, cp.data_ptr(), cp._version)
        if self._packed_cache is None or self._packed_cache[0] != key:
            self._packed_cache = (key, fo.pack_weights(sp, cp))
        return self._packed_cache[1]

    # ------------------------------------------------------------------ the field (packed encoder, then the MLP launches over its plane set)

    def forward(self, x, d, message=None, fixed=None, twin=False):
        if twin:
            raise NotImplementedError("clean_twin on a released model: it holds no clean field apart from the signed one (render the source model)")
        if fixed is not None:
            raise NotImplementedError("fixed= points on a packed released model: kept base planes belong to the training step (render the fp32 model, or unpack())")
        return fo.field_forward_packed(x, d, self.bound, self.encoder.codes(), self.signature.codes, self.format, self.table_params, self._packed())

    def _eval_field_rows(self, capacity, message):
        return fo.field_rows_runner_packed(capacity, self.bound, self.encoder.codes(), self.signature.codes, self.format, self.table_params, self._packed())

    def run(self, *args, **kwargs):
        raise NotImplementedError("a released model on the uniform-sample `run` path (cuda_ray=False): its re-sampled points are evaluated without the message "
                                  "(renderer_wtmk.py:187), which needs the clean field a released model does not hold; it renders on the occupancy-grid path")

    def render(self, rays_o, rays_d, staged=False, max_ray_batch=4096, **kwargs):
        """{"image", "depth"(, "weights_sum")}: ReleasedModel.render's contract.  Takes no message."""
        message = kwargs.get("message")
        if (torch.is_tensor(staged) and staged.dim() == 2) or (message is not None and is_multi_message(message)):
            raise NotImplementedError("a render under K messages [K, D] on a packed released model: it carries ONE signature and takes no message")
        if "message" in kwargs or torch.is_tensor(staged) or staged not in (False, True):
            raise TypeError("PackedReleasedModel.render takes no message: the model carries one signature (release(model, message))")
        if kwargs.get("clean_twin"):
            raise NotImplementedError("clean_twin on a released model: it holds no clean field apart from the signed one (render the source model)")
        if torch.is_grad_enabled():
            raise RuntimeError("a released model is inference only (forward, no gradients): call render under torch.no_grad()")
        return super().render(rays_o, rays_d, None, staged=staged, max_ray_batch=max_ray_batch, **kwargs)

    def tamper(self):
        raise NotImplementedError("tamper() on a packed released model: the tampering kernels rewrite fp32 tensors -- unpack() it and tamper the ReleasedModel")

    def update_extra_state(self, *args, **kwargs):
        raise NotImplementedError("update_extra_state on a packed released model: it does not carry the fp32 density grid (only the bitfield the render reads)")

    def mark_untrained_grid(self, *args, **kwargs):
        raise NotImplementedError("mark_untrained_grid on a packed released model: it does not carry the fp32 density grid (only the bitfield the render reads)")

    # ------------------------------------------------------------------ back to fp32, checkpoint

    def _all_codes(self):
        return [*self.encoder.codes(), self.signature.codes]

    def unpack(self):
        """The ReleasedModel with the decoded fp32 tables (pk_unpack_tables; a CPU model: the same arithmetic with torch operators) and this model's own MLP vectors
        and buffers; its density grid is the zero grid."""
        codes = self._all_codes()
        with torch.no_grad():
            tables = fo.unpack_tables(codes, self.format, self.table_params) if codes[0].is_cuda else fo.unpack_tables_cpu(codes, self.format, self.table_params)
        buffers = {"aabb_train": self.aabb_train, "aabb_infer": self.aabb_infer, "density_grid": self.density_grid, "density_bitfield": self.density_bitfield,
                   "step_counter": self.step_counter.detach().clone()}
        out = ReleasedModel(tables[:16], tables[16], self.sigma_net.params.detach(), self.color_net.params.detach(), {k: getattr(self, k) for k in _SCALARS}, buffers,
                            mean_count=self.mean_count, mean_density=self.mean_density)
        out.iter_density, out.local_step = self.iter_density, self.local_step
        out.train(self.training)
        return out

    def save(self, path):
        """ReleasedModel.save's dict with the packed keys; 'release' gains 'format'.  No fp32 density grid."""
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        torch.save({"model": {k: v.detach().cpu() for k, v in self.state_dict().items()}, "mean_count": self.mean_count, "mean_density": self.mean_density,
                    "release": {**{k: getattr(self, k) for k in _SCALARS}, "format": self.format}}, path)
        return path

    @classmethod
    def load(cls, path_or_dict, device=None):
        ckpt = torch.load(path_or_dict, map_location="cpu", weights_only=False) if isinstance(path_or_dict, (str, os.PathLike)) else path_or_dict
        sd, rel = ckpt["model"], ckpt.get("release", {})
        if SIGNATURE_CODES_KEY not in sd or "format" not in rel:
            raise ValueError("not a packed released model" + (": this is an fp32 release, load it with ReleasedModel.load (and pack() it)" if SIGNATURE_KEY in sd else
                                                              f": the checkpoint has no '{SIGNATURE_CODES_KEY}'"))
        to = (lambda t: t.to(device)) if device is not None else (lambda t: t)
        base = [to(sd[f"encoder.embeddings.{i}.codes"]) for i in range(16)]
        model = cls(base, to(sd[SIGNATURE_CODES_KEY]), to(sd[TABLE_PARAMS_KEY].float()), rel["format"], to(sd["sigma_net.params"].float()),
                    to(sd["color_net.params"].float()), rel, mean_count=ckpt.get("mean_count", 0), mean_density=ckpt.get("mean_density", 0))
        if device is not None:
            model.to(device)
        missing, unexpected = model.load_state_dict({k: to(v) for k, v in sd.items()}, strict=False)
        if unexpected or missing:
            raise ValueError(f"packed released checkpoint with unexpected keys {list(unexpected)} or missing keys {list(missing)}")
        return model.train()


def pack(released, format):
    """The packed form of a ReleasedModel (see PackedReleasedModel): format "f16" | "q8" | "q4".  A CUDA model: tm_stats, then ONE pk_pack_tables pass over the 17
    tables, then one host read of the non-finite word; a CPU model (format conversion without a GPU, the CPU tests): the same arithmetic with torch operators, bit
    for bit.  The MLP vectors, the bitfield and the other buffers are the release's own tensors; the fp32 density grid is not carried.  A table with a value
    that is not finite cannot be coded by the q formats: ValueError."""
    if isinstance(released, PackedReleasedModel):
        raise ValueError("pack: the model is packed already (unpack() it to change the format)")
    if not isinstance(released, ReleasedModel):
        raise TypeError("pack takes a ReleasedModel (release(model, message)): the unreleased model carries 2 D codebook tables, not one signature")
    format = fo.pack_format(format)
    tables = [*released.encoder.tables(), released.signature.weight]
    with torch.no_grad():
        if tables[0].is_cuda:
            codes, params, bad = fo.pack_tables(tables, format)
            bad = int(bad.item())                                     # (the one host read)
        else:
            codes, params, bad = fo.pack_tables_cpu(tables, format)
    if bad:
        raise ValueError(f"pack: {bad} table value(s) are not finite and have no {format} code (f16 stores them; q8 / q4 cannot)")
    buffers = {"aabb_train": released.aabb_train, "aabb_infer": released.aabb_infer, "density_bitfield": released.density_bitfield,
               "step_counter": released.step_counter.detach().clone()}
    out = PackedReleasedModel(codes[:16], codes[16], params, format, released.sigma_net.params.detach(), released.color_net.params.detach(),
                              {k: getattr(released, k) for k in _SCALARS}, buffers, mean_count=released.mean_count, mean_density=released.mean_density)
    if released.density_grid.device != out.density_grid.device:
        out.density_grid = out.density_grid.to(released.density_grid.device)
    out.iter_density, out.local_step = released.iter_density, released.local_step
    out.train(released.training)
    return out


# ---------------------------------------------------------------------------------------------------- the key

_MEAN, _STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
POSES_FILE, BLOCKS_FILE, KEY_FILE = "keyposes.npy", "keyblocks.npy", "key.pt"


class SignatureKey:
    """What the signer keeps.  poses [n, 4, 4] float32 and blocks [D, 4] int64 (row0, col0, row1, col1) are the reference's key files; a key built from ready
    block rays (from_block_rays: the synthetic stage) has neither and stores the rays themselves."""

    def __init__(self, message, decoder_state, intrinsics=None, H=None, W=None, poses=None, blocks=None, render_kwargs=None, block_o=None, block_d=None,
                 mean=_MEAN, std=_STD):
        self.message = torch.as_tensor(message).detach().to("cpu", torch.float32).reshape(-1)
        self.decoder_state = {k: v.detach().to("cpu", copy=True) for k, v in decoder_state.items()}
        self.intrinsics = None if intrinsics is None else tuple(float(v) for v in intrinsics)
        self.H, self.W = (None if H is None else int(H)), (None if W is None else int(W))
        self.poses = None if poses is None else np.asarray(poses.detach().cpu().numpy() if torch.is_tensor(poses) else poses, dtype=np.float32).reshape(-1, 4, 4)
        self.blocks = None if blocks is None else np.asarray(blocks.detach().cpu().numpy() if torch.is_tensor(blocks) else blocks, dtype=np.int64).reshape(-1, 4)
        kw = dict(render_kwargs or {})
        self.render_kwargs = {"dt_gamma": float(kw.get("dt_gamma", 0.0)), "max_steps": int(kw.get("max_steps", 1024)), "bg_color": 1}
        self.block_o = None if block_o is None else block_o.detach().to("cpu", copy=True)
        self.block_d = None if block_d is None else block_d.detach().to("cpu", copy=True)
        self.mean, self.std = tuple(float(v) for v in mean), tuple(float(v) for v in std)
        if (self.poses is None) != (self.blocks is None) or (self.poses is None and self.block_o is None):
            raise ValueError("a key needs key poses AND block coordinates, or ready block rays")
        if self.blocks is not None and len(self.blocks) != self.D:
            raise ValueError(f"{len(self.blocks)} blocks for a message of {self.D} bits")
        self._decoder = {}
        self._rays = {}

    @property
    def D(self):
        return int(self.message.numel())

    @classmethod
    def from_block_rays(cls, message, decoder, block_o, block_d, render_kwargs=None):
        return cls(message, decoder.state_dict() if isinstance(decoder, nn.Module) else decoder, block_o=block_o, block_d=block_d, render_kwargs=render_kwargs)

    def with_message(self, message):
        """The same key for another message (a signer's second model: same poses, blocks and decoder)."""
        other = SignatureKey.__new__(SignatureKey)
        other.__dict__.update(self.__dict__)
        other.message = torch.as_tensor(message).detach().to("cpu", torch.float32).reshape(-1)
        if other.D != self.D:
            raise ValueError(f"message has {other.D} bits, the key {self.D}")
        return other

    def save(self, directory):
        os.makedirs(directory, exist_ok=True)
        if self.poses is not None:
            np.save(os.path.join(directory, POSES_FILE), self.poses)          # float32 [n, 4, 4], provider_wtmk.py:451
            np.save(os.path.join(directory, BLOCKS_FILE), self.blocks)        # int64 [D, 4], provider_wtmk.py:475
        torch.save({"message": self.message, "decoder": self.decoder_state, "intrinsics": self.intrinsics, "H": self.H, "W": self.W, "render_kwargs": self.render_kwargs,
                    "block_o": self.block_o, "block_d": self.block_d, "mean": self.mean, "std": self.std}, os.path.join(directory, KEY_FILE))
        return directory

    @classmethod
    def load(cls, directory):
        rest = torch.load(os.path.join(directory, KEY_FILE), map_location="cpu", weights_only=False)
        pf, bf = os.path.join(directory, POSES_FILE), os.path.join(directory, BLOCKS_FILE)
        poses, blocks = (np.load(pf), np.load(bf)) if os.path.exists(pf) else (None, None)
        return cls(rest["message"], rest["decoder"], rest["intrinsics"], rest["H"], rest["W"], poses, blocks, rest["render_kwargs"], rest["block_o"], rest["block_d"],
                   rest["mean"], rest["std"])

    def block_rays(self, device="cuda"):
        """(rays_o, rays_d) [D, bh, bw, 3] of the key blocks on `device`: the stored ones, or rebuilt from pose and block coordinates (rays.get_rays +
        blocks.block_rays, as provider_wtmk.py:455,481-494).  Kept per device."""
        device = torch.device(device)
        if device not in self._rays:
            if self.block_o is not None:
                self._rays[device] = (self.block_o.to(device).contiguous(), self.block_d.to(device).contiguous())
            else:
                from . import blocks as blk, rays
                if self.poses.shape[0] != 1:
                    raise NotImplementedError("block rays of more than one key pose: the reference reshapes the key view to [1, H, W, 3] (provider_wtmk.py:465)")
                r = rays.get_rays(torch.from_numpy(self.poses).to(device), self.intrinsics, self.H, self.W, -1)
                self._rays[device] = blk.block_rays(r["rays_o"].reshape(1, self.H, self.W, 3), r["rays_d"].reshape(1, self.H, self.W, 3), torch.from_numpy(self.blocks))
        return self._rays[device]

    def decoder(self, device):
        """The decoder module with the key's weights on `device` (built once per device), in training mode: its BatchNorm layers take batch statistics over
        the D blocks, as in every evaluation of the reference (which never calls eval(), utils_wtmk_disen.py:951)."""
        device = torch.device(device)
        if device not in self._decoder:
            from .hidden_models import get_hidden_decoder_multi_views
            dec = get_hidden_decoder_multi_views(num_bits=1, redundancy=1, num_blocks=8, input_ch=3, channels=64)
            dec.load_state_dict(self.decoder_state)
            self._decoder[device] = dec.to(device).train()
        return self._decoder[device]

    def normalize(self, x):
        mean = torch.tensor(self.mean, dtype=x.dtype, device=x.device).view(-1, 1, 1)
        std = torch.tensor(self.std, dtype=x.dtype, device=x.device).view(-1, 1, 1)
        return (x - mean) / std


# ---------------------------------------------------------------------------------------------------- the verdict

def p_value(D, k):
    """P(at least k of D fair coin flips agree) = sum_{j >= k} C(D, j) / 2^D, exact in Python integers, converted to float once."""
    if not 0 <= k <= D:
        raise ValueError(f"{k} matches of {D} bits")
    return sum(math.comb(D, j) for j in range(k, D + 1)) / (1 << D)


@torch.no_grad()
def verify(render, key):
    """Does the model behind `render` carry the key's message?  render: a ReleasedModel, a PackedReleasedModel, or ANY callable (rays_o, rays_d) -> image [..., 3] over the key's block
    rays [D, bh, bw, 3] (black-box verification of a suspect model).  The image is clamped to [0, 1] and goes through the decoder path of every evaluation
    (trainer.eval_step); bits = sign of the logits.  One host read.
    -> {"bits": [D] of 0/1, "matches": k, "bit_accuracy": k / D, "p_value": the chance of >= k matches from a model that knows nothing of the message}"""
    device = next(render.parameters()).device if isinstance(render, nn.Module) else None
    o, d = key.block_rays(device if device is not None else "cuda")
    if isinstance(render, (ReleasedModel, PackedReleasedModel)):
        image = render.render(o, d, staged=False, perturb=False, force_all_rays=True, **key.render_kwargs)["image"]
    else:
        image = render(o, d)
        image = image["image"] if isinstance(image, dict) else image
    image = torch.clamp(image.reshape(*o.shape[:-1], 3).float(), min=0, max=1)
    logits = key.decoder(image.device)(key.normalize(image.permute(0, 3, 1, 2))).reshape(-1)
    D = key.D
    if logits.numel() != D:
        raise ValueError(f"the decoder returned {logits.numel()} logits for a key of {D} bits")
    bits = (logits > 0).to(torch.uint8).cpu()                 # (the one host read)
    return verdict(bits, key.message)


def verdict(bits, message):
    """The record of `verify` for decoded bits against a message (host tensors or lists)."""
    bits = [int(b) for b in torch.as_tensor(bits).reshape(-1).tolist()]
    want = [int(v > 0) for v in torch.as_tensor(message).reshape(-1).tolist()]
    D = len(want)
    k = sum(int(a == b) for a, b in zip(bits, want))
    return {"bits": bits, "matches": k, "bit_accuracy": k / D, "p_value": p_value(D, k)}
