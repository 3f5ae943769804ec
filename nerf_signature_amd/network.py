"""NeRFNetwork: the watermarked field network behind the reference's class surface
(/root/reference/nerf/network_wtmk_tcnn.py:15-194), evaluated by libnerfsig's fused field kernels.

Sub-module names reproduce the reference's state_dict keys: `encoder` (16 base tables), `msg_encoder`
(2*message_dim codebook tables), `sigma_net.params`, `encoder_dir.params`, `color_net.params`,
`msg_decoder.*`, plus the renderer's buffers.  As in the reference the base encoder and both MLPs are
frozen (network_wtmk_tcnn.py:90-95) and `get_params` exposes only the codebook and the decoder."""
import torch

from . import fieldops as fo
from . import raymarching
from . import tcnn_compat as tcnn
from .hash_encoding import HashEmbedder
from .hash_encoding_wtmk_bit import HashEmbedder as HashEmbedder_msg
from .hidden_models import get_hidden_decoder_multi_views, normalize_img
from .renderer import NeRFRenderer


def _data_parallel():
    """More than one rank: the reference's Trainer wraps the model in DistributedDataParallel, which reduces the `.grad` autograd hands it -- the shared
    gradient would bypass it."""
    import torch.distributed as dist
    return dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1


class NeRFNetwork(NeRFRenderer):
    def __init__(self, num_layers=2, hidden_dim=64, geo_feat_dim=15, num_layers_color=3, hidden_dim_color=64, bound=1, message_dim=16,
                 n_views=1, finetune_decoder=False, **kwargs):
        super().__init__(bound, **kwargs)
        if (num_layers, hidden_dim, geo_feat_dim, num_layers_color, hidden_dim_color) != (2, 64, 15, 3, 64):
            raise NotImplementedError("the native field network implements the reference's default architecture: "
                                      "sigma 32->64->1+15, color 16+15->64->64->3")
        self.finetune_decoder = finetune_decoder
        self.num_layers, self.hidden_dim, self.geo_feat_dim = num_layers, hidden_dim, geo_feat_dim
        self.num_layers_color, self.hidden_dim_color = num_layers_color, hidden_dim_color
        self.message_dim = message_dim

        self.encoder = HashEmbedder(bounding_box=(0, 1), n_levels=16, n_features_per_level=2, log2_hashmap_size=19,
                                    base_resolution=16, finest_resolution=2048)
        self.msg_encoder = HashEmbedder_msg(bounding_box=(0, 1), n_levels=message_dim * 2, n_features_per_level=2,
                                            log2_hashmap_size=19, base_resolution=2048, finest_resolution=2048, message_dim=message_dim)
        self.msg_decoder = get_hidden_decoder_multi_views(num_bits=1, redundancy=1, num_blocks=8, input_ch=n_views * 3, channels=64)
        self.normalization = normalize_img
        mlp = {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None"}
        self.sigma_net = tcnn.Network(n_input_dims=32, n_output_dims=1 + geo_feat_dim,
                                      network_config={**mlp, "n_neurons": hidden_dim, "n_hidden_layers": num_layers - 1}, seed=1337)
        self.encoder_dir = tcnn.Encoding(n_input_dims=3, encoding_config={"otype": "SphericalHarmonics", "degree": 4})
        self.in_dim_color = self.encoder_dir.n_output_dims + geo_feat_dim
        self.color_net = tcnn.Network(n_input_dims=self.in_dim_color, n_output_dims=3,
                                      network_config={**mlp, "n_neurons": hidden_dim_color, "n_hidden_layers": num_layers_color - 1}, seed=1338)

        frozen = [*self.encoder.parameters(), *self.color_net.parameters(), *self.sigma_net.parameters()]
        if finetune_decoder:
            frozen += [*self.msg_encoder.parameters()]
        for p in frozen:
            p.requires_grad = False

        self._packed_cache = None   # (key, packed weight image)
        self._presum_cache = None   # (key, S)
        self._multi_presum = None   # forward_multi's own buffer of up to NSIG_MULTI_MAX_MESSAGES row-interleaved pre-sums (never the cache above)
        self.grad_sink = None       # optional fieldops.GradSink: backward accumulates the shared gradient there
        # shared_gradient_step (the drop-in modules switch it on): under a foreign training loop -- zero_grad / backward / GradScaler / torch.optim.Adam.step,
        # the reference Trainer's -- the D identical dense gradients are never materialised: fieldops.SharedGradient + optim.install_shared_gradient_hook
        self.shared_gradient_step = False
        self._shared_sink = None
        self.device_select = False  # True: CUDA messages select their tables on the device (graph-capturable step)
        self.codebook_shard = None  # (first bit, last bit) this rank's optimiser owns (dp.optimizer_shard): pre-sums are partial + all-reduced

    # ------------------------------------------------------------------ cached device images

    def _packed(self):
        sp, cp = self.sigma_net.params, self.color_net.params
        key = (sp.data_ptr(), sp._version, cp.data_ptr(), cp._version)
        if self._packed_cache is None or self._packed_cache[0] != key:
            # re-packed IN PLACE when a buffer exists: a captured graph holds its address (checkpoint.invalidate_derived)
            self._packed_cache = (key, fo.pack_weights(sp, cp, out=None if self._packed_cache is None else self._packed_cache[1]))
        return self._packed_cache[1]

    def _presum(self, selected, bits):
        """S = sum of the selected codebook tables; reused while neither the message nor the tables change
        (the two renders of one training step, every chunk of a staged full-image render)."""
        key = (bits, tuple((t.data_ptr(), t._version) for t in selected))
        if self._presum_cache is None or self._presum_cache[0] is None or self._presum_cache[0] != key:
            S = self._presum_cache[1] if self._presum_cache is not None else None
            self._presum_cache = (key, fo.codebook_presum(selected, out=S))
            self._presum_produced()
        else:
            self._presum_consumed()
        return self._presum_cache[1]

    def _presum_produced(self):
        """Remember where the pre-sum was computed: a render on another stream must wait for it (trainer.train_step issues the
        content render first, on its side stream, so the pre-sum runs beside the block render's march instead of before it)."""
        if self._presum_cache[1].is_cuda:
            self._presum_stream = torch.cuda.current_stream()
            self._presum_event = torch.cuda.Event()
            self._presum_event.record(self._presum_stream)

    def _presum_consumed(self):
        ev = getattr(self, "_presum_event", None)
        if ev is not None and self._presum_cache[1].is_cuda and torch.cuda.current_stream() != self._presum_stream:
            torch.cuda.current_stream().wait_event(ev)
            self._presum_cache[1].record_stream(torch.cuda.current_stream())

    def _message_bits(self, message):
        """fo.message_bits with the answer remembered for a device tensor seen before (same object, unmodified): the reference's Trainer hands one device
        tensor to both renders of a step -- one read-back per step instead of one per render."""
        if not (torch.is_tensor(message) and message.is_cuda):
            return fo.message_bits(message)
        import weakref
        cached = getattr(self, "_bits_cache", None)
        if cached is not None and cached[0]() is message and cached[1] == (message.data_ptr(), message._version):
            return cached[2]
        bits = fo.message_bits(message)
        self._bits_cache = (weakref.ref(message), (message.data_ptr(), message._version), bits)
        return bits

    def _select(self, message):
        if message is None:
            return (), None, None
        if getattr(self, "_codebook_stale", False):
            raise RuntimeError("host-side table selection while the codebook optimiser is sharded over the ranks: this rank's copies of the "
                               "other ranks' tables are stale -- call GraphedWatermarkLoop.gather_codebook() on every rank first")
        bits = self._message_bits(message)
        if len(bits) != self.message_dim:
            raise ValueError(f"message has {len(bits)} bits, the network was built with message_dim={self.message_dim}")
        selected = fo.select_tables(self.msg_encoder.tables(), bits)
        return selected, bits, self._presum(selected, bits)

    # ------------------------------------------------------------------ reference surface

    def _select_on_device(self, message):
        """All 2D tables + the pre-sum chosen by the device-resident message (no host read of its bits)."""
        tables = self.msg_encoder.tables()
        key = ("dev", message.data_ptr(), message._version, tuple((t.data_ptr(), t._version) for t in tables))
        if self._presum_cache is None or self._presum_cache[0] is None or self._presum_cache[0] != key:
            S = self._presum_cache[1] if self._presum_cache is not None else None
            if self.codebook_shard is not None:       # this rank holds current values only for the tables of its own bits
                import torch.distributed as dist
                from . import dp
                b0, b1 = self.codebook_shard
                S = fo.codebook_presum_sel(tables[2 * b0:2 * b1], message[b0:b1], out=S)
                dp.collective(lambda: dist.all_reduce(S, op=dist.ReduceOp.SUM), name="all_reduce_presum")
                self._presum_cache = (key, S)
            else:
                self._presum_cache = (key, fo.codebook_presum_sel(tables, message, out=S))
            self._presum_produced()
        else:
            self._presum_consumed()
        return tables, self._presum_cache[1]

    def adopt_presum(self, message):
        """Declare the existing pre-sum buffer valid for the device-resident `message` WITHOUT computing it: whoever calls this has
        arranged for the buffer to be filled before the renders run (the captured loop's optimiser kernel writes the next step's
        pre-sum, opt_codebook_adam_sel_next).  Returns the buffer."""
        if self._presum_cache is None:
            raise RuntimeError("adopt_presum: no pre-sum buffer exists yet (run prepare_message once)")
        tables = self.msg_encoder.tables()
        key = ("dev", message.data_ptr(), message._version, tuple((t.data_ptr(), t._version) for t in tables))
        self._presum_cache = (key, self._presum_cache[1])
        self._presum_produced()
        return self._presum_cache[1]

    def prepare_message(self, message):
        """Compute (or find cached) the pre-summed codebook of `message` now, on the current stream -- so that renders issued on
        different streams afterwards (trainer.train_step's overlapped content render) only read it."""
        if message is None:
            return
        if self.device_select and message.is_cuda:
            self._select_on_device(message)
        else:
            self._select(message)

    def forward(self, x, d, message, fixed=None, twin=False, rows_dev=None):
        """x: [N,3] in [-bound,bound], d: [N,3] unit, message: [message_dim] of 0./1. or None -> (sigma [N], color [N,3]).
        fixed: the fieldops.FixedPoints of exactly these points (fix_rays), or None.
        twin: -> (sigma, color, sigma_clean, color_clean): the field without the message at the same points, from the same launch (needs a message).
        rows_dev: a device count of the rows of x that hold points (a captured loop's padded buffers), or None: the backward pass stops there."""
        if twin and message is None:
            raise ValueError("forward(twin=True) needs a message: without one the field is the clean one")
        if self.device_select and message is not None and message.is_cuda:
            if self.grad_sink is None and torch.is_grad_enabled():
                raise RuntimeError("device_select needs a grad_sink: which tables were selected is not known on the host")
            tables, S = self._select_on_device(message)
            return fo.field_apply(x, d, self.bound, self._packed(), self.encoder.tables(), tables, S, self.grad_sink, fixed, twin, rows_dev)
        selected, _, S = self._select(message)
        sink = self.grad_sink
        if sink is None and self.shared_gradient_step and len(selected) and torch.is_grad_enabled() and x.is_cuda and not _data_parallel():
            if self._shared_sink is None or self._shared_sink.G.device != x.device:
                from .optim import install_shared_gradient_hook
                self._shared_sink = fo.SharedGradient(x.device)
                install_shared_gradient_hook(self._shared_sink)
            sink = self._shared_sink
        return fo.field_apply(x, d, self.bound, self._packed(), self.encoder.tables(), selected, S, sink, fixed, twin, rows_dev)

    # ------------------------------------------------------------------ one set of points under K messages (inference)

    def _check_multi_messages(self, messages, clean_twin=False):
        super()._check_multi_messages(messages, clean_twin)
        self._refuse_multi_when_sharded()

    def _refuse_multi_when_sharded(self):
        if _data_parallel() or self.codebook_shard is not None or getattr(self, "_codebook_stale", False):
            raise NotImplementedError("K messages under data-parallel table sharding: this rank holds current values only for the tables of its own bits, and the "
                                      "multi-message pre-sum reads all of them in one pass (gather the codebook and render on one rank)")

    def forward_multi_chunks(self, x, d, messages, fixed=None):
        """The field at points x under K messages [K, D] (host or device; a host tensor is copied once, nothing is read back), at most
        fieldops.MULTI_MAX_MESSAGES per launch: yields (sigma [k, N], color [k, N, 3]) chunk by chunk, in message order.  The 16 base planes are encoded once for
        all chunks (or are the kept ones of `fixed`, which is left untouched); per chunk one pass over the 2 D codebook tables (into a buffer of this model's own:
        `_presum_cache` is neither used nor invalidated), one K-plane gather and one MLP launch.  Inference only."""
        if torch.is_grad_enabled():
            raise RuntimeError("forward_multi is inference only (forward, no gradients): call it under torch.no_grad()")
        if not torch.is_tensor(messages) or messages.dim() != 2 or messages.shape[0] < 1 or messages.shape[1] != self.message_dim:
            raise ValueError(f"messages must be a [K, {self.message_dim}] tensor with K >= 1")
        self._refuse_multi_when_sharded()
        messages = messages.detach().to(device=x.device, dtype=torch.float32).contiguous()
        tables, base = self.msg_encoder.tables(), self.encoder.tables()
        packed = self._packed()
        x, d = x.contiguous().float(), d.contiguous().float()
        planes = fo.encode_base_planes(x, self.bound, base) if fixed is None and x.shape[0] else None
        for a, b in fo.message_chunks(messages.shape[0], fo.MULTI_MAX_MESSAGES):
            need = (b - a) * fo.T_ROWS * 2
            if self._multi_presum is None or self._multi_presum.numel() < need or self._multi_presum.device != x.device:
                self._multi_presum = torch.empty(need, dtype=torch.float32, device=x.device)
            S = fo.codebook_presum_multi(tables, messages[a:b], out=self._multi_presum)
            yield fo.field_forward_multi(x, d, self.bound, base, S, b - a, packed, fixed=fixed, planes=planes)

    def forward_multi(self, x, d, messages, fixed=None):
        """(sigma [K, N], color [K, N, 3]) for K messages [K, D]: slice k has the bits of forward(x, d, messages[k]) through a plane set.  See forward_multi_chunks."""
        chunks = list(self.forward_multi_chunks(x, d, messages, fixed=fixed))
        if len(chunks) == 1:
            return chunks[0]
        return torch.cat([c[0] for c in chunks]), torch.cat([c[1] for c in chunks])

    @torch.no_grad()
    def _eval_field_rows(self, capacity, message):
        """The field pass of the device-controlled eval loop (renderer._eval_loop_on_device): tables selected and the pre-sum computed ONCE per render;
        returns fn(xyzs, dirs, rows_dev, sigmas, rgbs) that evaluates the first *rows_dev rows (a device count) with launches sized for `capacity`."""
        _, _, S = self._select(message)
        return fo.field_rows_runner(capacity, self.bound, self.encoder.tables(), S, self._packed())

    def _count_points(self, o, d, dt_gamma, max_steps):
        """Padded sample total of these rays through the current grid (one counting march, one host read)."""
        nears, fars = raymarching.near_far_from_aabb(o, d, self.aabb_train, self.min_near)
        counter = torch.zeros(2, dtype=torch.int32, device=o.device)
        raymarching.march_rays_train_device(o, d, self.bound, self.density_bitfield, self.cascade, self.grid_size, nears, fars, counter, None, dt_gamma, int(max_steps))
        return raymarching.padded_point_count(int(counter[0]))      # (walk and offsets enqueued; no samples written)

    def fix_rays(self, rays_o, rays_d, dt_gamma=0, max_steps=1024):
        """Declare these ray tensors constant from step to step -- the watermark-block rays, one pair of tensors per dataset
        (nerf/provider_wtmk.py:442-494), rendered without jitter through a grid the watermark stage never updates: their samples are
        marched now, once, and the part of the field pass no step changes (the 16 frozen base levels' features, the scatter plan) is
        kept beside them (fieldops.FixedPoints).  Training renders of the same, unmodified tensors (`render(..., perturb=False,
        force_all_rays=True)`, the way train_step calls it) then gather only the codebook level, evaluate the MLPs and composite --
        bit-identical results.  An in-place change of the rays drops them out of the cache by itself (run_cuda matches tensors by
        address AND version); a changed occupancy grid or base table is noticed at the next eager render and refreshed in place.
        Buffer sizes: `point_capacity` for this ray count when a captured loop set one (trainer.GraphedWatermarkLoop: its overflow check
        covers these rays), otherwise one counting march here (a host read -- this is a set-up call) sizes them, and a later re-march
        that no longer fits (the grid changed) sizes them again.  Calling it again re-marches and refreshes in place.

        For the reference's own Trainer driving this model: one call after the dataset exists,
        `model.fix_rays(dataset.rays_o_block, dataset.rays_d_block, opt.dt_gamma, opt.max_steps)`, and train_step's block render
        (utils_wtmk_disen.py:590) takes this route."""
        _, o, d = self._flatten_rays(rays_o, rays_d)
        loop_capacity = self.capacity_for(o.shape[0])
        known = self.find_marched(o, d, fixed=True)
        capacity = loop_capacity if loop_capacity is not None else (known.capacity if known is not None else None)
        if capacity is None:
            capacity = self._count_points(o, d, dt_gamma, max_steps)
        rec = self.march_ahead(rays_o, rays_d, dt_gamma, max_steps, capacity=capacity)
        if loop_capacity is None and int(rec.counter[0]) > capacity:       # self-sized and outgrown: new buffers (nothing captured holds them)
            capacity = raymarching.padded_point_count(int(rec.counter[0]))
            rec = self.march_ahead(rays_o, rays_d, dt_gamma, max_steps, capacity=capacity)
        if rec.fixed is None:
            rec.fixed = fo.FixedPoints(rec.xyzs, self.bound, self.encoder.tables())
        else:
            rec.fixed.refresh(rec.xyzs, self.encoder.tables())
        rec.fixed_args, rec.grid_key = (dt_gamma, max_steps), self.grid_key()
        rec.rays_ref = (rays_o, rays_d)      # the cache is keyed by address + version: keep the tensors alive, or a later allocation could take the address
        return rec

    def density(self, x, message=None):
        selected, _, S = self._select(message)
        if torch.is_grad_enabled() and x.is_cuda and len(selected) and any(t.requires_grad for t in selected):
            # a caller differentiating density() directly (the reference reaches it under autograd from `run`, which goes through the joint field pass here)
            sigma, geo = fo.density_apply(x, self.bound, self._packed(), self.encoder.tables(), selected, S, self.grad_sink, self.sigma_net.params)
            return {"sigma": sigma, "geo_feat": geo}
        sigma, _, geo, _ = fo.field_forward(x, None, self.bound, self.encoder.tables(), S, self._packed(), want_rgb=False, want_geo=True)
        return {"sigma": sigma, "geo_feat": geo}

    def color(self, x, d, mask=None, geo_feat=None, **kwargs):
        grad = torch.is_grad_enabled() and geo_feat is not None and geo_feat.requires_grad and d.is_cuda
        one = (lambda dd, gg: fo.color_apply(dd, gg, self._packed(), self.color_net.params)) if grad else (lambda dd, gg: fo.field_color(dd, gg, self._packed()))
        if mask is not None:
            rgbs = torch.zeros(mask.shape[0], 3, dtype=torch.float32, device=x.device)
            if not mask.any():
                return rgbs
            rgbs[mask] = one(d[mask], geo_feat[mask])
            return rgbs
        return one(d, geo_feat)

    def get_params(self, lr):
        if self.finetune_decoder:
            params = [{"params": self.msg_decoder.parameters(), "lr": lr}]
        else:
            params = [{"params": self.msg_encoder.parameters(), "lr": lr}, {"params": self.msg_decoder.parameters(), "lr": lr}]
        if self.bg_radius > 0:
            raise NotImplementedError("background model (bg_radius > 0) is asserted off on this path (main_nerf_wtmk.py:86)")
        return params
