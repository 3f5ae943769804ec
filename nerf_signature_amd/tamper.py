"""Model tampering on the device (csrc/tamper.hip, include/nerfsig.h section "model tampering"): what a holder of released weights does to them --
global magnitude pruning, parameter noise, uniform quantisation, fp16 storage -- computed from a pristine copy into the live tensors.

    stats(tensors)                    -> [n, 4] float64 device tensor: per tensor min, max, mean, unbiased deviation of its finite elements (tm_stats)
    abs_kth(tensors, k)               -> (threshold_bits uint32 [1], count_le int64 [1]) device tensors: the k-th smallest magnitude over all values (tm_abs_kth)
    apply(src, dst, kind, ...)        -> one tm_apply pass
    Tamper(tensors, on_write=None)    apply(kind, strength, seed) / restore() on a fixed list with its pristine copy

Nothing here reads the device: a sweep enqueues select / statistics, the pass and whatever on_write invalidates, and goes on to render.  There is no CPU path."""
import ctypes

import torch

from . import _native as nv

KINDS = {"prune": 0, "noise": 1, "quantize": 2, "half": 3}      # include/nerfsig.h NSIG_TAMPER_*


def _list(tensors, what):
    tensors = list(tensors)
    if not tensors:
        raise ValueError(f"{what}: the tensor list is empty")
    for i, t in enumerate(tensors):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise nv.NativeError(f"{what}: tensor {i} is not on the GPU (the tampering kernels have no CPU path)")
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError(f"{what}: tensor {i} must be contiguous float32, got {t.dtype} with strides {t.stride()}")
        if t.numel() >= 1 << 32:
            raise ValueError(f"{what}: tensor {i} has {t.numel()} elements (at most 2^32 - 1 per tensor)")
        if t.device != tensors[0].device:
            raise ValueError(f"{what}: tensor {i} is on {t.device}, tensor 0 on {tensors[0].device}")
    return [t.detach() for t in tensors]


class _Launch:
    """The host side of one tensor list: pointer table(s), element counts and the scratch, built once."""

    def __init__(self, src, dst=None, what="tamper"):
        self.src = _list(src, what)
        self.dst = None if dst is None else _list(dst, what)
        if self.dst is not None and [t.numel() for t in self.dst] != [t.numel() for t in self.src]:
            raise ValueError(f"{what}: the source and destination lists differ in their element counts")
        self.n = len(self.src)
        self.total = sum(t.numel() for t in self.src)
        self.device = self.src[0].device
        ptrs = lambda ts: (ctypes.c_void_p * len(ts))(*[t.data_ptr() if t.numel() else None for t in ts])
        self.src_ptrs = ptrs(self.src)
        self.dst_ptrs = None if self.dst is None else ptrs(self.dst)
        self.numel = (ctypes.c_uint32 * self.n)(*[t.numel() for t in self.src])
        self._scratch = None

    def scratch(self):
        if self._scratch is None:
            self._scratch = torch.empty(int(nv.fn("tm_scratch_bytes")(self.n)), dtype=torch.uint8, device=self.device)
        return self._scratch

    def stats(self, out=None):
        out = torch.empty(self.n, 4, dtype=torch.float64, device=self.device) if out is None else out
        with torch.cuda.device(self.device):
            nv.call("tm_stats", self.src_ptrs, self.numel, self.n, nv.ptr(out), nv.ptr(self.scratch()), nv.stream())
        return out

    def abs_kth(self, k, out=None):
        threshold, count_le = out if out is not None else (torch.empty(1, dtype=torch.int32, device=self.device), torch.empty(1, dtype=torch.int64, device=self.device))
        with torch.cuda.device(self.device):
            nv.call("tm_abs_kth", self.src_ptrs, self.numel, self.n, int(k), nv.ptr(threshold), nv.ptr(count_le), nv.ptr(self.scratch()), nv.stream())
        return threshold, count_le

    def apply(self, kind, strength=0.0, bits=0, threshold=None, stats=None, seed=0):
        if self.dst is None:
            raise ValueError("tamper: this list has no destination")
        with torch.cuda.device(self.device):
            nv.call("tm_apply", self.src_ptrs, self.dst_ptrs, self.numel, self.n, KINDS[kind] if isinstance(kind, str) else int(kind), float(strength), int(bits),
                    nv.ptr(threshold), nv.ptr(stats), int(seed) & 0xFFFFFFFFFFFFFFFF, nv.stream())


def stats(tensors):
    return _Launch(tensors, what="tamper.stats").stats()


def abs_kth(tensors, k):
    """(threshold_bits [1] int32 holding the uint32 pattern, count_le [1] int64), on the device."""
    return _Launch(tensors, what="tamper.abs_kth").abs_kth(k)


def apply(src, dst, kind, strength=0.0, bits=0, threshold=None, stats=None, seed=0):
    _Launch(src, dst, what="tamper.apply").apply(kind, strength, bits, threshold, stats, seed)


class Tamper:
    """A fixed list of live fp32 device tensors and ONE pristine copy of them.  apply() always computes from the pristine copy into the live tensors, so calls
    never accumulate and a sweep needs no restore pass between its points; restore() copies the pristine values back.  on_write() runs after every write --
    whoever caches images of these tensors (release.ReleasedModel: packed MLP weights, kept ray samples) drops them there.

    kind / strength:  "prune"     the fraction p in [0, 1] of ALL listed values to zero, smallest magnitudes first: k = round(p * total), values tied with the
                                  k-th go too; p = 0 is a plain copy (no select)
                      "noise"     sigma relative to each tensor's own standard deviation; seed picks the draw
                      "quantize"  bits, 2 .. 16, uniform between each tensor's own min and max
                      "half"      through fp16 and back (strength is ignored)"""

    def __init__(self, tensors, on_write=None):
        live = _list(tensors, "Tamper")
        self.pristine = [t.clone() for t in live]
        self.launch = _Launch(self.pristine, live, what="Tamper")
        self.on_write = on_write
        dev = self.launch.device
        self._stats = torch.empty(self.launch.n, 4, dtype=torch.float64, device=dev)
        self._stats_valid = False          # (the pristine copy never changes: its statistics are taken once)
        self._threshold = (torch.empty(1, dtype=torch.int32, device=dev), torch.empty(1, dtype=torch.int64, device=dev))

    @property
    def total(self):
        return self.launch.total

    def _wrote(self):
        if self.on_write is not None:
            self.on_write()

    def restore(self):
        for p, t in zip(self.pristine, self.launch.dst):
            t.copy_(p)
        self._wrote()

    def apply(self, kind, strength=0.0, seed=0):
        if kind not in KINDS:
            raise ValueError(f"Tamper.apply: unknown kind {kind!r} (prune | noise | quantize | half)")
        if kind == "prune":
            p = float(strength)
            if not 0.0 <= p <= 1.0:
                raise ValueError(f"Tamper.apply: prune takes the fraction of values to remove, 0 .. 1, got {strength!r}")
            k = int(round(p * self.total))
            if k == 0:
                return self.restore()
            self.launch.abs_kth(k, out=self._threshold)
            self.launch.apply("prune", threshold=self._threshold[0])
        elif kind == "half":
            self.launch.apply("half")
        else:
            if not self._stats_valid:
                self.launch.stats(out=self._stats)
                self._stats_valid = True
            if kind == "noise":
                self.launch.apply("noise", strength=float(strength), stats=self._stats, seed=seed)
            else:
                if int(strength) != strength:
                    raise ValueError(f"Tamper.apply: quantize takes a whole number of bits, got {strength!r}")
                self.launch.apply("quantize", bits=int(strength), stats=self._stats)
        self._wrote()
