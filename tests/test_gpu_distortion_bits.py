"""The distortion layer's output BITS, pinned: SHA-256 of the raw bytes every native distortion entry point (and the fused decoder with the layer inside it)
writes for fixed seeded inputs, against tests/golden/distortion_bits.json -- recorded once on an MI355X from the commit the file names.  The mixed-versus-single
tests prove the two paths equal each other; this one proves that neither moved.  A hash that differs means a floating-point statement was reordered or contracted
differently: find it by reading and restore it -- the file is not re-recorded."""
import functools
import hashlib
import json
import math
import os

import numpy as np
import pytest
import torch

import mixed_distortion_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "distortion_bits.json")
SHAPES = [(4, 2, 2, 3),       # reflection maps two taps onto one row and one column
          (5, 9, 14, 3)]      # 1890 elements: several 256-thread blocks with a ragged last one
DRAWS = [(3, 0), (2 ** 32 + 5, 65535)]      # (seed, step)
SIX, TWO = R.SETS["six"], R.SETS["two"]


def _sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().contiguous().cpu().numpy().tobytes())
    return h.hexdigest()


def _tag(shape):
    return "x".join(str(s) for s in shape)


def _raw(shape, seed=1):
    """Rendered blocks with pixels below 0, above 1, and at exactly 0, 1 and -0 (test_gpu_mixed_distortion._raw)."""
    rng = np.random.RandomState(seed)
    raw = rng.uniform(-0.25, 1.25, shape).astype(np.float32)
    flat = raw.reshape(-1)
    flat[::7], flat[3::11], flat[5::13] = 0.0, 1.0, -0.0
    return torch.from_numpy(raw)


def _noise(shape):
    return torch.from_numpy(np.random.RandomState(2).normal(0, math.sqrt(0.1), shape).astype(np.float32)).to(DEV)


def _randn(shape, seed=3):
    return torch.from_numpy(np.random.RandomState(seed).randn(*shape).astype(np.float32)).to(DEV)


def _forced(names, kind, shape, noise):
    """A mixed layer over `names` whose block holds `kind` and its parameter (mixed_distortion_ref.forced_parameters)."""
    from nerf_signature_amd.distortion import DistortionLayer
    layer = DistortionLayer(names, 3)
    layer._buffers(shape, torch.device(DEV))
    layer.set_mixed(kind, noise=noise if kind == "noise" else None, **R.forced_parameters(kind, shape[0]))
    return layer


def _draws():
    from nerf_signature_amd.distortion import DistortionLayer
    out, shape, dev = {}, SHAPES[1], torch.device(DEV)
    for seed, step in DRAWS:
        counter = torch.tensor([step], dtype=torch.int32, device=DEV)
        for what in ("noise", "brightness", "blurring", "rotation", SIX, TWO):
            layer = DistortionLayer(what, seed)
            layer.draw_on_device(counter, shape, dev)
            name = what if isinstance(what, str) else "+".join(what)
            out[f"draw/{seed}/{step}/{name}"] = _sha(layer.param, *([] if layer.noise is None else [layer.noise]))
    return out


def _layer_alone():
    from nerf_signature_amd import _native as nv
    out = {}
    for shape in SHAPES:
        B, H, W, C = shape
        raw, noise, g = _raw(shape).to(DEV), _noise(shape), _randn(shape)
        single = {"none": (0, None, None), "noise": (1, None, noise), "brightness": (2, torch.tensor([1.37], device=DEV), None),
                  "blurring": (3, torch.tensor([0.45], device=DEV), None)}
        cases = [(name, *v) for name, v in single.items()]
        for kind in SIX:
            layer = _forced(SIX, kind, shape, noise)
            cases.append((f"mixed:{kind}", layer.code, layer.param, layer.noise))
        for name, code, param, nz in cases:
            y, gx = torch.full_like(raw, -7.0), torch.full_like(raw, -7.0)
            nv.call("wm_distort_fwd", nv.ptr(raw), B, H, W, C, code, nv.ptr(param), nv.ptr(nz), nv.ptr(y), nv.stream())
            nv.call("wm_distort_bwd", nv.ptr(g), nv.ptr(raw), B, H, W, C, code, nv.ptr(param), nv.ptr(nz), nv.ptr(gx), nv.stream())
            out[f"layer/{_tag(shape)}/{name}/fwd"], out[f"layer/{_tag(shape)}/{name}/bwd"] = _sha(y), _sha(gx)
    return out


def _geometry():
    from nerf_signature_amd import _native as nv
    from nerf_signature_amd.distortion import scaled_width
    out = {}
    for shape in SHAPES:
        B, H, W, C = shape
        raw = _raw(shape).to(DEV)
        angles = {"identity": None, "spread": R.forced_parameters("rotation", B)["radians"], "alternating": [0.3 * (i + 1) * (-1) ** i for i in range(B)]}
        cases = []
        for name, radians in angles.items():
            pairs = [[1.0, 0.0]] * B if radians is None else [[math.cos(a), math.sin(a)] for a in radians]
            cases.append((f"rotation:{name}", 4, torch.tensor(pairs, dtype=torch.float32).reshape(-1).to(DEV), W))
        for sf in (0.75, 1.2, 1.01):      # 1.01: floor(W * sf) == W for both widths, the operator's copy case
            cases.append((f"scaling:{sf}", 5, torch.tensor([sf], dtype=torch.float32, device=DEV), scaled_width(W, sf)))
        assert scaled_width(W, 1.01) == W
        for name, kind, param, Wo in cases:
            y = torch.full((B, H, Wo, C), -7.0, device=DEV)
            clamped, gx = torch.full_like(raw, -7.0), torch.full_like(raw, -7.0)
            g = _randn((B, H, Wo, C))
            nv.call("wm_distort_geom_fwd", nv.ptr(raw), B, H, W, C, kind, nv.ptr(param), Wo, nv.ptr(y), nv.ptr(clamped), nv.stream())
            nv.call("wm_distort_geom_bwd", nv.ptr(g), nv.ptr(raw), B, H, W, C, kind, nv.ptr(param), Wo, nv.ptr(gx), nv.stream())
            out[f"geom/{_tag(shape)}/{name}/fwd"], out[f"geom/{_tag(shape)}/{name}/bwd"] = _sha(y, clamped), _sha(gx)
    return out


def _decoder():
    from nerf_signature_amd.hidden_models import get_hidden_decoder_multi_views
    torch.manual_seed(5)
    dec = get_hidden_decoder_multi_views(num_bits=1, redundancy=1, num_blocks=8, input_ch=3, channels=64).to(DEV)
    out = {}
    for shape in SHAPES:
        raw, noise = _raw(shape), _noise(shape)
        msg = torch.from_numpy(np.random.RandomState(4).randint(0, 2, (shape[0], 1)).astype(np.float32)).to(DEV)
        layers = {"none": None}
        for kind in ("noise", "brightness", "blurring"):
            layers[kind] = R.single_layer(kind, shape, torch.device(DEV), R.forced_parameters(kind, shape[0]), noise)
        for kind in ("brightness", "blurring"):
            layers[f"mixed:{kind}"] = _forced(SIX, kind, shape, noise)
        for name, layer in layers.items():
            for p in dec.parameters():
                p.grad = None
            a = raw.to(DEV).requires_grad_(True)
            decoded, pred = dec.decode_rendered(a, layer)
            torch.nn.functional.binary_cross_entropy_with_logits(decoded * 10.0, msg).backward()
            grads = [p.grad for p in dec.parameters() if p.grad is not None]
            assert len(grads) == 29
            key = f"decoder/{_tag(shape)}/{name}"
            out[key + "/decoded"], out[key + "/clamped"], out[key + "/grad_img"], out[key + "/grad_params"] = _sha(decoded), _sha(pred), _sha(a.grad), _sha(*grads)
    return out


GROUPS = {"draw": _draws, "layer": _layer_alone, "geom": _geometry, "decoder": _decoder}


@functools.lru_cache(maxsize=None)
def computed(group):
    return GROUPS[group]()


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_output_bits_are_the_recorded_ones(group):
    """Every hash of the group equals the recorded one, and the record holds exactly the group's items."""
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert len(golden["recorded_from"]) == 40
    want = {k: v for k, v in golden["sha256"].items() if k.startswith(group + "/")}
    got = computed(group)
    assert sorted(got) == sorted(want)
    differ = sorted(k for k in got if got[k] != want[k])
    assert not differ, f"{len(differ)} of {len(got)} outputs differ from commit {golden['recorded_from'][:7]}: {differ}"
