"""Released model, key, verdict and the tampering kernels' host side -- everything that needs no GPU: the p-value, the restatement's own checks (the unit
normal's moments, the fp32 noise arithmetic inside the noise bound, every mutant outside), the key files, the native refusals word for word against the built
library, and ReleasedModel on the CPU (refusals, state-dict keys, a released state dict loading into a clean network as the clean model)."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tamper_ref as tr  # noqa: E402


# ---------------------------------------------------------------------------------------------------- the verdict

def test_p_value_is_the_exact_binomial_tail():
    from nerf_signature_amd.release import p_value, verdict
    assert p_value(32, 32) == 2.0 ** -32
    for D in (1, 8, 32, 48, 64):
        assert p_value(D, 0) == 1.0
        for k in range(D + 1):
            assert p_value(D, k) == float(tr.p_value_exact(D, k))
    for k, want in ((29, 1.278e-6), (30, 1.232e-7), (31, 7.68e-9)):
        assert p_value(32, k) == pytest.approx(want, rel=1e-3)
    with pytest.raises(ValueError):
        p_value(32, 33)
    v = verdict([1, 0, 1, 1], [1.0, 0.0, 0.0, 1.0])
    assert v["matches"] == 3 and v["bit_accuracy"] == 0.75 and v["p_value"] == float(tr.p_value_exact(4, 3)) and v["bits"] == [1, 0, 1, 1]


# ---------------------------------------------------------------------------------------------------- the restatement's own checks

def test_unit_normal_of_the_documented_hash_is_a_unit_normal():
    n = 1 << 20
    z = tr.unit_normal(seed=7, i=3, n=n)
    assert abs(z.mean()) <= 5 / math.sqrt(n)
    assert abs(z.var() - 1.0) <= 5 * math.sqrt(2.0 / n)
    assert abs((z ** 4).mean() - 3.0) <= 5 * math.sqrt(96.0 / n)          # var z^4 = E z^8 - 9 = 96
    assert np.abs(z).max() <= 5.77                                         # u1 >= 2^-24: |z| <= sqrt(48 ln 2)
    assert not np.array_equal(z, tr.unit_normal(seed=8, i=3, n=n)) and not np.array_equal(z, tr.unit_normal(seed=7, i=4, n=n))
    u1, u2 = tr.noise_uniforms(7, 3, n)
    assert u1.min() > 0 and u1.max() <= 1 and u2.min() >= 0 and u2.max() < 1
    assert np.array_equal(tr.unit_normal(7, 3, 100, first=1000), z[1000:1100])      # a function of (seed, tensor, element) alone


def _lists():
    rng = np.random.RandomState(5)
    return [[rng.randn(65).astype(np.float32), (100 * rng.randn(7)).astype(np.float32), (0.01 * rng.randn(257)).astype(np.float32)],
            [rng.randn(1025).astype(np.float32), np.zeros(0, np.float32), rng.randn(7).astype(np.float32)]]


def _noise_f32(arrays, strength, seed, biased=False):
    out = []
    for i, a in enumerate(arrays):
        s = tr.noise_scale(strength, tr.finite_stats(a, biased)[3])
        out.append((a + s * tr.unit_normal_f32(seed, i, a.size)).astype(np.float32))
    return out


def _inside(arrays, ys, strength, seed):
    ok = True
    for a, y, (want, s, z) in zip(arrays, ys, tr.noise64(arrays, strength, seed)):
        ok = ok and bool(np.all(np.abs(y.astype(np.float64) - want) <= tr.noise_bound(a, s, z, tr.EPS_Z)))
    return ok


def test_fp32_noise_arithmetic_lies_inside_the_bound_and_the_biased_mutant_outside():
    assert tr.EPS_Z is not None and tr.EPS_Z == 4 * tr.Z_ERR_MEASURED
    for arrays in _lists():
        for strength in (0.0, 0.01, 1.0):
            assert _inside(arrays, _noise_f32(arrays, strength, 11), strength, 11)
    arrays = _lists()[0]
    assert not _inside(arrays, _noise_f32(arrays, 1.0, 11, biased=True), 1.0, 11)          # deviation with n for n - 1
    assert not _inside(arrays, _noise_f32(arrays, 1.0, 12), 1.0, 11)                       # another seed


def test_prune_mutants_differ_from_the_restatement():
    arrays = _lists()[0]
    same = lambda a, b: all(np.array_equal(x, y) for x, y in zip(a, b))
    want = tr.prune_fraction(arrays, 0.5)
    total = sum(a.size for a in arrays)
    assert sum(int((w == 0).sum()) for w in want) == round(0.5 * total)
    assert not same(want, tr.prune_fraction(arrays, 0.5, strict=True))             # `<` for `<=`: the k-th value itself survives
    assert not same(want, tr.prune_fraction(arrays, 0.5, per_tensor=True))         # a threshold per tensor: the 0.01-scale tensor is not emptied first
    assert int((want[2] == 0).sum()) > 0.95 * round(0.5 * total) and int((want[1] == 0).sum()) == 0      # (almost all of the k values go from the smallest-scale tensor)
    assert same(tr.prune_fraction(arrays, 0.0), arrays) and all(not w.any() for w in tr.prune_fraction(arrays, 1.0))
    again = tr.prune_fraction(want, 0.5)
    assert same(again, want)                                                         # applied to its own result: the zeros are the smallest magnitudes


def test_quantise_mutants_differ_from_the_restatement():
    arrays = _lists()[0]
    same = lambda a, b: all(np.array_equal(x, y) for x, y in zip(a, b))
    for bits in (2, 8, 16):
        want = tr.quantize(arrays, bits)
        assert not same(want, tr.quantize(arrays, bits, levels_plus_one=True))
        assert not same(want, tr.quantize(arrays, bits, floor=True))
        for a, w in zip(arrays, want):
            assert len(np.unique(w)) <= (1 << bits) and w.min() == a.min() and abs(float(w.max()) - float(a.max())) <= 2.0 ** -20 * (float(a.max()) - float(a.min()))
    const = [np.full(9, 3.25, np.float32)]
    assert same(tr.quantize(const, 4), const)
    odd = [np.array([1.0, np.inf, -2.0, np.nan, 0.5], np.float32)]
    q = tr.quantize(odd, 3)[0]
    assert np.isinf(q[1]) and np.isnan(q[3]) and q[0] == 1.0 and q[2] == -2.0


def test_statistics_restatement_and_its_biased_mutant():
    x = np.array([1.0, 2.0, 3.0, 4.0, np.inf, np.nan], np.float32)
    assert tr.finite_stats(x) == (1.0, 4.0, 2.5, math.sqrt(5.0 / 3.0))
    assert tr.finite_stats(x, biased=True)[3] == math.sqrt(5.0 / 4.0)
    assert tr.finite_stats(np.zeros(0, np.float32)) == (0.0, 0.0, 0.0, 0.0) and tr.finite_stats(np.array([7.0], np.float32)) == (7.0, 7.0, 7.0, 0.0)
    assert tr.abs_kth([np.array([3.0, -1.0], np.float32), np.array([-2.0, 1.0], np.float32)], 2) == (0x3F800000, 2)


# ---------------------------------------------------------------------------------------------------- the key

def _decoder_state():
    from nerf_signature_amd.hidden_models import get_hidden_decoder_multi_views
    torch.manual_seed(3)
    return get_hidden_decoder_multi_views(num_bits=1, redundancy=1, num_blocks=8, input_ch=3, channels=64).state_dict()


def test_key_files_are_the_references_arrays_and_round_trip(tmp_path):
    from nerf_signature_amd import blocks
    from nerf_signature_amd.release import BLOCKS_FILE, KEY_FILE, POSES_FILE, SignatureKey
    D = 6
    torch.manual_seed(1)
    poses = blocks.rand_poses(1, "cpu", radius=2.0)                               # provider_wtmk.py:446: [n_views, 4, 4] float32
    coords = torch.tensor([[r * 8, c * 8, r * 8 + 8, c * 8 + 8] for r, c in ((0, 1), (2, 3), (4, 4), (1, 0), (3, 3), (5, 2))])      # process_image: int64 [D, 4]
    message = torch.tensor([1., 0., 0., 1., 1., 0.])
    key = SignatureKey(message, _decoder_state(), intrinsics=(60.0, 60.0, 24.0, 24.0), H=48, W=48, poses=poses, blocks=coords, render_kwargs={"dt_gamma": 1 / 128, "max_steps": 512})
    key.save(str(tmp_path))
    assert sorted(os.listdir(tmp_path)) == sorted([POSES_FILE, BLOCKS_FILE, KEY_FILE])
    p, b = np.load(tmp_path / POSES_FILE), np.load(tmp_path / BLOCKS_FILE)
    assert p.shape == (1, 4, 4) and p.dtype == np.float32 and np.array_equal(p, poses.numpy())          # what np.save(path, watermark_poses.cpu().numpy()) writes
    assert b.shape == (D, 4) and b.dtype == np.int64 and np.array_equal(b, coords.numpy())              # what np.save(path, block_coordinates.cpu().numpy()) writes
    back = SignatureKey.load(str(tmp_path))
    assert torch.equal(back.message, message) and back.D == D and back.intrinsics == (60.0, 60.0, 24.0, 24.0) and (back.H, back.W) == (48, 48)
    assert back.render_kwargs == {"dt_gamma": 1 / 128, "max_steps": 512, "bg_color": 1}
    assert np.array_equal(back.poses, p) and np.array_equal(back.blocks, b)
    assert back.decoder_state.keys() == key.decoder_state.keys() and all(torch.equal(back.decoder_state[k], v) for k, v in key.decoder_state.items())
    assert back.mean == key.mean == (0.485, 0.456, 0.406) and back.std == (0.229, 0.224, 0.225)
    # a key of ready block rays (the synthetic stage) has no pose files and keeps the rays
    o, d = torch.rand(D, 4, 5, 3), torch.rand(D, 4, 5, 3)
    ray_key = SignatureKey.from_block_rays(message, _decoder_state(), o, d, {"dt_gamma": 0.0, "max_steps": 1024})
    ray_key.save(str(tmp_path / "rays"))
    assert os.listdir(tmp_path / "rays") == [KEY_FILE]
    back = SignatureKey.load(str(tmp_path / "rays"))
    bo, bd = back.block_rays("cpu")
    assert torch.equal(bo, o) and torch.equal(bd, d) and back.poses is None
    assert torch.equal(key.with_message(1 - message).message, 1 - message) and key.with_message(message).blocks is key.blocks
    with pytest.raises(ValueError):
        SignatureKey(message, _decoder_state())
    with pytest.raises(ValueError):
        SignatureKey(message, _decoder_state(), poses=poses, blocks=coords[:3], intrinsics=(1, 1, 1, 1), H=8, W=8)


# ---------------------------------------------------------------------------------------------------- native refusals

def _fake(n=1):
    return ctypes.c_void_p(4096 * n)      # a non-null address nobody reads: every refusal below comes before a launch


def test_native_refusals_word_for_word():
    from nerf_signature_amd import _native as nv

    def refused(name, *args):
        with pytest.raises(ValueError) as e:
            nv.call(name, *args)
        return str(e.value).split(": ", 1)[1]

    assert nv.fn("nsig_abi_version")() == 1
    assert nv.fn("tm_scratch_bytes")(0) == 0 and nv.fn("tm_scratch_bytes")(1) > 0 and nv.fn("tm_scratch_bytes")(33) > nv.fn("tm_scratch_bytes")(32)
    two = (ctypes.c_void_p * 2)(4096, 8192)
    hole = (ctypes.c_void_p * 2)(4096, None)
    odd = (ctypes.c_void_p * 2)(4096, 8194)
    numel = (ctypes.c_uint32 * 2)(5, 7)
    empty = (ctypes.c_uint32 * 2)(5, 0)
    calls = {"tm_stats": lambda src, num, n: refused("tm_stats", src, num, n, _fake(3), _fake(4), None),
             "tm_abs_kth": lambda src, num, n: refused("tm_abs_kth", src, num, n, 1, _fake(3), _fake(4), _fake(5), None),
             "tm_apply": lambda src, num, n: refused("tm_apply", src, two, num, n, 3, 0.0, 0, None, None, 0, None)}
    for who, call in calls.items():
        assert call(None, numel, 2) == f"{who}: null pointer"
        assert call(two, None, 2) == f"{who}: null pointer"
        assert call(two, numel, 0) == f"{who}: the tensor list is empty (n = 0)"
        assert call(hole, numel, 2) == f"{who}: tensor 1 has a null or misaligned pointer"
        assert call(odd, numel, 2) == f"{who}: tensor 1 has a null or misaligned pointer"
    assert refused("tm_stats", two, numel, 2, None, _fake(4), None) == "tm_stats: null pointer"
    assert refused("tm_stats", two, numel, 2, _fake(3), None, None) == "tm_stats: null pointer"
    assert refused("tm_stats", two, numel, 2, _fake(3), ctypes.c_void_p(4104), None) == "tm_stats: scratch must be 16-byte aligned, stats 8-byte aligned"
    kth = lambda k, num=numel, t=_fake(3), c=_fake(4), s=_fake(5): refused("tm_abs_kth", two, num, 2, k, t, c, s, None)
    assert kth(0) == "tm_abs_kth: k = 0 is out of range (1 .. 12, the number of listed values)"
    assert kth(13) == "tm_abs_kth: k = 13 is out of range (1 .. 12, the number of listed values)"
    assert kth(6, num=empty) == "tm_abs_kth: k = 6 is out of range (1 .. 5, the number of listed values)"
    assert kth(1, t=None) == kth(1, c=None) == kth(1, s=None) == "tm_abs_kth: null pointer"
    assert kth(1, s=ctypes.c_void_p(4104)) == "tm_abs_kth: scratch must be 16-byte aligned, count_le 8-byte aligned"
    apply = lambda kind, strength=0.0, bits=0, thr=None, stats=None, dst=two: refused("tm_apply", two, dst, numel, 2, kind, strength, bits, thr, stats, 0, None)
    assert apply(3, dst=None) == "tm_apply: null pointer"
    assert apply(3, dst=hole) == "tm_apply: tensor 1 has a null or misaligned pointer"
    assert apply(4) == "tm_apply: unknown kind 4 (0 prune, 1 noise, 2 quantize, 3 half)"
    for bad in (-0.5, float("inf"), float("nan")):
        for kind in (0, 1, 2, 3):
            assert apply(kind, bad, 8, _fake(6), _fake(7)) == "tm_apply: the strength must be a finite number >= 0"
    for bits in (0, 1, 17, 32):
        assert apply(2, 0.0, bits, None, _fake(7)) == f"tm_apply: quantize to {bits} bits is out of range (2 .. 16)"
    assert apply(0, 0.0, 0, None, _fake(7)) == "tm_apply: prune needs the threshold (threshold_bits, tm_abs_kth's)"
    assert apply(1, 0.5, 0, _fake(6), None) == apply(2, 0.0, 8, _fake(6), None) == "tm_apply: noise and quantize need the statistics (stats, tm_stats')"


def test_tamper_has_no_cpu_path():
    from nerf_signature_amd import _native as nv, tamper
    with pytest.raises(nv.NativeError, match="not on the GPU"):
        tamper.Tamper([torch.zeros(4)])
    with pytest.raises(ValueError, match="empty"):
        tamper.stats([])
    assert tamper.KINDS == tr.KINDS


# ---------------------------------------------------------------------------------------------------- ReleasedModel on the CPU

@pytest.fixture(scope="module")
def signed():
    from nerf_signature_amd.network import NeRFNetwork
    torch.manual_seed(0)
    model = NeRFNetwork(bound=1.0, cuda_ray=True, density_scale=1, min_near=0.2, density_thresh=10, bg_radius=-1, message_dim=2, n_views=1)
    for t in model.msg_encoder.tables():
        t.data.uniform_(-1e-2, 1e-2)
    model.density_grid.uniform_(0, 1)
    return model


def test_released_state_dict_has_one_signature_and_no_codebook(signed):
    from nerf_signature_amd.release import ReleasedModel, release
    message = torch.tensor([1., 0.])
    rel = release(signed, message)
    sd = rel.state_dict()
    assert not [k for k in sd if k.startswith(("msg_encoder.", "msg_decoder."))]
    clean_keys = {k for k in signed.state_dict() if not k.startswith(("msg_encoder.", "msg_decoder."))}
    assert set(sd) == clean_keys | {"signature.weight"}
    two_column = [k for k, v in sd.items() if tuple(v.shape) == (1 << 19, 2) and not k.startswith("encoder.")]
    assert two_column == ["signature.weight"]
    tabs = signed.msg_encoder.tables()
    assert torch.equal(sd["signature.weight"], tabs[1].detach() + tabs[2].detach())              # table[2 i + bit_i], summed in bit order
    assert sum(t.numel() for t in rel.tampered_tensors()) == 17 * (1 << 20) + 10240 == 17836032
    assert rel.encoder.tables()[3].data_ptr() == signed.encoder.tables()[3].data_ptr()          # references ...
    assert release(signed, message, copy=True).encoder.tables()[3].data_ptr() != signed.encoder.tables()[3].data_ptr()      # ... or copies
    assert all(not p.requires_grad for p in rel.parameters()) and rel.training == signed.training
    # a round trip through the dict keeps every tensor
    back = ReleasedModel.load({"model": sd, "release": {k: getattr(rel, k) for k in ("bound", "density_scale", "min_near", "density_thresh", "bg_radius")}})
    assert back.state_dict().keys() == sd.keys() and all(torch.equal(back.state_dict()[k], v) for k, v in sd.items())
    with pytest.raises(ValueError, match="not a released model"):
        ReleasedModel.load({"model": {k: v for k, v in sd.items() if k != "signature.weight"}, "release": {}})


def test_released_state_dict_loads_into_a_clean_network_as_the_clean_model(signed):
    from nerf_signature_amd import checkpoint
    from nerf_signature_amd.network import NeRFNetwork
    from nerf_signature_amd.release import release
    sd = release(signed, torch.tensor([0., 1.])).state_dict()
    torch.manual_seed(9)
    clean = NeRFNetwork(bound=1.0, cuda_ray=True, density_scale=1, min_near=0.2, density_thresh=10, bg_radius=-1, message_dim=2, n_views=1)
    before = {k: v.clone() for k, v in clean.state_dict().items() if k.startswith(("msg_encoder.", "msg_decoder."))}
    missing, unexpected, _ = checkpoint.load_checkpoint({"model": sd}, clean, model_only=True)
    assert unexpected == ["signature.weight"]
    assert missing and all(k.startswith(("msg_encoder.", "msg_decoder.")) for k in missing)
    now, src = clean.state_dict(), signed.state_dict()
    for k in sd:
        if k != "signature.weight":
            assert torch.equal(now[k], src[k]), k                       # the clean field of the source model, the grid included
    assert all(torch.equal(now[k], v) for k, v in before.items())      # nothing of the signature reached the network


def test_release_and_render_refusals(signed):
    from nerf_signature_amd.release import release
    message = torch.tensor([1., 1.])
    with pytest.raises(NotImplementedError, match=r"release under K messages \[K, D\]: a released model carries ONE signature"):
        release(signed, torch.ones(3, 2))
    with pytest.raises(ValueError, match="message has 3 bits"):
        release(signed, torch.ones(3))
    with pytest.raises(ValueError, match="release needs a message"):
        release(signed, None)
    signed.cuda_ray = False
    try:
        with pytest.raises(NotImplementedError, match=r"uniform-sample `run` path \(cuda_ray=False\)"):
            release(signed, message)
    finally:
        signed.cuda_ray = True
    signed.codebook_shard = (0, 1)
    try:
        with pytest.raises(NotImplementedError, match="release under data-parallel table sharding"):
            release(signed, message)
    finally:
        signed.codebook_shard = None
    rel = release(signed, message)
    o, d = torch.zeros(1, 4, 3), torch.ones(1, 4, 3)
    with pytest.raises(RuntimeError, match="inference only"):
        rel.render(o, d)
    with torch.no_grad():
        with pytest.raises(NotImplementedError, match="clean_twin on a released model"):
            rel.render(o, d, clean_twin=True)
        with pytest.raises(TypeError, match="takes no message"):
            rel.render(o, d, message=message)
        with pytest.raises(TypeError, match="takes no message"):
            rel.render(o, d, message)
        with pytest.raises(NotImplementedError, match="uniform-sample `run` path"):
            rel.run(o, d, None)
    rel._packed_cache = ("key", "image")
    rel._premarched = object()
    rel._marched = {1: object()}
    rel.invalidate()
    assert rel._packed_cache is None and rel._premarched is None and rel.marched_records() == []
