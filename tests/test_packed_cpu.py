"""Packed released model, everything that needs no GPU: the restatement of the three formats (tests/packed_ref.py) against the tamper restatement bit for bit,
byte and nibble order by literals, its mutants, the product's CPU pack / unpack against the restatement, the checkpoint (keys, size, round trip), the native
refusals word for word through the built library and the Python refusals."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import packed_ref as pr  # noqa: E402
import tamper_ref as tr  # noqa: E402
from packed_ref import half_table, tables  # noqa: E402

T = 1 << 19
MIB = 1 << 20
FORMATS = ("f16", "q8", "q4")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------- the restatement against tamper_ref

def test_pk_table_bytes():
    from nerf_signature_amd import _native as nv, fieldops as fo
    assert [fo.pk_table_bytes(f) for f in FORMATS] == [2 * MIB, MIB, MIB // 2] == [T * pr.ROW_BYTES[f] for f in FORMATS]
    assert [fo.pk_table_bytes(c) for c in (0, 1, 2)] == [2 * MIB, MIB, MIB // 2]
    assert nv.fn("pk_table_bytes")(3) == 0 and nv.fn("pk_table_bytes")(-1) == 0
    assert fo.PACK_FORMATS == pr.FORMATS
    with pytest.raises(ValueError, match="unknown packed format"):
        fo.pk_table_bytes("q2")


@pytest.mark.parametrize("fmt", ("q8", "q4"))
def test_quantised_round_trip_is_tamper_refs_quantize_bit_for_bit(fmt):
    bits = pr.BITS[fmt]
    arrays = tables(bits)
    want = tr.quantize(arrays, bits)
    for i, (a, w) in enumerate(zip(arrays, want)):
        b, lo, step, bad = pr.pack(a, fmt)
        assert b.dtype == np.uint8 and b.size == T * pr.ROW_BYTES[fmt] and bad == 0
        assert np.array_equal(_bits(pr.unpack(b, fmt, lo, step)), _bits(w)), i
    assert pr.pack(arrays[1], fmt)[1:3] == (0.0, 0.0) and not pr.pack(arrays[1], fmt)[0].any()       # the constant table: code 0, step 0, decodes to lo
    lo, step, _ = pr.scalars(arrays[3], bits)
    assert (lo, step) == (0.0, 1.0)                                                                    # (the tie table really has unit steps ...)
    q = pr.codes(arrays[3], bits)[0].reshape(-1)
    assert q[1] == 2 and q[2] == 2 and q[3] == 4                                                       # (... and 1.5, 2.5, 3.5 go to the even code)


def test_half_round_trip_is_tamper_refs_half_bit_for_bit():
    arrays = [tables()[0], half_table()]
    for a, w in zip(arrays, tr.half(arrays)):
        b, _, _, bad = pr.pack(a, "f16")
        assert b.size == 4 * T and bad == 0
        assert np.array_equal(_bits(pr.unpack(b, "f16")), _bits(w))
    back = pr.round_trip(half_table(), "f16").reshape(-1)
    assert np.isinf(back[8194]) and back[8193] == 65504.0 and np.isinf(back[8197]) and back[8197] < 0 and back[8201] == 0.0 and back[8202] == 2.0 ** -23


def test_byte_and_nibble_order_by_literals():
    a = np.zeros((4, 2), np.float32)
    a[0] = (3.0, 12.0)
    a[1] = (0.0, 15.0)
    b, lo, step, _ = pr.pack(a, "q4")
    assert (lo, step) == (0.0, 1.0) and b.tolist() == [0xC3, 0xF0, 0x00, 0x00]
    assert pr.unpack(np.array([0xC3], np.uint8), "q4", 0.0, 1.0).tolist() == [[3.0, 12.0]]
    a[1] = (0.0, 255.0)
    b, lo, step, _ = pr.pack(a, "q8")
    assert (lo, step) == (0.0, 1.0) and b.tolist() == [3, 12, 0, 255, 0, 0, 0, 0]
    assert pr.unpack(np.array([3, 12], np.uint8), "q8", 0.0, 1.0).tolist() == [[3.0, 12.0]]
    h = np.array([[1.0, -2.0]], np.float32)
    assert pr.pack(h, "f16")[0].tolist() == [0x00, 0x3C, 0x00, 0xC0]                                 # 0x3C00 = 1.0 in bits 0..15, 0xC000 = -2.0 above
    # a non-finite value: code 0, counted; decode of the rest unchanged
    a[2, 1] = np.inf
    b, lo, step, bad = pr.pack(a, "q8")
    assert bad == 1 and (lo, step) == (0.0, 1.0) and b.tolist() == [3, 12, 0, 255, 0, 0, 0, 0]


@pytest.mark.parametrize("fmt", ("q8", "q4"))
def test_mutants_of_the_restatement_differ_from_tamper_ref(fmt):
    bits = pr.BITS[fmt]
    arrays = [tables(bits)[0], tables(bits)[3]]
    want = tr.quantize(arrays, bits)
    same = lambda **mutant: all(np.array_equal(_bits(pr.round_trip(a, fmt, **mutant)), _bits(w)) for a, w in zip(arrays, want))
    assert same()
    assert not same(floor=True)
    assert not same(levels_plus_one=True)
    if fmt == "q4":
        assert not same(swap_nibbles=True)


# ---------------------------------------------------------------------------------------------------- the product's CPU path

@pytest.mark.parametrize("fmt", FORMATS)
def test_cpu_pack_and_unpack_equal_the_restatement(fmt):
    from nerf_signature_amd import fieldops as fo
    arrays = tables(pr.BITS.get(fmt, 8)) + [half_table()]
    codes, params, bad = fo.pack_tables_cpu([torch.from_numpy(a) for a in arrays], fmt)
    assert bad == 0 and params.dtype == torch.float32 and tuple(params.shape) == (len(arrays), 2)
    for i, a in enumerate(arrays):
        b, lo, step, _ = pr.pack(a, fmt)
        assert codes[i].dtype == torch.uint8 and codes[i].dim() == 1 and codes[i].is_contiguous()
        assert np.array_equal(codes[i].numpy(), b), i
        assert params[i].tolist() == [float(lo), float(step)], i
    back = fo.unpack_tables_cpu(codes, fmt, params)
    for i, a in enumerate(arrays):
        assert np.array_equal(_bits(back[i].numpy()), _bits(pr.round_trip(a, fmt))), i
    bad_table = torch.from_numpy(arrays[0].copy())
    bad_table[5, 1] = float("nan")
    assert fo.pack_tables_cpu([bad_table], fmt)[2] == (0 if fmt == "f16" else 1)


# ---------------------------------------------------------------------------------------------------- the model on the CPU

@pytest.fixture(scope="module")
def released():
    from nerf_signature_amd.network import NeRFNetwork
    from nerf_signature_amd.release import release
    torch.manual_seed(0)
    model = NeRFNetwork(bound=1.0, cuda_ray=True, density_scale=1, min_near=0.2, density_thresh=10, bg_radius=-1, message_dim=2, n_views=1)
    for t in model.msg_encoder.tables():
        t.data.uniform_(-1e-2, 1e-2)
    model.density_grid.uniform_(0, 1)
    model.density_bitfield.random_(0, 256)
    return release(model, torch.tensor([1., 0.]))


PACKED_KEYS = ({f"encoder.embeddings.{i}.codes" for i in range(16)}
               | {"signature.codes", "table_params", "sigma_net.params", "color_net.params", "aabb_train", "aabb_infer", "density_bitfield", "step_counter"})


@pytest.mark.parametrize("fmt", FORMATS)
def test_cpu_pack_of_a_model_saves_small_and_loads_identical(released, fmt, tmp_path):
    from nerf_signature_amd import fieldops as fo
    from nerf_signature_amd.release import PackedReleasedModel, ReleasedModel, pack
    packed = pack(released, fmt)
    sd = packed.state_dict()
    assert set(sd) == PACKED_KEYS and packed.format == fmt
    tabs = [*released.encoder.tables(), released.signature.weight]
    for i, t in enumerate(tabs):
        b, lo, step, _ = pr.pack(t.detach().numpy(), fmt)
        c = sd[f"encoder.embeddings.{i}.codes"] if i < 16 else sd["signature.codes"]
        assert c.dtype == torch.uint8 and tuple(c.shape) == (fo.pk_table_bytes(fmt),) and np.array_equal(c.numpy(), b), i
        assert sd["table_params"][i].tolist() == [float(lo), float(step)]
    assert sd["sigma_net.params"].data_ptr() == released.sigma_net.params.data_ptr() and sd["sigma_net.params"].dtype == torch.float32      # the MLP vectors stay fp32
    # the file: smaller than the fp32 release's by at least the tables' saving (the dropped grid is the margin)
    small, big = packed.save(str(tmp_path / "packed.pth")), released.save(str(tmp_path / "released.pth"))
    assert os.path.getsize(big) - os.path.getsize(small) >= 17 * (4 * MIB - fo.pk_table_bytes(fmt))
    ckpt = torch.load(small, map_location="cpu", weights_only=False)
    assert ckpt["release"]["format"] == fmt and "density_grid" not in ckpt["model"] and set(ckpt["model"]) == PACKED_KEYS
    back = PackedReleasedModel.load(small)
    assert set(back.state_dict()) == PACKED_KEYS and back.format == fmt and back.training
    assert all(torch.equal(back.state_dict()[k], v) for k, v in sd.items())
    assert (back.mean_count, back.mean_density, back.bound) == (packed.mean_count, packed.mean_density, packed.bound)
    assert not back.density_grid.any() and tuple(back.density_grid.shape) == tuple(released.density_grid.shape)      # the constructor's zero grid
    for m in (packed, back):
        with pytest.raises(NotImplementedError, match="does not carry the fp32 density grid"):
            m.update_extra_state()
        with pytest.raises(NotImplementedError, match="does not carry the fp32 density grid"):
            m.mark_untrained_grid(None, None)
    # each loader names the other
    with pytest.raises(ValueError, match=r"PackedReleasedModel\.load"):
        ReleasedModel.load(small)
    with pytest.raises(ValueError, match=r"ReleasedModel\.load"):
        PackedReleasedModel.load(big)
    # unpack: the decoded tables, the same buffers
    plain = back.unpack()
    assert isinstance(plain, ReleasedModel) and plain.density_bitfield.data_ptr() == back.density_bitfield.data_ptr()
    for i, (t, got) in enumerate(zip(tabs, [*plain.encoder.tables(), plain.signature.weight])):
        assert np.array_equal(_bits(got.detach().numpy()), _bits(pr.round_trip(t.detach().numpy(), fmt))), i
    assert torch.equal(plain.sigma_net.params, released.sigma_net.params) and torch.equal(plain.color_net.params, released.color_net.params)


def test_python_refusals(released):
    from nerf_signature_amd.release import PackedReleasedModel, pack
    with pytest.raises(ValueError, match="unknown packed format"):
        pack(released, "q2")
    with pytest.raises(TypeError, match="pack takes a ReleasedModel"):
        pack(torch.nn.Linear(1, 1), "q8")
    packed = pack(released, "q8")
    with pytest.raises(ValueError, match="packed already"):
        pack(packed, "q4")
    o, d = torch.zeros(1, 4, 3), torch.ones(1, 4, 3)
    with pytest.raises(RuntimeError, match=r"a released model is inference only \(forward, no gradients\): call render under torch.no_grad\(\)"):
        packed.render(o, d)
    with torch.no_grad():
        with pytest.raises(NotImplementedError, match="clean_twin on a released model"):
            packed.render(o, d, clean_twin=True)
        with pytest.raises(TypeError, match="takes no message"):
            packed.render(o, d, message=torch.ones(2))
        with pytest.raises(TypeError, match="takes no message"):
            packed.render(o, d, torch.ones(2))
        with pytest.raises(NotImplementedError, match=r"K messages \[K, D\]"):
            packed.render(o, d, message=torch.ones(3, 2))
        with pytest.raises(NotImplementedError, match=r"K messages \[K, D\]"):
            packed.render(o, d, torch.ones(3, 2))
        with pytest.raises(NotImplementedError, match="uniform-sample `run` path"):
            packed.run(o, d, None)
        with pytest.raises(NotImplementedError, match="clean_twin on a released model"):
            packed(o[0], d[0], twin=True)
        with pytest.raises(NotImplementedError, match="fixed= points on a packed released model"):
            packed(o[0], d[0], fixed=object())
    with pytest.raises(NotImplementedError, match=r"unpack\(\)"):
        packed.tamper()
    # a value without a code: the q formats refuse, f16 stores it
    released.signature.weight.data[7, 0] = float("inf")
    try:
        for fmt in ("q8", "q4"):
            with pytest.raises(ValueError, match=f"1 table value\\(s\\) are not finite and have no {fmt} code"):
                pack(released, fmt)
        assert torch.isinf(pack(released, "f16").unpack().signature.weight[7, 0])
    finally:
        released.signature.weight.data[7, 0] = 0.0
    with pytest.raises(ValueError, match="expected a flat uint8 tensor"):
        PackedReleasedModel([torch.zeros(4, dtype=torch.uint8)] * 16, torch.zeros(4, dtype=torch.uint8), torch.zeros(17, 2), "q8", released.sigma_net.params,
                            released.color_net.params, {k: getattr(released, k) for k in ("bound", "density_scale", "min_near", "density_thresh", "bg_radius")})


# ---------------------------------------------------------------------------------------------------- native refusals

def _fake(n=1):
    return ctypes.c_void_p(4096 * n)      # a non-null, 16-byte aligned address nobody reads: every refusal below comes before a launch


def test_native_refusals_word_for_word():
    from nerf_signature_amd import _native as nv

    def refused(name, *args):
        with pytest.raises(ValueError) as e:
            nv.call(name, *args)
        return str(e.value).split(": ", 1)[1]

    assert nv.fn("nsig_abi_version")() == 1
    two = (ctypes.c_void_p * 2)(4096, 8192)
    hole = (ctypes.c_void_p * 2)(4096, None)
    odd = (ctypes.c_void_p * 2)(4096, 8200)
    pack = lambda src=two, n=2, fmt=1, stats=_fake(3), dst=two, params=_fake(4), bad=_fake(5): refused("pk_pack_tables", src, n, fmt, stats, dst, params, bad, None)
    unpack = lambda src=two, n=2, fmt=1, params=_fake(4), dst=two: refused("pk_unpack_tables", src, n, fmt, params, dst, None)
    for who, call in (("pk_pack_tables", pack), ("pk_unpack_tables", unpack)):
        assert call(fmt=3) == f"{who}: unknown format 3 (0 f16, 1 q8, 2 q4)"
        assert call(fmt=-1) == f"{who}: unknown format -1 (0 f16, 1 q8, 2 q4)"
        assert call(src=None) == call(dst=None) == f"{who}: null pointer"
        assert call(n=0) == f"{who}: n = 0 tables is out of range (1 .. 17)"
        assert call(n=18) == f"{who}: n = 18 tables is out of range (1 .. 17)"
        assert call(src=hole) == call(dst=hole) == call(src=odd) == call(dst=odd) == f"{who}: table 1 is null or not 16-byte aligned"
    for fmt in (1, 2):
        assert pack(fmt=fmt, stats=None) == pack(fmt=fmt, params=None) == pack(fmt=fmt, bad=None) == "pk_pack_tables: the q8 and q4 formats need stats (tm_stats'), params and nonfinite"
        assert unpack(fmt=fmt, params=None) == "pk_unpack_tables: the q8 and q4 formats need the per-table parameters (params, pk_pack_tables')"
    assert pack(params=ctypes.c_void_p(4100)) == pack(stats=ctypes.c_void_p(4100)) == pack(bad=ctypes.c_void_p(4098)) \
        == "pk_pack_tables: stats and params must be 8-byte aligned, nonfinite 4-byte aligned"
    assert unpack(params=ctypes.c_void_p(4100)) == "pk_unpack_tables: params must be 8-byte aligned"

    seventeen = (ctypes.c_void_p * 17)(*[4096 * (i + 1) for i in range(17)])
    no_signature = (ctypes.c_void_p * 17)(*[4096 * (i + 1) for i in range(16)], None)
    hole17 = (ctypes.c_void_p * 17)(*[None if i == 3 else 4096 * (i + 1) for i in range(17)])
    odd17 = (ctypes.c_void_p * 17)(*[4096 * (i + 1) + (8 if i == 16 else 0) for i in range(17)])
    enc = lambda xyzs=_fake(1), M=64, rows=None, bound=1.0, tabs=seventeen, fmt=1, params=_fake(2), planes=_fake(3), layout=0: \
        refused("hg_encode_planes_packed", xyzs, M, rows, bound, tabs, fmt, params, planes, layout, None)
    who = "hg_encode_planes_packed"
    assert enc(fmt=3) == f"{who}: unknown format 3 (0 f16, 1 q8, 2 q4)"
    assert enc(layout=2) == f"{who}: planes_layout must be NSIG_PLANES_F32 (0) or NSIG_PLANES_MIXED (1)"
    assert enc(xyzs=None) == enc(planes=None) == enc(tabs=None) == f"{who}: null pointer"
    assert enc(fmt=1, params=None) == enc(fmt=2, params=None) == f"{who}: the q8 and q4 formats need the per-table parameters (params, pk_pack_tables')"
    assert enc(bound=0.0) == enc(bound=-1.0) == f"{who}: bound must be positive"
    assert enc(planes=ctypes.c_void_p(4100)) == enc(params=ctypes.c_void_p(4100)) == f"{who}: planes and params must be 8-byte aligned"
    assert enc(tabs=hole17) == f"{who}: table 3 is null or not 16-byte aligned"
    assert enc(tabs=odd17) == f"{who}: table 16 is null or not 16-byte aligned"
    assert nv.fn(who)(_fake(1), 0, None, 1.0, no_signature, 0, None, _fake(3), 0, None) == 0          # (no signature, f16 without params, no rows: accepted; M = 0 launches nothing)

    fwd = lambda dirs=_fake(1), M=64, rows=None, packed=_fake(2), planes=_fake(3), layout=0, cb=1, sigmas=_fake(4), rgbs=_fake(5), geo=None: \
        refused("field_fwd_planes", dirs, M, rows, packed, planes, layout, cb, sigmas, rgbs, geo, None)
    who = "field_fwd_planes"
    assert fwd(packed=None) == fwd(planes=None) == fwd(sigmas=None) == f"{who}: null pointer"
    assert fwd(dirs=None) == f"{who}: dirs is required when rgbs is requested"
    assert fwd(packed=ctypes.c_void_p(4104)) == f"{who}: packed must be 16-byte aligned"
    assert fwd(planes=ctypes.c_void_p(4100)) == f"{who}: planes must be 8-byte aligned"
    assert fwd(layout=7) == f"{who}: planes_layout must be NSIG_PLANES_F32 (0) or NSIG_PLANES_MIXED (1)"

    # the mixed layout belongs to the fp16 MLP: both entry points refuse it under split-bf16
    before = nv.fn("mlp_get_precision")()
    nv.call("mlp_set_precision", 0)
    try:
        assert enc(layout=1) == "hg_encode_planes_packed: the mixed layout carries the fp16 MLP's operands (mlp_set_precision(1))"
        assert fwd(layout=1) == "field_fwd_planes: this plane set was written in the mixed (fp16) layout; the split-bf16 MLP needs an fp32 set (NSIG_PLANES_F32)"
    finally:
        nv.call("mlp_set_precision", before)
