"""Packed released model on the device (include/nerfsig.h "packed released model").  Everything here is an EQUALITY against kernels
that are tested elsewhere: the packed tables decode to what tm_apply leaves in fp32 tables, so codes, plane sets, MLP outputs, images and verdicts are compared
bit for bit (whole buffers as bytes, floats as int32 words) with the existing fp32 path over the tm_apply-rounded tables.  No tolerance anywhere."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from packed_ref import half_table, tables  # noqa: E402

pytestmark = pytest.mark.gpu

FORMATS = ("f16", "q8", "q4")
TAMPER = {"f16": ("half", 0), "q8": ("quantize", 8), "q4": ("quantize", 4)}
BOUND = 1.0
FILL = 0xA5


def _words(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    """Bit equality of float tensors (NaN-safe)."""
    return a.shape == b.shape and torch.equal(_words(a), _words(b))


def _rounded(tabs, fmt):
    """The fp32 tables tm_apply leaves for the format's tampering kind (fresh tensors)."""
    from nerf_signature_amd import tamper
    kind, bits = TAMPER[fmt]
    out = [torch.empty_like(t) for t in tabs]
    tamper.apply(tabs, out, kind, bits=bits, stats=tamper.stats(tabs) if kind == "quantize" else None)
    return out


@pytest.fixture(scope="module")
def f16_mlp():
    """The module runs under the default (fp16) MLP, whatever ran before it; the two-precision test switches by itself (mlp_prec)."""
    from nerf_signature_amd import _native as nv
    before = nv.fn("mlp_get_precision")()
    nv.call("mlp_set_precision", 1)
    yield
    nv.call("mlp_set_precision", before)


@pytest.fixture(scope="module")
def hard_tables():
    """17 device tables: hash-table-like uniform values, with the CPU tests' hard tables among them (ties at 8 and at 4 bits, all +0.0, extremes in the first
    and last row) -- on a fine level, a coarse level and as the signature."""
    rng = np.random.RandomState(31)
    host = [rng.uniform(-1e-4, 1e-4, (1 << 19, 2)).astype(np.float32) for _ in range(17)]
    t8, t4 = tables(8), tables(4)
    host[0], host[3], host[9], host[12], host[15], host[16] = t8[3], t8[1], t8[2], t4[3], t4[3] * np.float32(1e-5), t8[2] * np.float32(0.5)
    return [torch.from_numpy(h).cuda() for h in host]


@pytest.fixture(scope="module")
def packed_sets(hard_tables, f16_mlp):
    """{format: (codes, params, rounded fp32 tables)}: packed once, the reference rounded once by tm_apply; never modified."""
    from nerf_signature_amd import fieldops as fo
    out = {}
    for fmt in FORMATS:
        codes, params, bad = fo.pack_tables(hard_tables, fmt)
        assert int(bad.item()) == 0
        out[fmt] = (codes, params, _rounded(hard_tables, fmt))
    return out


@pytest.fixture(scope="module")
def points():
    """[1025, 3]: first the edge cases -- +-bound exactly on each axis, +-1.5 bound outside, the origin, points whose finest-level cell is the last one (with
    all, two and one coordinate there) -- then uniform points of the box.  A test takes the first M; from M = 31 on every edge case is inside."""
    b = BOUND
    eye = torch.eye(3)
    last = b * (1.0 - 1e-4)      # x01 = 0.99995: cell 2046 of 2047 at the finest level, cell 2047 of the signature level
    special = torch.cat([b * eye, -b * eye, 1.5 * b * eye, -1.5 * b * eye, torch.zeros(1, 3), torch.tensor([[last, last, last], [last, last, 0.1], [last, -0.3, 0.2], [b, b, b],
                                                                                                             [-b, -b, -b], [1.5 * b, -1.5 * b, 0.0]])])
    gen = torch.Generator().manual_seed(5)
    rest = (torch.rand(1025 - special.shape[0], 3, generator=gen) * 2 - 1) * b
    return torch.cat([special, rest]).float().cuda().contiguous()


# ---------------------------------------------------------------------------------------------------- 1. pack

@pytest.mark.parametrize("fmt", FORMATS)
def test_pack_equals_the_cpu_pack_and_unpack_equals_tm_apply(fmt, hard_tables, f16_mlp):
    from nerf_signature_amd import fieldops as fo
    tabs = hard_tables[:6] + [torch.from_numpy(half_table()).cuda()]      # (ties 8, uniform, uniform, zeros, uniform, uniform, f16's hard values)
    tabs[4], tabs[5] = hard_tables[9], hard_tables[12]                     # (extremes at the ends, ties 4)
    codes, params, bad = fo.pack_tables(tabs, fmt)
    want_codes, want_params, want_bad = fo.pack_tables_cpu([t.cpu() for t in tabs], fmt)
    assert int(bad.item()) == want_bad == 0
    assert params.dtype == torch.float32 and tuple(params.shape) == (len(tabs), 2) and _same(params.cpu(), want_params)
    for i, (c, w) in enumerate(zip(codes, want_codes)):
        assert c.dtype == torch.uint8 and tuple(c.shape) == (fo.pk_table_bytes(fmt),) and torch.equal(c.cpu(), w), i
    got = fo.unpack_tables(codes, fmt, params)
    for i, (g, w) in enumerate(zip(got, _rounded(tabs, fmt))):
        assert _same(g, w), i
    # the whole list in one call is the 17-table limit's case
    all_codes, all_params, _ = fo.pack_tables(hard_tables, fmt)
    assert torch.equal(all_codes[0], codes[0]) and _same(all_params[0], params[0])


@pytest.mark.parametrize("fmt", FORMATS)
def test_a_planted_infinity_is_counted_and_pack_refuses_it(fmt, hard_tables, f16_mlp):
    from nerf_signature_amd import fieldops as fo
    from nerf_signature_amd.release import ReleasedModel, pack
    sig = hard_tables[16].clone()
    sig[123456, 1] = float("inf")
    codes, params, bad = fo.pack_tables([hard_tables[1], sig], fmt)
    assert int(bad.item()) == (0 if fmt == "f16" else 1)
    clean_codes, clean_params, _ = fo.pack_tables([hard_tables[1], hard_tables[16]], fmt)
    if fmt != "f16":      # the infinity took no part in lo / step, and every other code is unchanged
        assert _same(params, clean_params)
        row = 123456 * (2 if fmt == "q8" else 1)
        keep = torch.ones_like(codes[1], dtype=torch.bool)
        keep[row:row + 2] = False
        assert torch.equal(codes[1][keep], clean_codes[1][keep])
    torch.manual_seed(1)
    scalars = dict(bound=BOUND, density_scale=1, min_near=0.2, density_thresh=10, bg_radius=-1)
    model = ReleasedModel(hard_tables[:16], sig, torch.randn(3072, device="cuda") * 0.1, torch.randn(7168, device="cuda") * 0.1, scalars).cuda()
    if fmt == "f16":
        assert torch.isinf(pack(model, fmt).unpack().signature.weight[123456, 1])
    else:
        with pytest.raises(ValueError, match=f"1 table value\\(s\\) are not finite and have no {fmt} code"):
            pack(model, fmt)


# ---------------------------------------------------------------------------------------------------- 2. planes, 3. rows

def _planes_pair(fmt, layout, signature, M, pts, packed_sets, rows=None):
    """(packed encoder's buffer, fp32 encoder's buffer over the rounded tables), both prefilled with FILL."""
    from nerf_signature_amd import _native as nv, fieldops as fo
    codes, params, rounded = packed_sets[fmt]
    n = int(nv.fn("hg_planes_bytes")(M))
    got, want = torch.full((n,), FILL, dtype=torch.uint8, device="cuda"), torch.full((n,), FILL, dtype=torch.uint8, device="cuda")
    rows_dev = None if rows is None else torch.tensor([rows], dtype=torch.int32, device="cuda")
    ptrs = fo.packed_ptrs(codes[:16], codes[16] if signature else None, fmt)
    nv.call("hg_encode_planes_packed", nv.ptr(pts), M, nv.ptr(rows_dev), BOUND, ptrs, fo.PACK_FORMATS[fmt], nv.ptr(params), nv.ptr(got), layout, nv.stream())
    base, S = nv.ptr_array(rounded[:16]), (rounded[16] if signature else None)
    if layout == fo.PLANES_MIXED:
        nv.call("hg_encode_planes_mixed", nv.ptr(pts), M, nv.ptr(rows_dev), BOUND, base, nv.ptr(S), nv.ptr(want), nv.stream())
    elif rows is not None:
        nv.call("hg_encode_planes_rows", nv.ptr(pts), M, nv.ptr(rows_dev), BOUND, base, nv.ptr(S), nv.ptr(want), nv.stream())
    else:
        nv.call("hg_encode_planes", nv.ptr(pts), M, BOUND, base, nv.ptr(S), nv.ptr(want), nv.stream())
    return got, want


@pytest.mark.parametrize("M", (1, 31, 32, 33, 255, 256, 257, 1025))
@pytest.mark.parametrize("signature", (True, False), ids=("signature", "no-signature"))
@pytest.mark.parametrize("layout", (0, 1), ids=("f32", "mixed"))
@pytest.mark.parametrize("fmt", FORMATS)
def test_packed_planes_are_the_fp32_encoders_bytes(fmt, layout, signature, M, points, packed_sets):
    pts = points[:M].contiguous()
    got, want = _planes_pair(fmt, layout, signature, M, pts, packed_sets)
    assert torch.equal(got, want)
    assert bool((want != FILL).any())                                         # (something was written at all)
    if not signature and layout == 0:                                         # plane 16 of an fp32 set without a signature is never touched
        stride = (M + 31) // 32 * 32
        assert bool((got[16 * stride * 8:] == FILL).all())


@pytest.mark.parametrize("rows", (0, 1, 33, 1056))
@pytest.mark.parametrize("layout", (0, 1), ids=("f32", "mixed"))
@pytest.mark.parametrize("fmt", FORMATS)
def test_packed_planes_under_a_device_row_count(fmt, layout, rows, points, packed_sets):
    capacity = 1056
    pts = torch.cat([points, points[:capacity - points.shape[0]]]).contiguous()
    got, want = _planes_pair(fmt, layout, True, capacity, pts, packed_sets, rows=rows)
    assert torch.equal(got, want)
    assert bool((want == FILL).all()) == (rows == 0)                          # a count of zero writes nothing


# ---------------------------------------------------------------------------------------------------- 4. the MLP over a finished plane set

@pytest.mark.parametrize("with_codebook", (True, False), ids=("codebook", "clean"))
def test_field_fwd_planes_equals_field_fwd_over_the_same_set(mlp_prec, with_codebook, points, hard_tables):
    from nerf_signature_amd import _native as nv, fieldops as fo
    M = points.shape[0]
    torch.manual_seed(2)
    weights = fo.pack_weights(torch.randn(3072, device="cuda") * 0.2, torch.randn(7168, device="cuda") * 0.2)
    dirs = torch.nn.functional.normalize(torch.randn(M, 3, device="cuda"), dim=-1).contiguous()
    tabs = [t * 1000 for t in hard_tables[1:3]] * 8 + [hard_tables[2] * 500]      # (features of a size the MLP responds to)
    base, S = nv.ptr_array(tabs[:16]), (tabs[16] if with_codebook else None)
    layouts = (fo.PLANES_F32, fo.PLANES_MIXED) if mlp_prec == "f16" else (fo.PLANES_F32,)      # (F32 planes under split-bf16: it refuses the mixed set)
    f32 = dict(dtype=torch.float32, device="cuda")
    for layout in layouts:
        ws = torch.empty(int(nv.fn("hg_planes_bytes")(M)), dtype=torch.uint8, device="cuda")
        if layout == fo.PLANES_MIXED:
            nv.call("hg_encode_planes_mixed", nv.ptr(points), M, None, BOUND, base, nv.ptr(S), nv.ptr(ws), nv.stream())
        else:
            nv.call("hg_encode_planes", nv.ptr(points), M, BOUND, base, nv.ptr(S), nv.ptr(ws), nv.stream())
        for geo in (False, True):      # (without geo features: the pipelined launch under fp16; with them: the plain loop)
            want = [torch.full((M,), -7.0, **f32), torch.full((M, 3), -7.0, **f32), torch.full((M, 15), -7.0, **f32) if geo else None]
            got = [torch.full_like(w, -7.0) if w is not None else None for w in want]
            nv.call("field_fwd", nv.ptr(points), nv.ptr(dirs), M, BOUND, base, nv.ptr(S), nv.ptr(weights), nv.ptr(want[0]), nv.ptr(want[1]), nv.ptr(want[2]), None,
                    nv.ptr(ws), layout, nv.stream())
            nv.call("field_fwd_planes", nv.ptr(dirs), M, None, nv.ptr(weights), nv.ptr(ws), layout, int(with_codebook), nv.ptr(got[0]), nv.ptr(got[1]), nv.ptr(got[2]),
                    nv.stream())
            for g, w in zip(got, want):
                assert w is None or (_same(g, w) and not bool((w == -7.0).any()))
            sig, rgb, _ = fo.field_planes(dirs, M, weights, ws, layout, with_codebook, want_rgb=geo)      # (the Python helper; density only when geo is False)
            assert _same(sig, want[0]) and (rgb is None or _same(rgb, want[1]))
        # a device row count: the first 33 rows, the rest untouched
        rows_dev = torch.tensor([33], dtype=torch.int32, device="cuda")
        want, got = [torch.full((M,), -7.0, **f32), torch.full((M, 3), -7.0, **f32)], [torch.full((M,), -7.0, **f32), torch.full((M, 3), -7.0, **f32)]
        nv.call("field_fwd_rows", nv.ptr(points), nv.ptr(dirs), M, nv.ptr(rows_dev), BOUND, base, nv.ptr(S), nv.ptr(weights), nv.ptr(want[0]), nv.ptr(want[1]), nv.ptr(ws),
                layout, nv.stream())
        nv.call("field_fwd_planes", nv.ptr(dirs), M, nv.ptr(rows_dev), nv.ptr(weights), nv.ptr(ws), layout, int(with_codebook), nv.ptr(got[0]), nv.ptr(got[1]), None, nv.stream())
        assert _same(got[0], want[0]) and _same(got[1], want[1]) and bool((got[0][33:] == -7.0).all()) and not bool((got[0][:33] == -7.0).any())


# ---------------------------------------------------------------------------------------------------- 5. the model

@pytest.fixture(scope="module")
def trained(f16_mlp):
    from nerf_signature_amd import quality, rays
    stage = quality.watermark_stage()
    quality.train(stage, mode="graphed", log_every=0)
    message = quality.messages(stage["D"], 1)[0].to(stage["device"])
    r = rays.get_rays(stage["test_poses"][:1], stage["intr"], stage["H"], stage["W"], -1)
    return stage, message, (r["rays_o"], r["rays_d"])


def _block_kw(stage):
    return dict(staged=False, bg_color=1, perturb=False, force_all_rays=True, **stage["render_kwargs"])


def _full_kw(stage):
    return dict(staged=True, bg_color=1, perturb=False, force_all_rays=True, **stage["render_kwargs"])


def _same_render(a, b, weights=True):
    return torch.equal(a["image"], b["image"]) and _same(a["depth"], b["depth"]) and (not weights or torch.equal(a["weights_sum"], b["weights_sum"]))


@pytest.mark.parametrize("fmt", FORMATS)
def test_packed_model_renders_the_bits_of_the_tampered_fp32_release(fmt, trained, tmp_path):
    from nerf_signature_amd.release import PackedReleasedModel, SignatureKey, pack, release, verify
    from nerf_signature_amd.tamper import Tamper
    stage, message, (fo_, fd_) = trained
    model, bo, bd = stage["model"], stage["block_o"], stage["block_d"]
    key = SignatureKey.from_block_rays(message, model.msg_decoder, bo, bd, stage["render_kwargs"])
    with torch.no_grad():
        packed = pack(release(model, message), fmt)
        tampered = release(model, message, copy=True)
        Tamper([*tampered.encoder.tables(), tampered.signature.weight], on_write=tampered.invalidate).apply(*TAMPER[fmt])
        pristine = release(model, message).render(bo, bd, **_block_kw(stage))
        want_block, want_full = tampered.render(bo, bd, **_block_kw(stage)), tampered.render(fo_, fd_, **_full_kw(stage))
        assert not torch.equal(want_block["image"], pristine["image"])      # (the coarse storage is visible in the bits at all)
        back = PackedReleasedModel.load(packed.save(str(tmp_path / f"{fmt}.pth")), device=stage["device"])
        assert back.format == fmt and not back.density_grid.any()
        for name, m in (("packed", packed), ("unpacked", packed.unpack()), ("loaded", back)):
            assert _same_render(m.render(bo, bd, **_block_kw(stage)), want_block), name                    # block rays, unstaged
            assert _same_render(m.render(fo_, fd_, **_full_kw(stage)), want_full, weights=False), name     # one full view, staged
        tampered.eval(), packed.eval(), back.eval()
        try:
            want = tampered.render(bo, bd, **_block_kw(stage))
            assert _same_render(packed.render(bo, bd, **_block_kw(stage)), want, weights=False)
            assert _same_render(back.render(bo, bd, **_block_kw(stage)), want, weights=False)
        finally:
            tampered.train(), packed.train(), back.train()
        v = verify(packed, key)
        print(f"{fmt}: matches {v['matches']} of {stage['D']}, p = {v['p_value']:.3e}")
        assert v == verify(tampered, key) == verify(back, key)
    with pytest.raises(RuntimeError, match="inference only"):
        packed.render(bo, bd, **_block_kw(stage))


def test_packed_report_has_one_record_per_format(trained):
    from nerf_signature_amd import quality
    stage, message, _ = trained
    out = quality.packed_report(stage, message, repeats=1)
    assert list(out) == ["fp32", "f16", "q8", "q4"]
    for name, rec in out.items():
        print(name, rec)
        assert set(rec) == {"bytes", "verify", "psnr", "render_ms", "render_ms_all"} and rec["render_ms"] > 0 and len(rec["render_ms_all"]) == 1
        assert set(rec["verify"]) == {"bits", "matches", "bit_accuracy", "p_value"}
    assert out["fp32"]["psnr"] == float("inf")
    table = 1 << 22
    for name, per in (("f16", table // 2), ("q8", table // 4), ("q4", table // 8)):
        assert out["fp32"]["bytes"] - out[name]["bytes"] >= 17 * (table - per)
