"""One set of points under K messages in a single field pass, on the GPU: every new launch and every layer above it against the single-message path it stands for,
bit for bit -- hg_codebook_presum_multi against hg_codebook_presum_sel, the K-plane gather against hg_encode_codebook_plane, field_fwd_multi against field_fwd over
planes, render with a [K, D] message against K renders, quality.test_bitacc(message_batch=16) against its loop.  No tolerance anywhere."""
import numpy as np
import pytest
import torch

import closed_form as cf
import mlp_ref as mr
from oracle import field_ref as fr
from test_gpu_render import _data, _model

pytestmark = pytest.mark.gpu

KW = dict(dt_gamma=0, max_steps=1024)
RENDER = dict(staged=False, bg_color=1, perturb=False, force_all_rays=True, **KW)
COUNTS = (1, 31, 32, 33, 127, 128, 129, 1025)
PLANE_COUNTS = (1, 31, 32, 33, 127, 128, 129, 255, 256, 257, 1025)
SETTINGS = [("f16", "1"), ("f16", "0"), ("bf16x3", "1")]      # (MLP arithmetic, NERFSIG_HALF_PLANES) -> fp16 + mixed, fp16 + fp32 planes, split bf16 + fp32 planes
RAY_COUNTS = (1, 63, 64, 65, 257)
T = 1 << 19


def _message_rows(K, D, seed=0):
    """[K, D] of 0. / 1.: all-zero, all-one, a random row and its copy, then random rows."""
    rng = np.random.RandomState(900 + seed + D)
    rows = [np.zeros(D), np.ones(D), rng.randint(0, 2, D)]
    rows.append(rows[2].copy())
    while len(rows) < K:
        rows.append(rng.randint(0, 2, D))
    return torch.from_numpy(np.stack(rows[:K]).astype(np.float32))


@pytest.fixture(scope="module")
def fo():
    from nerf_signature_amd import fieldops
    return fieldops


@pytest.fixture(scope="module")
def field(fo):
    """Tables, weights, the walking-count points, 16 messages of 32 bits with their single pre-sums and their multi pre-sum: computed once, never modified."""
    base = [torch.from_numpy(cf.table(l)).cuda() for l in range(16)]
    cb = [torch.from_numpy(cf.table(100 + l, scale=0.05)).cuda() for l in range(64)]
    cb128 = cb + [(cb[l].roll(l + 1, 0) * -1.5).contiguous() for l in range(64)]      # tables 64..127 (D up to 64): other values, made on the device
    sp, cp = torch.from_numpy(cf.mlp_params(3072, 1337)).cuda(), torch.from_numpy(cf.mlp_params(7168, 1338)).cuda()
    n = mr.walking_count(torch.cuda.get_device_properties(0).multi_processor_count)
    pts, dirs, _, _ = (t.cuda() for t in mr.case(n))
    edge = torch.from_numpy(cf.points(256)).cuda() * 2 - 1        # exact 0 and 1 and cell boundaries (golden G1's points), mapped to [-1, 1] exactly
    pts = torch.cat([edge, pts[256:]]).contiguous()
    msgs = _message_rows(16, 32).cuda()
    S_single = [fo.codebook_presum_sel(cb, msgs[k].contiguous()) for k in range(16)]
    assert not torch.equal(S_single[0], S_single[1]) and torch.equal(S_single[2], S_single[3])
    return {"base": base, "cb": cb, "cb128": cb128, "sp": sp, "cp": cp, "n": n, "pts": pts, "dirs": dirs, "msgs": msgs, "S": S_single}


@pytest.mark.parametrize("D", [5, 8, 13, 32, 48, 64])
def test_presum_multi_is_the_single_presum_per_message(fo, field, D):
    """Both sides of the single pass's unroll by 8, a remainder and the largest D; K on both sides of every accumulator count, odd (8-byte stores) and even."""
    tables = field["cb128"][:2 * D]
    for K in (1, 2, 3, 15, 16):
        msgs = _message_rows(K, D, seed=K).cuda()
        buf = torch.full((16 * T * 2 + 8,), float("nan"), device="cuda")
        S = fo.codebook_presum_multi(tables, msgs, out=buf)
        assert S.shape == (T, K, 2) and S.data_ptr() == buf.data_ptr()
        for k in range(K):
            single = fo.codebook_presum_sel(tables, msgs[k].contiguous())
            assert torch.equal(S[:, k], single), (D, K, k)
        assert torch.isnan(buf[K * T * 2:]).all(), (D, K, "wrote past K pre-sums")
    fresh = fo.codebook_presum_multi(tables, msgs)
    assert torch.equal(fresh, S)


def _plane16(nv, pts, M, S):
    """Plane 16 of a plane set of M points as hg_encode_codebook_plane writes it from S ([stride, 2])."""
    stride = (M + 31) // 32 * 32
    ws = torch.zeros(int(nv.fn("hg_planes_bytes")(M)), dtype=torch.uint8, device="cuda")
    nv.call("hg_encode_codebook_plane", nv.ptr(pts), M, 1.0, nv.ptr(S), nv.ptr(ws), 0, None, nv.stream())
    return ws.view(torch.float32).view(17, stride, 2)[16]


def test_codebook_planes_multi_are_plane_16_per_message(fo, field):
    from nerf_signature_amd import _native as nv
    for K in (1, 2, 3, 16):
        S = fo.codebook_presum_multi(field["cb"], field["msgs"][:K].contiguous())
        for M in PLANE_COUNTS + ((field["n"],) if K == 3 else ()):
            pts = field["pts"][:M].contiguous()
            stride = (M + 31) // 32 * 32
            assert int(nv.fn("hg_multi_planes_bytes")(M, K)) == K * stride * 8
            cplanes = torch.full((K * stride * 2 + 16,), float("nan"), device="cuda")
            nv.call("hg_encode_codebook_planes_multi", nv.ptr(pts), M, 1.0, nv.ptr(S), K, nv.ptr(cplanes), nv.stream())
            assert torch.isnan(cplanes[K * stride * 2:]).all(), (K, M, "wrote past K planes")
            planes = cplanes[:K * stride * 2].view(K, stride, 2)
            for k in range(K):
                assert torch.equal(planes[k, :M], _plane16(nv, pts, M, field["S"][k])[:M]), (K, M, k)      # rows [M, stride) are never compared
    assert float(planes.abs().max()) > 0


@pytest.mark.parametrize("pipelined", [2, 3], ids=["plain_loop", "pipelined"])
@pytest.mark.parametrize("arith,half", SETTINGS, ids=["f16_mixed", "f16_f32planes", "bf16x3_f32planes"])
def test_field_fwd_multi_slices_are_the_single_launches(fo, field, arith, half, pipelined, monkeypatch):
    """field_fwd_multi at every row count where a tile, a workgroup or a wave's walk ends: slice k of sigma and rgb is field_fwd's with S_k over a plane set encoded
    with S_k, whichever loop the single launch takes; the same through the kept planes of a FixedPoints, which are left byte for byte as they were."""
    from nerf_signature_amd import _native as nv
    monkeypatch.setenv("NERFSIG_HALF_PLANES", half)
    prec, pipe = nv.fn("mlp_get_precision")(), nv.fn("mlp_get_pipelined")()
    nv.set_mlp_precision(arith)
    nv.call("mlp_set_pipelined", pipelined)
    try:
        assert fo.mixed_planes() == (arith == "f16" and half == "1")
        packed = fo.pack_weights(field["sp"], field["cp"])
        S_multi = {K: fo.codebook_presum_multi(field["cb"], field["msgs"][:K].contiguous()) for K in (1, 2, 3, 16)}
        for M in COUNTS + (field["n"],):
            pts, dirs = field["pts"][:M].contiguous(), field["dirs"][:M].contiguous()
            single = {}
            for K in ((3,) if M == field["n"] else (1, 2, 16)):
                s, c = fo.field_forward_multi(pts, dirs, 1.0, field["base"], S_multi[K], K, packed)
                assert s.shape == (K, M) and c.shape == (K, M, 3)
                assert not torch.isnan(s).any() and not torch.isnan(c).any(), (M, K)
                for k in range(K):
                    if k not in single:
                        single[k] = fo.field_forward(pts, dirs, 1.0, field["base"], field["S"][k], packed, planes=True)[:2]
                    assert torch.equal(s[k], single[k][0]) and torch.equal(c[k], single[k][1]), (M, K, k)
                assert K == 1 or M < 32 or not torch.equal(s[0], s[1]), (M, K, "two messages gave one field: the case proves nothing")
            if M in (33, 1025):
                fixed = fo.FixedPoints(pts, 1.0, field["base"])
                nv.call("hg_encode_codebook_plane", nv.ptr(pts), M, 1.0, nv.ptr(field["S"][1]), nv.ptr(fixed.planes), fixed.layout, None, nv.stream())      # a plane 16 to find again
                kept, plan = fixed.planes.clone(), fixed.plan.buf.clone()
                sf, cf_ = fo.field_forward_multi(pts, dirs, 1.0, field["base"], S_multi[16], 16, packed, fixed=fixed)
                assert torch.equal(sf, s) and torch.equal(cf_, c), M
                assert torch.equal(fixed.planes, kept) and torch.equal(fixed.plan.buf, plan), (M, "the kept plane set or its scatter plan was written")
                assert fixed.refreshes == 1
    finally:
        nv.call("mlp_set_pipelined", pipe)
        nv.call("mlp_set_precision", prec)


def _equal_render(out, k, single, N):
    assert torch.equal(out["image"][k], single["image"]), (N, k)
    assert torch.equal(out["depth"][k].nan_to_num(nan=-1.0), single["depth"].nan_to_num(nan=-1.0)), (N, k)      # (a ray that misses the box has depth NaN, as in the reference)
    if "weights_sum" in single:
        assert torch.equal(out["weights_sum"][k], single["weights_sum"]), (N, k)


def test_render_under_k_messages_is_k_renders(mlp_prec):
    """render(o, d, messages [K, D]) under no_grad: image / depth / weights_sum [k] are render(o, d, messages[k])'s; the march's side effects are ONE render's; the
    single-message pre-sum cache survives; the same for rays declared constant (fix_rays)."""
    m, _, _ = _model()
    _, _, co, cd, _ = _data(n_content=max(RAY_COUNTS))
    msgs = _message_rows(17, 32)
    with torch.no_grad():
        for N in RAY_COUNTS:
            o, d = co[:, :N].contiguous().cuda(), cd[:, :N].contiguous().cuda()
            singles = [m.render(o, d, msgs[k], **RENDER) for k in range(17)]
            before = m.render(o, d, msgs[5], **RENDER)
            cache = m._presum_cache
            for K in (1, 3, 17):
                step, ring = m.local_step, m.step_counter.clone()
                out = m.render(o, d, msgs[:K] if K != 3 else msgs[:K].cuda(), **RENDER)          # host and device messages
                assert set(out) == {"image", "depth", "weights_sum"}
                assert out["image"].shape == (K, 1, N, 3) and out["depth"].shape == (K, 1, N) and out["weights_sum"].shape == (K, N)
                assert m.local_step == step + 1, "the march ran more than once"
                row = step % 16
                assert torch.equal(m.step_counter[row], ring[(step - 1) % 16])          # the same rays as the render before: the same totals
                others = [r for r in range(16) if r != row]
                assert torch.equal(m.step_counter[others], ring[others])
                for k in range(K):
                    _equal_render(out, k, singles[k], N)
            assert N < 64 or not torch.equal(out["image"][0], out["image"][1])
            assert m._presum_cache is cache, "the single-message pre-sum cache was replaced"
            after = m.render(o, d, msgs[5], **RENDER)
            assert m._presum_cache is cache, "the cached pre-sum was not found again"
            _equal_render({k: v[None] for k, v in after.items()}, 0, before, N)
        # rays declared constant: the kept base planes, one march long ago
        rec = m.fix_rays(o, d, **KW)
        singles = [m.render(o, d, msgs[k], **RENDER) for k in range(17)]
        kept, step = rec.fixed.planes.clone(), m.local_step
        for K in (3, 17):
            out = m.render(o, d, msgs[:K], **RENDER)
            for k in range(K):
                _equal_render(out, k, singles[k], "fixed")
        assert m.local_step == step and torch.equal(rec.fixed.planes, kept) and m.get_marched(o.view(-1, 3), d.view(-1, 3)) is rec


@pytest.mark.parametrize("fused", ["1", "0"], ids=["fused_superchunk", "chunk_loop"])
def test_staged_render_under_k_messages(fused, monkeypatch):
    """render(staged=True) of a 70 x 70 view in chunks of 1024 rays, on the fused super-chunk route and the plain chunk loop: [K, B, N(, 3)] results, each the staged
    render of its message; local_step and the step_counter ring as after ONE staged render."""
    monkeypatch.setenv("NERFSIG_STAGED_FUSED", fused)
    m, _, _ = _model()
    pose, intr, _ = cf.orbit_rays(8)
    full_o, full_d = fr.get_rays(torch.from_numpy(pose)[None], intr, 400, 400)
    crop = lambda t: t.view(400, 400, 3)[165:235, 165:235].reshape(1, 4900, 3).contiguous().cuda()
    o, d = crop(full_o), crop(full_d)
    msgs = _message_rows(17, 32).cuda()
    kw = dict(RENDER, staged=True, max_ray_batch=1024)
    with torch.no_grad():
        singles = [m.render(o, d, msgs[k], **kw) for k in range(17)]
        m.local_step = 0
        m.step_counter.zero_()
        m.render(o, d, msgs[0], **kw)
        step, ring = m.local_step, m.step_counter.clone()
        assert step == 5
        for K in (3, 17):
            m.local_step = 0
            m.step_counter.zero_()
            out = m.render(o, d, msgs[:K], **kw)
            assert set(out) == {"image", "depth"} and out["image"].shape == (K, 1, 4900, 3) and out["depth"].shape == (K, 1, 4900)
            assert m.local_step == step and torch.equal(m.step_counter, ring)
            for k in range(K):
                _equal_render(out, k, singles[k], 4900)
        assert not torch.equal(out["image"][0], out["image"][1])


def test_render_refuses_what_it_does_not_do(monkeypatch):
    from nerf_signature_amd import network
    m, _, _ = _model()
    _, _, co, cd, _ = _data(n_content=64)
    o, d = co.cuda(), cd.cuda()
    msgs = _message_rows(3, 32)
    with pytest.raises(RuntimeError, match=r"inference only .*torch\.no_grad\(\)"):
        m.render(o, d, msgs, **RENDER)
    with torch.no_grad():
        with pytest.raises(ValueError, match="message_dim=32"):
            m.render(o, d, _message_rows(3, 31), **RENDER)
        with pytest.raises(NotImplementedError, match="clean_twin together with K messages"):
            m.render(o, d, msgs, clean_twin=True, **RENDER)
        with pytest.raises(NotImplementedError, match="clean_twin together with K messages"):
            m.render(o, d, msgs, clean_twin=True, **dict(RENDER, staged=True))
        with monkeypatch.context() as mp:
            mp.setattr(network, "_data_parallel", lambda: True)
            with pytest.raises(NotImplementedError, match="data-parallel table sharding"):
                m.render(o, d, msgs, **RENDER)
        m.cuda_ray = False
        with pytest.raises(NotImplementedError, match="uniform-sample `run` path"):
            m.render(o, d, msgs, **RENDER)
        m.cuda_ray = True
        out = m.render(o, d, msgs, **RENDER)
        assert out["image"].shape == (3, 1, 64, 3)
        m.eval()
        with pytest.raises(NotImplementedError, match="terminates rays per field"):
            m.render(o, d, msgs, **RENDER)


@pytest.mark.parametrize("distortion", ["none", "noise"])
def test_bitacc_in_batches_returns_the_loop_s_numbers(distortion):
    """quality.test_bitacc over 20 messages, 16 at a time (a full launch and a partial one), against its one-render-per-message loop: the same three numbers -- with a
    distortion layer too, whose per-call draws keep their order; and eval_blocks_multi's rendered blocks and decoder outputs, message by message, torch.equal to eval_step's."""
    from nerf_signature_amd import quality, trainer
    torch.manual_seed(3)
    m, _, _ = _model()
    bo, bd, co, cd, gt = _data(n_content=256)
    data = {"watermark": {"rays_o_block": bo.cuda(), "rays_d_block": bd.cuda()}, "content": {"rays_o": co.cuda(), "rays_d": cd.cuda(), "images": gt.cuda()}}
    opt = torch.optim.Adam(m.get_params(1e-2))
    for i, msg in enumerate(_message_rows(12, 32, seed=7)):      # a dozen steps: a decoder and a codebook that are not their initial values
        opt.zero_grad()
        trainer.train_step(m, data, msg.cuda(), dict(KW))[-1].backward()
        opt.step()
    stage = {"model": m, "D": 32, "device": torch.device("cuda"), "block_o": data["watermark"]["rays_o_block"], "block_d": data["watermark"]["rays_d_block"],
             "render_kwargs": dict(KW)}
    state = {k: v.clone() for k, v in m.msg_decoder.state_dict().items()}
    loop = quality.test_bitacc(stage, n_messages=20, distortion=distortion)
    m.msg_decoder.load_state_dict(state)
    batched = quality.test_bitacc(stage, n_messages=20, distortion=distortion, message_batch=16)
    print(f"\ntest_bitacc {distortion}: loop {loop}, batched {batched}")
    assert batched == loop
    # message by message: what the decoder returns (its BatchNorm over ONE message's D blocks) and what it was shown (the layer's draws in message order)
    from nerf_signature_amd.distortion import DistortionLayer
    wm, msgs = data["watermark"], _message_rows(5, 32, seed=11).cuda()
    layer = lambda: None if distortion == "none" else DistortionLayer(distortion, 4321)
    with torch.no_grad():
        m.msg_decoder.load_state_dict(state)
        draws = layer()
        singles = [trainer.eval_step(m, wm, msgs[k], dict(KW), render_whole=False, distortion=draws) for k in range(5)]
        m.msg_decoder.load_state_dict(state)
        pred_rgb, decoded = trainer.eval_blocks_multi(m, wm, msgs, dict(KW), distortion=layer())
    assert pred_rgb.shape == (5, 32, 6, 6, 3) and decoded.shape == (5, 32, 1)
    for k in range(5):
        assert torch.equal(pred_rgb[k], singles[k][0]) and torch.equal(decoded[k], singles[k][3]), (distortion, k)
    assert not torch.equal(decoded[0], decoded[1])
