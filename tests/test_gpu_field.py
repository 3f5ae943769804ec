"""GPU parity of the hash-grid and field-network kernels against the golden vectors / the CPU oracle,
through the C ABI.  Tolerances: hash rows bit-exact; encoder features to fp32 round-off; sigma/rgb and
gradients within the path's stated 1e-3 (north_star), measured far tighter."""
import math
import os

import numpy as np
import pytest
import torch

import closed_form as cf
import mlp_ref as mr
from oracle import field_ref as fr

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def fo():
    from nerf_signature_amd import fieldops
    return fieldops


@pytest.fixture(scope="module")
def tables():
    base = [torch.from_numpy(cf.table(l)) for l in range(16)]
    cb = [torch.from_numpy(cf.table(100 + l, scale=0.05)) for l in range(96)]
    return base, cb, [t.cuda() for t in base], [t.cuda() for t in cb]


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def test_hash_rows_bit_exact_vs_reference(fo):
    g = np.load(os.path.join(G, "g1_base_encoder.npz"))
    x = _cuda(cf.points())
    for l, res in enumerate(g["resolutions"]):
        rows, w = fo.level_lookup(x, float(res))
        np.testing.assert_array_equal(rows.cpu().numpy(), g["rows"][l])
        np.testing.assert_array_equal(w.cpu().numpy(), g["weights"][l])
    rows, _ = fo.level_lookup(x, 2048.0)
    want, _, _ = fr.voxel_lookup(torch.from_numpy(cf.points()), torch.tensor(2048.0))
    np.testing.assert_array_equal(rows.cpu().numpy(), want.numpy().astype(np.int32))


def test_base_encoder_features_vs_reference(fo, tables):
    g = np.load(os.path.join(G, "g1_base_encoder.npz"))
    feat = fo.encode(_cuda(cf.points()), tables[2])
    np.testing.assert_array_equal(feat.cpu().numpy(), g["features"])


@pytest.mark.parametrize("D", [32, 48])
def test_codebook_forward_literal_and_presummed(fo, tables, D):
    g = np.load(os.path.join(G, "g2_codebook.npz"))
    base, cb, base_d, cb_d = tables
    x = _cuda(cf.points())
    clean = fo.encode(x, base_d)
    for k, msg in enumerate(cf.messages(D)):
        sel = fo.select_tables(cb_d[:2 * D], fo.message_bits(torch.from_numpy(msg)))
        lit = fo.codebook_encode_literal(x, sel)
        np.testing.assert_allclose(lit.cpu().numpy(), g[f"out_D{D}_m{k}"], rtol=0, atol=3e-7)
        S = fo.codebook_presum(sel)
        want_S = torch.stack([t.cpu() for t in sel]).double().sum(0)
        np.testing.assert_allclose(S.cpu().numpy(), want_S.numpy(), rtol=0, atol=1e-6)  # fp32 sum of D terms of magnitude <= 0.05
        feat = fo.encode(x, base_d, S)
        np.testing.assert_array_equal(feat[:, :30].cpu().numpy(), clean[:, :30].cpu().numpy())
        np.testing.assert_allclose((feat[:, 30:] - clean[:, 30:]).cpu().numpy(), g[f"out_D{D}_m{k}"], rtol=0, atol=1e-6)


@pytest.mark.parametrize("D", [32, 48])
def test_codebook_backward_scatter_and_fanout(fo, D):
    g = np.load(os.path.join(G, "g2_codebook.npz"))
    x = _cuda(cf.points())
    Gbuf = torch.zeros(1 << 19, 2, device="cuda")
    fo.codebook_scatter(x, _cuda(g["rvec"]), Gbuf)
    nz = torch.nonzero(Gbuf.abs().sum(-1)).squeeze(-1)
    k = 2
    np.testing.assert_array_equal(nz.cpu().numpy().astype(np.int32), g[f"grad_rows_D{D}_m{k}"])
    np.testing.assert_allclose(Gbuf[nz].cpu().numpy(), g[f"grad_vals_D{D}_m{k}"], rtol=1e-5, atol=1e-7)
    grads = [torch.full((1 << 19, 2), 7.0, device="cuda") for _ in range(3)]
    fo.fanout_grad(Gbuf, grads, accumulate=False)
    assert all(torch.equal(t, Gbuf) for t in grads)
    fo.fanout_grad(Gbuf, grads, accumulate=True)
    assert all(torch.equal(t, 2 * Gbuf) for t in grads)


def _params(tables, D=32):
    base, cb, base_d, cb_d = tables
    sp, cp = torch.from_numpy(cf.mlp_params(3072, 1337)), torch.from_numpy(cf.mlp_params(7168, 1338))
    P = {"bound": 1.0, "base_tables": base, "cb_tables": [t.clone().requires_grad_(True) for t in cb[:2 * D]], "sigma_params": sp, "color_params": cp}
    return P, sp.cuda(), cp.cuda()


# measured agreement per arithmetic (max relative sigma error, max absolute rgb error): both far inside the stated 1e-3
MEASURED = {"bf16x3": (2e-4, 5e-5), "f16": (5e-4, 2.5e-4)}


@pytest.mark.parametrize("bound", [1.0, 2.0])
def test_field_forward_vs_oracle_and_reference_glue(fo, tables, bound, mlp_prec):
    base, cb, base_d, cb_d = tables
    P, sp, cp = _params(tables)
    P["bound"] = bound
    packed = fo.pack_weights(sp, cp)
    rng = np.random.RandomState(0)
    M = 4133  # not a multiple of 32
    pts = torch.from_numpy(((rng.rand(M, 3) * 2 - 1) * bound).astype(np.float32))
    dirs = torch.from_numpy(cf.unit_dirs(M, seed=5))
    msg = torch.from_numpy(cf.messages(32)[2])
    for message in (msg, None):
        with torch.no_grad():
            s0, c0 = fr.field_forward(pts, dirs, message, P)
            geo0 = fr.density(pts, message, P)["geo_feat"]
        S = fo.codebook_presum(fo.select_tables(cb_d[:64], fo.message_bits(message))) if message is not None else None
        s1, c1, geo1, _ = fo.field_forward(pts.cuda(), dirs.cuda(), bound, base_d, S, packed, want_geo=True)
        np.testing.assert_allclose(s1.cpu().numpy(), s0.numpy(), rtol=1e-3, atol=1e-6)
        np.testing.assert_allclose(c1.cpu().numpy(), c0.numpy(), rtol=0, atol=1e-3)
        np.testing.assert_allclose(geo1.cpu().numpy(), geo0.numpy(), rtol=0, atol=1e-3)
        # measured agreement is far inside the stated tolerance
        assert float((s1.cpu() / s0 - 1).abs().max()) < MEASURED[mlp_prec][0] and float((c1.cpu() - c0).abs().max()) < MEASURED[mlp_prec][1]
        # density-only and color-only entry points agree with the fused one
        s2, none_rgb, geo2, _ = fo.field_forward(pts.cuda(), None, bound, base_d, S, packed, want_rgb=False, want_geo=True)
        assert none_rgb is None and torch.equal(s2, s1) and torch.equal(geo2, geo1)
        c2 = fo.field_color(dirs.cuda(), geo1, packed)
        np.testing.assert_allclose(c2.cpu().numpy(), c1.cpu().numpy(), rtol=0, atol=1e-6)
    if bound == 1.0:  # values the reference's own NeRFNetwork.forward produced (with stand-in MLPs)
        g = np.load(os.path.join(G, "g8_g9_glue.npz"))
        S = fo.codebook_presum(fo.select_tables(cb_d[:64], fo.message_bits(torch.from_numpy(g["msg"]))))
        s1, c1, _, _ = fo.field_forward(_cuda(g["pts"]), _cuda(g["dirs"]), 1.0, base_d, S, packed)
        np.testing.assert_allclose(s1.cpu().numpy(), g["sigma_msg"], rtol=1e-3, atol=1e-6)
        np.testing.assert_allclose(c1.cpu().numpy(), g["rgb_msg"], rtol=0, atol=1e-3)
        s1, c1, _, _ = fo.field_forward(_cuda(g["pts"]), _cuda(g["dirs"]), 1.0, base_d, None, packed)
        np.testing.assert_allclose(s1.cpu().numpy(), g["sigma_clean"], rtol=1e-3, atol=1e-6)


def test_field_backward_vs_oracle_autograd(fo, tables, strict_mlp):
    base, cb, base_d, cb_d = tables
    P, sp, cp = _params(tables)
    packed = fo.pack_weights(sp, cp)
    rng = np.random.RandomState(1)
    M = 1500
    pts = torch.from_numpy((rng.rand(M, 3) * 2 - 1).astype(np.float32))
    dirs = torch.from_numpy(cf.unit_dirs(M, seed=6))
    msg = torch.from_numpy(cf.messages(32)[2])
    bits = fo.message_bits(msg)
    gs = torch.from_numpy(rng.randn(M).astype(np.float32))
    gc = torch.from_numpy(rng.randn(M, 3).astype(np.float32))
    gs[:7] = 0
    gc[:7] = 0           # rows with exactly zero upstream gradient (padding / terminated rays)
    s0, c0 = fr.field_forward(pts, dirs, msg, P)
    ((s0 * gs).sum() + (c0 * gc).sum()).backward()
    sel0 = fr_sel = [P["cb_tables"][2 * i + b] for i, b in enumerate(bits)]
    G0 = sel0[0].grad
    assert all(P["cb_tables"][2 * i + 1 - b].grad is None for i, b in enumerate(bits))

    # functional path: dfeat and the scatter
    S = fo.codebook_presum(fo.select_tables(cb_d[:64], bits))
    s1, c1, _, masks = fo.field_forward(pts.cuda(), dirs.cuda(), 1.0, base_d, S, packed, want_masks=True)
    G1 = torch.zeros(1 << 19, 2, device="cuda")
    dfeat = fo.field_backward(pts.cuda(), 1.0, gs.cuda(), gc.cuda(), s1, c1, masks, packed, G=G1, want_dfeat=True)
    assert torch.all(dfeat[:7] == 0)
    scale = float(G0.abs().max())
    np.testing.assert_allclose(G1.cpu().numpy(), G0.numpy(), rtol=1e-3, atol=1e-4 * scale)
    assert float((G1.cpu() - G0).abs().max()) < 2e-5 * scale
    # dfeat alone re-scattered through the stand-alone kernel gives the same G
    G2 = torch.zeros(1 << 19, 2, device="cuda")
    fo.codebook_scatter((pts.cuda() + 1) / 2, dfeat, G2)
    np.testing.assert_allclose(G2.cpu().numpy(), G1.cpu().numpy(), rtol=1e-4, atol=1e-6 * scale)

    # autograd path: selected tables get the gradient, unselected get None
    cb_params = [t.clone().requires_grad_(True) for t in cb_d[:64]]
    s2, c2 = fo.field_apply(pts.cuda(), dirs.cuda(), 1.0, packed, base_d, fo.select_tables(cb_params, bits))  # S computed inside
    ((s2 * gs.cuda()).sum() + (c2 * gc.cuda()).sum()).backward()
    for i, b in enumerate(bits):
        assert cb_params[2 * i + 1 - b].grad is None
        np.testing.assert_allclose(cb_params[2 * i + b].grad.cpu().numpy(), G0.numpy(), rtol=1e-3, atol=1e-4 * scale)


def _oracle_per_point(pts, dirs, msg, P, gs, gc, operands=None):
    """Oracle forward (fp32, or with the default arithmetic's fp16 operand rounding emulated: fr.round_operand) with every ReLU pre-activation
    exposed, and its per-point gradient w.r.t. the codebook feature (channels 30:32): returns (dfeat [M,2], smallest |pre-activation| of the point
    over the 192 hidden neurons)."""
    q = lambda t: fr.round_operand(t, operands)
    x01 = (pts + P["bound"]) / (2 * P["bound"])
    cbf = fr.codebook_encode(x01, msg, P["cb_tables"]).detach().requires_grad_(True)
    base = fr.base_encode(x01, P["base_tables"]).detach()
    feat = torch.cat([base[:, :-2], base[:, -2:] + cbf], dim=-1)
    ws, wc = fr.split_mlp_params(P["sigma_params"], fr.SIGMA_WIDTHS), fr.split_mlp_params(P["color_params"], fr.COLOR_WIDTHS)
    pre_s = q(feat) @ q(ws[0]).t()
    h = q(torch.relu(pre_s)) @ q(ws[1]).t()
    sigma = fr.trunc_exp(h[:, 0])
    cin = torch.cat([fr.sh4(((dirs + 1) / 2) * 2 - 1), h[:, 1:], torch.ones_like(h[:, :1])], dim=-1)
    pre_1 = q(cin) @ q(wc[0]).t()
    pre_2 = q(torch.relu(pre_1)) @ q(wc[1]).t()
    rgb = torch.sigmoid((q(torch.relu(pre_2)) @ q(wc[2]).t())[:, :3])
    ((sigma * gs).sum() + (rgb * gc).sum()).backward()
    margin = torch.cat([pre_s, pre_1, pre_2], dim=-1).detach().abs().min(dim=-1).values
    return cbf.grad, margin


def test_field_backward_away_from_relu_kinks(fo, tables, mlp_prec):
    """What limits gradient agreement with the fp32 oracle at fp16 operand precision is WHICH SIDE of a ReLU kink a pre-activation
    within rounding of zero lands on, not the arithmetic: per point, d feature[30:32] agrees to 5e-3 relative L2 over all points whose
    192 hidden pre-activations keep a margin from zero, in both arithmetics; the points inside the margin are counted."""
    base, cb, base_d, cb_d = tables
    P, sp, cp = _params(tables)
    packed = fo.pack_weights(sp, cp)
    rng = np.random.RandomState(11)
    M = 20000
    pts = torch.from_numpy((rng.rand(M, 3) * 2 - 1).astype(np.float32))
    dirs = torch.from_numpy(cf.unit_dirs(M, seed=12))
    msg = torch.from_numpy(cf.messages(32)[2])
    gs, gc = torch.from_numpy(rng.randn(M).astype(np.float32)), torch.from_numpy(rng.randn(M, 3).astype(np.float32))
    d0, margin = _oracle_per_point(pts, dirs, msg, P, gs, gc)
    S = fo.codebook_presum(fo.select_tables(cb_d[:64], fo.message_bits(msg)))
    s1, c1, _, masks = fo.field_forward(pts.cuda(), dirs.cuda(), 1.0, base_d, S, packed, want_masks=True)
    d1 = fo.field_backward(pts.cuda(), 1.0, gs.cuda(), gc.cuda(), s1, c1, masks, packed, want_dfeat=True).cpu()
    delta = {"bf16x3": 2e-5, "f16": 3e-4}[mlp_prec]           # a few times the pre-activation error of the arithmetic
    safe = margin > delta
    frac_near = 1.0 - float(safe.float().mean())
    rel_safe = float((d1[safe] - d0[safe]).norm() / d0[safe].norm())
    rel_all = float((d1 - d0).norm() / d0.norm())
    print(f"\n[{mlp_prec}] points within {delta:g} of a ReLU kink: {100 * frac_near:.2f} %; d feature rel. L2 error: {rel_safe:.2e} away from kinks, {rel_all:.2e} over all points")
    assert frac_near < {"bf16x3": 0.05, "f16": 0.35}[mlp_prec]
    assert rel_safe < {"bf16x3": 1e-4, "f16": 5e-3}[mlp_prec]
    assert rel_all < {"bf16x3": 5e-3, "f16": 5e-2}[mlp_prec]
    # loss-scaled upstream gradients (GradScaler's 65536x and far beyond fp16's range): the result scales exactly
    big = fo.field_backward(pts.cuda(), 1.0, gs.cuda() * 65536.0 * 1024.0, gc.cuda() * 65536.0 * 1024.0, s1, c1, masks, packed, want_dfeat=True).cpu()
    assert torch.isfinite(big).all()
    np.testing.assert_allclose((big / (65536.0 * 1024.0)).numpy(), d1.numpy(), rtol=1e-6, atol=0)
    tiny = fo.field_backward(pts.cuda(), 1.0, gs.cuda() * 2.0 ** -60, gc.cuda() * 2.0 ** -60, s1, c1, masks, packed, want_dfeat=True).cpu()
    np.testing.assert_allclose((tiny * 2.0 ** 60).numpy(), d1.numpy(), rtol=1e-6, atol=0)


def test_default_arithmetic_pinned_elementwise_by_an_operand_rounding_oracle(fo, tables):
    """the DEFAULT arithmetic (fp16 operands, fp32 accumulate) was checked against the fp32 oracle only in aggregate, because a few
    per cent of the points take the other side of a ReLU kink.  Here the oracle rounds every matrix operand to fp16 exactly where the kernels do
    (fr.round_operand, straight-through): the same values reach every ReLU, so the same side of (almost) every kink is taken and the per-point gradient
    of the codebook feature agrees over ALL 20 000 points -- what remains is the fp16 rounding of the backward's own operands and the order of the fp32
    accumulation.  Also the forward: sigma / rgb agree 10x tighter than against the fp32 oracle."""
    from nerf_signature_amd import _native as nv
    before = nv.fn("mlp_get_precision")()
    nv.set_mlp_precision("f16")
    try:
        base, cb, base_d, cb_d = tables
        P, sp, cp = _params(tables)
        packed = fo.pack_weights(sp, cp)
        rng = np.random.RandomState(11)
        M = 20000
        pts = torch.from_numpy((rng.rand(M, 3) * 2 - 1).astype(np.float32))
        dirs = torch.from_numpy(cf.unit_dirs(M, seed=12))
        msg = torch.from_numpy(cf.messages(32)[2])
        gs, gc = torch.from_numpy(rng.randn(M).astype(np.float32)), torch.from_numpy(rng.randn(M, 3).astype(np.float32))
        d32, _ = _oracle_per_point(pts, dirs, msg, P, gs, gc)
        d16, margin = _oracle_per_point(pts, dirs, msg, P, gs, gc, operands="f16")
        S = fo.codebook_presum(fo.select_tables(cb_d[:64], fo.message_bits(msg)))
        s1, c1, _, masks = fo.field_forward(pts.cuda(), dirs.cuda(), 1.0, base_d, S, packed, want_masks=True)
        d1 = fo.field_backward(pts.cuda(), 1.0, gs.cuda(), gc.cuda(), s1, c1, masks, packed, want_dfeat=True).cpu()
        P16 = dict(P, mlp_operands="f16")
        with torch.no_grad():
            s0, c0 = fr.field_forward(pts, dirs, msg, P16)
    finally:
        nv.call("mlp_set_precision", before)
    rel_vs_f32 = float((d1 - d32).norm() / d32.norm())
    rel_vs_f16 = float((d1 - d16).norm() / d16.norm())
    per_point = (d1 - d16).norm(dim=-1) / (d16.norm(dim=-1) + 1e-3 * float(d16.norm(dim=-1).mean()))
    flipped = float((per_point > 0.05).float().mean())
    err_s = float(((s1.cpu() - s0).abs() / s0.abs().clamp_min(1e-6)).max())
    err_c = float((c1.cpu() - c0).abs().max())
    print(f"\nd feature, all {M} points, rel. L2: vs fp32 oracle {rel_vs_f32:.2e}, vs operand-rounding oracle {rel_vs_f16:.2e}; points off by > 5 %: {100 * flipped:.3f} %; "
          f"forward vs operand-rounding oracle: sigma {err_s:.1e} rel, rgb {err_c:.1e}")
    assert rel_vs_f16 < 2e-3 and rel_vs_f16 < 0.2 * rel_vs_f32        # measured 3.5e-4 over ALL points (against the fp32 oracle: 1.6e-2, the kinks)
    assert flipped < 1e-3                                             # a kink taken on the other side: only where the accumulation order decides (measured: none)
    assert err_s < 2e-4 and err_c < 1e-4                              # (measured 4.7e-5 / 4.4e-5: fast exp in the kernel's sigmoid / trunc_exp)


def test_trunc_exp_clamp_in_backward(fo, tables, strict_mlp):
    """Log-densities beyond +-15 use the clamped derivative (activation.py:14)."""
    base, cb, base_d, cb_d = tables
    rng = np.random.RandomState(2)
    pts = torch.from_numpy((rng.rand(512, 3) * 2 - 1).astype(np.float32))
    dirs = torch.from_numpy(cf.unit_dirs(512, seed=7))
    msg = torch.from_numpy(cf.messages(32)[2])
    bits = fo.message_bits(msg)
    seen_hi = seen_lo = False
    for gain in (250.0, -250.0):
        sp, cp = cf.mlp_params(3072, 1337).copy(), cf.mlp_params(7168, 1338)
        sp[2048:2048 + 64] *= gain       # row 0 of the sigma head: large |h0| of either sign
        P = {"bound": 1.0, "base_tables": base, "cb_tables": [t.clone().requires_grad_(True) for t in cb[:64]],
             "sigma_params": torch.from_numpy(sp), "color_params": torch.from_numpy(cp)}
        packed = fo.pack_weights(torch.from_numpy(sp).cuda(), torch.from_numpy(cp).cuda())
        s0, c0 = fr.field_forward(pts, dirs, msg, P)
        h0 = torch.log(s0.detach())
        seen_hi |= bool((h0 > 15).any())
        seen_lo |= bool((h0 < -15).any())
        s0.sum().backward()
        G0 = P["cb_tables"][bits[0]].grad
        S = fo.codebook_presum(fo.select_tables(cb_d[:64], bits))
        s1, c1, _, masks = fo.field_forward(pts.cuda(), dirs.cuda(), 1.0, base_d, S, packed, want_masks=True)
        np.testing.assert_allclose(s1.cpu().numpy(), s0.detach().numpy(), rtol=5e-3)
        G1 = torch.zeros(1 << 19, 2, device="cuda")
        fo.field_backward(pts.cuda(), 1.0, torch.ones(512, device="cuda"), torch.zeros(512, 3, device="cuda"), s1, c1, masks, packed, G=G1)
        scale = float(G0.abs().max())
        np.testing.assert_allclose(G1.cpu().numpy(), G0.numpy(), rtol=5e-3, atol=5e-4 * scale)
    assert seen_hi and seen_lo


def test_sliced_scatter_equals_pointwise_scatter(fo, tables):
    """hg_scatter_sliced (LDS-owned slices) accumulates the same G as the point-wise atomic scatter; rows bit-identical."""
    base, cb, base_d, cb_d = tables
    P, sp, cp = _params(tables)
    packed = fo.pack_weights(sp, cp)
    rng = np.random.RandomState(3)
    M = 20011
    pts = torch.from_numpy((rng.rand(M, 3) * 2 - 1).astype(np.float32)).cuda()
    pts[:5] = torch.tensor([[-1., -1, -1], [1, 1, 1], [0, 0, 0], [1, -1, 0.5], [0.25, 0.5, 0.75]], device="cuda")   # box faces / exact grid points
    dirs = torch.from_numpy(cf.unit_dirs(M, seed=8)).cuda()
    S = fo.codebook_presum(fo.select_tables(cb_d[:64], fo.message_bits(torch.from_numpy(cf.messages(32)[2]))))
    s1, c1, _, masks = fo.field_forward(pts, dirs, 1.0, base_d, S, packed, want_masks=True)
    gs, gc = torch.randn(M, device="cuda"), torch.randn(M, 3, device="cuda")
    gs[100:200] = 0
    gc[100:200] = 0
    dfeat, rec = fo.field_backward(pts, 1.0, gs, gc, s1, c1, masks, packed, want_dfeat=True, want_rec=True)
    # the record: integer cell of the 2048^3 codebook grid, interpolation weights, the two feature gradients
    assert rec.shape == (M, 8) and torch.equal(rec[:, 5:7].contiguous(), dfeat)
    words = rec.view(torch.int32)
    x01 = ((pts + 1.0) / 2.0)
    cell = torch.floor(x01.clamp(0, 1) * 2048.0).int()
    assert torch.equal(words[:, 0] & 0xFFFF, cell[:, 0]) and torch.equal(words[:, 0] >> 16, cell[:, 1]) and torch.equal(words[:, 1], cell[:, 2])
    np.testing.assert_array_equal(rec[:, 2:5].cpu().numpy(), ((x01 - cell.float() * (1.0 / 2048.0)) * 2048.0).cpu().numpy())
    G1 = torch.zeros(1 << 19, 2, device="cuda")
    fo.codebook_scatter((pts + 1.0) / 2.0, dfeat, G1)
    for binned in (False, True):                       # every owner tests every point | hits grouped by slice first
        G2 = torch.full((1 << 19, 2), 0.5, device="cuda")
        fo.codebook_scatter_sliced(rec, G2, binned=binned)            # accumulates into what is there
        G2 -= 0.5
        assert torch.equal(G1 != 0, G2.abs() > 1e-12) or float(((G1 != 0) != (G2.abs() > 1e-9)).float().mean()) < 1e-4
        assert float((G1 - G2).norm() / G1.norm()) < 1e-5
    # degenerate input: every point in one cell (all hits land in at most four slices)
    same = rec[:1].repeat(5000, 1).contiguous()
    Ga, Gb = torch.zeros(1 << 19, 2, device="cuda"), torch.zeros(1 << 19, 2, device="cuda")
    fo.codebook_scatter_sliced(same, Ga, binned=False)
    fo.codebook_scatter_sliced(same, Gb, binned=True)
    assert float((Ga - Gb).norm() / Ga.norm()) < 1e-5 and int((Gb != 0).sum()) <= 16
    xs, ds = ((pts[:1] + 1.0) / 2.0).repeat(5000, 1).cpu(), same[:, 5:7].cpu()          # ... and both against the float64 sum
    stats, ref = fr.scatter_row_stats(xs, ds, CB_RES), fr.scatter_ref(xs, ds, CB_RES)
    fr.assert_scatter_close(Ga, ref, stats, False, what="5000 copies, sliced")
    fr.assert_scatter_close(Gb, ref, stats, True, quantum=fr.fixed_quantum(float(ds.abs().max()), 4 * 5000), what="5000 copies, binned")
    # planned route: destinations from the positions alone (also on a side stream), gradients written straight into the queue
    for stream in (None, torch.cuda.Stream()):
        prev = fo.set_plan_stream(stream)
        try:
            plan = fo.ScatterPlan(pts, 1.0)
        finally:
            fo.set_plan_stream(prev)
        G3 = torch.full((1 << 19, 2), 0.5, device="cuda")
        fo.field_backward_planned(pts, 1.0, gs, gc, s1, c1, masks, packed, plan, G3)
        G3 -= 0.5
        assert float((G1 - G3).norm() / G1.norm()) < 1e-5
        assert float(((G1 != 0) != (G3.abs() > 1e-9)).float().mean()) < 1e-4
    # queue contents: the plan's destinations are a permutation of [0, 4M) grouped by slice, and the entries equal k_bin_write's
    M4 = 4 * M
    hdr = 4 * (64 + 4 + 256 * 64)
    dest = plan.buf[hdr + 16 * M4: hdr + 16 * M4 + 16 * M].view(torch.int32).view(M, 4)
    assert torch.equal(torch.sort(dest.reshape(-1)).values, torch.arange(M4, device="cuda", dtype=torch.int32))
    counts = plan.buf[:256].view(torch.int32)
    assert int(counts.sum()) == M4
    queue = plan.buf[hdr: hdr + 16 * M4].view(torch.int32).view(M4, 4)
    hy = (cell[:, 1].long() * 2654435761) & 0xFFFFFFFF
    hz = (cell[:, 2].long() * 805459861) & 0xFFFFFFFF
    starts = torch.cumsum(counts.long(), 0) - counts.long()
    sl0 = ((hy ^ hz) >> 13) & 63                              # the (dy, dz) = (0, 0) pair
    d0 = dest[:, 0].long()
    assert bool(((d0 >= starts[sl0]) & (d0 < starts[sl0] + counts.long()[sl0])).all())
    e0 = queue[d0]
    assert torch.equal(e0[:, 0] & 0xFFFF, cell[:, 0]) and torch.equal((e0[:, 0] >> 16) & 0x1FFF, ((hy ^ hz) & 0x1FFF).int())
    assert torch.equal(e0[:, 1], words[:, 2])                 # the x weight, bit for bit


# ---- every codebook scatter route against the float64 sum (oracle.field_ref.scatter_ref) -------------------------------------------------------------------
T_ROWS = 1 << 19
CB_RES = fr.level_resolutions(64, 2048, 2048)[0]


def _records(x01, dfeat):
    """[M,8] scatter records of points x01 [M,3] (device, fp32) with feature gradients dfeat [M,2]: the layout pinned in
    test_sliced_scatter_equals_pointwise_scatter (integer cell, the three weights, the two gradients, one pad word)."""
    M = x01.shape[0]
    cell = torch.floor(x01.clamp(0, 1) * 2048.0).int()
    rec = torch.zeros(M, 8, dtype=torch.float32, device=x01.device)
    words = rec.view(torch.int32)
    words[:, 0] = cell[:, 0] | (cell[:, 1] << 16)
    words[:, 1] = cell[:, 2]
    rec[:, 2:5] = (x01 - cell.float() * (1.0 / 2048.0)) * 2048.0
    rec[:, 5:7] = dfeat
    return rec


def _cb_case(name, seed=0):
    """(x01 [M,3], dfeat [M,2]) on the CPU for one hit distribution of the codebook scatter tests."""
    rng = np.random.RandomState(seed)
    if name.startswith(("vertex", "cell")):            # hot rows: N copies of one point, gradient 1.0 | 0.75 | random sign
        kind, N, g = name.split("_")
        N = int(N)
        p = np.array([1000, 517, 1301], np.float32) / np.float32(2048) if kind == "vertex" else np.array([0.37, 0.61, 0.19], np.float32)
        x = np.repeat(p[None], N, 0)
        if g == "mixed":
            d = rng.choice([-1.0, 1.0], (N, 2)).astype(np.float32)
        else:
            d = np.full((N, 2), float(g), np.float32)
        return torch.from_numpy(x), torch.from_numpy(d)
    M = 65536
    x = rng.rand(M, 3).astype(np.float32)
    x[:8] = [[0, 0, 0], [1, 1, 1], [0.5, 0.5, 0.5], [1, 0, 0.25], [np.float32(1) - np.float32(2 ** -24)] * 3, [0.3, 0.7, 0.9], [0.3, 0.7, 0.9], [2 / 2048, 4 / 2048, 8 / 2048]]
    d = rng.randn(M, 2).astype(np.float32)
    if name == "uniform":
        d[100:200] = 0.0
    elif name == "cancel":                             # equal and opposite pairs on the same rows: exactly 0 on the fixed-point routes
        x[1::2] = x[0::2]
        d[1::2] = -d[0::2]
    elif name == "hotcancel":
        x[:] = x[2]
        d[:] = 1.0
        d[1::2] = -1.0
    elif name == "range":                              # one outlier 2^30 x the rest: rows with small contributions only
        d *= np.float32(2.0 ** -30)
        d[5] = (1.0, -1.0)
    elif name.startswith("gmax"):                      # the largest |gradient| a power of two | the float below one | subnormal | all zero
        v = {"gmax_pow2": 4.0, "gmax_below": float(np.nextafter(np.float32(4), np.float32(0))), "gmax_subnormal": 2.0 ** -130, "gmax_zero": 0.0}[name]
        d = (np.sign(d) * np.float32(v)).astype(np.float32)
        if name == "gmax_subnormal":
            x[:] = x[7]                                # a vertex: weights 0 and 1, the products exact
    return torch.from_numpy(x), torch.from_numpy(d)


CB_CASES = ["uniform", "cancel", "hotcancel", "range", "gmax_pow2", "gmax_below", "gmax_subnormal", "gmax_zero"] + \
    [f"{k}_{n}_{g}" for k in ("vertex", "cell") for n in (4095, 8193, 65536) for g in ("1.0", "0.75", "mixed")]
CB_ROUTES = ["pointwise", "sliced", "binned"]


def _cb_route(fo, route, x01, dfeat, G):
    if route == "pointwise":
        fo.codebook_scatter(x01, dfeat, G)
    elif route == "auto":
        fo.codebook_scatter_sliced(_records(x01, dfeat), G)
    else:
        fo.codebook_scatter_sliced(_records(x01, dfeat), G, binned=(route == "binned"))
    return G


@pytest.mark.parametrize("case", CB_CASES)
def test_codebook_scatter_routes_vs_float64(fo, case):
    """The point-wise (fp32 global atomics), sliced (fp32 LDS atomics) and binned (fixed point, four replicas + the exact merge) codebook
    scatters against the float64 sum, on a pre-filled G they must accumulate into; the fixed-point route twice: the same bits.  Hot rows
    (up to 65536 hits on one row) are where a fixed-point scale that ignores the hit count wraps."""
    x, d = _cb_case(case)
    ref = fr.scatter_ref(x, d, CB_RES)
    xd, dd = x.cuda(), d.cuda()
    assert torch.equal(_records(xd, dd)[:, 5:7], dd)
    prefill = torch.from_numpy(np.random.RandomState(1).randn(T_ROWS, 2).astype(np.float32))
    want = prefill.double() + ref
    M, stats = x.shape[0], fr.scatter_row_stats(x, d, CB_RES)
    for route in CB_ROUTES:
        G = _cb_route(fo, route, xd, dd, prefill.cuda())
        fixed = route == "binned"
        fr.assert_scatter_close(G, want, stats, fixed, prefill=prefill, quantum=fr.fixed_quantum(float(d.abs().max()), 4 * M), what=f"{case} {route}")
        if fixed:
            assert torch.equal(G, _cb_route(fo, route, xd, dd, prefill.cuda())), "fixed point: two runs, the same bits"
            if case in ("cancel", "hotcancel"):
                Gz = _cb_route(fo, route, xd, dd, torch.zeros(T_ROWS, 2, device="cuda"))
                assert int((Gz != 0).sum()) == 0, "equal and opposite contributions cancel exactly in fixed point"
    if case == "gmax_zero":
        for route in CB_ROUTES:
            assert torch.equal(_cb_route(fo, route, xd, dd, prefill.cuda()).cpu(), prefill), route


def test_codebook_scatter_auto_route_and_tiny_binned_launches(fo, monkeypatch):
    """codebook_scatter_sliced(binned=None) on both sides of fieldops.BINNED_MIN_POINTS with every point on one vertex (the binned route is
    taken from 65536 points; NERFSIG_DETERMINISTIC=1 takes it at every size), and the binned route at M = 1, 2, 3, 5: fewer entries than
    replicas, empty replicas at the merge."""
    assert fo.BINNED_MIN_POINTS == 65536
    p = torch.tensor([[1000 / 2048, 517 / 2048, 1301 / 2048]], dtype=torch.float32)
    for M in (65535, 65536, 65537):
        x, d = p.repeat(M, 1), torch.ones(M, 2)
        d[::3] = 0.75
        want = fr.scatter_ref(x, d, CB_RES)
        G = _cb_route(fo, "auto", x.cuda(), d.cuda(), torch.zeros(T_ROWS, 2, device="cuda"))
        fixed = M >= fo.BINNED_MIN_POINTS
        fr.assert_scatter_close(G, want, fr.scatter_row_stats(x, d, CB_RES), fixed, quantum=fr.fixed_quantum(1.0, 4 * M), what=f"auto M={M}")
    monkeypatch.setenv("NERFSIG_DETERMINISTIC", "1")
    assert fo.binned_min_points() == 1
    x, d = p.repeat(9000, 1), torch.full((9000, 2), -1.0)
    G = _cb_route(fo, "auto", x.cuda(), d.cuda(), torch.zeros(T_ROWS, 2, device="cuda"))
    fr.assert_scatter_close(G, fr.scatter_ref(x, d, CB_RES), fr.scatter_row_stats(x, d, CB_RES), True, quantum=fr.fixed_quantum(1.0, 4 * 9000), what="deterministic")
    monkeypatch.delenv("NERFSIG_DETERMINISTIC")
    rng = np.random.RandomState(4)
    for M in (1, 2, 3, 5):
        x = torch.from_numpy(rng.rand(M, 3).astype(np.float32))
        d = torch.from_numpy(rng.randn(M, 2).astype(np.float32))
        prefill = torch.full((T_ROWS, 2), 0.5)
        G = _cb_route(fo, "binned", x.cuda(), d.cuda(), prefill.cuda())
        fr.assert_scatter_close(G, 0.5 + fr.scatter_ref(x, d, CB_RES), fr.scatter_row_stats(x, d, CB_RES), True, prefill=prefill, quantum=fr.fixed_quantum(float(d.abs().max()), 4 * M),
                             what=f"binned M={M}")
        assert int((G != 0.5).sum()) <= 16 * M      # (8 corners x 2 features per point)


@pytest.mark.parametrize("case", ["uniform", "vertex", "cell"])
def test_planned_scatter_vs_float64(fo, tables, case):
    """The headline's route (ScatterPlan + field_backward_planned: the MLP backward writes the queue, four replicas + the exact merge) against the
    float64 sum of the feature gradients field_backward reports for the same points (the same kernel arithmetic), accumulated into a pre-filled G;
    65536 points spread out, all on one vertex, or all in one cell.  Twice: the same bits.  (Exact cancellation in the owners and the merge:
    test_codebook_scatter_routes_vs_float64's binned route, the same kernels.)"""
    _, sp, cp = _params(tables)
    packed = fo.pack_weights(sp, cp)
    base_d, cb_d = tables[2], tables[3]
    M = 65536
    rng = np.random.RandomState(6)
    if case == "uniform":
        x01 = rng.rand(M, 3).astype(np.float32)
    else:
        p = np.array([0.37, 0.61, 0.19] if case == "cell" else [1000, 517, 1301], np.float32) / np.float32(1 if case == "cell" else 2048)
        x01 = np.repeat(p[None], M, 0)
    pts = torch.from_numpy(x01 * np.float32(2) - np.float32(1)).cuda()
    dirs = torch.from_numpy(cf.unit_dirs(M, seed=8)).cuda()
    gs, gc = torch.from_numpy(rng.randn(M).astype(np.float32)).cuda(), torch.from_numpy(rng.randn(M, 3).astype(np.float32)).cuda()
    S = fo.codebook_presum(fo.select_tables(cb_d[:64], fo.message_bits(torch.from_numpy(cf.messages(32)[2]))))
    s1, c1, _, masks = fo.field_forward(pts, dirs, 1.0, base_d, S, packed, want_masks=True)
    dfeat = fo.field_backward(pts, 1.0, gs, gc, s1, c1, masks, packed, want_dfeat=True)
    x, d = ((pts + 1.0) / 2.0).cpu(), dfeat.cpu()
    prefill = torch.from_numpy(np.random.RandomState(1).randn(T_ROWS, 2).astype(np.float32))
    got = []
    for _ in range(2):
        G = prefill.cuda()
        fo.field_backward_planned(pts, 1.0, gs, gc, s1, c1, masks, packed, fo.ScatterPlan(pts, 1.0), G)
        got.append(G)
    assert torch.equal(got[0], got[1])
    fr.assert_scatter_close(got[0], prefill.double() + fr.scatter_ref(x, d, CB_RES), fr.scatter_row_stats(x, d, CB_RES), True, prefill=prefill,
                         quantum=fr.fixed_quantum(float(d.abs().max()), 4 * M), what=f"planned {case}")


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -float("inf")])
def test_codebook_scatter_routes_leave_a_non_finite_gradient_visible(fo, bad):
    """One non-finite feature gradient among 65536: the float routes carry it into the rows it reaches; the fixed-point routes poison every
    row with NaN (csrc/hashgrid.hip k_scatter_binned) -- either way GradScaler's inf check sees it."""
    x, d = _cb_case("uniform")
    d[1234, 1] = bad
    xd, dd = x.cuda(), d.cuda()
    rows, _, _ = fr.voxel_lookup(x[1234:1235], CB_RES)
    for route in CB_ROUTES:
        G = _cb_route(fo, route, xd, dd, torch.zeros(T_ROWS, 2, device="cuda"))
        assert not bool(torch.isfinite(G).all()), route
        if route == "binned":
            assert bool(torch.isnan(G).all()), route
        else:
            assert not bool(torch.isfinite(G[rows[0].cuda(), 1]).any()), route


def test_pipelined_training_launches_equal_the_plain_loops_bit_for_bit(fo, tables):
    """k_field_fwd_train / k_field_bwd_train (software-pipelined over a wave's tiles: include/nerfsig.h mlp_set_pipelined) against the plain per-tile
    loops they replace on the training render's path: sigma and rgb bit for bit, the scattered codebook gradient G to half an ulp of its largest entry
    (what two runs of the same kernels differ by), for point counts that are and are not multiples of the tile; and hg_warm_tables changes nothing."""
    from nerf_signature_amd import _native as nv
    base, cb, base_d, cb_d = tables
    _, sp, cp = _params(tables)
    packed = fo.pack_weights(sp, cp)
    before_prec, before_pipe = nv.fn("mlp_get_precision")(), nv.fn("mlp_get_pipelined")()
    nv.set_mlp_precision("f16")
    try:
        for M in (70001, 262144):           # (both above fieldops.BINNED_MIN_POINTS: the planned backward)
            rng = np.random.RandomState(M)
            pts = torch.from_numpy((rng.rand(M, 3) * 2 - 1).astype(np.float32)).cuda()
            dirs = torch.from_numpy(cf.unit_dirs(M, seed=5)).cuda()
            msg = torch.from_numpy(cf.messages(32)[1])
            selected = fo.select_tables(cb_d[:64], fo.message_bits(msg))
            gs, gc = torch.from_numpy(rng.randn(M).astype(np.float32)).cuda(), torch.from_numpy(rng.randn(M, 3).astype(np.float32)).cuda()
            got = {}
            for mask in (0, 3, 1, 2):
                nv.call("mlp_set_pipelined", mask)
                sink = fo.GradSink(pts.device)
                for t in selected:
                    t.requires_grad_(True)
                sigma, rgb = fo.field_apply(pts, dirs, 1.0, packed, base_d, selected, sink=sink)
                torch.autograd.backward([sigma, rgb], [gs, gc])
                torch.cuda.synchronize()
                got[mask] = (sigma.detach().clone(), rgb.detach().clone(), sink.G.clone())
            assert fo.BINNED_MIN_POINTS <= M
            for k in (3, 1, 2):
                assert torch.equal(got[0][0], got[k][0]) and torch.equal(got[0][1], got[k][1])
                # G: the owners' fixed-point scale is re-derived per launch and the sum rounded to fp32 once: two runs of the SAME kernels differ
                # by half an ulp in a few rows; the queue entries (gradient pairs) themselves are identical
                np.testing.assert_allclose(got[k][2].cpu().numpy(), got[0][2].cpu().numpy(), rtol=0, atol=1.2e-7 * float(got[0][2].abs().max()))
            assert float(got[3][2].abs().max()) > 0
        # the warm-up pass only reads
        S = fo.codebook_presum(selected)
        snap = [t.clone() for t in base_d] + [S.clone()]
        sink_word = torch.zeros(1, dtype=torch.float32, device="cuda")
        nv.call("hg_warm_tables", nv.ptr_array([t.detach() for t in base_d]), nv.ptr(S), nv.ptr(sink_word), nv.stream())
        nv.call("hg_warm_tables", nv.ptr_array([t.detach() for t in base_d]), None, nv.ptr(sink_word), nv.stream())      # (a clean model: no pre-sum)
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(snap, base_d + [S])) and float(sink_word) == 0.0
        with pytest.raises(ValueError):       # (argument errors surface as ValueError: _native.call)
            nv.call("hg_warm_tables", nv.ptr_array([t.detach() for t in base_d]), nv.ptr(S), None, nv.stream())
        with pytest.raises(ValueError):
            nv.call("mlp_set_pipelined", 4)
    finally:
        nv.call("mlp_set_precision", before_prec)
        nv.call("mlp_set_pipelined", before_pipe)


def test_mixed_plane_sets_equal_fp32_plane_sets_bit_for_bit(fo, tables, monkeypatch):
    """hg_encode_planes_mixed (levels 0..14 as the fp16 pairs of the fp16 MLP's first-layer operand, level 15 + codebook as float2: 76 instead of 136 bytes per
    point) against fp32 plane sets (NERFSIG_HALF_PLANES=0) through every consumer: the pipelined training launch (sigma, rgb, ReLU masks), the plain loop
    (geo features requested), the kept route (FixedPoints + hg_encode_codebook_plane), a device row count; with and without a codebook; point counts that are
    and are not multiples of the tile.  Same bits everywhere.  And the guards: a set declared mixed is refused by the split-bf16 MLP; the layout is an argument its owner passes (no registry by address)."""
    from nerf_signature_amd import _native as nv
    base, cb, base_d, cb_d = tables
    _, sp, cp = _params(tables)
    packed = fo.pack_weights(sp, cp)
    before = nv.fn("mlp_get_precision")()
    nv.set_mlp_precision("f16")
    try:
        msg = torch.from_numpy(cf.messages(32)[1])
        S = fo.codebook_presum(fo.select_tables(cb_d[:64], fo.message_bits(msg)))
        for M in (20000, 70001):
            rng = np.random.RandomState(M)
            pts = torch.from_numpy((rng.rand(M, 3) * 2 - 1).astype(np.float32)).cuda()
            dirs = torch.from_numpy(cf.unit_dirs(M, seed=6)).cuda()
            got = {}
            for half in ("0", "1"):
                monkeypatch.setenv("NERFSIG_HALF_PLANES", half)
                assert fo.mixed_planes() == (half == "1")
                out = []
                for s_ in (S, None):
                    out += [t for t in fo.field_forward(pts, dirs, 1.0, base_d, s_, packed, want_masks=True, planes=True) if t is not None]      # pipelined launch
                    out += [t for t in fo.field_forward(pts, dirs, 1.0, base_d, s_, packed, want_geo=True, planes=True) if t is not None]        # plain loop
                kept = fo.FixedPoints(pts, 1.0, base_d)
                out += [t for t in fo.field_forward(pts, dirs, 1.0, base_d, S, packed, want_masks=True, fixed=kept) if t is not None]
                rows = torch.tensor([M - 777], dtype=torch.int32, device="cuda")
                ws = torch.zeros(int(nv.fn("hg_planes_bytes")(M)), dtype=torch.uint8, device="cuda")
                sig, rgb = torch.zeros(M, device="cuda"), torch.zeros(M, 3, device="cuda")
                base_ptrs = nv.ptr_array([t.detach() for t in base_d])
                layout = fo.encode_planes(pts, M, 1.0, base_ptrs, S, ws, rows)
                assert layout == (fo.PLANES_MIXED if half == "1" else fo.PLANES_F32)
                nv.call("field_fwd_rows", nv.ptr(pts), nv.ptr(dirs), M, nv.ptr(rows), 1.0, base_ptrs, nv.ptr(S), nv.ptr(packed), nv.ptr(sig), nv.ptr(rgb), nv.ptr(ws), layout, nv.stream())
                out += [sig, rgb]
                torch.cuda.synchronize()
                got[half] = [t.clone() for t in out]
            assert len(got["0"]) == len(got["1"]) >= 14
            for a, b in zip(got["0"], got["1"]):
                assert a.shape == b.shape and torch.equal(a, b)
            assert float(got["1"][-1][M - 700:].abs().max()) == 0.0 and float(got["1"][-1][:M - 777].abs().max()) > 0      # rows beyond the device count: untouched
        # guards
        monkeypatch.setenv("NERFSIG_HALF_PLANES", "1")
        M = 20000
        pts, dirs = pts[:M].contiguous(), dirs[:M].contiguous()
        ws = torch.zeros(int(nv.fn("hg_planes_bytes")(M)), dtype=torch.uint8, device="cuda")
        base_ptrs = nv.ptr_array([t.detach() for t in base_d])
        layout = fo.encode_planes(pts, M, 1.0, base_ptrs, S, ws)
        assert layout == fo.PLANES_MIXED
        sig, rgb = torch.zeros(M, device="cuda"), torch.zeros(M, 3, device="cuda")
        nv.set_mlp_precision("bf16x3")
        assert not fo.mixed_planes()
        with pytest.raises(ValueError, match="mixed"):
            nv.call("field_fwd", nv.ptr(pts), nv.ptr(dirs), M, 1.0, base_ptrs, nv.ptr(S), nv.ptr(packed), nv.ptr(sig), nv.ptr(rgb), None, None, nv.ptr(ws), layout, nv.stream())
        with pytest.raises(ValueError, match="fp16"):
            nv.call("hg_encode_planes_mixed", nv.ptr(pts), M, None, 1.0, base_ptrs, nv.ptr(S), nv.ptr(ws), nv.stream())
        with pytest.raises(ValueError, match="planes_layout"):      # the layout is an explicit argument (no registry by address): anything but the two constants is refused
            nv.call("field_fwd", nv.ptr(pts), nv.ptr(dirs), M, 1.0, base_ptrs, nv.ptr(S), nv.ptr(packed), nv.ptr(sig), nv.ptr(rgb), None, None, nv.ptr(ws), 7, nv.stream())
        nv.call("hg_encode_planes", nv.ptr(pts), M, 1.0, base_ptrs, nv.ptr(S), nv.ptr(ws), nv.stream())       # the same buffer written as fp32 again, and said so
        nv.call("field_fwd", nv.ptr(pts), nv.ptr(dirs), M, 1.0, base_ptrs, nv.ptr(S), nv.ptr(packed), nv.ptr(sig), nv.ptr(rgb), None, None, nv.ptr(ws), fo.PLANES_F32, nv.stream())
        torch.cuda.synchronize()
        assert float(sig.abs().max()) > 0
    finally:
        nv.call("mlp_set_precision", before)


# ---- the render-path MLP kernels: position independence in both arithmetics, float64 chain bound in split bf16 (tests/mlp_ref.py) --------------------------------


@pytest.fixture(scope="module")
def walk():
    """The walking-count case (every MLP launch has waves that walk three tiles or more, the last tile partial), the same upstream gradients without
    the scaled blocks, and a seeded permutation of the rows: computed once, never modified."""
    n = mr.walking_count(torch.cuda.get_device_properties(0).multi_processor_count)
    pts, dirs, gs, gc = (t.cuda() for t in mr.case(n))
    gs_plain, gc_plain = (t.cuda() for t in mr.case(n, scaled=False)[2:])
    perm = torch.from_numpy(np.random.RandomState(77).permutation(n)).cuda()
    return {"n": n, "pts": pts, "dirs": dirs, "gs": gs, "gc": gc, "gs_plain": gs_plain, "gc_plain": gc_plain, "perm": perm, "inv": torch.argsort(perm)}


def _point_words(masks, M):
    """Mask words [tiles * 32, 6] -> the six words of each live point [M, 6] (layer, lane half): lane p of a tile is point p, wherever the tile sits."""
    return masks.view(-1, 3, 2, 32).permute(0, 3, 1, 2).reshape(-1, 6)[:M]


FWD_ROUTES = ["fused_geo_masks", "planes_masks", "planes_geo", "planes_f32_masks", "rows", "color"]


def _fwd_route(fo, route, pts, dirs, base_d, S, packed, monkeypatch, geo_in=None):
    """One forward entry point / route on the rows given -> the list of its per-point outputs."""
    from nerf_signature_amd import _native as nv
    M = pts.shape[0]
    monkeypatch.setenv("NERFSIG_HALF_PLANES", "0" if route == "planes_f32_masks" else "1")
    if route == "color":
        return [fo.field_color(dirs, geo_in, packed)]
    if route == "rows":
        base_ptrs = nv.ptr_array([t.detach() for t in base_d])
        ws = torch.zeros(int(nv.fn("hg_planes_bytes")(M)), dtype=torch.uint8, device="cuda")
        rows = torch.tensor([M], dtype=torch.int32, device="cuda")
        sig, rgb = torch.full((M,), float("nan"), device="cuda"), torch.full((M, 3), float("nan"), device="cuda")
        layout = fo.encode_planes(pts, M, 1.0, base_ptrs, S, ws, rows)
        nv.call("field_fwd_rows", nv.ptr(pts), nv.ptr(dirs), M, nv.ptr(rows), 1.0, base_ptrs, nv.ptr(S), nv.ptr(packed), nv.ptr(sig), nv.ptr(rgb), nv.ptr(ws), layout, nv.stream())
        return [sig, rgb]
    kw = {"fused_geo_masks": dict(planes=False, want_geo=True, want_masks=True), "planes_masks": dict(planes=True, want_masks=True),
          "planes_geo": dict(planes=True, want_geo=True), "planes_f32_masks": dict(planes=True, want_masks=True)}[route]
    s, c, geo, masks = fo.field_forward(pts, dirs, 1.0, base_d, S, packed, **kw)
    return [s, c] + ([geo] if geo is not None else []) + ([_point_words(masks, M)] if masks is not None else [])


@pytest.mark.parametrize("route", FWD_ROUTES)
def test_forward_routes_are_position_independent_and_within_the_chain_bound_against_float64(fo, tables, walk, route, mlp_prec, monkeypatch):
    """field_fwd (planes NULL | a plane set: pipelined launch with masks, plain loop with geo features | fp32 planes under the fp16 MLP), field_fwd_rows and
    field_color_fwd.  A row's outputs do not depend on where the row sits: for every edge count M the outputs of pts[:M] are the first M rows of the
    walking-count run (where waves walk up to three tiles) bit for bit (sigma, rgb, geo, the mask words), and so is a run on a seeded permutation of the rows,
    un-permuted -- every tile, workgroup and grid edge thereby reduces to rows the oracle tests judge.  Split bf16: sigma, geo and rgb against float64 within the chain bound at the walking count
    and at 1, 33, 1025 rows (fp16: the worst-case chain bound is as large as the logits; nothing is asserted against it)."""
    base, cb, base_d, cb_d = tables
    _, sp, cp = _params(tables)
    packed = fo.pack_weights(sp, cp)
    S = fo.codebook_presum(fo.select_tables(cb_d[:64], fo.message_bits(torch.from_numpy(cf.messages(32)[2]))))
    n, pts, dirs = walk["n"], walk["pts"], walk["dirs"]
    geo_all = fo.field_forward(pts, None, 1.0, base_d, S, packed, want_rgb=False, want_geo=True)[2] if route == "color" else None
    run = lambda idx: _fwd_route(fo, route, pts[idx].contiguous(), dirs[idx].contiguous(), base_d, S, packed, monkeypatch, None if geo_all is None else geo_all[idx].contiguous())
    big = run(slice(0, n))
    torch.cuda.synchronize()
    assert all(not torch.isnan(t.float()).any() for t in big)
    for a, b in zip(big, run(walk["perm"])):
        assert torch.equal(a, b[walk["inv"]]), "a permutation of the rows changed a row's output"
    for M in mr.EDGE_COUNTS:
        for a, b in zip(big, run(slice(0, M))):
            assert b.shape[0] == M and torch.equal(a[:M], b), (M, "the first M rows alone give other bits")
    if mlp_prec == "bf16x3":
        W = mr.split_params(sp, cp)
        feat = fo.encode((pts + 1) / 2, base_d, S).double().cpu()
        ref = mr.forward(feat, dirs.cpu(), W)          # (field_color_fwd was given field_fwd's geo features: the chain from the features holds for its rgb)
        b = mr.forward_chain_bound(ref, W, mr.U_BF16X3)      # (the features are exact: every encoder route equals hg_encode_fwd bit for bit, test (e) below)
        names = {"color": ["rgb"], "rows": ["sigma", "rgb"], "planes_masks": ["sigma", "rgb"], "planes_f32_masks": ["sigma", "rgb"]}.get(route, ["sigma", "rgb", "geo"])
        r = {nm: mr.ratio(t, ref[nm], b[nm]) for nm, t in zip(names, big)}
        for M in (1, 33, 1025):
            for nm, t in zip(names, run(slice(0, M))):
                r[f"{nm}@{M}"] = mr.ratio(t, ref[nm][:M], b[nm][:M])
        print(f"\n[c] {route}: largest error / chain bound " + ", ".join(f"{k} {v:.4f}" for k, v in r.items()))
        assert max(r.values()) <= 1.0, r


@pytest.mark.parametrize("pipe", [0, 3])
def test_backward_given_masks_is_position_independent_and_within_the_chain_bound_against_float64(fo, tables, walk, pipe, mlp_prec):
    """field_bwd (dfeat_out, rec_out, G) and field_bwd_planned + the planned scatter, fed the sigma, rgb and masks the forward produced -- given those the
    backward is a linear map of the upstream gradient, so a float64 reference has no kink ambiguity and no row is excluded.  Both arithmetics: d feature[30:32]
    of pts[:M] is the walking-count run's first M rows bit for bit, and so is a permuted run un-permuted (the fp16 path's power-of-two normalisation is per
    point: checked here, not assumed).  Split bf16: d feature against mlp_ref's backward-given-masks within the chain bound over ALL rows (zero rows, rows
    scaled by 2^30 and 2^-40 included); G of the atomic and of the planned route against the float64 scatter of the reference's d feature, the scatter's own
    tolerance widened by the scattered chain bound -- with the seeded gradients, where the 2^30 block is the sum, and with the same gradients unscaled."""
    from nerf_signature_amd import _native as nv
    base, cb, base_d, cb_d = tables
    _, sp, cp = _params(tables)
    packed = fo.pack_weights(sp, cp)
    S = fo.codebook_presum(fo.select_tables(cb_d[:64], fo.message_bits(torch.from_numpy(cf.messages(32)[2]))))
    n = walk["n"]
    before = nv.fn("mlp_get_pipelined")()
    nv.call("mlp_set_pipelined", pipe)
    try:
        def run(idx, scatter=False, grads=("gs", "gc")):
            pts, dirs, gs, gc = (walk[k][idx].contiguous() for k in ("pts", "dirs") + grads)
            s, c, _, masks = fo.field_forward(pts, dirs, 1.0, base_d, S, packed, want_masks=True)
            dfeat, rec = fo.field_backward(pts, 1.0, gs, gc, s, c, masks, packed, want_dfeat=True, want_rec=True)
            assert torch.equal(rec[:, 5:7].contiguous(), dfeat)
            out = {"dfeat": dfeat, "rec": rec[:, :7].contiguous(), "sigma": s, "rgb": c, "masks": masks}
            if scatter:
                out["G"] = torch.zeros(1 << 19, 2, device="cuda")
                assert fo.field_backward(pts, 1.0, gs, gc, s, c, masks, packed, G=out["G"], want_dfeat=True).equal(dfeat)
                out["G_planned"] = torch.zeros(1 << 19, 2, device="cuda")
                fo.field_backward_planned(pts, 1.0, gs, gc, s, c, masks, packed, fo.ScatterPlan(pts, 1.0), out["G_planned"])
            return out
        big = run(slice(0, n), scatter=True)
        torch.cuda.synchronize()
        assert not torch.isnan(big["dfeat"]).any()
        other = run(walk["perm"])
        assert torch.equal(big["dfeat"], other["dfeat"][walk["inv"]]) and torch.equal(big["rec"], other["rec"][walk["inv"]])
        for M in mr.EDGE_COUNTS:
            small = run(slice(0, M))
            assert torch.equal(big["dfeat"][:M], small["dfeat"]) and torch.equal(big["rec"][:M], small["rec"]), M
        if mlp_prec == "bf16x3":
            W = mr.split_params(sp, cp)
            x01 = ((walk["pts"] + 1.0) / 2.0).cpu()
            r = {}
            # twice: the seeded gradients (d feature is per row: every row judged; G is a sum over rows that the 2^30 block dominates, and the planned route's
            # fixed-point quantum follows the largest gradient) and the same gradients unscaled, where G sees every row
            for tag, got, grads in (("", big, ("gs", "gc")), ("_plain", run(slice(0, n), scatter=True, grads=("gs_plain", "gc_plain")), ("gs_plain", "gc_plain"))):
                bits = mr.unpack_masks(got["masks"], n)
                ref = mr.backward(walk[grads[0]].cpu(), walk[grads[1]].cpu(), got["sigma"].cpu(), got["rgb"].cpu(), bits, W)
                bound = mr.backward_chain_bound(ref, bits, W, mr.U_BF16X3)
                want, e = ref["d_feat"][:, 30:32], bound["d_feat"][:, 30:32]
                r["d_feat" + tag] = mr.ratio(got["dfeat"], want, e)
                Gref, stats = fr.scatter_ref(x01, want, CB_RES), fr.scatter_row_stats(x01, want, CB_RES)
                carried = fr.scatter_ref(x01, e, CB_RES)
                quantum = fr.fixed_quantum(float(got["dfeat"].abs().max()), 4 * n)
                r["G" + tag] = mr.ratio(got["G"], Gref, fr.scatter_tolerance(Gref, stats, False) + carried)
                r["G_planned" + tag] = mr.ratio(got["G_planned"], Gref, fr.scatter_tolerance(Gref, stats, True, quantum=quantum) + carried)
            print(f"\n[d] pipelined={pipe}: largest error / bound " + ", ".join(f"{k} {v:.4f}" for k, v in r.items()))
            assert max(r.values()) <= 1.0, r
    finally:
        nv.call("mlp_set_pipelined", before)


# ---- the hot-path plane encoders on the edge points ---------------------------------------------------------------------------------------------------------

def _edge_rows(M, bound, seed):
    """M positions in [-bound, bound]^3: seeded rows with closed_form.points() (box faces, exact and nearly exact cell boundaries of several levels) mapped
    to the box and placed first, last (an odd count then shifts the lane pairing) and, from an odd row on, across the 256-point tile boundary.  (Near -bound
    an fp32 position is coarser than the unit-box coordinate it stands for: a point a few ulp off a cell boundary can land ON it after the trip through
    [-bound, bound].  The exact boundaries, the box faces and the points off a boundary by more than 2^-24 survive; the full set is hg_encode_fwd's own test.)"""
    rng = np.random.RandomState(seed)
    E = (cf.points() * np.float32(2 * bound) - np.float32(bound)).astype(np.float32)
    x = ((rng.rand(M, 3) * 2 - 1) * bound).astype(np.float32)
    n = min(M, 256)
    x[:n] = E[:n]
    n = min(M, 40)
    x[M - n:] = E[:n]
    if M > 300:
        x[225:289] = E[:64]
    return torch.from_numpy(x).cuda()


def _f32_planes(ws, M):
    st = (M + 31) // 32 * 32
    return ws.view(torch.float32).view(17, st, 2)


@pytest.mark.parametrize("bound", [1.0, 2.0])
def test_plane_encoders_against_float64_bit_exact_on_the_edge_points(fo, tables, bound, mlp_prec):
    """hg_encode_planes, hg_encode_planes_rows, hg_encode_planes_mixed (fp16 MLP) and hg_encode_codebook_plane, with and without the pre-summed codebook, at every
    edge count: k_encode_planes shares axis_cell and trilerp with the stand-alone k_encode (csrc/hashgrid.h), which the golden vectors pin bit-exactly -- so every
    plane equals hg_encode_fwd's feature pair bit for bit (lane pairs trade corners by DPP: the same corners must arrive), the codebook plane the literal
    one-table gather, and level 15 + codebook the fused channel 30:32.  Mixed sets: levels 0..14 are the fp32 value rounded to fp16, nearest even.  Rows between
    the count and the stride are never consumed (NaN there changes nothing downstream); rows past a device row count's last tile are untouched."""
    from nerf_signature_amd import _native as nv
    base, cb, base_d, cb_d = tables
    _, sp, cp = _params(tables)
    packed = fo.pack_weights(sp, cp)
    S = fo.codebook_presum(fo.select_tables(cb_d[:64], fo.message_bits(torch.from_numpy(cf.messages(32)[2]))))
    base_ptrs = nv.ptr_array([t.detach() for t in base_d])
    for M in mr.EDGE_COUNTS:
        pts = _edge_rows(M, bound, seed=M)
        x01 = (pts + bound) / (2 * bound)
        st = (M + 31) // 32 * 32
        nbytes = int(nv.fn("hg_planes_bytes")(M))
        assert nbytes == 17 * st * 8
        clean, marked = fo.encode(x01, base_d), fo.encode(x01, base_d, S)
        cbf = fo.codebook_encode_literal(x01, [S])
        assert torch.equal(clean[:, 30:] + cbf, marked[:, 30:])
        if M == 1025:      # ... and the pinned encoder itself against a float64 trilinear blend: 7 fp32 lerps of 3 roundings each and the three 1 - w: 16 u of the largest corner
            xc = x01.cpu()
            for l, res in enumerate(fr.level_resolutions(16, 16, 2048)):
                rows_l, w_l, _ = fr.voxel_lookup(xc, res)
                corners = base[l][rows_l].double()
                err = (clean[:, 2 * l:2 * l + 2].double().cpu() - fr.trilerp(corners, w_l.double())).abs()
                assert bool((err <= 16 * fr.U32 * corners.abs().amax(dim=(1, 2)).unsqueeze(-1)).all()), (l, float(err.max()))
        for s_ in (None, S):
            ws = torch.full((nbytes // 4,), float("nan"), device="cuda").view(torch.uint8)
            nv.call("hg_encode_planes", nv.ptr(pts), M, bound, base_ptrs, nv.ptr(s_), nv.ptr(ws), nv.stream())
            pl = _f32_planes(ws, M)
            assert torch.equal(pl[:16, :M].permute(1, 0, 2).reshape(M, 32), clean), (M, "hg_encode_planes")
            if s_ is not None:
                assert torch.equal(pl[16, :M], cbf) and torch.equal(pl[15, :M] + pl[16, :M], marked[:, 30:]), M
            # a device row count inside a capacity 1.5 times larger
            cap = M + (M + 1) // 2
            big = torch.cat([pts, torch.full((cap - M, 3), float("nan"), device="cuda")])
            rows = torch.tensor([M], dtype=torch.int32, device="cuda")
            ws2 = torch.full((int(nv.fn("hg_planes_bytes")(cap)) // 4,), float("nan"), device="cuda").view(torch.uint8)
            nv.call("hg_encode_planes_rows", nv.ptr(big), cap, nv.ptr(rows), bound, base_ptrs, nv.ptr(s_), nv.ptr(ws2), nv.stream())
            pl2 = _f32_planes(ws2, cap)
            n_pl = 17 if s_ is not None else 16
            assert torch.equal(pl2[:n_pl, :M], pl[:n_pl, :M]), (M, "hg_encode_planes_rows")
            assert torch.isnan(pl2[:, st:]).all(), (M, "rows past the device count's last tile were written")
            # the rows between M and the stride are never consumed: NaN there, the same outputs
            sig, rgb = (torch.empty(M, device="cuda"), torch.empty(M, 3, device="cuda"))
            dirs = mr.case(M)[1].cuda()
            outs = []
            for poison in (False, True):
                if poison:
                    pl[:, M:] = float("nan")
                nv.call("field_fwd", nv.ptr(pts), nv.ptr(dirs), M, bound, base_ptrs, nv.ptr(s_), nv.ptr(packed), nv.ptr(sig), nv.ptr(rgb), None, None, nv.ptr(ws), fo.PLANES_F32, nv.stream())
                outs.append((sig.clone(), rgb.clone()))
            assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]) and not torch.isnan(outs[1][0]).any() and not torch.isnan(outs[1][1]).any(), M
            # the codebook level alone into a set whose base planes are there: plane 16 the same bits, the rest untouched
            if s_ is not None:
                ws3 = torch.full((nbytes // 4,), float("nan"), device="cuda").view(torch.uint8)
                nv.call("hg_encode_planes", nv.ptr(pts), M, bound, base_ptrs, None, nv.ptr(ws3), nv.stream())
                pl3 = _f32_planes(ws3, M)
                keep = pl3[:16].clone()
                nv.call("hg_encode_codebook_plane", nv.ptr(pts), M, bound, nv.ptr(S), nv.ptr(ws3), fo.PLANES_F32, None, nv.stream())
                assert torch.equal(pl3[16, :M], cbf) and torch.equal(pl3[:16, :M], keep[:, :M]), (M, "hg_encode_codebook_plane")
            if mlp_prec == "f16":
                for rows_dev in (None, rows):
                    cap_m, src = (M, pts) if rows_dev is None else (cap, big)
                    stm = (cap_m + 31) // 32 * 32
                    wm = torch.full((int(nv.fn("hg_planes_bytes")(cap_m)) // 4,), float("nan"), device="cuda").view(torch.uint8)
                    nv.call("hg_encode_planes_mixed", nv.ptr(src), cap_m, nv.ptr(rows_dev), bound, base_ptrs, nv.ptr(s_), nv.ptr(wm), nv.stream())
                    halves = wm[:15 * stm * 4].view(torch.float16).view(15, stm, 2)
                    tail = wm[15 * stm * 4:15 * stm * 4 + 2 * stm * 8].view(torch.float32).view(2, stm, 2)
                    assert torch.equal(halves[:, :M].view(torch.int16), clean[:, :30].reshape(M, 15, 2).permute(1, 0, 2).half().view(torch.int16)), (M, "mixed levels 0..14")
                    assert torch.equal(tail[0, :M], clean[:, 30:]), (M, "mixed level 15")
                    if s_ is not None:
                        assert torch.equal(tail[1, :M], cbf), (M, "mixed codebook level")
                        wm2 = wm.clone()
                        tail2 = wm2[15 * stm * 4:15 * stm * 4 + 2 * stm * 8].view(torch.float32).view(2, stm, 2)
                        tail2[1] = float("nan")
                        if rows_dev is None:
                            nv.call("hg_encode_codebook_plane", nv.ptr(src), M, bound, nv.ptr(S), nv.ptr(wm2), fo.PLANES_MIXED, None, nv.stream())
                            assert torch.equal(tail2[1, :M], cbf) and torch.equal(wm2[:15 * stm * 4], wm[:15 * stm * 4]), (M, "hg_encode_codebook_plane, mixed")
                    if rows_dev is not None:
                        words = wm[:15 * stm * 4].view(torch.int32).view(15, stm)      # (the fill is an fp32 NaN: as words, whatever a plane's element type)
                        assert bool((words[:, st:] == 0x7FC00000).all()) and torch.isnan(tail[:, st:]).all(), (M, "mixed rows past the device count")
