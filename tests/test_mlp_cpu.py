"""tests/mlp_ref.py proven without a GPU: the float64 restatement against the fp32 oracle (oracle/field_ref.py) and against float64 autograd of its
own forward; an fp32 NumPy restatement of the kernels' arithmetic (split bf16 with lo x lo dropped / fp16 operands, fp32 accumulation in k-steps
of 16) lies inside the single-layer and the chain bound on every seeded case -- the bound is attainable -- and seven mutants of that restatement
each break it -- the bound bites; the mask words round-trip; the share of pre-activations inside the bound's band around zero stays under its cap."""
import numpy as np
import pytest
import torch

import closed_form as cf
import mlp_ref as mr
from oracle import field_ref as fr

CPU_COUNTS = mr.EDGE_COUNTS + (mr.walking_count(8),)      # (the tile walk is a property of the launch, not of the arithmetic: a small walking count here)


@pytest.fixture(scope="module")
def tables():
    return [torch.from_numpy(cf.table(l)) for l in range(16)]


@pytest.fixture(scope="module")
def W():
    return mr.split_params(*mr.weights())


@pytest.fixture(scope="module")
def cases(tables):
    """{M: (feat fp32 [M,32], dirs, gs, gc, the same gradients without the scaled blocks)}: the features the oracle's encoder gives for the seeded positions."""
    out = {}
    for M in CPU_COUNTS:
        pts, dirs, gs, gc = mr.case(M)
        out[M] = (fr.base_encode((pts + 1) / 2, tables), dirs, gs, gc, mr.case(M, scaled=False)[2:])
    return out


# ---- the kernels' arithmetic, restated in NumPy fp32 ---------------------------------------------------------------------------------------------------

def _bf16(a):
    b = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    return (((b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)).view(np.float32)


def emu_product(a, w, arith, drop_lo_hi=False, skip_kstep=None):
    """a [M,K] fp32 (the B operand: activations), w [N,K] fp32 (the A operand: weights) -> a @ w^T as csrc/fieldmlp.h mac() forms it."""
    a, w = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(w, np.float32)
    acc = np.zeros((a.shape[0], w.shape[0]), np.float32)
    for ks in range(a.shape[1] // 16):
        if ks == skip_kstep:
            continue
        x, y = a[:, 16 * ks:16 * ks + 16], w[:, 16 * ks:16 * ks + 16]
        if arith == "f16":
            terms = [(x.astype(np.float16), y.astype(np.float16))]
        else:
            xh, yh = _bf16(x), _bf16(y)
            xl, yl = _bf16(x - xh), _bf16(y - yh)
            terms = [(xh, yl), (xl, yh), (xh, yh)]          # w_lo x_hi, w_hi x_lo, w_hi x_hi
            if drop_lo_hi:
                del terms[1]
        for p, q in terms:
            acc = (acc.astype(np.float64) + p.astype(np.float64) @ q.astype(np.float64).T).astype(np.float32)
    return acc


def _np_params():
    sp, cp = mr.weights()
    return {"W1s": sp[:2048].reshape(64, 32), "W2s": sp[2048:].reshape(16, 64), "Wc1": cp[:2048].reshape(64, 32),
            "Wc2": cp[2048:6144].reshape(64, 64), "Wc3": cp[6144:].reshape(16, 64)}


def emu_forward(feat, dirs, arith="bf16x3", mutant=None):
    P = _np_params()
    kw = lambda layer: {"drop_lo_hi": mutant == "lo_hi", "skip_kstep": 1 if mutant == f"kstep_{layer}" else None}
    feat = feat.numpy()
    pre_s = emu_product(feat, P["W1s"], arith, **kw("s"))
    hs = np.maximum(pre_s, 0)
    h = emu_product(hs, P["W2s"], arith, **kw("h"))
    d = dirs.numpy()
    sh = fr.sh4(torch.from_numpy((d + np.float32(1)) / np.float32(2) * np.float32(2) - np.float32(1))).numpy()      # fp32, as the kernel evaluates it
    geo = h[:, 1:16] if mutant != "geo_offset" else h[:, 0:15]
    cin = np.concatenate([sh, geo, np.ones((feat.shape[0], 1), np.float32)], axis=1)
    pre_1 = emu_product(cin, P["Wc1"], arith, **kw("1"))
    h1 = np.maximum(pre_1, 0)
    pre_2 = emu_product(h1, P["Wc2"], arith, **kw("2"))
    h2 = np.maximum(pre_2, 0)
    logits = emu_product(h2, P["Wc3"], arith, **kw("l"))
    out = {"hs": hs, "cin": cin, "h1": h1, "h2": h2, "sigma": np.exp(h[:, 0]), "geo": h[:, 1:16], "rgb": 1 / (1 + np.exp(-logits[:, :3])),
           "masks": np.concatenate([pre_s > 0, pre_1 > 0, pre_2 > 0], axis=1)}
    if mutant == "lane_pair":      # rows p and p ^ 1 of every tile exchanged (an odd last row keeps its place)
        M = feat.shape[0]
        perm = np.arange(M) ^ 1
        perm[perm >= M] = M - 1
        out = {n: v[perm] for n, v in out.items()}
    return {n: torch.from_numpy(np.ascontiguousarray(v)) for n, v in out.items()}


def emu_backward(gs, gc, sigma, rgb, masks, arith="bf16x3", mutant=None):
    P = _np_params()
    kw = {"drop_lo_hi": mutant == "lo_hi"}
    gs, gc, sigma, rgb, m = gs.numpy(), gc.numpy(), sigma.numpy().astype(np.float32), rgb.numpy().astype(np.float32), masks.numpy().copy()
    if mutant == "mask_swap":
        m[:, [64 + 5, 64 + 6]] = m[:, [64 + 6, 64 + 5]]
    M = gs.shape[0]
    d_out = np.zeros((M, 16), np.float32)
    d_out[:, :3] = gc * (rgb * (np.float32(1) - rgb))
    clamped = sigma if mutant == "no_clamp" else np.minimum(np.maximum(sigma, np.exp(np.float32(-15))), np.exp(np.float32(15)))
    d_h0 = gs * clamped
    d_h2 = emu_product(d_out, P["Wc3"].T, arith, **kw) * m[:, 128:192]
    d_h1 = emu_product(d_h2, P["Wc2"].T, arith, **kw) * m[:, 64:128]
    d_cin = emu_product(d_h1, P["Wc1"].T, arith, **kw)
    d_so = np.concatenate([d_h0[:, None], d_cin[:, 16:31]], axis=1).astype(np.float32)
    d_hs = emu_product(d_so, P["W2s"].T, arith, **kw) * m[:, 0:64]
    d_feat = emu_product(d_hs, P["W1s"].T, arith, **kw)
    return {n: torch.from_numpy(np.ascontiguousarray(v, np.float32)) for n, v in
            (("d_out", d_out), ("d_h2", d_h2), ("d_h1", d_h1), ("d_so", d_so), ("d_hs", d_hs), ("d_feat", d_feat))}


def emu_wgrad(d, inputs, stale=False):
    """The five K = points products in 32-point k-steps' worth of split bf16 (two 16-wide steps).  stale: the rows of the last tile past the live
    count keep the previous tile's values instead of contributing nothing."""
    out = []
    for a, b in mr.WGRAD_PAIRS:
        x, y = d[a].numpy().astype(np.float32), inputs[b].numpy().astype(np.float32)
        M = x.shape[0]
        pad = -M % 32
        if pad:
            fill = (lambda v: v[np.arange(M, M + pad) - 32] if M >= 32 else np.repeat(v[:1], pad, 0)) if stale else (lambda v: np.zeros((pad, v.shape[1]), np.float32))
            x, y = np.concatenate([x, fill(x)]), np.concatenate([y, fill(y)])
        out.append(torch.from_numpy(emu_product(x.T, y.T, "bf16x3")).reshape(-1))
    return torch.cat(out[:2]), torch.cat(out[2:])


def _worst(ratios):
    return max(ratios.values())


def _chain_ratios(feat, dirs, got, W, u_op):
    ref = mr.forward(feat, dirs, W)
    b = mr.forward_chain_bound(ref, W, u_op)
    return {n: mr.ratio(got[n], ref[n], b[n]) for n in ("sigma", "geo", "rgb", "hs", "h1", "h2")}


# ---- the reference against the oracle and autograd --------------------------------------------------------------------------------------------------------

def test_reference_agrees_with_the_fp32_oracle(tables, W):
    """field_ref.field_forward / density / color evaluate the same network in fp32: they lie inside the chain bound with exact operands (u_op = 0: what is
    left is fp32 accumulation), from the very features the oracle's encoder produced.  The oracle stays the check of the restated parameter layout."""
    sp, cp = (torch.from_numpy(p) for p in mr.weights())
    P = {"bound": 1.0, "base_tables": tables, "cb_tables": [], "sigma_params": sp, "color_params": cp}
    assert [tuple(m.shape) for m in fr.split_mlp_params(sp, fr.SIGMA_WIDTHS) + fr.split_mlp_params(cp, fr.COLOR_WIDTHS)] == [tuple(W[n].shape) for n in ("W1s", "W2s", "Wc1", "Wc2", "Wc3")]
    for n, m in zip(("W1s", "W2s", "Wc1", "Wc2", "Wc3"), fr.split_mlp_params(sp, fr.SIGMA_WIDTHS) + fr.split_mlp_params(cp, fr.COLOR_WIDTHS)):
        assert torch.equal(W[n], m.double())
    pts, dirs, _, _ = mr.case(4096, seed=3)
    with torch.no_grad():
        s0, c0 = fr.field_forward(pts, dirs, None, P)
        dn = fr.density(pts, None, P)
        c1 = fr.color(dirs, dn["geo_feat"], P)
    ref = mr.forward(fr.base_encode((pts + 1) / 2, tables), dirs, W)
    b = mr.forward_chain_bound(ref, W, 0.0)
    worst = {"sigma": mr.ratio(s0, ref["sigma"], b["sigma"]), "density": mr.ratio(dn["sigma"], ref["sigma"], b["sigma"]), "geo": mr.ratio(dn["geo_feat"], ref["geo"], b["geo"]),
             "rgb": mr.ratio(c0, ref["rgb"], b["rgb"]), "color": mr.ratio(c1, ref["rgb"], b["rgb"])}
    print(f"\nfp32 oracle inside the exact-operand chain bound: {worst}")
    assert _worst(worst) <= 1.0, worst
    assert float((s0.double() / ref["sigma"] - 1).abs().max()) < 1e-5 and float((c0.double() - ref["rgb"]).abs().max()) < 1e-6      # fp32 round-off, in plain numbers


def test_backward_given_masks_equals_float64_autograd(cases, W):
    """Masks = the signs: the explicit backward equals autograd of forward() -- every pre-activation gradient, d feature and the five weight gradients --
    on rows without a pre-activation of exactly 0 (where autograd's ReLU subgradient is a convention)."""
    feat, dirs, gs, gc, _ = cases[1025]
    Wg = {n: m.clone().requires_grad_(True) for n, m in W.items()}
    x = feat.double().requires_grad_(True)
    out = mr.forward(x, dirs, Wg)
    for n in ("pre_s", "h", "pre_1", "pre_2", "logits"):
        out[n].retain_grad()
    # trunc_exp's derivative is exp inside +-15: the suite's weights keep h0 there, so plain autograd is the same function
    assert float(out["h"][:, 0].detach().abs().max()) < 15
    ((out["sigma"] * gs.double()).sum() + (out["rgb"] * gc.double()).sum()).backward()
    keep = ~(torch.cat([out["pre_s"], out["pre_1"], out["pre_2"]], dim=-1) == 0).any(dim=-1)
    assert int(keep.sum()) >= 1000
    det = {n: v.detach() for n, v in out.items()}
    got = mr.backward(gs, gc, det["sigma"], det["rgb"], mr.signs(det), W)
    for mine, theirs in (("d_out", out["logits"].grad), ("d_h2", out["pre_2"].grad), ("d_h1", out["pre_1"].grad), ("d_so", out["h"].grad), ("d_hs", out["pre_s"].grad), ("d_feat", x.grad)):
        scale = float(theirs[keep].abs().max())
        assert float((got[mine][keep] - theirs[keep]).abs().max()) <= 1e-12 * scale, mine
    assert bool(keep.all())      # (no exact zero among the seeded rows: the weight gradients below are over all of them)
    g_s, g_c = mr.weight_grads(got, det)
    want_s, want_c = torch.cat([Wg["W1s"].grad.reshape(-1), Wg["W2s"].grad.reshape(-1)]), torch.cat([Wg[n].grad.reshape(-1) for n in ("Wc1", "Wc2", "Wc3")])
    assert float((g_s - want_s).abs().max()) <= 1e-12 * float(want_s.abs().max()) and float((g_c - want_c).abs().max()) <= 1e-12 * float(want_c.abs().max())
    assert float(g_c[6144 + 3 * 64:].abs().max()) == 0.0


def test_trunc_exp_clamp_in_the_reference_backward():
    """d h0 = g sigma inside exp(+-15), g exp(+-15) beyond (activation.py:14)."""
    sigma = torch.tensor([1e-9, 1.0, 1e9], dtype=torch.float64)
    d_h0, _ = mr.seeds(torch.ones(3), torch.zeros(3, 3), sigma, torch.full((3, 3), 0.5))
    assert torch.equal(d_h0, torch.tensor([1 / mr.E15, 1.0, mr.E15], dtype=torch.float64))


@pytest.mark.parametrize("arith", ["bf16x3", "f16"])
def test_mask_words_round_trip(arith):
    rng = np.random.RandomState(5)
    for M in (1, 31, 33, 257):
        bits = torch.from_numpy(rng.rand(M, 192) < 0.5)
        words = mr.pack_masks(bits, arith)
        assert words.shape == ((M + 31) // 32 * 32, mr.MASK_WORDS) and words.dtype == torch.int32
        assert torch.equal(mr.unpack_masks(words, M, arith), bits)
    one = torch.zeros(33, 192, dtype=torch.bool)
    one[32, 64 + 37] = True      # point 0 of tile 1, colour hidden layer 1, neuron 37 = 32 + row_of_reg16(h = 1, r = 1): lane 32, activation i = 17
    w = mr.pack_masks(one, arith).reshape(-1)
    assert int((w != 0).sum()) == 1 and int(w[192 + 64 + 32]) == 1 << (17 if arith == "bf16x3" else 16 + 8)


# ---- the bound is attainable and bites -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("arith", ["bf16x3", "f16"])
def test_restated_kernel_arithmetic_lies_inside_both_bounds_on_every_case(cases, W, arith):
    u = mr.U_OP[arith]
    worst = {}
    for M, (feat, dirs, gs, gc, plain) in cases.items():
        got = emu_forward(feat, dirs, arith)
        r = dict(mr.forward_layer_ratios(feat, dirs, got, W, u))
        r.update({"chain_" + n: v for n, v in _chain_ratios(feat, dirs, got, W, u).items()})
        if arith == "bf16x3":      # (the fp16 backward normalises every point by a power of two and is held to no bound on the GPU: forward only)
            sigma = got["sigma"].clone()
            if M >= 8:
                sigma[1], sigma[3] = 1e9, 1e-9       # beyond the clamp of the derivative on either side
            back = emu_backward(gs, gc, sigma, got["rgb"], got["masks"], arith)
            r.update(mr.backward_layer_ratios(gs, gc, sigma, got["rgb"], got["masks"], back, W, u))
            ref = mr.backward(gs, gc, sigma, got["rgb"], got["masks"], W)
            bb = mr.backward_chain_bound(ref, got["masks"], W, u)
            r.update({"chain_" + n: mr.ratio(back[n], ref[n], bb[n]) for n in bb})
            inputs = dict(got, feat=feat)
            g_s, g_c = emu_wgrad(back, inputs)
            want_s, want_c = mr.weight_grads(back, inputs)
            b_s, b_c = mr.weight_grad_bounds(back, inputs, u)
            r.update({"wgrad_sigma": mr.ratio(g_s, want_s, b_s), "wgrad_colour": mr.ratio(g_c, want_c, b_c)})
            back = emu_backward(*plain, sigma, got["rgb"], got["masks"], arith)      # sums over the rows: also without the 2^30 block that dominates them
            g_s, g_c = emu_wgrad(back, inputs)
            want_s, want_c = mr.weight_grads(back, inputs)
            b_s, b_c = mr.weight_grad_bounds(back, inputs, u)
            r.update({"wgrad_sigma_plain": mr.ratio(g_s, want_s, b_s), "wgrad_colour_plain": mr.ratio(g_c, want_c, b_c)})
        for n, v in r.items():
            worst[n] = max(worst.get(n, 0.0), v)
        assert _worst(r) <= 1.0, (M, r)
    print(f"\n[{arith}] restated arithmetic, largest error / bound over {len(cases)} cases: " + ", ".join(f"{n} {v:.3f}" for n, v in worst.items()))
    assert max(v for n, v in worst.items() if n not in ("one", "d_out_pad")) > 1e-3      # the bound is not vacuous: honest arithmetic uses a visible part of it


MUTANTS = ["lo_hi", "kstep_1", "mask_swap", "lane_pair", "stale_rows", "geo_offset", "no_clamp"]


@pytest.mark.parametrize("mutant", MUTANTS)
def test_every_mutant_of_the_restated_arithmetic_breaks_the_bound(cases, W, mutant):
    """Each restated mistake leaves the single-layer bound on at least one seeded case (split bf16, the sharp arithmetic).  The stale rows of a partial
    tile are judged on the gradients without the scaled blocks (a sum over the rows: mlp_ref.case) and must be caught at EVERY edge count with a partial tile."""
    u = mr.U_BF16X3
    caught = []
    for M, (feat, dirs, gs, gc, plain) in cases.items():
        good = emu_forward(feat, dirs)
        got = emu_forward(feat, dirs, mutant=mutant)
        sigma = good["sigma"].clone()
        if M >= 8:
            sigma[1], sigma[3] = 1e9, 1e-9
        if mutant == "lane_pair":        # the outputs land on the neighbouring row: against the reference of the row they claim to be
            ref = mr.forward(feat, dirs, W)
            b = mr.forward_chain_bound(ref, W, u)
            r = {n: mr.ratio(got[n], ref[n], b[n]) for n in ("sigma", "rgb", "geo")}
        elif mutant in ("lo_hi", "kstep_1", "geo_offset"):
            r = mr.forward_layer_ratios(feat, dirs, got, W, u)
        elif mutant in ("mask_swap", "no_clamp"):
            back = emu_backward(gs, gc, sigma, good["rgb"], good["masks"], mutant=mutant)
            r = mr.backward_layer_ratios(gs, gc, sigma, good["rgb"], good["masks"], back, W, u)
        else:
            back = emu_backward(*plain, sigma, good["rgb"], good["masks"])
            inputs = dict(good, feat=feat)
            g_s, g_c = emu_wgrad(back, inputs, stale=True)
            want_s, want_c = mr.weight_grads(back, inputs)
            b_s, b_c = mr.weight_grad_bounds(back, inputs, u)
            r = {"wgrad_sigma": mr.ratio(g_s, want_s, b_s), "wgrad_colour": mr.ratio(g_c, want_c, b_c)}
        if _worst(r) > 1.0:
            caught.append(M)
    print(f"\nmutant {mutant}: caught on {len(caught)} of {len(cases)} cases {caught}")
    assert caught, mutant
    if mutant == "stale_rows":
        assert [M for M in mr.EDGE_COUNTS if M % 32] == [M for M in caught if M in mr.EDGE_COUNTS], caught


def test_one_split_bf16_product_exceeds_two_to_the_minus_16():
    """Why u_op is 3 2^-16 and not 2^-16: bf16 keeps 8 significant bits, so hi hi + hi lo + lo hi loses each operand's split residual (up to 2^-16) and lo lo
    (up to 2^-8 2^-8).  One product a w of the restated arithmetic, both operands just above a bf16 rounding tie, is off by more than 2^-16 |a w| -- and by
    less than 3 2^-16 |a w|."""
    v = np.float32(1 + 2.0 ** -8 - 2.0 ** -16 - 2.0 ** -17)       # hi = 1 + 2^-7, lo ~ -2^-8: the largest lo, and a residual left by its own rounding
    a = np.zeros((1, 16), np.float32)
    a[0, 0] = v
    got = float(emu_product(a, a, "bf16x3")[0, 0])
    rel = abs(got - float(v) ** 2) / float(v) ** 2
    print(f"\none split-bf16 product: relative error {rel / 2.0 ** -16:.3f} x 2^-16")
    assert 2.0 ** -16 < rel < mr.U_BF16X3


def test_band_share_stays_under_its_cap(tables, W):
    """The share of (row, neuron) pairs whose float64 pre-activation lies within the bound of zero -- where a correct kernel may flag the other side --
    is at most 1 %, from the reference alone: single-layer band (what the GPU mask check uses) and the wider chain band, split bf16, 4096 seeded points."""
    pts, dirs, _, _ = mr.case(4096, seed=3)
    ref = mr.forward(fr.base_encode((pts + 1) / 2, tables), dirs, W)
    single = {"pre_s": mr.product_bound(ref["feat"], W["W1s"].t(), mr.U_BF16X3), "pre_1": mr.product_bound(ref["cin"], W["Wc1"].t(), mr.U_BF16X3),
              "pre_2": mr.product_bound(ref["h1"], W["Wc2"].t(), mr.U_BF16X3)}
    chain = mr.forward_chain_bound(ref, W, mr.U_BF16X3)
    s, c = mr.band_share(ref, single), mr.band_share(ref, chain)
    print(f"\nband share, split bf16: single-layer {100 * s:.3f} %, chain {100 * c:.3f} %")
    assert s <= c <= 0.01
