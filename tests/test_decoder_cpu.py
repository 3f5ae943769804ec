"""tests/decoder_ref.py against torch autograd, its bounds against the fp32 restatement of the kernels' arithmetic and nine mutants of it, and the GPU tests'
shape list against the built library (host-only calls: no GPU here)."""
import ctypes

import pytest
import torch

import decoder_ref as dr
from mlp_ref import ratio

EPS = 1e-3


def _case(shape, mode=0, offset=False):
    prm = dr.make_params(shape[1], offset=offset)
    img, gd = dr.make_case(shape, mode=mode)
    v, e_v = dr.input_transform(img, mode)
    return prm, dr.params64(prm), img, gd, v, e_v


def _all_ratios(shape, mut=(), mode=0, offset=False):
    prm, p64, img, gd, v, e_v = _case(shape, mode, offset)
    k = dr.sim_chain(v, prm, gd, EPS, dr.geometry(*shape), img=img, mode=mode, mut=mut)
    f = dr.forward_ratios(k, v, e_v, p64, EPS)
    b, dxs = dr.backward_ratios(k, v, p64, gd.double(), img=img, mode=mode)
    return {**f, **b, **dr.grad_ratios(k, v, e_v, p64, gd.double(), dxs)}


@pytest.mark.parametrize("shape,mode", [((2, 3, 5, 13), 0), ((2, 3, 17, 17), 1), ((2, 8, 6, 6), 0)])
def test_restatement_matches_autograd(shape, mode):
    """The stock Conv2d / BatchNorm2d / GELU / AdaptiveAvgPool2d / Linear chain in float64 and its autograd == decoder_ref.reference, 1e-12 relative, on
    every intermediate and every gradient."""
    B, Cin, H, W = shape
    prm, p64, img, gd, v, _ = _case(shape, mode)
    blocks = []
    for l in range(dr.LAYERS):
        conv = torch.nn.Conv2d(p64["w"][l].shape[1], p64["w"][l].shape[0], 3, padding=1, bias=False)
        bn = torch.nn.BatchNorm2d(p64["w"][l].shape[0], eps=EPS, track_running_stats=False)
        blocks.append(torch.nn.Sequential(conv, bn, torch.nn.GELU()).double())
        with torch.no_grad():
            conv.weight.copy_(p64["w"][l]), bn.weight.copy_(p64["gamma"][l]), bn.bias.copy_(p64["beta"][l])
    lin = torch.nn.Linear(1, 1).double()
    with torch.no_grad():
        lin.weight.fill_(float(p64["lin_w"])), lin.bias.fill_(float(p64["lin_b"]))
    im = img.double().requires_grad_(True)
    a = im if mode == 0 else (im.clamp(0, 1).permute(0, 3, 1, 2) - torch.tensor([float(torch.tensor(m)) for m in dr.MEAN[:3]], dtype=dr.F64).view(1, 3, 1, 1)) / \
        torch.tensor([float(torch.tensor(s)) for s in dr.STD[:3]], dtype=dr.F64).view(1, 3, 1, 1)
    xs, zs, acts = [], [], []
    for blk in blocks:
        xs.append(blk[0](a))
        zs.append(blk[1](xs[-1]))
        a = blk[2](zs[-1])
        acts.append(a)
        for t in (xs[-1], zs[-1], a):
            t.retain_grad()
    decoded = lin(torch.nn.AdaptiveAvgPool2d(1)(a).flatten(1)).view(-1)
    decoded.backward(gd.double())
    ref = dr.reference(v, p64, gd.double(), EPS, img=img, mode=mode)

    def close(got, want, what):
        scale = float(want.abs().max())
        assert float((got - want).abs().max()) <= 1e-12 * max(scale, 1e-300), what
    close(decoded.detach(), ref["decoded"], "decoded")
    close(im.grad, ref["grad_img"], "grad_img")
    for l, blk in enumerate(blocks):
        close(xs[l].detach(), ref["x"][l], ("x", l))
        close(acts[l].detach(), ref["act"][l], ("act", l))
        close(xs[l].grad, ref["dx"][l], ("dx", l))
        close(blk[0].weight.grad, ref["grads"]["w"][l], ("dW", l))
        close(blk[1].weight.grad, ref["grads"]["gamma"][l], ("dgamma", l))
        close(blk[1].bias.grad, ref["grads"]["beta"][l], ("dbeta", l))
        m, inv = dr.batch_stats(xs[l].detach(), EPS)
        close(torch.stack([m, inv]), ref["minv"][l], ("minv", l))
        c4 = lambda t: t.view(1, -1, 1, 1)
        close(ref["xhat"][l] * c4(p64["gamma"][l]) + c4(p64["beta"][l]), zs[l].detach(), ("xhat", l))          # z = gamma xhat + beta is BatchNorm2d's output
        close(ref["dz"][l], zs[l].grad, ("dz", l))
        close(ref["gprime"][l] * acts[l].grad, zs[l].grad, ("gprime", l))
        close(ref["bsum"][l][..., 0].sum(dim=(0, 1)), blk[1].bias.grad, ("bsum dz", l))
        close(ref["bsum"][l][..., 1].sum(dim=(0, 1)), blk[1].weight.grad, ("bsum dz xhat", l))
        # the forward partials: the sums add up to N mean, and M2_i + n_i (mean_i - mean)^2 to N var
        n_i = torch.tensor([min(64, H * W - 64 * p) for p in range(ref["stat"][l].shape[0])], dtype=dr.F64).view(-1, 1, 1)
        st = ref["stat"][l]
        close(st[..., 0].sum(dim=(0, 1)) / (B * H * W), m, ("stat sum", l))
        var = (st[..., 1] + n_i * (st[..., 0] / n_i - m) ** 2).sum(dim=(0, 1)) / (B * H * W)
        close(1.0 / torch.sqrt(var + EPS), inv, ("stat M2", l))
    close(lin.weight.grad.view(()), ref["grads"]["lin_w"], "dlin_w")
    close(lin.bias.grad.view(()), ref["grads"]["lin_b"], "dlin_b")
    if mode == 1:
        seed = dr.bce_seed(ref["decoded"], torch.ones(B, dtype=dr.F64), 10.0, 0.7)
        d = ref["decoded"].clone().requires_grad_(True)
        (0.7 / 10.0 * B * torch.nn.functional.binary_cross_entropy_with_logits(10.0 * d, torch.ones(B, dtype=dr.F64))).backward()
        close(seed, d.grad, "bce_seed")


@pytest.mark.parametrize("shape", dr.SHAPES)
def test_kernel_arithmetic_lies_inside_every_bound(shape):
    """The fp32 restatement of the kernels' arithmetic (split-bf16 products, tile / pair / group statistics, A&S GELU) is inside every single-layer bound."""
    r = _all_ratios(shape)
    dr.report(f"cpu restatement {shape}", r)
    assert max(r.values()) <= 1.0, {n: v for n, v in r.items() if v > 1.0}


def test_kernel_arithmetic_inside_bounds_mode1_and_offset():
    for kw in (dict(mode=1), dict(offset=True), dict(offset="centre")):
        r = _all_ratios((2, 3, 5, 13), **kw)
        dr.report(f"cpu restatement (2, 3, 5, 13) {kw}", r)
        assert max(r.values()) <= 1.0, {n: v for n, v in r.items() if v > 1.0}


def _offset_stats(mut):
    """Layer-3 statistics of x with |mean| / spread = 2^8 per channel: (ratio of the mean, of inv)."""
    g = torch.Generator().manual_seed(77)
    s = torch.rand(64, generator=g).view(1, 64, 1, 1) + 0.5
    x32 = (256.0 * s + s * torch.randn(2, 64, 5, 13, generator=g)).float()
    part = dr.sim_partials(x32, 3)
    m, inv = dr.sim_stats(x32, part, 3, EPS, frozenset(mut))
    x = x32.double()
    e_s, e_M2 = dr.partial_bounds(x, 3)
    want = dr.pair_partials(x)
    assert ratio(part[..., 0].double(), want[..., 0], e_s) <= 1 and ratio(part[..., 1].double(), want[..., 1], e_M2) <= 1
    wm, winv = dr.batch_stats(x, EPS)
    e_m, e_inv = dr.stats_bounds(x, 3, EPS)
    return ratio(m.double(), wm, e_m), ratio(inv.double(), winv, e_inv)


# mutant -> (what it is, shapes tried in order, input mode)
MUTANTS = {
    "lohi": ("(a) the lo hi product dropped", [(2, 3, 4, 8)], 0),
    "halo": ("(b) a pair's halo row beyond its own pixels read as zero", [(2, 3, 8, 8), (2, 3, 5, 13)], 0),
    "count": ("(c) the last pair's count taken as 64 in the statistics merge", [(2, 3, 8, 8), (2, 3, 3, 11)], 0),
    "noflip": ("(d) taps not flipped in the data gradient", [(2, 3, 4, 8)], 0),
    "band": ("(e) a weight-gradient band without the neighbouring band's activation row", [(2, 3, 8, 8), (2, 3, 64, 1)], 0),
    "stride": ("(f) a halo-linear row stride of W instead of W + 2", [(2, 3, 4, 8)], 0),
    "gelu": ("(g) GELU' without its z phi(z) term", [(2, 3, 4, 8)], 0),
    "mask": ("(i) the clamp mask missing from the image gradient", [(2, 3, 4, 8)], 1),
}


@pytest.mark.parametrize("mut", sorted(MUTANTS))
def test_each_mutant_exceeds_a_bound(mut):
    """Each mutant of the restatement exceeds a bound on a listed shape (the first of its list that has the edge it needs: (8, 8) is a single whole pair and a
    single band, where (b), (c) and (e) change nothing and must pass)."""
    what, shapes, mode = MUTANTS[mut]
    for shape in shapes:
        assert shape in dr.SHAPES
        r = _all_ratios(shape, mut={mut}, mode=mode)
        worst = max(r, key=r.get)
        if r[worst] > 1.0:
            print(f"[decoder] mutant {what}: killed on {shape} by {worst[0]}[{worst[1]}] at ratio {r[worst]:.3g}")
            assert shape == shapes[-1], "a shape without the mutant's edge must not see it"
            return
        print(f"[decoder] mutant {what}: not visible on {shape} (largest ratio {r[worst]:.3g})")
    pytest.fail(f"mutant {what} stayed inside every bound on {shapes}")


def test_variance_mutant_dies_on_the_offset_case():
    """(h) variance as E[x^2] - E[x]^2 at |mean| / spread = 2^8: the kernels' pipeline is inside the spread-relative bound, the mutant is not."""
    m, inv = _offset_stats(())
    mm, minv = _offset_stats({"ex2"})
    print(f"[decoder] offset statistics (mean/spread 2^8): mean {m:.3g} inv {inv:.3g}; mutant (h) E[x^2]-E[x]^2: mean {mm:.3g} inv {minv:.3g}")
    assert m <= 1 and inv <= 1 and minv > 1


# ---- the shape list against the built library ----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def native():
    from nerf_signature_amd import build, _native
    build.build()
    return _native


def layout(native, shape):
    off, geom = (ctypes.c_uint64 * 72)(), (ctypes.c_uint32 * 6)()
    native.call("dec_workspace_layout", *shape, off, geom)
    return list(off), dict(zip(("ntile", "npair", "rows_max", "nband", "R", "RS"), geom))


def test_shape_list_is_legal_and_reaches_its_edges(native):
    wb = native.fn("dec_workspace_bytes")
    geo = {}
    for s in dr.SHAPES:
        assert wb(*s) > 0, s
        geo[s] = layout(native, s)[1]
        assert geo[s] == dr.geometry(*s), s                      # the restatement's group sizes are the library's
    bands = {s: (g["nband"], s[2] - (g["nband"] - 1) * g["R"]) for s, g in geo.items()}       # (bands, rows of the last one)
    assert bands[(2, 3, 64, 1)] == (2, 32) and geo[(2, 3, 64, 1)]["rows_max"] == 66
    assert bands[(2, 3, 17, 17)] == (2, 8) and geo[(2, 3, 17, 17)]["R"] == 9                  # 9 + 8
    assert bands[(2, 3, 23, 23)] == (3, 7) and geo[(2, 3, 23, 23)]["ntile"] == 17             # 8 + 8 + 7, an odd tile count
    assert bands[(2, 3, 32, 32)] == (6, 2) and geo[(2, 3, 32, 32)]["npair"] == 16
    assert bands[(2, 3, 31, 33)] == (6, 1) and 31 * 33 - 32 * (geo[(2, 3, 31, 33)]["ntile"] - 1) == 31
    for s in ((2, 3, 1, 65), (2, 3, 64, 1)):                     # more staged positions than the preloaded batch: the prologue's batched tail runs
        assert geo[s]["rows_max"] * (s[3] + 2) * 16 > 2048 and geo[s]["rows_max"] * (s[3] + 2) in (201, 198)
    assert [geo[s]["ntile"] for s in ((2, 3, 4, 8), (2, 3, 3, 11), (2, 3, 7, 9), (2, 3, 8, 8), (2, 3, 5, 13))] == [1, 2, 2, 2, 3]
    assert 97 * geo[(97, 3, 5, 5)]["npair"] == 97 and 192 * geo[(192, 3, 5, 5)]["npair"] == 192
    for s in ((193, 3, 5, 5), (2, 3, 4, 200), (2, 3, 8, 126)):
        assert wb(*s) == 0, s
        with pytest.raises(ValueError, match="unsupported image shape"):
            layout(native, s)


def test_supported_shapes_are_what_the_header_lists(native):
    """dec_workspace_bytes accepts exactly the shapes the header's list describes (decoder_ref.supported restates it): every H x W up to 1024 pixels and
    beyond, every Cin from 1 to 33; the batch limits at 5x5 and 9x9; the largest Cin at the sizes the header quotes, found by search."""
    wb = native.fn("dec_workspace_bytes")
    sizes = [(H, W) for H in range(1, 1030) for W in range(1, 1030 // H + 1)]
    wrong = [(2, c, H, W) for H, W in sizes for c in range(1, 34) if (wb(2, c, H, W) > 0) != dr.supported(2, c, H, W)]
    assert not wrong, wrong[:10]
    wrong = [(b, 3, n, n) for n in (1, 5, 9) for b in range(0, 200) if (wb(b, 3, n, n) > 0) != dr.supported(b, 3, n, n)]
    assert not wrong, wrong[:10]
    largest = {hw: max(c for c in range(1, 65) if wb(2, c, *hw)) for hw in ((6, 6), (12, 12), (16, 16), (24, 24), (32, 32))}
    assert largest == {(6, 6): dr.MAX_CIN_6X6, (12, 12): 23, (16, 16): 23, (24, 24): 20, (32, 32): 12}
    assert (2, dr.MAX_CIN_6X6, 6, 6) in dr.SHAPES and wb(2, 0, 6, 6) == 0
