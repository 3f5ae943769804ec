"""The fused decoder's kernels (csrc/decoder_fused.hip) against the float64 restatement of tests/decoder_ref.py, layer by layer and element by element, at
tile, pair, halo and band edges.  dec_forward / dec_backward run on a workspace the test owns; the workspace is copied to the CPU and sliced with
dec_workspace_layout; every saved array is compared with the float64 value of the kernel's own saved input, and the only number asserted on is
decoder_ref's ratio (largest error / derived bound) <= 1.  The end-to-end comparison with the stock operators stays in test_gpu_render.py.

MEASURED on an MI355X: largest error / bound per quantity over all 75 cases (18 shapes, both input modes where mode 1 is accepted, both offset cases, the loss-seed case, the
permuted batches), with the layer and the case where it occurred.  All 75 are inside the bounds; no kernel defect was found.
    bce_seed     0.77     rendered input and loss seed (97, 3, 5, 5)
    xhat         0.661    layer 0, forward (2, 3, 17, 17)                    two roundings against an allowance of three
    dz           0.574    layer 8, backward (97, 3, 5, 5) mode 1             three roundings against an allowance of four
    decoded      0.561    forward (192, 3, 5, 5)
    dW           0.42     layer 5, parameter gradients (3, 3, 1, 1)          0.2 at 6x6, 0.004 at 32x32, where K 2^-23 dominates the bound
    inv          0.346    layer 3, forward (1, 3, 1, 2)
    stat_sum     0.25     layer 8, offset (2, 3, 5, 13) centre tap only
    stat_M2      0.242    layer 8, forward (192, 3, 5, 5)
    act          0.239    layer 6, forward (2, 3, 7, 9)
    bsum_dzxhat  0.216    layer 2, backward (2, 3, 23, 23) mode 0
    bsum_dz      0.182    layer 3, backward (2, 3, 23, 23) mode 1
    x            0.139    layer 0, forward (2, 1, 6, 6)                      0.06 - 0.09 for the split-bf16 layers
    gprime       0.133    layer 5, forward (2, 3, 31, 33)
    dlin_w       0.117    parameter gradients (2, 3, 32, 32)
    mean         0.0848   layer 8, rotated batch (3, 3, 5, 13)
    dlin_b       0.0796   rotated batch (3, 3, 5, 13)
    dbeta        0.0448   layer 8, parameter gradients (2, 3, 8, 8)
    grad_img     0.0312   backward (1, 3, 1, 2) mode 1
    pool         0.0307   rendered input and loss seed (97, 3, 5, 5)
    dgamma       0.03     layer 1, parameter gradients (3, 3, 1, 1)
Offset statistics, smallest |mean| / spread over the channels of x_1 .. x_7: 0.008 - 0.12 with random 3x3 weights (the zero padding spreads the outputs),
360 - 931 with the centre tap only.  One stream and two streams: every gradient bit-identical on every shape.  The whole file runs in 5 s.
"""
import ctypes
import functools

import pytest
import torch

import decoder_ref as dr

pytestmark = pytest.mark.gpu
EPS = 1e-3
NAMES = ("x", "xhat", "gprime", "dz", "act", "stat", "bsum", "minv")
SHAPE_NOTES = {
    (3, 3, 1, 1): "one pixel", (1, 3, 1, 2): "two pixels, one image", (2, 3, 4, 8): "P=32: the pair's second tile inactive", (2, 3, 3, 11): "P=33: a one-pixel tile",
    (2, 3, 7, 9): "P=63", (2, 3, 8, 8): "P=64", (2, 3, 5, 13): "P=65: a one-pixel last pair, the pair seam in mid-row",
    (2, 3, 1, 65): "a single row, 201 staged positions: the prologue's batched tail", (2, 3, 64, 1): "a single column, 66 halo rows, two bands",
    (2, 3, 17, 17): "two bands of 9 + 8", (2, 3, 23, 23): "three bands of 8 + 8 + 7, 17 tiles", (2, 3, 32, 32): "P=1024, six bands, the last of 2 rows",
    (2, 3, 31, 33): "P=1023, a last tile of 31, a last band of one row", (97, 3, 5, 5): "97 partials: the second register half", (192, 3, 5, 5): "192 partials: the cap",
    (2, 1, 6, 6): "Cin=1: layer 0's weights in LDS", (2, 8, 6, 6): "Cin=8", (2, dr.MAX_CIN_6X6, 6, 6): "the largest Cin accepted at 6x6"}
assert set(SHAPE_NOTES) == set(dr.SHAPES)
ALL = [pytest.param(s, id="x".join(map(str, s)) + ": " + SHAPE_NOTES[s]) for s in dr.SHAPES]
# input mode 1 (rendered blocks, clamp and normalisation on load) is accepted up to Cin = 8: every shape but the Cin = 25 one runs in both modes
MODES = [pytest.param(s, m, id="x".join(map(str, s)) + f" mode {m}") for s in dr.SHAPES for m in ((0, 1) if s[1] <= 8 else (0,))]


def _nv():
    from nerf_signature_amd import _native
    return _native


def _layout(shape):
    off, geom = (ctypes.c_uint64 * 72)(), (ctypes.c_uint32 * 6)()
    _nv().call("dec_workspace_layout", *shape, off, geom)
    return list(off)


def _device_params(prm):
    ps = []
    for l in range(dr.LAYERS):
        ps += [prm["w"][l], prm["gamma"][l], prm["beta"][l]]
    ps += [prm["lin_w"].view(1, 1), prm["lin_b"].view(1)]
    return [p.contiguous().cuda() for p in ps]


def _read_workspace(ws, shape):
    """The workspace on the CPU, sliced by dec_workspace_layout -> lists per layer, image layout, float64."""
    B, _, H, W = shape
    P = H * W
    npair = dr.geometry(*shape)["npair"]
    raw, off, k, n = ws.cpu(), _layout(shape), {name: [None] * dr.LAYERS for name in NAMES}, 0
    take = lambda o, count: raw[o:o + 4 * count].view(torch.float32)
    for l in range(dr.LAYERS):
        C = 64 if l < 8 else 1
        for name in NAMES:
            if name == "act" and l == 8:
                continue
            o, n = off[n], n + 1
            if name in ("stat", "bsum"):
                k[name][l] = take(o, npair * B * C * 2).double().reshape(npair, B, C, 2)
            elif name == "minv":
                k[name][l] = take(o, 2 * C).double().reshape(2, C)
            else:
                k[name][l] = dr.ws_image(take(o, B * P * C), B, H, W, C)
    k["pool"] = take(off[n], B).double()
    assert n == 71
    return k


def _grads_dict(grads):
    g = [t.cpu() for t in grads]
    return {"w": [g[3 * l].double() for l in range(9)], "gamma": [g[3 * l + 1].double() for l in range(9)], "beta": [g[3 * l + 2].double() for l in range(9)],
            "lin_w": g[27].double().reshape(()), "lin_b": g[28].double().reshape(())}


def _launch(shape, prm, img, gd, mode, side=False, train=None):
    """dec_forward + dec_backward (train: (message, temp, scale) -> dec_forward_train with the loss seed, dec_backward_train seeded by it).
    Returns the kernels' arrays (float64, image layout) and the raw fp32 outputs for bit comparisons."""
    nv = _nv()
    B, Cin, H, W = shape
    ps, im, gdev = _device_params(prm), img.contiguous().cuda(), gd.contiguous().cuda()
    nbytes = nv.fn("dec_workspace_bytes")(*shape)
    assert nbytes > 0
    ws = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    decoded, grad_img = torch.zeros(B, device="cuda"), torch.full_like(im, float("nan"))
    grads = [torch.full_like(p, float("nan")) for p in ps]
    mean = std = clamped = seed = None
    if mode == 1:
        mean, std = (ctypes.c_float * Cin)(*dr.MEAN[:Cin]), (ctypes.c_float * Cin)(*dr.STD[:Cin])
        clamped = torch.full_like(im, float("nan"))
    s = nv.stream()
    if train is not None:
        msg, temp, scale = train
        msg, seed = msg.cuda(), torch.full((B,), float("nan"), device="cuda")
        nv.call("dec_forward_train", nv.ptr(im), mean, std, nv.ptr_array(ps), B, Cin, H, W, EPS, nv.ptr(ws), nv.ptr(decoded), nv.ptr(clamped), 0, None, None,
                nv.ptr(msg), float(temp), float(scale), nv.ptr(seed), s)
        nv.call("dec_backward_train", nv.ptr(seed), nv.ptr(im), mean, std, nv.ptr_array(ps), B, Cin, H, W, nv.ptr(ws), nv.ptr_array(grads), nv.ptr(grad_img),
                0, None, None, None, s, s)
    else:
        nv.call("dec_forward", nv.ptr(im), mode, mean, std, nv.ptr_array(ps), B, Cin, H, W, EPS, nv.ptr(ws), nv.ptr(decoded), nv.ptr(clamped), s)
        second = torch.cuda.Stream() if side else None
        nv.call("dec_backward", nv.ptr(gdev), nv.ptr(im), mode, mean, std, nv.ptr_array(ps), B, Cin, H, W, nv.ptr(ws), nv.ptr_array(grads), nv.ptr(grad_img),
                s, second.cuda_stream if side else s)
        if side:
            second.synchronize()          # the caller joins the weights stream before reading the gradients
    torch.cuda.synchronize()
    k = _read_workspace(ws, shape)
    k["decoded"], k["grads"] = decoded.cpu().double(), _grads_dict(grads)
    gi = grad_img.cpu()
    k["grad_img"] = gi.double()
    raw = {"grads": [g.cpu() for g in grads], "grad_img": gi, "decoded": decoded.cpu(), "clamped": None if clamped is None else clamped.cpu(),
           "seed": None if seed is None else seed.cpu()}
    return k, raw


def _run(shape, mode=0, offset=False, side=False):
    """One GPU run and its inputs per (shape, mode, parameters), shared by the tests."""
    return _run_cached(tuple(shape), mode, offset, side)


@functools.lru_cache(maxsize=None)
def _run_cached(shape, mode, offset, side):
    prm = dr.make_params(shape[1], offset=offset)
    img, gd = dr.make_case(shape, mode=mode)
    k, raw = _launch(shape, prm, img, gd, mode, side=side)
    v, e_v = dr.input_transform(img, mode)
    return {"k": k, "raw": raw, "p64": dr.params64(prm), "img": img, "gd": gd.double(), "v": v, "e_v": e_v}


def _check(tag, ratios):
    dr.report(tag, ratios)
    assert max(ratios.values()) <= 1.0, {n: v for n, v in ratios.items() if not v <= 1.0}


@pytest.mark.parametrize("shape", ALL)
def test_fused_decoder_matches_float64_forward_per_layer(shape):
    """minv_l and the stat_l partials against the kernel's own x_l; xhat / gprime / act_l against own x_l and minv_l; x_{l+1} against own act_l and the
    weights (x_0 against the image); pool and decoded.  Every element."""
    r = _run(shape)
    _check(f"forward {shape}", dr.forward_ratios(r["k"], r["v"], r["e_v"], r["p64"], EPS))


@pytest.mark.parametrize("shape,mode", MODES)
def test_fused_decoder_matches_float64_backward_per_layer(shape, mode):
    """dz_8 and bsum_8 from the head; dz_{l-1} and bsum_{l-1} against own dz_l, xhat_l, gprime_{l-1}, minv_l and the sums, l = 8..1; the image gradient in both
    input modes (mode 1: through the normalisation and the clamp's mask)."""
    r = _run(shape, mode)
    out, _ = dr.backward_ratios(r["k"], r["v"], r["p64"], r["gd"], img=r["img"], mode=mode)
    if mode == 1:                 # layer 0 reads the transformed image: its output against the float64 transform, and the clamped copy exactly
        out.update({n: v for n, v in dr.forward_ratios(r["k"], r["v"], r["e_v"], r["p64"], EPS).items() if n == ("x", 0)})
        assert torch.equal(r["raw"]["clamped"], r["img"].clamp(0, 1))
    _check(f"backward {shape} mode {mode}", out)


@pytest.mark.parametrize("shape", ALL)
def test_fused_decoder_matches_float64_parameter_gradients(shape):
    """All 29 gradient tensors, element-wise, against the kernels' own dz, xhat and act; with weights_stream == stream and with a second stream joined before
    reading: bit-identical."""
    r, r2 = _run(shape), _run(shape, side=True)
    _, dxs = dr.backward_ratios(r["k"], r["v"], r["p64"], r["gd"])
    _check(f"parameter gradients {shape}", dr.grad_ratios(r["k"], r["v"], r["e_v"], r["p64"], r["gd"], dxs))
    for a, b in zip(r["raw"]["grads"], r2["raw"]["grads"]):
        assert torch.equal(a, b) and bool(torch.isfinite(a).all())
    assert torch.equal(r["raw"]["grad_img"], r2["raw"]["grad_img"]) and torch.equal(r["raw"]["decoded"], r2["raw"]["decoded"])


@pytest.mark.parametrize("weights", [True, "centre"], ids=["random 3x3 weights", "centre tap only"])
def test_fused_decoder_matches_float64_with_offset_statistics(weights):
    """Every hidden BatchNorm at gamma = 0.02, beta = 3: each convolution's input is about 3 with a spread of 0.02.  With random 3x3 weights the zero padding
    spreads the outputs all the same (|mean| / spread below 1 in some channel of every layer, measured); with only the centre tap of layers 1..7, positive, |mean| >> spread in every one of
    them (asserted of the inputs: >= 2^7).  The statistics bounds are relative to the spread: forward, backward and parameter gradients stay inside them."""
    shape = (2, 3, 5, 13)
    r = _run(shape, offset=weights)
    rel = []
    for l in range(1, 8):
        m, inv = dr.batch_stats(r["k"]["x"][l], 0.0)
        rel.append(float((m.abs() * inv).min()))
    print(f"[decoder] offset case, {weights}: smallest |mean| / spread over the channels of x_1..x_7: " + " ".join(f"{v:.3g}" for v in rel))
    assert weights is True or min(rel) >= 2.0 ** 7
    out = dr.forward_ratios(r["k"], r["v"], r["e_v"], r["p64"], EPS)
    b, dxs = dr.backward_ratios(r["k"], r["v"], r["p64"], r["gd"])
    _check(f"offset {shape} {weights}", {**out, **b, **dr.grad_ratios(r["k"], r["v"], r["e_v"], r["p64"], r["gd"], dxs)})


def test_fused_decoder_matches_float64_on_rendered_input_with_the_loss_seed():
    """dec_forward_train on rendered [B,H,W,3] input holding values below 0, above 1 and exactly 0 and 1, no distortion, the loss seed on, temp * decoded
    reaching +-90 (lin_w scaled): clamped_out == clamp(img) exactly; bce_seed finite and within its bound; dec_backward_train seeded by it: grad_img exactly
    0 outside [0, 1], non-zero at exactly 0 and 1, within its bound everywhere."""
    shape, temp, scale = (97, 3, 5, 5), 10.0, 0.7 * 10.0 / 97
    B = shape[0]
    prm = dr.make_params(3)
    img, _ = dr.make_case(shape, mode=1)
    assert bool((img < 0).any() and (img > 1).any() and (img == 0).any() and (img == 1).any())
    pool = _launch(shape, prm, img, torch.zeros(B), 1)[0]["pool"]          # a first pass: where the pooled values lie
    lo, hi = float(pool.min()), float(pool.max())
    prm["lin_w"] = torch.tensor([19.0 / (hi - lo)])
    prm["lin_b"] = torch.tensor([-19.0 / (hi - lo) * 0.5 * (hi + lo)])
    msg = (torch.arange(B) % 2).float()
    k, raw = _launch(shape, prm, img, torch.zeros(B), 1, train=(msg, temp, scale))
    p64, (v, e_v) = dr.params64(prm), dr.input_transform(img, 1)
    td = temp * k["decoded"]
    assert float(td.max()) >= 90 and float(td.min()) <= -90
    assert torch.equal(raw["clamped"], img.clamp(0, 1))
    assert bool(torch.isfinite(raw["seed"]).all())
    out = {("bce_seed", 8): dr.seed_ratio(raw["seed"], k["decoded"], msg, temp, scale)}
    out.update(dr.forward_ratios(k, v, e_v, p64, EPS))
    b, dxs = dr.backward_ratios(k, v, p64, raw["seed"].double(), img=img, mode=1)
    out.update(b)
    out.update(dr.grad_ratios(k, v, e_v, p64, raw["seed"].double(), dxs))
    _check(f"rendered input and loss seed {shape}", out)
    g = raw["grad_img"]
    outside = (img < 0) | (img > 1)
    assert float(g[outside].abs().max()) == 0.0
    assert bool((g[(img == 0) | (img == 1)] != 0).all())


def test_fused_decoder_matches_itself_under_a_permutation_of_the_batch():
    """Two images, one pair, one band: every sum across the batch has two terms and fp32 addition commutes, so swapping the images swaps every per-image
    output bit for bit and leaves every batch-wide one unchanged.  With more partials the order of the sums changes with the permutation and bit equality is
    not owed: three images of two pairs, rotated, are held to the per-layer bounds instead, against the float64 value of the rotated inputs."""
    shape = (2, 3, 7, 9)
    prm = dr.make_params(3)
    img, gd = dr.make_case(shape)
    perm = torch.tensor([1, 0])
    k1, raw1 = _launch(shape, prm, img, gd, 0)
    k2, raw2 = _launch(shape, prm, img[perm].contiguous(), gd[perm].contiguous(), 0)
    for name in ("x", "xhat", "gprime", "dz", "act"):
        for l in range(dr.LAYERS - (name == "act")):
            assert torch.equal(k1[name][l][perm], k2[name][l]), (name, l)
    for name in ("stat", "bsum"):
        for l in range(dr.LAYERS):
            assert torch.equal(k1[name][l][:, perm], k2[name][l]), (name, l)
    for l in range(dr.LAYERS):
        assert torch.equal(k1["minv"][l], k2["minv"][l]), l
    assert torch.equal(k1["pool"][perm], k2["pool"]) and torch.equal(raw1["decoded"][perm], raw2["decoded"]) and torch.equal(raw1["grad_img"][perm], raw2["grad_img"])
    for a, b in zip(raw1["grads"], raw2["grads"]):
        assert torch.equal(a, b)

    shape, perm = (3, 3, 5, 13), torch.tensor([2, 0, 1])
    img, gd = dr.make_case(shape)
    img, gd = img[perm].contiguous(), gd[perm].contiguous()
    k, _ = _launch(shape, prm, img, gd, 0)
    p64, (v, e_v) = dr.params64(prm), dr.input_transform(img, 0)
    out = dr.forward_ratios(k, v, e_v, p64, EPS)
    b, dxs = dr.backward_ratios(k, v, p64, gd.double())
    _check(f"rotated batch {shape}", {**out, **b, **dr.grad_ratios(k, v, e_v, p64, gd.double(), dxs)})
