"""tests/mlp_ref.py -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

Float64 restatement of the two field MLPs (network_wtmk_tcnn.py:52-88,97-176: 32 -> 64 -> 1+15 and 31 pad 32 -> 64 -> 64 -> 3 pad 16, no biases,
ReLU, trunc_exp / sigmoid heads), of their backward GIVEN the ReLU masks (then a linear map of the upstream gradient: no kink ambiguity), of the
five weight gradients, of the kernels' mask words, and the error bound the GPU tests hold the kernels to.  torch float64 on the CPU; imports nothing
of the product and nothing of the oracle (tests/test_mlp_cpu.py ties it to oracle/field_ref.py and to autograd).  Matrices are [rows, width].

The bound (derived, not tuned).  One product y_r = sum_k a_k w_rk over K terms, computed with rounded operands and fp32 accumulation:
    |error| <= (u_op + K 2^-23) sum_k |a_k| |w_rk|  (+ sum_k e_k |w_rk| where the input carries an error e)
  u_op = 3 2^-16  split bf16 (hi hi + hi lo + lo hi).  bf16 keeps 8 significant bits: rounding to nearest leaves |lo| = |a - hi| <= 2^-8 |a|, and lo rounded
                to bf16 leaves a residual <= 2^-16 |a|.  Lost: the residual of each operand (2^-16 each) and the dropped lo lo (2^-8 2^-8).  (2^-16 alone would take bf16
                for a 9-bit format: tests/test_mlp_cpu.py::test_one_split_bf16_product_exceeds_two_to_the_minus_16 exhibits a product beyond it.)
  u_op = 2^-10  fp16 operands: 2^-11 for each operand;
  K 2^-23       fp32 accumulation of K terms in any order (K 2^-24), doubled once: the MFMA's internal order and rounding are not documented.
Single-layer form: the input is the kernel's own saved layer input (e = 0).  Chain form: e is carried through the layers, ReLU and the masks being
1-Lipschitz; the operand term is then taken of |a| + e.  Heads: sigma (e_h0 + 2^-20), 0.25 e_logit + 2^-20 -- 2^-20 for the exponential and the
reciprocal (1-ulp instructions, |x| 2^-24 of argument scaling), 48 times below the tighter arithmetic's operand term.  Backward seeds g sigma_clamped
and g c (1 - c): at most 3 fp32 roundings and the fp32 clamp constants, 4 2^-24 relative.  SH inputs: polynomials of degree <= 3 evaluated in fp32
with fp32 constants, at most SH_ROUNDINGS roundings, each relative to the polynomial with every term taken positive (sh4_abs).
"""
import math

import numpy as np
import torch

F64 = torch.float64
U_BF16X3, U_F16, U_ACC, HEAD = 3 * 2.0 ** -16, 2.0 ** -10, 2.0 ** -23, 2.0 ** -20
U_OP = {"bf16x3": U_BF16X3, "f16": U_F16}
SEED_U = 4 * 2.0 ** -24
SH_ROUNDINGS = 12
E15 = math.exp(15.0)
MASK_WORDS = 6                     # include/nerfsig.h FIELD_MASK_WORDS: 3 layers x 2 lane halves, 192 words per 32-row tile
EDGE_COUNTS = (1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025)
SIGMA_SEED, COLOR_SEED = 1337, 1338


def walking_count(cus=256):
    """Rows at which every MLP launch (at most 4 workgroups of 128 rows per CU) has waves that walk at least three tiles, the last tile partial."""
    return 2 * 128 * (4 * cus) + 3 * 128 + 17


def _f64(t):
    return torch.as_tensor(np.asarray(t) if isinstance(t, np.ndarray) else t).detach().cpu().to(F64)


def split_params(sigma_params, color_params):
    """The two flat tcnn vectors -> the five matrices, each [out, in] row-major, stored one after the other."""
    s, c = _f64(sigma_params).reshape(-1), _f64(color_params).reshape(-1)
    assert s.numel() == 3072 and c.numel() == 7168
    return {"W1s": s[:2048].view(64, 32), "W2s": s[2048:].view(16, 64),
            "Wc1": c[:2048].view(64, 32), "Wc2": c[2048:6144].view(64, 64), "Wc3": c[6144:].view(16, 64)}


def sh_input(dirs):
    """The direction as the SH encoding sees it: mapped to [0, 1] and back in fp32 (network_wtmk_tcnn.py:114-115): the one step that rounds."""
    d = torch.as_tensor(dirs).detach().cpu().float()
    return (((d + 1) / 2) * 2 - 1).to(F64)


def _sh_terms(x, y, z, sub):
    xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
    return [torch.full_like(x, 0.28209479177387814),
            0.4886025119029199 * y, 0.4886025119029199 * z, 0.4886025119029199 * x,
            1.0925484305920792 * xy, 1.0925484305920792 * yz, 0.31539156525252005 * sub(sub(2.0 * zz, xx), yy),
            1.0925484305920792 * xz, 0.5462742152960396 * sub(xx, yy),
            0.5900435899266435 * y * sub(3 * xx, yy), 2.890611442640554 * xy * z,
            0.4570457994644658 * y * sub(sub(4 * zz, xx), yy), 0.3731763325901154 * z * sub(sub(2 * zz, 3 * xx), 3 * yy),
            0.4570457994644658 * x * sub(sub(4 * zz, xx), yy), 1.445305721320277 * z * sub(xx, yy),
            0.5900435899266435 * x * sub(xx, 3 * yy)]


_SH_SIGN = torch.tensor([1, -1, 1, -1, 1, -1, 1, -1, 1, -1, 1, -1, 1, -1, 1, -1], dtype=F64)


def sh4(d):
    """Degree-4 real spherical harmonics of d in [-1,1]^3 (hash_encoding.py:157-183) -> [M,16] float64."""
    x, y, z = d.to(F64).unbind(-1)
    return torch.stack(_sh_terms(x, y, z, lambda a, b: a - b), dim=-1) * _SH_SIGN


def sh4_abs(d):
    """sh4 with every term taken positive: what one fp32 rounding inside the evaluation is relative to."""
    x, y, z = d.to(F64).abs().unbind(-1)
    return torch.stack(_sh_terms(x, y, z, lambda a, b: a + b), dim=-1)


def sh_bound(d):
    return SH_ROUNDINGS * 2.0 ** -24 * sh4_abs(d)


def forward(feat, dirs, W):
    """Features [M,32] and view directions [M,3] -> every intermediate.  Differentiable (torch ops only)."""
    feat = feat.to(F64)
    pre_s = feat @ W["W1s"].t()
    hs = torch.relu(pre_s)
    h = hs @ W["W2s"].t()
    sigma, geo = torch.exp(h[:, 0]), h[:, 1:]
    sh_in = sh_input(dirs)
    cin = torch.cat([sh4(sh_in), geo, torch.ones(feat.shape[0], 1, dtype=F64)], dim=-1)
    pre_1 = cin @ W["Wc1"].t()
    h1 = torch.relu(pre_1)
    pre_2 = h1 @ W["Wc2"].t()
    h2 = torch.relu(pre_2)
    logits = h2 @ W["Wc3"].t()
    return {"feat": feat, "sh_in": sh_in, "pre_s": pre_s, "hs": hs, "h": h, "sigma": sigma, "geo": geo, "cin": cin, "pre_1": pre_1, "h1": h1,
            "pre_2": pre_2, "h2": h2, "logits": logits, "rgb": torch.sigmoid(logits[:, :3])}


def signs(out):
    """[M,192] bool: pre-activation > 0 of the sigma hidden layer and the two colour hidden layers."""
    return torch.cat([out["pre_s"] > 0, out["pre_1"] > 0, out["pre_2"] > 0], dim=-1)


def seeds(g_sigma, g_rgb, sigma, rgb):
    """(d h0 [M], d logit [M,3]): d h0 = g sigma with sigma clamped to exp(+-15) (activation.py:14), d logit = g c (1 - c)."""
    g_sigma, g_rgb, sigma, rgb = (_f64(t) for t in (g_sigma, g_rgb, sigma, rgb))
    return g_sigma * sigma.clamp(1.0 / E15, E15), g_rgb * (rgb * (1.0 - rgb))


def backward(g_sigma, g_rgb, sigma, rgb, masks, W):
    """Backward with the ReLU masks GIVEN (masks [M,192] bool: sigma hidden | colour hidden 1 | colour hidden 2): every pre-activation gradient and d feature."""
    d_h0, d_logit = seeds(g_sigma, g_rgb, sigma, rgb)
    M = d_h0.shape[0]
    ms, m1, m2 = (masks[:, 64 * k:64 * k + 64].to(F64) for k in range(3))
    d_out = torch.zeros(M, 16, dtype=F64)
    d_out[:, :3] = d_logit
    d_h2 = (d_out @ W["Wc3"]) * m2
    d_h1 = (d_h2 @ W["Wc2"]) * m1
    d_cin = d_h1 @ W["Wc1"]
    d_so = torch.cat([d_h0[:, None], d_cin[:, 16:31]], dim=-1)
    d_hs = (d_so @ W["W2s"]) * ms
    return {"d_out": d_out, "d_h2": d_h2, "d_h1": d_h1, "d_cin": d_cin, "d_so": d_so, "d_hs": d_hs, "d_feat": d_hs @ W["W1s"]}


WGRAD_PAIRS = (("d_hs", "feat"), ("d_so", "hs"), ("d_h1", "cin"), ("d_h2", "h1"), ("d_out", "h2"))


def weight_grads(d, inputs):
    """The five products d^T input over the rows given -> (sigma [3072], colour [7168]) in the parameter vectors' layout."""
    g = [(_f64(d[a]).t() @ _f64(inputs[b])).reshape(-1) for a, b in WGRAD_PAIRS]
    return torch.cat(g[:2]), torch.cat(g[2:])


def weight_grad_bounds(d, inputs, u_op):
    g = [product_bound(_f64(d[a]).t(), _f64(inputs[b]), u_op).reshape(-1) for a, b in WGRAD_PAIRS]
    return torch.cat(g[:2]), torch.cat(g[2:])


# ---- the bound -----------------------------------------------------------------------------------------------------------------------------------------

def product_bound(a, wt, u_op, e_in=None):
    """Bound of |computed - exact| of a @ wt (a [M,K] the input as the reference has it, wt [K,N]); e_in [M,K]: the error the input already carries."""
    a, wt = a.abs(), wt.abs()
    c = u_op + a.shape[1] * U_ACC
    if e_in is None:
        return c * (a @ wt)
    return c * ((a + e_in) @ wt) + e_in @ wt


def forward_chain_bound(ref, W, u_op, e_feat=None):
    """Errors carried from the features (exact unless e_feat is given) to sigma and rgb: per element, of every quantity of forward()."""
    e_s = product_bound(ref["feat"], W["W1s"].t(), u_op, e_feat)
    e_h = product_bound(ref["hs"], W["W2s"].t(), u_op, e_s)
    e_cin = torch.cat([sh_bound(ref["sh_in"]), e_h[:, 1:], torch.zeros_like(e_h[:, :1])], dim=-1)
    e_1 = product_bound(ref["cin"], W["Wc1"].t(), u_op, e_cin)
    e_2 = product_bound(ref["h1"], W["Wc2"].t(), u_op, e_1)
    e_l = product_bound(ref["h2"], W["Wc3"].t(), u_op, e_2)
    return {"pre_s": e_s, "hs": e_s, "h": e_h, "geo": e_h[:, 1:], "sigma": ref["sigma"] * (e_h[:, 0] + HEAD), "cin": e_cin, "pre_1": e_1, "h1": e_1,
            "pre_2": e_2, "h2": e_2, "logits": e_l, "rgb": 0.25 * e_l[:, :3] + HEAD}


def backward_chain_bound(ref, masks, W, u_op):
    """Errors carried from the two seeds to d feature, masks given (ref: backward()'s output)."""
    ms, m1, m2 = (masks[:, 64 * k:64 * k + 64].to(F64) for k in range(3))
    e_out = SEED_U * ref["d_out"].abs()
    e_h2 = product_bound(ref["d_out"], W["Wc3"], u_op, e_out) * m2
    e_h1 = product_bound(ref["d_h2"], W["Wc2"], u_op, e_h2) * m1
    e_cin = product_bound(ref["d_h1"], W["Wc1"], u_op, e_h1)
    e_so = torch.cat([SEED_U * ref["d_so"][:, :1].abs(), e_cin[:, 16:31]], dim=-1)
    e_hs = product_bound(ref["d_so"], W["W2s"], u_op, e_so) * ms
    return {"d_out": e_out, "d_h2": e_h2, "d_h1": e_h1, "d_so": e_so, "d_hs": e_hs, "d_feat": product_bound(ref["d_hs"], W["W1s"], u_op, e_hs)}


def ratio(got, want, bound):
    """Largest |got - want| / bound; an error where the bound is 0, or a NaN, counts as infinite."""
    got, want = _f64(got), _f64(want)
    err = (got - want).abs()
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
    r = torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)
    return float(r.max()) if r.numel() else 0.0


F16_EPS, F16_TINY = 2.0 ** -11, 2.0 ** -25      # one fp16 rounding: relative, and half the subnormal spacing


def _stored(e, want, half):
    return e + F16_EPS * (want.abs() + e) + F16_TINY if half else e


def forward_layer_ratios(feat, dirs, k, W, u_op, half=False):
    """Single-layer form.  k: the kernel's own saved rows, [M, width]: hs, cin, h1, h2, sigma, rgb.  Every saved layer input against the float64 product
    of the previous SAVED input.  half: the rows were kept in fp16 -- the stored value is rounded once, and the product the kernel formed read the
    unrounded input, which the saved input is within one fp16 rounding of.  Returns {name: largest error / bound}."""
    k = {n: _f64(v) for n, v in k.items()}
    feat = _f64(feat)
    e_in = (lambda a: F16_EPS * a.abs() + F16_TINY) if half else (lambda a: None)
    out = {}
    b = product_bound(feat, W["W1s"].t(), u_op)
    out["hs"] = ratio(k["hs"], torch.relu(feat @ W["W1s"].t()), _stored(b, feat @ W["W1s"].t(), half))
    h, b = k["hs"] @ W["W2s"].t(), product_bound(k["hs"], W["W2s"].t(), u_op, e_in(k["hs"]))
    out["sigma"] = ratio(k["sigma"], torch.exp(h[:, 0]), torch.exp(h[:, 0]) * (b[:, 0] + HEAD))
    out["geo"] = ratio(k["cin"][:, 16:31], h[:, 1:], _stored(b[:, 1:], h[:, 1:], half))
    d = sh_input(dirs)
    out["sh"] = ratio(k["cin"][:, :16], sh4(d), _stored(sh_bound(d), sh4(d), half))
    out["one"] = ratio(k["cin"][:, 31], torch.ones_like(k["cin"][:, 31]), torch.zeros_like(k["cin"][:, 31]))
    for name, src, w in (("h1", "cin", "Wc1"), ("h2", "h1", "Wc2")):
        pre = k[src] @ W[w].t()
        out[name] = ratio(k[name], torch.relu(pre), _stored(product_bound(k[src], W[w].t(), u_op, e_in(k[src])), pre, half))
    logit, b = (k["h2"] @ W["Wc3"].t())[:, :3], product_bound(k["h2"], W["Wc3"].t(), u_op, e_in(k["h2"]))[:, :3]
    out["rgb"] = ratio(k["rgb"], torch.sigmoid(logit), 0.25 * b + HEAD)
    return out


def backward_layer_ratios(g_sigma, g_rgb, sigma, rgb, masks, k, W, u_op):
    """Single-layer form of the backward.  k: the kernel's saved pre-activation gradients [M, width] d_out, d_h2, d_h1, d_so, d_hs and d_feat [M,32];
    sigma, rgb, masks: what the kernel was given."""
    k = {n: _f64(v) for n, v in k.items()}
    d_h0, d_logit = seeds(g_sigma, g_rgb, sigma, rgb)
    ms, m1, m2 = (masks[:, 64 * i:64 * i + 64].to(F64) for i in range(3))
    out = {"d_logit": ratio(k["d_out"][:, :3], d_logit, SEED_U * d_logit.abs()),
           "d_out_pad": ratio(k["d_out"][:, 3:], torch.zeros_like(k["d_out"][:, 3:]), torch.zeros_like(k["d_out"][:, 3:])),
           "d_h0": ratio(k["d_so"][:, 0], d_h0, SEED_U * d_h0.abs())}
    out["d_h2"] = ratio(k["d_h2"], (k["d_out"] @ W["Wc3"]) * m2, product_bound(k["d_out"], W["Wc3"], u_op))
    out["d_h1"] = ratio(k["d_h1"], (k["d_h2"] @ W["Wc2"]) * m1, product_bound(k["d_h2"], W["Wc2"], u_op))
    out["d_geo"] = ratio(k["d_so"][:, 1:], (k["d_h1"] @ W["Wc1"])[:, 16:31], product_bound(k["d_h1"], W["Wc1"], u_op)[:, 16:31])
    out["d_hs"] = ratio(k["d_hs"], (k["d_so"] @ W["W2s"]) * ms, product_bound(k["d_so"], W["W2s"], u_op))
    out["d_feat"] = ratio(k["d_feat"], k["d_hs"] @ W["W1s"], product_bound(k["d_hs"], W["W1s"], u_op))
    return out


def band_share(ref, bounds):
    """Share of (row, hidden neuron) pairs whose reference pre-activation lies within its bound of zero: where a correct kernel may take the other side."""
    inside = torch.cat([ref[n].abs() <= bounds[n] for n in ("pre_s", "pre_1", "pre_2")], dim=-1)
    return float(inside.double().mean())


# ---- the kernels' mask words (csrc/fieldmlp.h relu_to_operand / mask_bit, csrc/field.hip: mrow = masks + tile * 192 + lane) ----------------------------
# A tile is 32 points; lane = p + 32 h holds, of point p and each layer, the 32 neurons 32 rb + row_of_reg16(h, r) (activation i = 16 rb + r);
# word [tile][layer][lane] carries their flags: bit i (split bf16), or the pairwise order of the packed fp16 operand (fp16).

def _neuron(h, i):
    rb, r = divmod(i, 16)
    return 32 * rb + (r & 3) + 8 * (r >> 2) + 4 * h


def _bit(i, arith):
    if arith == "bf16x3":
        return i
    k = (i >> 4) * 8 + ((i & 15) >> 1)
    return 16 + k if i & 1 else k


def unpack_masks(words, M, arith="bf16x3"):
    """int32 words [>= ceil(M/32) * 192] -> [M,192] bool (sigma hidden | colour hidden 1 | colour hidden 2)."""
    n_tiles = (M + 31) // 32
    w = (torch.as_tensor(words).detach().cpu().reshape(-1)[:n_tiles * 192].to(torch.int64) & 0xFFFFFFFF).view(n_tiles, 3, 2, 32)
    out = torch.zeros(n_tiles, 32, 3, 64, dtype=torch.bool)
    for h in range(2):
        for i in range(32):
            out[:, :, :, _neuron(h, i)] = ((w[:, :, h, :] >> _bit(i, arith)) & 1).bool().permute(0, 2, 1)
    return out.reshape(n_tiles * 32, 192)[:M]


def pack_masks(bits, arith="bf16x3"):
    """[M,192] bool -> int32 [ceil(M/32) * 32, 6]: the tensor field_bwd reads (rows past M: no flag set)."""
    M = bits.shape[0]
    n_tiles = (M + 31) // 32
    b = torch.zeros(n_tiles * 32, 192, dtype=torch.int64)
    b[:M] = bits.to(torch.int64)
    b = b.view(n_tiles, 32, 3, 64)
    w = torch.zeros(n_tiles, 3, 2, 32, dtype=torch.int64)
    for h in range(2):
        for i in range(32):
            w[:, :, h, :] |= b[:, :, :, _neuron(h, i)].permute(0, 2, 1) << _bit(i, arith)
    w = torch.where(w >= 2 ** 31, w - 2 ** 32, w)
    return w.to(torch.int32).reshape(n_tiles * 32, MASK_WORDS)


# ---- the seeded cases ------------------------------------------------------------------------------------------------------------------------------------

def weights():
    import closed_form as cf
    return cf.mlp_params(3072, SIGMA_SEED), cf.mlp_params(7168, COLOR_SEED)


def case(M, seed=0, bound=1.0, scaled=True):
    """Seeded inputs of M rows (fp32 tensors): positions in [-bound, bound]^3, unit directions, upstream gradients of the size an unscaled MSE seed has,
    with a few rows exactly zero and, with `scaled`, one block of rows scaled by 2^30 and one by 2^-40.  A per-row quantity is judged row by row, so
    the scaled blocks cost it nothing; a sum over the rows (a weight gradient, a scattered table row) is dominated by the 2^30 block and cannot see the
    other rows: such sums are judged with scaled=False as well (the same draws, no scaling)."""
    rng = np.random.RandomState(1000 + seed)
    pts = ((rng.rand(M, 3) * 2 - 1) * bound).astype(np.float32)
    d = rng.randn(M, 3)
    dirs = (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(np.float32)
    gs, gc = (rng.randn(M) * 1e-4).astype(np.float32), (rng.randn(M, 3) * 1e-4).astype(np.float32)
    if M >= 4 and scaled:
        n = M // 8 + 1
        for lo, s in ((M // 4, 2.0 ** 30), (M // 2, 2.0 ** -40)):
            gs[lo:lo + n] *= np.float32(s)
            gc[lo:lo + n] *= np.float32(s)
    for r in (2, 7, M - 1):
        if 0 <= r < M and M >= 3:
            gs[r], gc[r] = 0.0, 0.0
    return tuple(torch.from_numpy(a) for a in (pts, dirs, gs, gc))
