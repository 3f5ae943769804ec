"""tests/decoder_ref.py -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

Float64 restatement of the HiDDeN message decoder that csrc/decoder_fused.hip computes (hidden_models.py:104-137: ConvBNRelu(Cin,64), 7 x ConvBNRelu(64,64),
ConvBNRelu(64,1), average pool, Linear(1,1); BatchNorm with batch statistics, GELU in the erf form, no conv bias), one function per step, each taking the
kernel's own saved input; the per-element error bounds the GPU tests hold the kernels to; and a restatement of the kernels' ARITHMETIC in fp32 on the CPU
(sim_chain) with which tests/test_decoder_cpu.py shows the bounds attainable and not vacuous (nine mutants of it each exceed one).  torch on the CPU;
imports nothing of the product.  Tensors are [B, C, H, W] here ("image layout"); ws_image() converts the kernels' [B][P][C].

Notation: u = 2^-24 (one fp32 rounding, relative), N = B P, n_i = pixels of pair i (a run of 64 consecutive pixels of one image; two 32-pixel tiles).
The library is built with -ffp-contract=off: a product and a sum round separately.

The bounds (derived, not tuned).
  Products (mlp_ref's formula): a sum of K products with fp32 accumulation is within (u_op + K 2^-23) sum |a||w| + sum e |w| of the exact one, e being the
    error an operand that is not stored carries.  u_op = mlp_ref.U_BF16X3 for the MFMA kernels (64 -> 64 forward and data gradient, K = 576; their weight
    gradients, K = B P), u_op = 0 for the VALU layers: layer 0 (K = 9 Cin), layer 8 forward (K = 576) and backward (K = 9: one output channel), their
    weight gradients (K = B P).
  dx = k (N dz - S1 - xhat S2) is not stored.  From stored dz, xhat, inv and the stored partial sums: e_S = G_BSUM u sum |partial| (G_BSUM = 32: the longest
    of the three combine orders, 24 register adds + 8 group adds with 256 threads); every operation of the bracket rounds relative to its result, which the
    three terms' absolute values bound: e_T = 3 u (|N dz| + |S1| + |xhat S2|) + e_S1 + |xhat| e_S2; k = gamma inv / N takes two roundings and the final
    product one: e_dx = |k| e_T + 3 u |dx|.
  Sums: gamma u sum |term|, gamma the longest chain of fp32 additions a term goes through (counted per kernel below, G_*).
  Pair partials of layers 1..7 (k_dec_conv's epilogue).  Per tile t: d = x - ref_t (ref_t the tile's first pixel), S = sum d and Q = sum d^2 by a chain of
    16 + 1 additions; sum_t = S + n_t ref_t: e_sum_t = 20 u (sum |d| + n_t |ref_t|); M2_t = Q - S^2 / n_t: e_M2_t = 40 u (sum d^2 + (sum |d|)^2 / n_t) + u M2_t
    (d, d^2, the chain, the square and the quotient: 2 x 18 + 4 roundings, all relative to DIFFERENCES from a sample of the same channel: to the spread).
    Chan's merge of the two tiles: delta = mean_B - mean_A carries e_delta = e_sum_A / n_A + e_sum_B / n_B + 2 u (|mean_A| + |mean_B|) + u |delta|, the merged M2
    e_M2_A + e_M2_B + (2 |delta| e_delta + e_delta^2) c + 5 u delta^2 c + 2 u M2, c = n_A n_B / n; the merged sum n (e_mean_A + (e_delta + 3 u |delta|) n_B / n + u |mean|) + u |sum|.
    The mean enters only through delta's rounding, multiplied by |delta| <= spread: an E[x^2] - E[x]^2 form would carry u n mean^2 instead.
  Pair partials of layers 0 and 8 (two passes inside the workgroup): e_sum = G u sum |x| (G_L0 = 19: 16 register adds + 3; G_L8 = 6: a wave butterfly),
    e_mean = (e_sum + u sum |x|) / n, and sum (x - m~)^2 = M2 + n (m - m~)^2 exactly, so e_M2 = (G + 4) u (M2 + n e_mean^2) + n e_mean^2.
  Batch statistics from the partials (combine_fwd_stats, k_dec_head_fwd): mean = sum_i s_i / N: e_mean = (sum e_sum_i + G_C u sum |s_i|) / N + u |mean|;
    d_i = s_i - n_i mean: e_d = e_sum_i + n_i e_mean + 2 u (|s_i| + n_i |mean|) + u |d_i|; q_i = M2_i + d_i^2 / n_i: e_q = e_M2_i + (2 |d_i| e_d + e_d^2) / n_i + 3 u q_i;
    var = sum q_i / N: e_var = (sum e_q + G_C u sum q_i) / N + u var; inv = 1 / sqrt(var + eps): e_inv = inv (e_var + u (var + eps)) / (2 (var + eps)) + 4 u inv
    (a correctly rounded square root and division, doubled).  G_C: 12 + 16 + 1 (512 threads, layers 0..6), 24 + 8 + 1 (256 threads, layer 7), 1 + 6 + 3 + 1 (head).
  xhat = (x - mean) inv: two roundings, (1 + u)^2 - 1 <= 3 u, relative.  z = xhat gamma + beta from the kernel's own xhat: e_z = 2 u (|xhat gamma| + |beta|).
  GELU (gelu_parts): Phi by Abramowitz & Stegun 7.1.26, the 1.5e-7 the kernel documents; + mlp_ref.HEAD for the fast exponential and the reciprocal (the
    reciprocal's 1-ulp error goes through the polynomial's derivative, sum i |c_i| <= 17); + 24 u for the 10 roundings of the Horner polynomial (partial sums
    <= sum |c_i| = 4.47, halved by the 0.5) and 1 - tail: E_PHI = 1.5e-7 + HEAD + 24 u.  phi <= 0.4 and |d (z phi) / dz| <= 0.4:
      e_a = |z| (E_PHI + 0.4 e_z) + (Phi + E_PHI) e_z + u |a|,   e_gp = E_PHI + 0.8 e_z + |z| phi (HEAD + 3 u) + 2 u |gp|.
  Head: pool = sum a_8 / P (a_8 recomputed from the stored xhat_8: e_a as above; chain 4 + 6 + 3): (sum e_a + 13 u sum |a|) / P + u |pool|;
    decoded = pool w + b: 2 u (|pool w| + |b|);  bce_seed = scale (sigmoid(temp decoded) - message): the exponential (2 ulp) of a rounded argument, a sum, a
    quotient, a difference and a product: |scale| (s (1 - s) (4 u + u |temp decoded|) + 3 u s + 2 u |s - message|) + 2^-126 |scale| (fp32's normal range: beyond
    +-88 the exponential overflows and the quotient is exactly 0).
  dz_8 = grad lin_w / P gprime_8: 4 u |dz_8|.  Backward pair sums: chain 16 + 1 + 1 (+ the product): G_PAIR = 20 u sum |dz|, 21 u sum |dz xhat| (k_dec_l8_bwd: 16 + 3).
  dz_{l-1} = G gprime_{l-1}: e_G |gprime| + u |dz|.  Image gradient, mode 1: G istd mask: e_G istd + 3 u |g|.
  dgamma / dbeta from stored dz, xhat: the pair chain and k_dec_sreduce's (up to 48 + 3 partials per thread): (21 + 51) u sum |dz xhat|, (20 + 51) u sum |dz|;
    layer 8's and the Linear's (one block: 1 + 6 + 3): (21 + 10) u, (20 + 10) u, 11 u sum |g pool|, 10 u sum |g|.
  Layer-0 input, mode 1: (clamp(x) - mean) istd with istd = fl(1 / std): e_v = 4 u |v|.
"""
import math

import torch
import torch.nn.functional as F

from mlp_ref import HEAD, U_ACC, U_BF16X3, ratio

F64 = torch.float64
U = 2.0 ** -24
TINY = 2.0 ** -126
E_PHI = 1.5e-7 + HEAD + 24 * U
G_BSUM, G_PAIR, G_L0, G_L8 = 32, 20, 19, 6
G_C = {**{l: 29 for l in range(7)}, 7: 33, 8: 11}
LAYERS = 9

# (B, Cin, H, W): what each shape is listed for (tests/test_decoder_cpu.py checks the geometry claims against the built library)
SHAPES = [(3, 3, 1, 1), (1, 3, 1, 2), (2, 3, 4, 8), (2, 3, 3, 11), (2, 3, 7, 9), (2, 3, 8, 8), (2, 3, 5, 13), (2, 3, 1, 65), (2, 3, 64, 1),
          (2, 3, 17, 17), (2, 3, 23, 23), (2, 3, 32, 32), (2, 3, 31, 33), (97, 3, 5, 5), (192, 3, 5, 5), (2, 1, 6, 6), (2, 8, 6, 6), (2, 25, 6, 6)]
MAX_CIN_6X6 = 25            # the largest Cin dec_workspace_bytes accepts at 6x6 (layer 0's 64 KiB of LDS; found by search in tests/test_decoder_cpu.py)
# per-channel mean and std of input mode 1: the three ImageNet figures the training step uses, then five more so that mode 1 runs at every Cin it accepts (<= 8)
MEAN, STD = (0.485, 0.456, 0.406, 0.5, 0.44, 0.47, 0.43, 0.52), (0.229, 0.224, 0.225, 0.25, 0.21, 0.23, 0.24, 0.22)


def supported(B, Cin, H, W):
    """The supported-shape list of include/nerfsig.h, condition by condition (tests/test_decoder_cpu.py sweeps it against dec_workspace_bytes)."""
    P = H * W
    if min(B, Cin, H, W) < 1 or B * P < 2 or P > 1024 or B * ceil_div(P, 64) > 192 or Cin > 32:
        return False
    R = max((min(64 * p + 64, P) - 1) // W - (64 * p) // W + 3 for p in range(ceil_div(P, 64)))
    if R * (W + 2) > 406:
        return False
    if Cin != 3 and Cin * (R * (W + 2) + 576) + 256 > 16384:
        return False
    return Cin * (H + 2) * (W + 2) + 2496 <= 16384


def ceil_div(a, b):
    return (a + b - 1) // b


def round_up(a, b):
    return ceil_div(a, b) * b


def geometry(B, Cin, H, W):
    """make_geom restated: {ntile, npair, rows_max, nband, R, RS} (compared with dec_workspace_layout by tests/test_decoder_cpu.py)."""
    P = H * W
    ntile = ceil_div(P, 32)
    npair = ceil_div(ntile, 2)
    rows_max = max((min(64 * p + 64, P) - 1) // W - (64 * p) // W + 3 for p in range(npair))
    RS = round_up(W + 2, 8)
    nband = 1
    while True:
        R = ceil_div(H, nband)
        Kpad = ceil_div(R * RS, 16) * 16
        pd, pa = round_up(Kpad * 2, 32) + 16, round_up((Kpad + 2 * RS + 16) * 2, 32) + 16
        if 128 * (pd + pa) + (3 * 64 + 1024) * 4 <= 160 * 1024 - 1024:
            break
        if nband >= H:
            raise ValueError(f"no weight-gradient band of {H}x{W} fits the LDS: the library refuses this shape")
        nband += 1
    return {"ntile": ntile, "npair": npair, "rows_max": rows_max, "nband": ceil_div(H, R), "R": R, "RS": RS}


def ws_image(flat, B, H, W, C):
    """The kernels' [B][P][C] -> [B, C, H, W] float64."""
    return torch.as_tensor(flat).detach().cpu().to(F64).reshape(B, H, W, C).permute(0, 3, 1, 2).contiguous()


# ---- the float64 restatement, one function per step ------------------------------------------------------------------------------------------------------

def input_transform(img, mode, mean=MEAN, std=STD):
    """Layer 0's input [B, Cin, H, W] and the error it carries.  mode 0: the image as it is; mode 1: rendered [B, H, W, Cin]: clamp, permute, (x - mean) / std."""
    img = torch.as_tensor(img).detach().cpu().to(F64)
    if mode == 0:
        return img, torch.zeros_like(img)
    C = img.shape[-1]
    m = torch.tensor([float(torch.tensor(v, dtype=torch.float32)) for v in mean[:C]], dtype=F64).view(1, C, 1, 1)
    s = torch.tensor([float(torch.tensor(v, dtype=torch.float32)) for v in std[:C]], dtype=F64).view(1, C, 1, 1)
    v = (img.clamp(0, 1).permute(0, 3, 1, 2) - m) / s
    return v, 4 * U * v.abs()


def conv(a, w):
    return F.conv2d(a, w, padding=1)


def conv_t(d, w):
    """The transposed convolution (the data gradient): channels swapped, taps flipped."""
    return F.conv2d(d, w.transpose(0, 1).flip(2, 3), padding=1)


def wgrad(dx, a):
    """dW[co, ci, ty, tx] = sum over images and pixels of dx[co](y, x) a[ci](y + ty - 1, x + tx - 1)."""
    H, W = dx.shape[2:]
    ap = F.pad(a, (1, 1, 1, 1))
    out = torch.zeros(dx.shape[1], a.shape[1], 3, 3, dtype=dx.dtype)
    for ty in range(3):
        for tx in range(3):
            out[:, :, ty, tx] = torch.einsum("bohw,bihw->oi", dx, ap[:, :, ty:ty + H, tx:tx + W])
    return out


def conv_bound(a, w, K, u_op, e=None, op=conv):
    c = u_op + K * U_ACC
    if e is None:
        return c * op(a.abs(), w.abs())
    return c * op(a.abs() + e, w.abs()) + op(e, w.abs())


def wgrad_bound(dx, e_dx, a, u_op, e_a=None):
    K = dx.shape[0] * dx.shape[2] * dx.shape[3]
    c = u_op + K * U_ACC
    if e_a is None:
        return c * wgrad(dx.abs() + e_dx, a.abs()) + wgrad(e_dx, a.abs())
    return c * wgrad(dx.abs() + e_dx, a.abs() + e_a) + wgrad(e_dx, a.abs() + e_a) + wgrad(dx.abs(), e_a)


def batch_stats(x, eps):
    """(mean, 1 / sqrt(var + eps)) per channel, biased variance over B P."""
    m = x.mean(dim=(0, 2, 3))
    var = ((x - m.view(1, -1, 1, 1)) ** 2).mean(dim=(0, 2, 3))
    return m, 1.0 / torch.sqrt(var + eps)


def gelu_parts(z):
    Phi = 0.5 * (1.0 + torch.erf(z / math.sqrt(2.0)))
    phi = torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)
    return z * Phi, Phi + z * phi, Phi, phi


def bn_gelu(x, mean, inv, gamma, beta):
    v = lambda t: t.view(1, -1, 1, 1)
    xhat = (x - v(mean)) * v(inv)
    a, gp, _, _ = gelu_parts(xhat * v(gamma) + v(beta))
    return xhat, a, gp


def pair_partials(x, y=None):
    """[npair, B, C, 2].  y None: (sum x, M2 about the pair mean) -- the forward's partials; else (sum x, sum x y) -- the backward's."""
    B, C = x.shape[:2]
    f = x.reshape(B, C, -1)
    g = None if y is None else y.reshape(B, C, -1)
    out = []
    for p in range(ceil_div(f.shape[2], 64)):
        s = f[:, :, 64 * p:64 * p + 64]
        if g is None:
            out.append(torch.stack([s.sum(2), ((s - s.mean(2, keepdim=True)) ** 2).sum(2)], -1))
        else:
            out.append(torch.stack([s.sum(2), (s * g[:, :, 64 * p:64 * p + 64]).sum(2)], -1))
    return torch.stack(out)


def head(a8, lin_w, lin_b):
    pool = a8.mean(dim=(1, 2, 3))
    return pool, pool * lin_w + lin_b


def bce_seed(decoded, message, temp, scale):
    return scale * (torch.sigmoid(temp * decoded) - message)


def head_backward(grad_dec, lin_w, gp8):
    P = gp8.shape[2] * gp8.shape[3]
    return (grad_dec * lin_w / P).view(-1, 1, 1, 1) * gp8


def bn_backward(dz, xhat, gamma, inv, partials):
    """dx = k (N dz - S1 - xhat S2), k = gamma inv / N, S from the partials [npair, B, C, 2]; and dx's error bound."""
    N = dz.shape[0] * dz.shape[2] * dz.shape[3]
    v = lambda t: t.view(1, -1, 1, 1)
    S = partials.sum(dim=(0, 1))
    eS = G_BSUM * U * partials.abs().sum(dim=(0, 1))
    k = gamma * inv / N
    t1, t2, t3 = N * dz, v(S[:, 0]), xhat * v(S[:, 1])
    dx = v(k) * (t1 - t2 - t3)
    e_T = 3 * U * (t1.abs() + t2.abs() + t3.abs()) + v(eS[:, 0]) + xhat.abs() * v(eS[:, 1])
    return dx, v(k.abs()) * e_T + 3 * U * dx.abs()


def image_grad(G, img, mode, std=STD):
    """G [B, Cin, H, W] (d loss / d layer-0 input) -> the gradient in img's layout; mode 1: through the normalisation and the clamp's mask."""
    if mode == 0:
        return G
    img = torch.as_tensor(img).detach().cpu().to(F64)
    C = img.shape[-1]
    istd = torch.tensor([1.0 / float(torch.tensor(v, dtype=torch.float32)) for v in std[:C]], dtype=F64)
    return G.permute(0, 2, 3, 1) * istd * ((img >= 0) & (img <= 1)).to(F64)


def reference(v, prm, grad_dec, eps, img=None, mode=0):
    """The whole chain in float64 from layer 0's input v: every intermediate and gradient, in the names of the kernels' workspace."""
    k = {n: [None] * LAYERS for n in ("x", "xhat", "gprime", "act", "dz", "stat", "bsum", "minv", "dx")}
    a = v
    for l in range(LAYERS):
        k["x"][l] = conv(a, prm["w"][l])
        k["stat"][l] = pair_partials(k["x"][l])
        m, inv = batch_stats(k["x"][l], eps)
        k["minv"][l] = torch.stack([m, inv])
        k["xhat"][l], a, k["gprime"][l] = bn_gelu(k["x"][l], m, inv, prm["gamma"][l], prm["beta"][l])
        k["act"][l] = a
    k["pool"], k["decoded"] = head(a, prm["lin_w"], prm["lin_b"])
    g = {"w": [None] * LAYERS, "gamma": [None] * LAYERS, "beta": [None] * LAYERS, "lin_w": (grad_dec * k["pool"]).sum(), "lin_b": grad_dec.sum()}
    k["dz"][8] = head_backward(grad_dec, prm["lin_w"], k["gprime"][8])
    for l in range(8, -1, -1):
        k["bsum"][l] = pair_partials(k["dz"][l], k["xhat"][l])
        g["beta"][l], g["gamma"][l] = k["bsum"][l][..., 0].sum(dim=(0, 1)), k["bsum"][l][..., 1].sum(dim=(0, 1))
        k["dx"][l], _ = bn_backward(k["dz"][l], k["xhat"][l], prm["gamma"][l], k["minv"][l][1], k["bsum"][l])
        g["w"][l] = wgrad(k["dx"][l], k["act"][l - 1] if l else v)
        G = conv_t(k["dx"][l], prm["w"][l])
        if l:
            k["dz"][l - 1] = G * k["gprime"][l - 1]
        else:
            k["grad_img"] = image_grad(G, img, mode)
    k["grads"] = g
    return k


# ---- the bounds ------------------------------------------------------------------------------------------------------------------------------------------

def _tile(t):
    n = t.shape[2]
    ref = t[:, :, :1]
    d = t - ref
    sd = d.abs().sum(2)
    m = t.mean(2)
    M2 = ((t - m.unsqueeze(2)) ** 2).sum(2)
    return {"n": n, "sum": t.sum(2), "mean": m, "M2": M2, "e_sum": 20 * U * (sd + n * ref[:, :, 0].abs()),
            "e_M2": 40 * U * ((d * d).sum(2) + sd * sd / n) + U * M2}


def partial_bounds(x, layer):
    """(e_sum, e_M2) [npair, B, C] of the forward pair partials of x = x_layer, by the producing kernel's arithmetic (see the module docstring)."""
    B, C = x.shape[:2]
    f = x.reshape(B, C, -1)
    es, eq = [], []
    for p in range(ceil_div(f.shape[2], 64)):
        s = f[:, :, 64 * p:64 * p + 64]
        n = s.shape[2]
        if layer in (0, 8):
            G = G_L0 if layer == 0 else G_L8
            sa = s.abs().sum(2)
            e_s = G * U * sa
            e_m = (e_s + U * sa) / n
            M2 = ((s - s.mean(2, keepdim=True)) ** 2).sum(2)
            es.append(e_s)
            eq.append((G + 4) * U * (M2 + n * e_m ** 2) + n * e_m ** 2)
            continue
        A = _tile(s[:, :, :32])
        if n <= 32:
            e_mean = A["e_sum"] / n + U * A["mean"].abs()
            es.append(n * e_mean + U * A["sum"].abs())
            eq.append(A["e_M2"])
            continue
        Bt = _tile(s[:, :, 32:])
        nA, nB = A["n"], Bt["n"]
        delta = Bt["mean"] - A["mean"]
        e_delta = A["e_sum"] / nA + Bt["e_sum"] / nB + 2 * U * (A["mean"].abs() + Bt["mean"].abs()) + U * delta.abs()
        c = nA * nB / n
        mean = s.mean(2)
        M2 = ((s - mean.unsqueeze(2)) ** 2).sum(2)
        e_mean = A["e_sum"] / nA + U * A["mean"].abs() + (e_delta + 3 * U * delta.abs()) * nB / n + U * mean.abs()
        es.append(n * e_mean + U * s.sum(2).abs())
        eq.append(A["e_M2"] + Bt["e_M2"] + (2 * delta.abs() * e_delta + e_delta ** 2) * c + 5 * U * delta ** 2 * c + 2 * U * M2)
    return torch.stack(es), torch.stack(eq)


def stats_bounds(x, layer, eps):
    """(e_mean, e_inv) [C] of the batch statistics the consumer of x_layer combines from the partials."""
    B, C = x.shape[:2]
    P = x.shape[2] * x.shape[3]
    N = B * P
    part = pair_partials(x)
    e_s, e_M2 = partial_bounds(x, layer)
    n_i = torch.tensor([min(64, P - 64 * p) for p in range(part.shape[0])], dtype=F64).view(-1, 1, 1)
    G = G_C[layer]
    s, M2 = part[..., 0], part[..., 1]
    mean = s.sum(dim=(0, 1)) / N
    e_mean = (e_s.sum(dim=(0, 1)) + G * U * s.abs().sum(dim=(0, 1))) / N + U * mean.abs()
    d = s - n_i * mean
    e_d = e_s + n_i * e_mean + 2 * U * (s.abs() + n_i * mean.abs()) + U * d.abs()
    q = M2 + d * d / n_i
    e_q = e_M2 + (2 * d.abs() * e_d + e_d ** 2) / n_i + 3 * U * q
    var = q.sum(dim=(0, 1)) / N
    e_var = (e_q.sum(dim=(0, 1)) + G * U * q.sum(dim=(0, 1))) / N + U * var
    inv = 1.0 / torch.sqrt(var + eps)
    return e_mean, inv * (e_var + U * (var + eps)) / (2 * (var + eps)) + 4 * U * inv


def gelu_bounds(xhat, gamma, beta):
    """(a, gprime, e_a, e_gp) from the kernel's own xhat."""
    v = lambda t: t.view(1, -1, 1, 1)
    z = xhat * v(gamma) + v(beta)
    e_z = 2 * U * ((xhat * v(gamma)).abs() + v(beta).abs())
    a, gp, Phi, phi = gelu_parts(z)
    e_a = z.abs() * (E_PHI + 0.4 * e_z) + (Phi + E_PHI) * e_z + U * a.abs()
    e_gp = E_PHI + 0.8 * e_z + z.abs() * phi * (HEAD + 3 * U) + 2 * U * gp.abs()
    return a, gp, e_a, e_gp


def _put(out, name, layer, r):
    out[(name, layer)] = r


def forward_ratios(k, v, e_v, prm, eps):
    """Single-layer form.  k: the kernels' saved arrays in image layout (lists per layer: x, xhat, gprime, act, stat [npair,B,C,2], minv [2,C]; pool, decoded);
    v, e_v: layer 0's input and its error; prm: float64 parameters.  {(quantity, layer): largest error / bound}, every element compared."""
    out = {}
    for l in range(LAYERS):
        x = k["x"][l]
        if l == 0:
            want, b = conv(v, prm["w"][0]), conv_bound(v, prm["w"][0], 9 * v.shape[1], 0.0, e_v if float(e_v.abs().max()) > 0 else None)
        elif l < 8:
            want, b = conv(k["act"][l - 1], prm["w"][l]), conv_bound(k["act"][l - 1], prm["w"][l], 576, U_BF16X3)
        else:
            want, b = conv(k["act"][7], prm["w"][8]), conv_bound(k["act"][7], prm["w"][8], 576, 0.0)
        _put(out, "x", l, ratio(x, want, b))
        part = pair_partials(x)
        e_s, e_M2 = partial_bounds(x, l)
        _put(out, "stat_sum", l, ratio(k["stat"][l][..., 0], part[..., 0], e_s))
        _put(out, "stat_M2", l, ratio(k["stat"][l][..., 1], part[..., 1], e_M2))
        m, inv = batch_stats(x, eps)
        e_m, e_inv = stats_bounds(x, l, eps)
        _put(out, "mean", l, ratio(k["minv"][l][0], m, e_m))
        _put(out, "inv", l, ratio(k["minv"][l][1], inv, e_inv))
        km, kinv = k["minv"][l][0].view(1, -1, 1, 1), k["minv"][l][1].view(1, -1, 1, 1)
        xh = (x - km) * kinv
        _put(out, "xhat", l, ratio(k["xhat"][l], xh, 3 * U * xh.abs()))
        a, gp, e_a, e_gp = gelu_bounds(k["xhat"][l], prm["gamma"][l], prm["beta"][l])
        _put(out, "gprime", l, ratio(k["gprime"][l], gp, e_gp))
        if l < 8:
            _put(out, "act", l, ratio(k["act"][l], a, e_a))
        else:
            P = a.shape[2] * a.shape[3]
            pool = a.mean(dim=(1, 2, 3))
            _put(out, "pool", 8, ratio(k["pool"], pool, (e_a.sum(dim=(1, 2, 3)) + 13 * U * a.abs().sum(dim=(1, 2, 3))) / P + U * pool.abs()))
            dec = k["pool"] * prm["lin_w"] + prm["lin_b"]
            _put(out, "decoded", 8, ratio(k["decoded"], dec, 2 * U * ((k["pool"] * prm["lin_w"]).abs() + prm["lin_b"].abs())))
    return out


def seed_ratio(seed, decoded, message, temp, scale):
    """bce_seed against the kernel's own decoded."""
    decoded, message = decoded.to(F64), message.to(F64)
    s = torch.sigmoid(temp * decoded)
    b = abs(scale) * (s * (1 - s) * (4 * U + U * (temp * decoded).abs()) + 3 * U * s + 2 * U * (s - message).abs() + TINY)
    return ratio(seed, bce_seed(decoded, message, temp, scale), b)


def backward_ratios(k, v, prm, grad_dec, img=None, mode=0):
    """Single-layer form of the backward: dz_8 and bsum_8 from the head; dz_{l-1}, bsum_{l-1} from the kernels' own dz_l, xhat_l, gprime_{l-1}, minv_l and
    bsum_l; the image gradient.  Returns ({(quantity, layer): ratio}, per layer (dx, e_dx) for the parameter gradients)."""
    out, dxs = {}, [None] * LAYERS
    dz8 = head_backward(grad_dec, prm["lin_w"], k["gprime"][8])
    _put(out, "dz", 8, ratio(k["dz"][8], dz8, 4 * U * dz8.abs()))
    for l in range(8, -1, -1):
        dz, xh = k["dz"][l], k["xhat"][l]
        want = pair_partials(dz, xh)
        bs = pair_partials(dz.abs(), xh.abs())
        g = G_PAIR
        _put(out, "bsum_dz", l, ratio(k["bsum"][l][..., 0], want[..., 0], g * U * bs[..., 0]))
        _put(out, "bsum_dzxhat", l, ratio(k["bsum"][l][..., 1], want[..., 1], (g + 1) * U * bs[..., 1]))
        dx, e_dx = bn_backward(dz, xh, prm["gamma"][l], k["minv"][l][1], k["bsum"][l])
        dxs[l] = (dx, e_dx)
        K, u_op = (9, 0.0) if l == 8 else (576, U_BF16X3)
        G, e_G = conv_t(dx, prm["w"][l]), conv_bound(dx, prm["w"][l], K, u_op, e_dx, op=conv_t)
        if l:
            gp = k["gprime"][l - 1]
            _put(out, "dz", l - 1, ratio(k["dz"][l - 1], G * gp, e_G * gp.abs() + U * (G * gp).abs()))
        else:
            want = image_grad(G, img, mode)
            b = e_G if mode == 0 else image_grad(e_G, img, mode) + 3 * U * want.abs()
            _put(out, "grad_img", 0, ratio(k["grad_img"], want, b))
    return out, dxs


def grad_ratios(k, v, e_v, prm, grad_dec, dxs):
    """The 29 parameter gradients, element-wise, against the kernels' own dz, xhat and act.  k["grads"]: {"w", "gamma", "beta": lists, "lin_w", "lin_b"}."""
    out, g = {}, k["grads"]
    for l in range(LAYERS):
        dx, e_dx = dxs[l]
        if l == 0:
            want, b = wgrad(dx, v), wgrad_bound(dx, e_dx, v, 0.0, e_v if float(e_v.abs().max()) > 0 else None)
        else:
            want, b = wgrad(dx, k["act"][l - 1]), wgrad_bound(dx, e_dx, k["act"][l - 1], U_BF16X3 if l < 8 else 0.0)
        _put(out, "dW", l, ratio(g["w"][l].reshape(want.shape), want, b))
        dz, xh = k["dz"][l], k["xhat"][l]
        extra = 51 if l < 8 else 10
        _put(out, "dgamma", l, ratio(g["gamma"][l].reshape(-1), (dz * xh).sum(dim=(0, 2, 3)), (G_PAIR + 1 + extra) * U * (dz * xh).abs().sum(dim=(0, 2, 3))))
        _put(out, "dbeta", l, ratio(g["beta"][l].reshape(-1), dz.sum(dim=(0, 2, 3)), (G_PAIR + extra) * U * dz.abs().sum(dim=(0, 2, 3))))
    gd = grad_dec.to(F64)
    _put(out, "dlin_w", 8, ratio(g["lin_w"].reshape(()), (gd * k["pool"]).sum(), 11 * U * (gd * k["pool"]).abs().sum()))
    _put(out, "dlin_b", 8, ratio(g["lin_b"].reshape(()), gd.sum(), 10 * U * gd.abs().sum()))
    return out


def by_quantity(ratios):
    """{quantity: (largest ratio, its layer)} of a {(quantity, layer): ratio} table."""
    best = {}
    for (name, l), r in ratios.items():
        if name not in best or r > best[name][0]:
            best[name] = (r, l)
    return best


def report(tag, ratios):
    print(f"[decoder] {tag}: " + "  ".join(f"{n}={r:.3g}@{l}" for n, (r, l) in sorted(by_quantity(ratios).items())))


# ---- the kernels' arithmetic, restated in fp32 on the CPU -------------------------------------------------------------------------------------------------
# Mutants (tests/test_decoder_cpu.py): "lohi" the lo hi product dropped; "halo" a pair's halo rows beyond its own pixels' rows read as zero; "count" the last
# pair's count taken as 64 in the statistics merge; "noflip" taps not flipped in the data gradient; "band" a weight-gradient band without its neighbours'
# activation rows; "stride" a halo-linear row stride of W instead of W + 2 (a +-1 column shift wraps into the next row); "gelu" GELU' without z phi(z);
# "ex2" variance as E[x^2] - E[x]^2; "mask" the image gradient without the clamp's mask.

F32 = torch.float32


def _split(t):
    hi = t.to(torch.bfloat16).to(F32)
    return hi, (t - hi).to(torch.bfloat16).to(F32)


def _sim_conv(a, w, mut, W_img=None):
    ah, al = _split(a)
    wh, wl = _split(w)

    def three(ah, al):
        out = conv(ah, wh) + conv(al, wh)
        return out if "lohi" in mut else out + conv(ah, wl)
    if "halo" not in mut:
        return three(ah, al)
    B, C, H, W = a.shape
    P = H * W
    out = torch.zeros(B, w.shape[0], P, dtype=F32)
    for p in range(ceil_div(P, 64)):
        q0, q1 = 64 * p, min(64 * p + 64, P) - 1
        rows = torch.zeros(1, 1, H, 1, dtype=F32)
        rows[:, :, q0 // W:q1 // W + 1] = 1
        out[:, :, q0:q1 + 1] = three(ah * rows, al * rows).reshape(B, -1, P)[:, :, q0:q1 + 1]
    return out.reshape(B, -1, H, W)


def _seq_sum(t, dim=0):
    acc = torch.zeros_like(t.select(dim, 0))
    for i in range(t.shape[dim]):
        acc = acc + t.select(dim, i)
    return acc


def sim_partials(x, layer):
    B, C = x.shape[:2]
    f = x.reshape(B, C, -1)
    out = []
    for p in range(ceil_div(f.shape[2], 64)):
        s = f[:, :, 64 * p:64 * p + 64]
        n = s.shape[2]
        if layer in (0, 8):
            ts = _seq_sum(s, 2)
            m = ts / n
            out.append(torch.stack([ts, _seq_sum((s - m.unsqueeze(2)) ** 2, 2)], -1))
            continue
        tiles = []
        for t in (s[:, :, :32], s[:, :, 32:]):
            if t.shape[2]:
                d = t - t[:, :, :1]
                S, Q, nt = _seq_sum(d, 2), _seq_sum(d * d, 2), float(t.shape[2])
                tiles.append((nt, S + nt * t[:, :, 0], Q - S * S / nt))
        cnt, mean, M2 = tiles[0][0], tiles[0][1] / tiles[0][0], tiles[0][2]
        if len(tiles) == 2:
            nb, sb, M2b = tiles[1]
            tot, delta = cnt + nb, sb / nb - mean
            mean = mean + delta * (nb / tot)
            M2 = M2 + (M2b + delta * delta * (cnt * nb / tot))
            cnt = tot
        out.append(torch.stack([mean * cnt, M2], -1))
    return torch.stack(out)


def _grouped_sum(v, kG):
    """sum over the partial index (dim 0, i = pair*B + image) as the kernels do: thread group i % kG adds its own in order, then the kG group sums are added."""
    n = v.shape[0]
    pad = torch.cat([v, torch.zeros((round_up(n, kG) - n,) + v.shape[1:], dtype=v.dtype)])
    return _seq_sum(_seq_sum(pad.reshape(-1, kG, *v.shape[1:]), 0), 0)


def sim_stats(x, part, layer, eps, mut):
    B, C = x.shape[:2]
    P = x.shape[2] * x.shape[3]
    N = float(B * P)
    if "ex2" in mut:
        m = _seq_sum(x.permute(0, 2, 3, 1).reshape(-1, C), 0) / N
        var = _seq_sum((x * x).permute(0, 2, 3, 1).reshape(-1, C), 0) / N - m * m
        return m, 1.0 / torch.sqrt(var + torch.tensor(eps, dtype=F32))
    kG = 16 if layer < 7 else 8
    flat = part.reshape(-1, C, 2)
    m = _grouped_sum(flat[..., 0], kG) / N
    n_i = torch.tensor([64.0 if "count" in mut else float(min(64, P - 64 * p)) for p in range(part.shape[0])], dtype=F32).repeat_interleave(B).view(-1, 1)
    d = flat[..., 0] - n_i * m
    M2 = _grouped_sum(flat[..., 1] + d * d * (1.0 / n_i), kG)
    return m, 1.0 / torch.sqrt(M2 / N + torch.tensor(eps, dtype=F32))


def _sim_gelu(z, mut):
    e = torch.exp(-0.5 * z * z)
    t = 1.0 / (1.0 + torch.tensor(0.3275911 * 0.70710678118654752, dtype=F32) * z.abs())
    poly = t * (0.254829592 + t * (-0.284496736 + t * (1.421413741 + t * (-1.453152027 + t * 1.061405429))))
    tail = 0.5 * poly * e
    Phi = torch.where(z >= 0, 1.0 - tail, tail)
    return z * Phi, Phi if "gelu" in mut else Phi + z * (torch.tensor(0.39894228040143268, dtype=F32) * e)


def _sim_bsum(dz, xh):
    B, C = dz.shape[:2]
    f, g = dz.reshape(B, C, -1), xh.reshape(B, C, -1)
    return torch.stack([torch.stack([_seq_sum(f[:, :, q:q + 64], 2), _seq_sum(f[:, :, q:q + 64] * g[:, :, q:q + 64], 2)], -1) for q in range(0, f.shape[2], 64)])


def _sim_wgrad(dx, a, geom, mut, split=True):
    B, Co, H, W = dx.shape
    P = H * W
    out = torch.zeros(Co, a.shape[1], 3, 3, dtype=F32)
    bands = [(r, min(H, r + geom["R"])) for r in range(0, H, geom["R"])] if split else [(0, H)]
    for lo, hi in bands:
        rows = torch.zeros(1, 1, H, 1, dtype=F32)
        rows[:, :, lo:hi] = 1
        d, aw = dx * rows, (a * rows if "band" in mut else a)
        planes = [(_split(d)[1], _split(aw)[0]), (_split(d)[0], _split(aw)[1]), (_split(d)[0], _split(aw)[0])] if split else [(d, aw)]
        for dd, aa in planes:
            if "stride" in mut:
                af = F.pad(aa.reshape(B, -1, P), (W + 1, W + 1))
                for ty in range(3):
                    for tx in range(3):
                        out[:, :, ty, tx] += torch.einsum("bop,bip->oi", dd.reshape(B, Co, P), af[:, :, ty * W + tx:ty * W + tx + P])
            else:
                out += wgrad(dd, aa)
    return out


def sim_chain(v, prm, grad_dec, eps, geom, img=None, mode=0, mut=()):
    """The kernels' arithmetic in fp32 on the CPU: split-bf16 products as three fp32 convolutions of the hi / lo planes, the partial-statistics pipeline with
    its group sizes (32-pixel tiles about a reference sample, Chan's merge, the grouped combine), the A&S GELU.  Returns the workspace's arrays as float64."""
    mut = frozenset(mut)
    v32 = v.to(F32)
    p32 = {n: ([t.to(F32) for t in x] if isinstance(x, list) else x.to(F32)) for n, x in prm.items()}
    gd = grad_dec.to(F32)
    k = {n: [None] * LAYERS for n in ("x", "xhat", "gprime", "act", "dz", "stat", "bsum", "minv")}
    c4 = lambda t: t.view(1, -1, 1, 1)
    a = v32
    for l in range(LAYERS):
        x = conv(a, p32["w"][l]) if l in (0, 8) else _sim_conv(a, p32["w"][l], mut)
        k["x"][l], k["stat"][l] = x, sim_partials(x, l)
        m, inv = sim_stats(x, k["stat"][l], l, eps, mut)
        k["minv"][l] = torch.stack([m, inv])
        k["xhat"][l] = (x - c4(m)) * c4(inv)
        a, k["gprime"][l] = _sim_gelu(k["xhat"][l] * c4(p32["gamma"][l]) + c4(p32["beta"][l]), mut)
        k["act"][l] = a
    P = v.shape[2] * v.shape[3]
    N = float(v.shape[0] * P)
    k["pool"] = a.reshape(a.shape[0], -1).sum(1) / P
    k["decoded"] = k["pool"] * p32["lin_w"] + p32["lin_b"]
    g = {"w": [None] * LAYERS, "gamma": [None] * LAYERS, "beta": [None] * LAYERS, "lin_w": (gd * k["pool"]).sum(), "lin_b": gd.sum()}
    k["dz"][8] = (gd * p32["lin_w"] / P).view(-1, 1, 1, 1) * k["gprime"][8]
    for l in range(8, -1, -1):
        k["bsum"][l] = _sim_bsum(k["dz"][l], k["xhat"][l])
        flat = k["bsum"][l].reshape(-1, k["bsum"][l].shape[2], 2)
        g["beta"][l], g["gamma"][l] = _grouped_sum(flat[..., 0], 4), _grouped_sum(flat[..., 1], 4)
        S = _grouped_sum(flat, 16)
        kk = p32["gamma"][l] * k["minv"][l][1] / N
        dx = c4(kk) * (N * k["dz"][l] - c4(S[:, 0]) - k["xhat"][l] * c4(S[:, 1]))
        g["w"][l] = _sim_wgrad(dx, k["act"][l - 1] if l else v32, geom, mut, split=0 < l < 8)
        w = p32["w"][l]
        wt = w.transpose(0, 1) if "noflip" in mut else w.transpose(0, 1).flip(2, 3)
        G = F.conv2d(dx, wt, padding=1) if l == 8 else _sim_conv(dx, wt, mut - {"halo"})
        if l:
            k["dz"][l - 1] = G * k["gprime"][l - 1]
        elif mode == 0:
            k["grad_img"] = G
        else:
            im = torch.as_tensor(img).to(F32)
            istd = torch.tensor([1.0 / s for s in STD[:im.shape[-1]]], dtype=F32)
            gi = G.permute(0, 2, 3, 1) * istd
            k["grad_img"] = gi if "mask" in mut else torch.where((im >= 0) & (im <= 1), gi, torch.zeros_like(gi))
    k["grads"] = g
    to64 = lambda t: [to64(e) for e in t] if isinstance(t, list) else ({n: to64(e) for n, e in t.items()} if isinstance(t, dict) else t.to(F64))
    return to64(k)


# ---- the seeded cases --------------------------------------------------------------------------------------------------------------------------------------

def make_params(Cin, seed=0, offset=False):
    """fp32 parameters away from their initial values (conv weights of the default init's size, BatchNorm weights about 1 and biases about 0 perturbed by 0.1,
    the Linear layer too).  offset: every hidden BatchNorm at gamma = 0.02, beta = 3 -- every convolution's input is then about 3 with a spread of 0.02.  With random
    3x3 weights the zero padding still spreads the OUTPUT (a border pixel lacks three to five taps); offset == "centre" also keeps only the centre tap of layers
    1..7, positive: their outputs then have |mean| / spread of several hundred."""
    g = torch.Generator().manual_seed(4000 + seed)
    prm = {"w": [], "gamma": [], "beta": []}
    for l in range(LAYERS):
        ci, co = (Cin if l == 0 else 64), (64 if l < 8 else 1)
        bound = 1.0 / math.sqrt(9 * ci)
        prm["w"].append(((torch.rand(co, ci, 3, 3, generator=g) * 2 - 1) * bound + 0.1 * bound * torch.randn(co, ci, 3, 3, generator=g)).float())
        prm["gamma"].append((1.0 + 0.1 * torch.randn(co, generator=g)).float())
        prm["beta"].append((0.1 * torch.randn(co, generator=g)).float())
        if offset and l < 8:
            prm["gamma"][l], prm["beta"][l] = torch.full((co,), 0.02), torch.full((co,), 3.0)
        if offset == "centre" and 1 <= l < 8:     # positive weights on the centre tap alone: no zero padding is read, and the border pixels see what the others see
            prm["w"][l][:, :, [0, 0, 0, 1, 1, 2, 2, 2], [0, 1, 2, 0, 2, 0, 1, 2]] = 0.0
            prm["w"][l] = prm["w"][l].abs() + 0.01
            prm["w"][l][:, :, [0, 0, 0, 1, 1, 2, 2, 2], [0, 1, 2, 0, 2, 0, 1, 2]] = 0.0
    prm["lin_w"] = (1.0 + 0.1 * torch.randn(1, generator=g)).float()
    prm["lin_b"] = (0.1 * torch.randn(1, generator=g)).float()
    return prm


def params64(prm):
    return {n: ([t.to(F64) for t in x] if isinstance(x, list) else x.to(F64).reshape(())) for n, x in prm.items()}


def make_case(shape, seed=0, mode=0):
    """Seeded fp32 inputs: the image (mode 0: randn [B,Cin,H,W]; mode 1: rendered [B,H,W,Cin] in about [-0.2, 1.2] with values exactly 0 and 1) and d loss / d decoded."""
    B, Cin, H, W = shape
    g = torch.Generator().manual_seed(5000 + seed)
    if mode == 0:
        img = torch.randn(B, Cin, H, W, generator=g)
    else:
        img = torch.rand(B, H, W, Cin, generator=g) * 1.4 - 0.2
        flat = img.view(-1)
        flat[0::7], flat[3::11] = 0.0, 1.0
    return img.float(), torch.randn(B, generator=g).float()
