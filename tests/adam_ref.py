"""A float64 statement of the optimiser passes (csrc/optim.hip, csrc/adam.h) with derived error bounds, their fp32 literal restatement, and the inputs the tests feed both.

Shares nothing with the kernels or with nerf_signature_amd/optim.py: numpy only.  What is stated:

  adam_step64    torch.optim.Adam's update of one step (no weight decay, no amsgrad), in float64 on the fp32 operands the kernels are handed
  step_scalars64 the two scalars of step t: lr / (1 - beta1^t) and 1 / sqrt(1 - beta2^t)
  ema64          torch_ema 0.3's update() with its warm-up
  adam_step32, ema32   the same in numpy float32, in exactly adam.h's / k_ema_dense's association

The bounds (derived, not tuned).  u = 2^-24 is one fp32 rounding to nearest, relative; gamma(k) = k u / (1 - k u) bounds k of them compounded ((1 + u)^k - 1 <= gamma(k);
its excess over k u, ~k^2 u^2, also covers float64's own roundings, 1e-16 relative each).  The library is built with -ffp-contract=off: no product and sum contract, every
operation below rounds once.  Division and square root are correctly rounded: one rounding each.  beta1, beta2, eps, grad_scale and the two step scalars are fp32 INPUTS
(exact); 1 - beta is exact in fp32 for beta in [0.5, 1] (Sterbenz), which adam_step64 requires.  With s = grad_scale and gs = g s:

  gs_ = fl(g s)                                            1 rounding
  m'  = fl(m + fl((1 - beta1) fl(gs_ - m)))                3 more.  Rounding 0 moves m' by (1 - beta1) u |gs|, the subtraction and the product by (1 - beta1) u (|gs| + |m|)
                                                           each, the sum by u |m'| with |m'| <= max(|m|, |gs|) (a convex combination): each is at most u (|m| + |gs|), so
                                                           |dm| <= gamma(4) (|m| + |gs|)                                   [C_M = 4 roundings]
  v'  = fl(fl(v beta2) + fl(fl((1 - beta2) gs_) gs_))      both terms are >= 0, so their relative errors do not add but take the larger.  v beta2: its product and the sum, 2.
                                                           (1 - beta2) gs^2: gs_ twice (2), the two products (2), the sum (1): 5.
                                                           |dv| <= gamma(5) v'                                             [C_V = 5 roundings]
  r   = fl(fl(sqrt(v')) ibc)                               sqrt moves by at most sqrt(v' + |dv|) - sqrt(v') or sqrt(v') - sqrt(v' - |dv|), then 2 roundings (sqrt, product)
  den = fl(r + eps)                                        1 rounding                                                      [C_DEN = 3 roundings behind sqrt's argument]
  q   = fl(m' / den)                                       |dm| / den_lo + |m'| |d den| / (den den_lo), den_lo = den - |d den|, then 1 rounding
  t   = fl(step_size q)                                    step_size |dq|, then 1 rounding
  p'  = fl(p - t)                                          |dt|, then 1 rounding: u |p'|                                   [C_P = 3 roundings behind m' and den]

Every rounding of a computed quantity x_ is taken on |x| + |dx|, not on |x|, so nothing is first-order only.  `tiny` adds 2^-126 (the smallest normal: what a flushed or
gradually underflowing result can lose) per operation, for inputs whose intermediates leave the normal range; the tests' main inputs do not.

The EMA: w = float32(1 - min(decay, (1 + n) / (10 + n))) is an input to both sides (python hands the double to mul_ as a float32 scalar).
  s' = fl(s - fl(fl(s - p) w))                             3 roundings: u |s - p|, times w; u |t_|; u |s'_|                 [C_EMA = 3 roundings]
"""
import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -126
C_M, C_V, C_DEN, C_P, C_EMA = 4, 5, 3, 3, 3      # roundings, as counted above (C_DEN, C_P, C_EMA are spelt out one by one in the code)

F32, F64 = np.float32, np.float64


def gamma(k):
    return k * U / (1.0 - k * U)


def _f32_scalar(x):
    """the float the C ABI receives, as a float64"""
    return float(F32(x))


def _betas(beta1, beta2):
    b1, b2 = _f32_scalar(beta1), _f32_scalar(beta2)
    assert 0.5 <= b1 <= 1.0 and 0.5 <= b2 <= 1.0, "1 - beta is exact in fp32 (Sterbenz) for beta in [0.5, 1] only"
    assert float(F32(1.0) - F32(beta1)) == 1.0 - b1 and float(F32(1.0) - F32(beta2)) == 1.0 - b2
    return b1, b2


def adam_step64(p, m, v, g, step_size, inv_bc2_sqrt, beta1, beta2, eps, grad_scale, tiny=0.0):
    """One step of torch.optim.Adam on the arrays p, m, v, g (any shape; the kernels' fp32 operands) in float64.  step_size = lr / (1 - beta1^t) and inv_bc2_sqrt =
    1 / sqrt(1 - beta2^t) are taken as given (hand it the fp32 scalars the update was handed); beta1, beta2, eps, grad_scale are rounded to fp32 first, as the C ABI does.  Returns (p', m', v'), (|dp|, |dm|, |dv|): what an
    fp32 evaluation in adam.h's operation order may differ by, element-wise.  tiny: an absolute allowance per operation (TINY for inputs that underflow)."""
    p, m, v, g = (np.asarray(a).astype(F64) for a in (p, m, v, g))
    b1, b2 = _betas(beta1, beta2)
    eps, s, ss, ib = _f32_scalar(eps), _f32_scalar(grad_scale), float(step_size), float(inv_bc2_sqrt)
    assert ss > 0 and ib > 0 and eps >= 0
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):      # (non-finite gradients go through as IEEE says)
        gs = g * s
        m1 = m + (1.0 - b1) * (gs - m)
        v1 = v * b2 + ((1.0 - b2) * gs) * gs
        root = np.sqrt(v1)
        r = root * ib
        den = r + eps
        q = m1 / den
        p1 = p - ss * q

        dm = gamma(C_M) * (np.abs(m) + np.abs(gs)) + C_M * tiny                        # 4 roundings
        dv = gamma(C_V) * v1 + C_V * tiny                                             # 5 roundings
        droot = np.maximum(np.sqrt(v1 + dv) - root, root - np.sqrt(np.maximum(v1 - dv, 0.0)))
        droot = droot + U * (root + droot) + tiny                                     # sqrt: 1 rounding
        dr = ib * droot + U * ib * (root + droot) + tiny                              # product: 1 rounding
        dden = dr + U * (den + dr) + tiny                                             # sum: 1 rounding
        den_lo = den - dden
        dq = np.where(den_lo > 0, dm / den_lo + np.abs(m1) * dden / (den * den_lo), np.inf)
        dq = np.where((m1 == 0) & (dm == 0), 0.0, dq)                                 # 0 / den is exactly 0 whatever den
        dq = dq + U * (np.abs(q) + dq) + tiny                                         # quotient: 1 rounding
        dt = ss * dq + U * ss * (np.abs(q) + dq) + tiny                               # product: 1 rounding
        dp = dt + U * (np.abs(p1) + dt) + tiny                                        # difference: 1 rounding
    return (p1, m1, v1), (dp, dm, dv)


def adam_step32(p, m, v, g, step_size, inv_bc2_sqrt, beta1, beta2, eps, grad_scale):
    """adam.h's adam_update in numpy float32, operation by operation in its association.  m' and v' are multiplies, adds and subtracts only: determinate to the bit on
    normal-range values.  (p' also takes a square root and a division, correctly rounded here.)"""
    p, m, v, g = (np.asarray(a, F32) for a in (p, m, v, g))
    b1, b2, eps, s, ss, ib = (F32(x) for x in (beta1, beta2, eps, grad_scale, step_size, inv_bc2_sqrt))
    one = F32(1.0)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore", under="ignore"):
        gs = g * s
        m1 = m + (one - b1) * (gs - m)
        v1 = v * b2 + ((one - b2) * gs) * gs
        den = np.sqrt(v1) * ib + eps
        p1 = p - ss * (m1 / den)
    assert p1.dtype == F32 and m1.dtype == F32 and v1.dtype == F32
    return p1, m1, v1


def step_scalars64(step, lr, beta1, beta2):
    """(lr / (1 - beta1^t), 1 / sqrt(1 - beta2^t)) of step t in float64: lr and the betas as the fp32 values the device reads, the powers by pow()."""
    t = float(step)
    b1, b2 = _f32_scalar(beta1), _f32_scalar(beta2)
    return _f32_scalar(lr) / (1.0 - b1 ** t), 1.0 / np.sqrt(1.0 - b2 ** t)


def ema_weight(num_updates, decay):
    """torch_ema 0.3: decay = min(decay, (1 + n) / (10 + n)) with n the count AFTER its increment; 1 - decay reaches mul_ as a float32 scalar"""
    n = float(num_updates)
    return F32(1.0 - min(float(decay), (1.0 + n) / (10.0 + n)))


def ema64(shadow, param, num_updates, decay):
    """torch_ema 0.3's update() of one tensor: shadow - (shadow - param) w in float64.  Returns s' and |ds|."""
    s, p = np.asarray(shadow, F32).astype(F64), np.asarray(param, F32).astype(F64)
    w = float(ema_weight(num_updates, decay))
    d = s - p
    t = d * w
    s1 = s - t
    dd = U * np.abs(d)                           # difference: 1 rounding
    dt = w * dd + U * (np.abs(t) + w * dd)       # product: 1 rounding
    ds = dt + U * (np.abs(s1) + dt)              # difference: 1 rounding
    return s1, ds


def ema32(shadow, param, num_updates, decay):
    """k_ema_dense's s - (s - p) w in numpy float32"""
    s, p = np.asarray(shadow, F32), np.asarray(param, F32)
    out = s - (s - p) * ema_weight(num_updates, decay)
    assert out.dtype == F32
    return out


def max_ratio(got, want, tol):
    """largest |got - want| / tol; an element off where the bound is zero counts as infinite"""
    err = np.abs(np.asarray(got, F64) - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / tol)
    return float(np.max(r, initial=0.0)) if not np.isnan(r).any() else float("inf")


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and bool(np.array_equal(a.view(np.uint32), b.view(np.uint32)))


# ----------------------------------------------------------------------------------------------------------------------------------------- the inputs
# One family for every Adam test, from fixed seeds.  Gradient magnitudes log-uniform over 1e-8 .. 1e2 with random sign, every third element exactly 0 (a row's
# gradient is zero where no ray went); the moments of matching magnitude (|m| within a factor 3 of |g s|, v within a factor 3 of (g s)^2, of the magnitude the
# element's gradient WOULD have where it is zero); every seventh element m = v = 0: with a gradient a row touched for the first time, with g = 0 as well (every 21st)
# a row no ray ever touched, whose parameter and moments must come back bit-identical.  Everything stays in fp32's normal range: the smallest product,
# (1 - beta2) (g s)^2 >= 1e-3 (0.25e-8)^2, is 6e-21.
BETA1, BETA2, BETA2_ALT, EPS, LR = 0.9, 0.99, 0.999, 1e-15, 1e-2
SCALE_CODEBOOK, SCALE_DENSE = 0.3, 0.25      # one is no power of two, and a swapped scale shows
G_LO, G_HI = 1e-8, 1e2
VACUOUS = 1e-3                               # a parameter bound above VACUOUS * lr says nothing about a step of ~lr


def adam_inputs(seed, numel, grad_scale, grad_seed=None):
    """fp32 arrays p, m, v, g of `numel` elements; grad_seed: the gradient (and the magnitudes the moments follow) from a seed of its own, for tensors that share one"""
    rs = np.random.RandomState(seed if grad_seed is None else grad_seed)
    idx = np.arange(numel)
    mag = np.exp(rs.uniform(np.log(G_LO), np.log(G_HI), numel))
    g = (mag * rs.choice([-1.0, 1.0], numel)).astype(F32)
    g[idx % 3 == 0] = 0.0
    rs = np.random.RandomState(seed + 50000)
    gs = mag * float(F32(grad_scale))
    m = (gs * np.exp(rs.uniform(np.log(1 / 3), np.log(3.0), numel)) * rs.choice([-1.0, 1.0], numel)).astype(F32)
    v = (gs * gs * np.exp(rs.uniform(np.log(1 / 3), np.log(3.0), numel))).astype(F32)
    m[idx % 7 == 0] = 0.0
    v[idx % 7 == 0] = 0.0
    p = (rs.standard_normal(numel) * 0.05).astype(F32)
    return p, m, v, g


def untouched(m, v, g):
    """rows no ray ever touched: the update must hand p, m, v back bit for bit"""
    return (np.asarray(g) == 0) & (np.asarray(m) == 0) & (np.asarray(v) == 0)


def tiny_inputs(seed, numel):
    """|g| ~ 1e-25: g^2 underflows.  Moments: m of g's magnitude; v zero, 1.18e-38 (normal; times beta2 it is not), 2e-38 or 1e-30.  Parameters ~1e-9, so that a step of lr 1e-25 / 1e-15 shows."""
    rs = np.random.RandomState(seed)
    g = (np.exp(rs.uniform(np.log(1e-26), np.log(1e-24), numel)) * rs.choice([-1.0, 1.0], numel)).astype(F32)
    m = (np.exp(rs.uniform(np.log(1e-26), np.log(1e-24), numel)) * rs.choice([-1.0, 1.0], numel)).astype(F32)
    v = rs.choice(np.array([0.0, 1.18e-38, 2e-38, 1e-30], F32), numel).astype(F32)
    p = (rs.standard_normal(numel) * 1e-9).astype(F32)
    return p, m, v, g


# Step counts BEFORE the call; the pass advances them by one.  They differ per table / tensor and include 0 (first step), a two-digit count and 999 -> 1000.
def host_lr(i):
    """opt_adam_dense_host takes its step sizes from the host: a learning rate per tensor"""
    return LR * (0.5, 1.0, 3.0)[i % 3]


def f32(x):
    return float(F32(x))


def step_before(i):
    return float((0, 11, 999, 2, 36, 5, 150)[i % 7] + 7 * (i // 7))


T_ROWS = 1 << 19                 # NSIG_TABLE_ROWS: a table is [T_ROWS, 2] floats
CODEBOOK_TABLES = 10             # 2 D at D = 5: float64 comparisons stay at D <= 5


def codebook_inputs():
    """(G, [p], [m], [v]) of CODEBOOK_TABLES tables (flat, 2 T_ROWS elements) under ONE shared gradient: the moments of every table match the gradient's magnitude."""
    ps, ms, vs, G = [], [], [], None
    for t in range(CODEBOOK_TABLES):
        p, m, v, G = adam_inputs(9001 + t, 2 * T_ROWS, SCALE_CODEBOOK, grad_seed=9000)
        ps.append(p), ms.append(m), vs.append(v)
    return G, ps, ms, vs


# Dense tensor lists (sizes in elements; a negative size -n: n elements viewed 4 bytes off a 16-byte boundary).  kDenseChunk = 1024, kDenseChunk4 = 4096,
# kDenseBigNumel = 65536, kDenseRideAlong = 1024, kAdamGroup = 32.
DENSE_ELEMENTWISE = (1, 3, 1023, 1024, 1025, 2049)
# 65540: the last 4096-chunk holds one float4 (the clamped duplicate load); 1024 .. 4100 ride along in the wide form; 1030 and the misaligned view stay element-wise
DENSE_WIDE = (65536, 65540, 69628, 1024, 1028, 4096, 4100, 1030, -4096)
# 33 tensors: two launch groups, the first a mixed wide / element-wise one (slot[] differs from the position in either kernel's list), the second one tensor
DENSE_33 = tuple((1, 3, 1023, 1024, 1025, 2049, 1028, 4100)[i % 8] for i in range(5)) + (65536,) + tuple((1, 3, 1023, 1024, 1025, 2049, 1028, 4100)[i % 8] for i in range(5, 31)) + (1030,)
DENSE_LISTS = {"elementwise": DENSE_ELEMENTWISE, "wide": DENSE_WIDE, "33": DENSE_33}
assert len(DENSE_33) == 33


def dense_inputs(name):
    """[(size, p, m, v, g, step_before)] of one list"""
    base = {"elementwise": 100, "wide": 200, "33": 300}[name]
    return [(size, *adam_inputs(base + i, abs(size), SCALE_DENSE), step_before(i)) for i, size in enumerate(DENSE_LISTS[name])]


def adam_input_sets():
    """every Adam input set the GPU tests use, by name: (p, m, v, g, grad_scale, step_before).  The codebook's is table 0 .. 9 under the shared gradient."""
    G, ps, ms, vs = codebook_inputs()
    for t in range(CODEBOOK_TABLES):
        yield f"codebook table {t}", (ps[t], ms[t], vs[t], G, SCALE_CODEBOOK, step_before(t))
    for name in DENSE_LISTS:
        for i, (size, p, m, v, g, step) in enumerate(dense_inputs(name)):
            yield f"dense {name}[{i}] ({size})", (p, m, v, g, SCALE_DENSE, step)


# The EMA's tensors: sizes around the 4096-element chunk; (size, p_off, s_off): a multiple of 4 viewed 4 bytes off as p, as s, as both -- the scalar branch; 32 in all
EMA_SIZES = (1, 3, 4, 4095, 4096, 4097, 4100, 8196)
EMA_TENSORS = tuple((s, 0, 0) for s in EMA_SIZES) + ((4100, 1, 0), (4100, 0, 1), (4100, 1, 1)) + tuple(((5, 8, 1020, 4096, 33, 2052, 7)[i % 7], 0, 0) for i in range(21))
assert len(EMA_TENSORS) == 32
EMA_CASES = tuple((n, 0.95) for n in (0, 1, 9, 170, 171, 10 ** 6)) + ((5, 0.0), (5, 1.0))      # (num_updates, decay)


def ema_inputs():
    """[(shadow, param)] fp32 arrays for EMA_TENSORS: shadows ~0.1, parameters a step of ~1e-2 away, every fifth element equal"""
    out = []
    for i, (size, _, _) in enumerate(EMA_TENSORS):
        rs = np.random.RandomState(500 + i)
        s = (rs.standard_normal(size) * 0.1).astype(F32)
        p = (s + rs.standard_normal(size) * 1e-2).astype(F32)
        p[::5] = s[::5]
        out.append((s, p))
    return out
