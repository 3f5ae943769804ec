"""Float64 restatement of the compositing kernels (csrc/composite.hip; the evaluation form in csrc/raymarch.hip), their error bound and the seeded case list
(tests/test_composite_cpu.py, tests/test_gpu_raymarch.py).  Plain numpy; nothing of the package is imported.

The kernels' inputs are taken as they are: sigmas[M], rgbs[M,3], deltas[M,2] = (dt, real dt), rays[N,3] = (id, offset, count), T_thresh,
and for the tails nears[N], fars[N], bg ([3] or [N,3]), gt[N,3], grad_scale, n_values.  Everything is computed in float64 from the float32
input VALUES (T_thresh included: the kernels compare against the float32 number).

Training form, per ray with 0 < count and offset + count <= M (any other ray yields zeros and owns no gradient row):
    alpha_j = 1 - exp(-sigma_j dt_j),  T_0 = 1,  T_{j+1} = T_j (1 - alpha_j),  w_j = alpha_j T_j,
    sample j is LIVE (accumulated) iff T_j >= T_thresh          -- a NaN transmittance is not >= anything: not live
    weights_sum = sum w_j,  image = sum w_j rgb_j,  depth = sum w_j t_j,  t_j = sum_{i<=j} deltas[i,1]      (sums over the live samples)
Evaluation form (`burst`): in-place state, T = 1 - weights_sum, the test `T < T_thresh` comes AFTER the sample was accumulated, and
deltas[.,0] == 0 ends the ray before it."""
import numpy as np

U32 = 2.0 ** -24          # unit round-off of float32 (round to nearest)
TINY32 = 2.0 ** -126      # smallest normal float32: what a flushed subnormal result can lose
MARGIN = 1e-3             # no transmittance of a case may lie within this relative distance of T_thresh (cases())


class Bag(dict):
    """dict with attribute access"""
    __getattr__ = dict.__getitem__
    __setattr__ = dict.__setitem__


def max_ratio(got, want, tol):
    """largest |got - want| / tol; an element off where the bound is zero counts as infinite"""
    err = np.abs(np.asarray(got, np.float64) - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / tol)
    return float(np.max(r, initial=0.0)) if not np.isnan(r).any() else float("inf")


def _f64(a):
    return None if a is None else np.asarray(a, dtype=np.float64)


def _fits(off, cnt, M):
    return cnt != 0 and off + cnt <= M


def _bg_rows(bg, N):
    bg = _f64(bg)
    return np.broadcast_to(bg, (N, 3)) if bg.ndim == 1 else bg


def train_forward(sigmas, rgbs, deltas, rays, T_thresh):
    """-> Bag(weights_sum[N], image[N,3], depth[N] indexed by ray id; live[M] bool; T_trace[M] = transmittance entering each sample of a ray
    that fits (NaN for rows of no such ray); alpha[M], q[M] = 1 - alpha, w[M] (0 where not live), t[M] = accumulated real deltas)."""
    s, c, dl = _f64(sigmas), _f64(rgbs), _f64(deltas)
    rays = np.asarray(rays)
    M, N = s.shape[0], rays.shape[0]
    thr = float(np.float32(T_thresh))
    out = Bag(weights_sum=np.zeros(N), image=np.zeros((N, 3)), depth=np.zeros(N), live=np.zeros(M, bool), T_trace=np.full(M, np.nan),
              alpha=np.zeros(M), q=np.ones(M), w=np.zeros(M), t=np.zeros(M))
    with np.errstate(all="ignore"):
        for rid, off, cnt in rays:
            if not _fits(off, cnt, M):
                continue
            sl = slice(off, off + cnt)
            q = np.exp(-s[sl] * dl[sl, 0])               # 1 - alpha, without the cancellation of forming it from alpha
            alpha = 1.0 - q
            T = np.concatenate(([1.0], np.cumprod(q)[:-1]))
            live = T >= thr
            w = np.where(live, alpha * T, 0.0)
            t = np.cumsum(dl[sl, 1])
            out.live[sl], out.T_trace[sl], out.alpha[sl], out.q[sl], out.w[sl], out.t[sl] = live, T, alpha, q, w, t
            out.weights_sum[rid] = w.sum()
            out.image[rid] = (w[:, None] * c[sl]).sum(0)
            out.depth[rid] = (w * t).sum()
    return out


def train_backward(grad_weights_sum, grad_image, sigmas, rgbs, deltas, rays, T_thresh, fwd=None):
    """Analytic gradient of sum_n (grad_weights_sum_n weights_sum_n + grad_image_n . image_n) of the truncated sums (the live set is held fixed):
        d/d rgb_j   = grad_image w_j
        d/d sigma_j = dt_j [ grad_image . ((1 - alpha_j) T_j rgb_j - sum_{i>j, live} w_i rgb_i) + grad_ws ((1 - alpha_j) T_j - sum_{i>j, live} w_i) ]
    (d alpha_j / d sigma_j = dt_j (1 - alpha_j), d T_i / d sigma_j = -dt_j T_i for i > j).  Rows that are not live are exactly zero; depth
    carries no gradient.  -> grad_sigmas[M], grad_rgbs[M,3]"""
    s, c, dl = _f64(sigmas), _f64(rgbs), _f64(deltas)
    rays = np.asarray(rays)
    M, N = s.shape[0], rays.shape[0]
    f = fwd if fwd is not None else train_forward(sigmas, rgbs, deltas, rays, T_thresh)
    gws = np.zeros(N) if grad_weights_sum is None else _f64(grad_weights_sum)
    gi = _f64(grad_image)
    gs, gc = np.zeros(M), np.zeros((M, 3))
    with np.errstate(all="ignore"):
        for rid, off, cnt in rays:
            if not _fits(off, cnt, M):
                continue
            sl = slice(off, off + cnt)
            live, w = f.live[sl], f.w[sl]
            T_after = f.T_trace[sl] * f.q[sl]
            wc = w[:, None] * c[sl]
            later_c = wc[::-1].cumsum(0)[::-1] - wc            # sum over i > j
            later_w = w[::-1].cumsum()[::-1] - w
            g = dl[sl, 0] * (((T_after[:, None] * c[sl] - later_c) * gi[rid]).sum(1) + gws[rid] * (T_after - later_w))
            gs[sl] = np.where(live, g, 0.0)
            gc[sl] = np.where(live[:, None], gi[rid] * w[:, None], 0.0)
    return gs, gc


def finish(weights_sum, image, depth, nears, fars, bg):
    """The render tail: image_out = image + (1 - weights_sum) bg,  depth_out = max(depth - near, 0) / (far - near)."""
    ws, img, d = _f64(weights_sum), _f64(image), _f64(depth)
    bgr = _bg_rows(bg, ws.shape[0])
    with np.errstate(all="ignore"):
        return img + (1.0 - ws)[:, None] * bgr, np.maximum(d - _f64(nears), 0.0) / (_f64(fars) - _f64(nears))


def finish_backward(grad_image_out, bg, grad_weights_sum=None):
    """Adjoint of the background mix: -> (grad_weights_sum - grad_image_out . bg, grad_image = grad_image_out).  depth_out carries no gradient."""
    g = _f64(grad_image_out)
    gws = np.zeros(g.shape[0]) if grad_weights_sum is None else _f64(grad_weights_sum)
    with np.errstate(all="ignore"):
        return gws - (g * _bg_rows(bg, g.shape[0])).sum(1), g


def mse_seed(image_out, gt, grad_scale, n_values):
    """d (grad_scale * mean over n_values of (image_out - gt)^2) / d image_out"""
    return float(np.float32(grad_scale)) * 2.0 / n_values * (_f64(image_out) - _f64(gt))


def burst(n_alive, n_step, rays_alive, rays_t, sigmas, rgbs, deltas, weights_sum, depth, image, T_thresh, density_scale=None, bound=None, trace=None):
    """One round of the evaluation form, in place on float64 state (rays_alive int32).  Entry n of rays_alive owns rows n*n_step .. +n_step of the
    inputs.  Per step: deltas[.,0] == 0 ends the ray; else accumulate with T = 1 - weights_sum, advance t, and end the ray if T < T_thresh.  A ray
    that ended gets rays_alive[n] = -1 (its rays_t stays); one that used all n_step steps stores its t.
    `bound` (burst_bound_state()) is advanced beside the state: see composite_tolerance.  `trace`: a list that receives every T that was compared.
    -> the step at which each entry stopped (n_step: it did not)."""
    s, c, dl = _f64(sigmas), _f64(rgbs), _f64(deltas)
    thr = float(np.float32(T_thresh))
    scale = 1.0 if density_scale is None else float(np.float32(density_scale))
    nx = 1 if density_scale is None else 2          # roundings in the exponent's argument
    stopped = np.full(n_alive, n_step, np.int64)
    for n in range(n_alive):
        rid = int(rays_alive[n])
        t, ws, d, im = rays_t[rid], weights_sum[rid], depth[rid], image[rid].copy()
        if bound is not None:
            e_ws, e_d, e_im, e_t = bound.weights_sum[rid], bound.depth[rid], bound.image[rid].copy(), bound.t[rid]
        step = 0
        while step < n_step:
            m = n * n_step + step
            if dl[m, 0] == 0.0:
                break
            x = scale * s[m] * dl[m, 0]
            alpha = 1.0 - np.exp(-x)
            T = 1.0 - ws
            w = alpha * T
            if bound is not None:      # before the state moves: every term from the reference's own quantities
                d_alpha = _alpha_err(np.float64(x), np.float64(alpha), nx)
                d_w = d_alpha * abs(T) + abs(alpha) * (e_ws + U32 * abs(T)) + U32 * abs(w)
                e_t = e_t + U32 * abs(t + dl[m, 1])
                e_ws = e_ws + d_w + U32 * abs(ws + w)
                e_d = e_d + d_w * abs(t + dl[m, 1]) + abs(w) * e_t + U32 * abs(d + w * (t + dl[m, 1]))
                e_im = e_im + d_w * np.abs(c[m]) + U32 * np.abs(im + w * c[m])
            if trace is not None:
                trace.append(T)
            ws += w
            t += dl[m, 1]
            d += w * t
            im += w * c[m]
            if T < thr:
                break
            step += 1
        stopped[n] = step
        if step < n_step:
            rays_alive[n] = -1
        else:
            rays_t[rid] = t
        weights_sum[rid], depth[rid], image[rid] = ws, d, im
        if bound is not None:
            bound.weights_sum[rid], bound.depth[rid], bound.image[rid], bound.t[rid] = e_ws, e_d, e_im, e_t
    return stopped


def burst_bound_state(N):
    return Bag(weights_sum=np.zeros(N), depth=np.zeros(N), image=np.zeros((N, 3)), t=np.zeros(N))


# ----------------------------------------------------------------------------------------------------------------------------- the bound

def _alpha_err(x, alpha, nx=1):
    """|alpha_kernel - alpha| for alpha = 1 - exp(-x), x = the exact product sigma dt (nx factors' roundings): see composite_tolerance."""
    e = 1.0 - alpha
    ax = np.minimum(np.abs(x), 200.0)        # beyond this the exponential has long underflowed (or overflowed: a non-finite case, not bounded)
    d_e = np.abs(e) * (2.0 + (nx + 1.5) * ax) * U32 + TINY32
    return d_e + U32 * np.abs(alpha)


def composite_tolerance(sigmas, rgbs, deltas, rays, T_thresh, fwd, grad_weights_sum=None, grad_image=None, bg=None, nears=None, fars=None,
                        gt=None, grad_scale=None, n_values=None, serial=False):
    """Per-element absolute bound on |kernel - float64 reference| for the training form, from the kernel's rounding steps, evaluated on the
    reference's own per-sample quantities (`fwd` = train_forward(...)).  u = 2^-24.  First order in u throughout, except the product, which is
    bounded by an interval.  -> Bag of arrays shaped like the outputs: weights_sum, image, depth, and, as far as their inputs are given,
    grad_sigmas, grad_rgbs (grad_image), image_out, depth_out (bg, nears, fars), and with gt/grad_scale/n_values the chain of the one-launch
    kernel: grad_image (the seed) and gradients whose bound includes the seed's own error.

    The exponential.  The kernel evaluates alpha = 1 - __expf(-(sigma dt)).  The HIP headers define __expf(x) as the hardware base-2
    exponential applied to fl(log2e_f32 * x) (clang's __clang_hip_math.h: `__builtin_amdgcn_exp2f(__log2_e * __x)`), and AMD's CDNA ISA
    reference documents that instruction (V_EXP_F32) as accurate to 1 ulp with subnormal results flushed.  That is the model assumed here; it
    was not fitted to the kernels' output:
        x  = fl(sigma dt)                       relative error u in the argument     -> e relative error |x| u
        y  = fl(log2e_f32 x)                    log2e_f32 is within 0.25 u of log2 e, the product rounds once: 1.25 u -> e relative 1.25 |x| u
        e^ = exp2(y) to 1 ulp = 2 u relative, a subnormal result flushed: 2^-126 absolute
      |e^ - e| <= e (2 + 2.5 |x|) u + 2^-126             (rounded up from 2.25; with density_scale one more rounding in x: 3.5 |x|)
      alpha^ = fl(1 - e^):   d_alpha = |e^ - e| + u |alpha|
      q^ = fl(1 - alpha^) (the scan's factor):   d_q = d_alpha + u |q|        -- absolute: behind an opaque sample q^ is a multiple of u, far from
                                                                                 q in relative terms, which is why nothing here is relative
    A libm expf (the serial oracle) is inside the same model.

    The transmittance.  T_j is a product of j factors q_i.  Whatever the association, the computed product of factors q_i^ in
    [q_i - d_q_i, q_i + d_q_i] with m_j roundings lies in [prod (q_i - d_q_i)^+ (1-u)^m_j, prod (q_i + d_q_i) (1+u)^m_j]; E_T(j) is the larger
    distance of T_j from those ends.  m_j: the Hillis-Steele scan multiplies log2(64) = 6 times and the carry through lane 63 once per chunk,
    so a value in chunk k (k = j div 64) has seen at most 7 (k + 1) products.  (serial=True, the oracle's loop: m_j = j.)

    The weights.  w_j = fl(alpha^ T^): d_w = d_alpha T_j + |alpha_j| E_T(j) + u |w_j| for live j.  The live set is the reference's: cases()
    keeps every T_j a relative 1e-3 away from T_thresh and tests/test_composite_cpu.py asserts E_T(j) is below that distance.

    The sums.  weights_sum, image and depth are sums of terms w_j v_j (v = 1, rgb, t): each term carries d_w |v| + |w| d_v + u |w v| (its product,
    fused or not), and the additions form a tree: a lane adds one term per chunk, wave_sum adds 6 levels, so a partial sum is rounded at most
    (chunks + 6) times, each by u of at most sum |w v|.  t_j itself is a prefix sum of positive numbers with 7 (k + 1) roundings, like T.
    (serial=True: count roundings.)

    grad_rgbs = fl(g w^):  |g| d_w + u |g w|.
    grad_sigmas = dt (sum_c g_c (T_after c_c - (rf_c - r_incl_c)) + tail).  rf is the forward's image (bound above: E_I), r_incl the running
    colour, a prefix sum through the scan: E_R(j) = sum_{i<=j} (d_w |c| + u |w c|) + 7 (k + 1) u sum_{i<=j} |w c|.  The difference cancels: it keeps
    the ABSOLUTE error E_I + E_R(j), which is of size u * depth-of-the-tree * |image| however small rf - r_incl is; times |g| dt that is the
    |grad_image| |image| dt term.  T_after has E_T(j + 1).  tail = fl(gws fl(1 - ws^)): |gws| (E_ws + u |1 - ws|) + u |tail|, and with a background
    gws = gws_in - g . bg carries 3 u sum |g_c bg_c| + u |gws|.  Eight further roundings join the terms and multiply by dt: 8 u of the sum of
    their magnitudes.

    The tail of the render.  image_out = fl(image^ + fl(fl(1 - ws^) bg)):  E_I + (E_ws + u |1 - ws|) |bg| + u |(1 - ws) bg| + u |image_out|.
    depth_out = fl(max(fl(d^ - near), 0) / fl(far - near)):  (E_d + u |d - near|) / (far - near) + 3 u |depth_out|.
    The seed g = fl(k fl(image_out^ - gt)), k = grad_scale * 2 / n_values rounded twice on the host:  |k| (E_out + u |image_out - gt|) + 3 u |g|;
    the gradients then carry E_g through their own derivative: E_g |w| and dt sum_c E_g_c (|T_after c_c - later_c| + |bg_c (1 - ws)|).

    The evaluation form (burst(..., bound=)) follows the serial chain step by step with the same d_alpha: T = fl(1 - ws^) carries E_ws + u |T|,
    w as above, and ws, depth and the colours take one rounding per step (an fma rounds once): E += d_w |v| + |w| d_v + u |partial|."""
    s, c, dl = _f64(sigmas), _f64(rgbs), _f64(deltas)
    rays = np.asarray(rays)
    M, N = s.shape[0], rays.shape[0]
    u = U32
    tol = Bag(weights_sum=np.zeros(N), image=np.zeros((N, 3)), depth=np.zeros(N), T_trace=np.zeros(M))      # T_trace: E_T, for the margin check
    gi = _f64(grad_image)
    e_g = None
    if bg is not None:
        bgr = np.abs(_bg_rows(bg, N))
    with np.errstate(all="ignore"):
        x = s * dl[:, 0]
        d_alpha = _alpha_err(x, fwd.alpha)
        d_q = d_alpha + u * np.abs(fwd.q)
        per_ray = {}
        for rid, off, cnt in rays:
            if not _fits(off, cnt, M):
                continue
            sl = slice(off, off + cnt)
            j = np.arange(cnt)
            m_T = j.astype(np.float64) if serial else 7.0 * (j // 64 + 1)
            q = fwd.q[sl]
            hi = np.concatenate(([1.0], np.cumprod(q + d_q[sl])))
            lo = np.concatenate(([1.0], np.cumprod(np.maximum(q - d_q[sl], 0.0))))
            T_all = np.concatenate((fwd.T_trace[sl], [fwd.T_trace[sl][-1] * q[-1]]))
            m_all = np.concatenate((m_T, [m_T[-1] + (1 if serial else 0)]))
            E_T_all = np.maximum(hi * (1 + u) ** m_all - T_all, T_all - lo * (1 - u) ** m_all)
            E_T, E_T_after, T_after = E_T_all[:-1], E_T_all[1:], T_all[1:]
            tol.T_trace[sl] = E_T
            live, w, alpha, T = fwd.live[sl], fwd.w[sl], fwd.alpha[sl], fwd.T_trace[sl]
            d_w = np.where(live, d_alpha[sl] * np.abs(T) + np.abs(alpha) * E_T + u * np.abs(w), 0.0)
            n_add = float(cnt) if serial else (cnt + 63) // 64 + 6.0
            t = fwd.t[sl]
            d_t = m_T * u * np.abs(t) if not serial else (j + 1.0) * u * np.abs(t)
            tol.weights_sum[rid] = d_w.sum() + n_add * u * np.abs(w).sum()
            wc = np.abs(w[:, None] * c[sl])
            term_c = d_w[:, None] * np.abs(c[sl]) + u * wc
            tol.image[rid] = term_c.sum(0) + n_add * u * wc.sum(0)
            tol.depth[rid] = (d_w * np.abs(t) + np.abs(w) * d_t + u * np.abs(w * t)).sum() + n_add * u * np.abs(w * t).sum()
            per_ray[rid] = (sl, live, w, d_w, T_after, E_T_after, term_c, wc, m_T if not serial else j + 1.0)
        if bg is not None:
            rest = 1.0 - fwd.weights_sum
            img_out, dep_out = finish(fwd.weights_sum, fwd.image, fwd.depth, nears, fars, bg) if nears is not None else (fwd.image + rest[:, None] * _bg_rows(bg, N), None)
            tol.image_out = tol.image + (tol.weights_sum + u * np.abs(rest))[:, None] * bgr + u * np.abs(rest[:, None] * bgr) + u * np.abs(img_out)
            if nears is not None:
                span = np.abs(_f64(fars) - _f64(nears))
                tol.depth_out = (tol.depth + u * np.abs(fwd.depth - _f64(nears))) / span + 3 * u * np.abs(dep_out)
            if gt is not None:
                k = float(np.float32(grad_scale)) * 2.0 / n_values
                gi = mse_seed(img_out, gt, grad_scale, n_values)
                e_g = abs(k) * (tol.image_out + u * np.abs(img_out - _f64(gt))) + 3 * u * np.abs(gi)
                tol.grad_image = e_g
        if gi is not None:
            gws = np.zeros(N) if grad_weights_sum is None else _f64(grad_weights_sum)
            e_gws = np.zeros(N)
            if bg is not None:
                gb = np.abs(gi * _bg_rows(bg, N)).sum(1)
                gws = gws - (gi * _bg_rows(bg, N)).sum(1)
                e_gws = 3 * u * gb + u * np.abs(gws)
                if e_g is not None:
                    e_gws = e_gws + (e_g * bgr).sum(1)
            tol.grad_sigmas, tol.grad_rgbs = np.zeros(M), np.zeros((M, 3))
            for rid, (sl, live, w, d_w, T_after, E_T_after, term_c, wc, m_scan) in per_ray.items():
                g = np.abs(gi[rid])
                eg = np.zeros(3) if e_g is None else e_g[rid]
                tol.grad_rgbs[sl] = np.where(live[:, None], g * d_w[:, None] + u * g * np.abs(w)[:, None] + eg * np.abs(w)[:, None], 0.0)
                signed_wc = w[:, None] * c[sl]
                later_c = signed_wc[::-1].cumsum(0)[::-1] - signed_wc
                E_R = term_c.cumsum(0) + (m_scan * u)[:, None] * wc.cumsum(0)
                Tc = T_after[:, None] * c[sl]
                part = np.abs(Tc) + np.abs(later_c)
                rest = 1.0 - fwd.weights_sum[rid]
                tail = gws[rid] * rest
                e_tail = abs(gws[rid]) * (tol.weights_sum[rid] + u * abs(rest)) + e_gws[rid] * abs(rest) + u * abs(tail)
                inner = (g * (E_T_after[:, None] * np.abs(c[sl]) + tol.image[rid] + E_R + u * part)).sum(1) + e_tail
                inner = inner + 8 * u * ((g * part).sum(1) + abs(tail)) + (eg * np.abs(Tc - later_c)).sum(1)
                tol.grad_sigmas[sl] = np.where(live, np.abs(dl[sl, 0]) * inner, 0.0)
    return tol


# ----------------------------------------------------------------------------------------------------------------------------- the cases

DT = 2.0 * 3.0 ** 0.5 / 1024          # the march's step in a unit-bound scene
# zero-count rays first, in the middle and last; every count next to a multiple of the 64-lane chunk; 1024 = max_steps
COUNTS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 0, 192, 1024, 200, 130, 0)
KNIVES = (0, 1, 62, 63, 64, 65, 127, 128, "last")
PREFIXES = (1, 2, 3, 4, 5, 8, 9)
BIG_PAD = 64 * 256 + 300              # more rows than the 64 tail workgroups cover in one pass of their stride loop


def ray_table(counts=COUNTS):
    """ids equal to the index, offsets ascending and gapless, a zero-count ray carries the running total (the marcher's contract)"""
    counts = np.asarray(counts, np.int64)
    off = np.concatenate(([0], np.cumsum(counts)[:-1]))
    return np.stack([np.arange(len(counts)), off, counts], 1).astype(np.int32)


def _case(name, seed, profile, T_thresh, counts=COUNTS, knife=None, N=None, pad=0, cut=None, permute=False, exact=False, poison=None):
    rng = np.random.RandomState(seed)
    table = ray_table(counts)
    total = int(table[:, 1:].sum(1).max())
    M = total + pad if cut is None else cut
    rows = max(M, total)
    dt = (DT * (1.0 + rng.rand(rows))).astype(np.float32)
    gap = np.where(rng.rand(rows) < 0.1, rng.rand(rows) * 0.05, 0.0).astype(np.float32)     # empty space skipped by the march
    dreal = (dt + gap).astype(np.float32)
    x = rng.rand(rows) * 0.004            # optical depth per sample: 1024 of them leave T ~ 0.13
    sig = x / dt
    for rid, off, cnt in table:
        if cnt == 0:
            continue
        if profile == "knife":
            k = cnt - 1 if knife == "last" else knife
            if k < cnt:
                sig[off + k] = (19.0 + 2.0 * rng.rand()) / dt[off + k]
        elif profile == "gradual" and cnt > 100:       # uniform opacity: T crosses T_thresh between samples 96 and 97
            sig[off:off + cnt] = -np.log(T_thresh) / 96.5 / dt[off:off + cnt]
        elif profile == "wall":
            sig[off] = np.inf
        elif profile == "zero":
            sig[off:off + cnt] = 0.0
        elif profile == "zero_then_dense":             # T stays exactly 1 up to the dense sample, which is therefore live at T_thresh = 1
            sig[off:off + cnt] = 0.0
            k = cnt // 2
            sig[off + k] = 3.0 / dt[off + k]
            sig[off + k + 1:off + cnt] = 50.0
    sig = sig.astype(np.float32)
    if poison is not None:                             # one -inf and one NaN density in one ray
        off = int(table[poison, 1])
        sig[off], sig[off + 5] = -np.inf, np.nan
    n_all = len(table)
    if permute:
        table = table[rng.permutation(n_all)]          # the reference's tables are in atomic order: ids and offsets in any order
    N = n_all if N is None else N
    nears = (0.2 + 0.3 * rng.rand(n_all)).astype(np.float32)
    return Bag(name=name, sigmas=sig[:M].copy(), rgbs=rng.rand(rows, 3).astype(np.float32)[:M].copy(),
               deltas=np.stack([dt, dreal], 1)[:M].copy(), rays=np.ascontiguousarray(table[:N]), N=N, M=M, T_thresh=T_thresh,
               in_order=not permute, exact=exact, poison=poison, total=total,
               nears=nears[:N], fars=(nears + 2.0 + rng.rand(n_all)).astype(np.float32)[:N], bg=rng.rand(3).astype(np.float32),
               bg_rays=rng.rand(n_all, 3).astype(np.float32)[:N], gt=rng.rand(n_all, 3).astype(np.float32)[:N],
               grad_weights_sum=rng.randn(n_all).astype(np.float32)[:N], grad_image=rng.randn(n_all, 3).astype(np.float32)[:N],
               grad_scale=0.5, n_values=3 * N)


_CASES = None


def cases():
    """The shared case list (built once; treat as read-only).  Rays that fit are numbered by id; outputs of ids >= N are nobody's."""
    global _CASES
    if _CASES is not None:
        return _CASES
    out, seed = [], 100
    def add(name, *a, **k):
        nonlocal seed
        seed += 1
        out.append(_case(name, seed, *a, **k))
    for thr in (1e-4, 1e-2, 0.0):
        add(f"thin-{thr:g}", "thin", thr, exact=thr == 0.0)
    for thr in (1e-4, 1e-2):
        for k in KNIVES:
            add(f"knife{k}-{thr:g}", "knife", thr, knife=k)
        add(f"gradual-{thr:g}", "gradual", thr)
    add("knife63-0", "knife", 0.0, knife=63, exact=True)
    add("wall-1e-4", "wall", 1e-4)
    add("wall-0", "wall", 0.0, exact=True)
    add("zero-1e-4", "zero", 1e-4)
    add("dense-1", "zero_then_dense", 1.0, exact=True)
    for n in PREFIXES:
        add(f"prefix{n}", "knife", 1e-4, knife=63, N=n)
    add("pad128", "knife", 1e-4, knife=64, pad=128)
    add("padbig", "knife", 1e-2, knife=1, pad=BIG_PAD)
    table = ray_table()
    off11 = int(table[11, 1])                          # the 1024-sample ray: cut it at a chunk boundary and off one; it and all later rays are dropped
    add("cut-chunk", "knife", 1e-4, knife=62, cut=off11 + 128)
    add("cut-odd", "thin", 1e-4, cut=off11 + 129)
    add("cut-ray-start", "knife", 1e-2, knife="last", cut=off11)
    add("permuted-knife", "knife", 1e-4, knife=65, permute=True)
    add("permuted-thin", "thin", 1e-2, permute=True)
    _CASES = out
    return out


def poisoned_case():
    """Rays 0..3 share a workgroup; ray 2 holds sigma = -inf at its sample 0 and NaN at its sample 5, the others are ordinary."""
    return _case("poisoned", 77, "knife", 1e-4, counts=(130, 64, 70, 65, 3), knife=64, poison=2)


def margin_violations(case, fwd):
    """T_trace values of a case within a relative MARGIN of T_thresh (cases where the comparison is exact in float32 have none by construction)."""
    if case.exact:
        return 0
    thr = float(np.float32(case.T_thresh))
    T = fwd.T_trace[~np.isnan(fwd.T_trace)]
    return int((np.abs(T - thr) <= MARGIN * thr).sum())


# ---- evaluation bursts

BURST_RAYS = 200
BURST_ALIVE = (1, 63, 64, 65, 200)


def burst_scene(seed=7):
    """Per ray a sample sequence, every delta a multiple of 2^-10 so that rays_t is exact in float32: rows past a sequence's end read
    deltas = 0 (the marcher left the buffer zeroed), which ends the ray -- at step 0 of a round or in mid-burst, wherever the end falls.
    Two rays in three carry one opaque sample (sigma dt ~ 20) at a position that walks through all residues: the NEXT sample sees T < T_thresh,
    is accumulated, and ends the ray.  One ray in eleven has no sample at all."""
    rng = np.random.RandomState(seed)
    seqs = []
    for i in range(BURST_RAYS):
        L = 0 if i % 11 == 10 else 3 + (i * 7 + 20) % 38
        dt = rng.randint(3, 9, size=L) / 1024.0
        dreal = dt + rng.randint(0, 3, size=L) / 1024.0
        sig = rng.rand(L) * 0.01 / np.maximum(dt, 1e-9)
        if i % 3 != 2 and L > 0:
            k = (i * 5 + 9) % max(L - 1, 1)
            sig[k] = (19.0 + 2.0 * rng.rand()) / dt[k]
        seqs.append(Bag(sigmas=sig.astype(np.float32), rgbs=rng.rand(L, 3).astype(np.float32),
                        deltas=np.stack([dt, dreal], 1).astype(np.float32).reshape(L, 2)))
    return Bag(seqs=seqs, rays_t0=(rng.randint(200, 500, size=BURST_RAYS) / 1024.0).astype(np.float32))


def burst_rounds(scene, n_alive0, first_step, density_scale=1.0):
    """Generator of the rounds of one evaluation run over rays 0 .. n_alive0-1: yields Bag(n_alive, n_step, rays_alive (int32, to be updated by
    the consumer via .send(new rays_alive)), sigmas, rgbs, deltas), n_step cycling through 1..8 from `first_step`.  Sigmas are stored divided by
    density_scale, so that a kernel that scales them back sees the scene's densities (to a rounding)."""
    alive = np.arange(n_alive0, dtype=np.int32)
    pos = np.zeros(BURST_RAYS, np.int64)
    n_step = first_step
    while alive.size:
        n = alive.size
        sig, rgb, dl = np.zeros(n * n_step, np.float32), np.zeros((n * n_step, 3), np.float32), np.zeros((n * n_step, 2), np.float32)
        for a, rid in enumerate(alive):
            q = scene.seqs[rid]
            take = min(n_step, len(q.sigmas) - pos[rid])
            lo = a * n_step
            sig[lo:lo + take] = q.sigmas[pos[rid]:pos[rid] + take] / np.float32(density_scale)
            rgb[lo:lo + take] = q.rgbs[pos[rid]:pos[rid] + take]
            dl[lo:lo + take] = q.deltas[pos[rid]:pos[rid] + take]
            pos[rid] += n_step
        after = yield Bag(n_alive=n, n_step=n_step, rays_alive=alive.copy(), sigmas=sig, rgbs=rgb, deltas=dl)
        alive = np.ascontiguousarray(after[after >= 0]).astype(np.int32)
        n_step = n_step % 8 + 1


def run_burst(n_alive0, first_step, T_thresh, density_scale=None, fp32=None):
    """The float64 reference over a whole run; with fp32 = a function (round, state) it is run beside it and rays_alive compared every round."""
    scene = burst_scene()
    N = BURST_RAYS
    st = Bag(t=scene.rays_t0.astype(np.float64), ws=np.zeros(N), d=np.zeros(N), im=np.zeros((N, 3)), bound=burst_bound_state(N))
    rounds = burst_rounds(scene, n_alive0, first_step, 1.0 if density_scale is None else density_scale)
    log = Bag(trace=[], first=0, last=0, zero_first=0, zero_mid=0, rounds=0, steps=set())
    rd = next(rounds)
    while True:
        alive = rd.rays_alive.copy()
        stopped = burst(rd.n_alive, rd.n_step, alive, st.t, rd.sigmas, rd.rgbs, rd.deltas, st.ws, st.d, st.im, T_thresh, density_scale,
                           bound=st.bound, trace=log.trace)
        if fp32 is not None:
            assert np.array_equal(fp32(rd), alive), f"rays_alive differs in round {log.rounds}"
        zero = rd.deltas[np.arange(rd.n_alive) * rd.n_step + np.minimum(stopped, rd.n_step - 1), 0] == 0
        ended = stopped < rd.n_step
        log.first += int((ended & ~zero & (stopped == 0)).sum())
        log.last += int((ended & ~zero & (stopped == rd.n_step - 1)).sum())
        log.zero_first += int((ended & zero & (stopped == 0)).sum())
        log.zero_mid += int((ended & zero & (stopped > 0)).sum())
        log.rounds += 1
        log.steps.add(rd.n_step)
        try:
            rd = rounds.send(alive)
        except StopIteration:
            return st, log
