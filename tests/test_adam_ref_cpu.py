"""tests/adam_ref.py judged on its own, without a GPU: the float64 statements against torch.optim.Adam and torch_ema's recurrence, the derived bounds against the
reference's OWN fp32 literal (never against the kernels), the inputs against the condition that makes a bound mean something, the step scalars against decimal arithmetic."""
import decimal

import numpy as np
import pytest
import torch

import adam_ref as ar

F32, F64 = np.float32, np.float64


def test_adam_step64_iterated_equals_torch_adam_in_float64():
    """Four steps of three parameters, one of which has grad=None at step 2 (torch skips it: its count does not advance)."""
    b1, b2, eps = ar.f32(ar.BETA1), ar.f32(ar.BETA2), ar.f32(ar.EPS)      # torch takes python doubles: hand it the values the C ABI rounds to (lr too: the device reads a float)
    scale = ar.f32(ar.SCALE_DENSE)
    rs = np.random.RandomState(3)
    sizes = (5, 300, 1025)
    P = [torch.nn.Parameter(torch.from_numpy(rs.standard_normal(n) * 0.05)) for n in sizes]
    start = [p.detach().numpy().copy() for p in P]
    opt = torch.optim.Adam(P, lr=ar.f32(ar.LR), betas=(b1, b2), eps=eps)
    mine = [(p.detach().numpy().copy(), np.zeros(n), np.zeros(n), 0) for p, n in zip(P, sizes)]
    for it in range(1, 5):
        for i, p in enumerate(P):
            if i == 1 and it == 2:
                p.grad = None
                continue
            g = ar.adam_inputs(40 * it + i, sizes[i], scale)[3]
            p.grad = torch.from_numpy(g.astype(F64) * scale)
            pp, m, v, t = mine[i]
            ss, ib = ar.step_scalars64(t + 1, ar.LR, ar.BETA1, ar.BETA2)
            (pp, m, v), _ = ar.adam_step64(pp, m, v, g, ss, ib, ar.BETA1, ar.BETA2, ar.EPS, ar.SCALE_DENSE)
            mine[i] = (pp, m, v, t + 1)
        opt.step()
    for i, p in enumerate(P):
        st = opt.state[p]
        assert float(st["step"]) == mine[i][3] == (3 if i == 1 else 4)
        np.testing.assert_allclose(mine[i][0], p.detach().numpy(), rtol=1e-12, atol=0)
        np.testing.assert_allclose(mine[i][1], st["exp_avg"].numpy(), rtol=1e-12, atol=0)
        np.testing.assert_allclose(mine[i][2], st["exp_avg_sq"].numpy(), rtol=1e-12, atol=0)
        assert np.abs(mine[i][0] - start[i]).max() > 1e-3      # (four steps of ~lr went by)


def _torch_ema(shadow, param, n, decay, weight_dtype):
    """test_parameter_ema_follows_torch_ema_inside_the_captured_step's restatement of torch_ema 0.3's update(), tensor operator by tensor operator"""
    decay = min(decay, (1 + n) / (10 + n))
    tmp = shadow - param
    tmp.mul_(float(weight_dtype(1.0 - decay)))      # (on float32 tensors mul_ takes the python double as a float32 scalar; in float64 that rounding is spelt out)
    shadow.sub_(tmp)
    return shadow


@pytest.mark.parametrize("n,decay", ar.EMA_CASES)
def test_ema64_and_ema32_equal_the_tensor_operator_restatement(n, decay):
    for s, p in ar.ema_inputs()[:12]:
        want64 = _torch_ema(torch.from_numpy(s.astype(F64)), torch.from_numpy(p.astype(F64)), n, decay, F32).numpy()
        np.testing.assert_allclose(ar.ema64(s, p, n, decay)[0], want64, rtol=1e-15, atol=0)
        want32 = _torch_ema(torch.from_numpy(s.copy()), torch.from_numpy(p.copy()), n, decay, F64).numpy()
        assert ar.bits_equal(ar.ema32(s, p, n, decay), want32)


def test_ema_warm_up_tie_and_ends():
    """(1 + 170) / (10 + 170) is 0.95 to the bit, the warm-up rules below 170 and decay above; decay 0 gives weight 1"""
    assert (1.0 + 170) / (10.0 + 170) == 0.95
    assert ar.ema_weight(169, 0.95) > ar.ema_weight(170, 0.95) == ar.ema_weight(171, 0.95) == ar.ema_weight(10 ** 6, 0.95) == F32(1.0 - 0.95)
    assert ar.ema_weight(0, 0.95) == F32(0.9) and ar.ema_weight(5, 0.0) == F32(1.0) and ar.ema_weight(5, 1.0) == F32(1.0 - 6.0 / 15.0)


@pytest.fixture(scope="module")
def sets():
    return dict(ar.adam_input_sets())


def _literal_against_bound(name, p, m, v, g, scale, step, lr, tiny=0.0):
    ss, ib = (ar.f32(x) for x in ar.step_scalars64(step + 1, lr, ar.BETA1, ar.BETA2))
    (p1, m1, v1), (dp, dm, dv) = ar.adam_step64(p, m, v, g, ss, ib, ar.BETA1, ar.BETA2, ar.EPS, scale, tiny=tiny)
    l_p, l_m, l_v = ar.adam_step32(p, m, v, g, ss, ib, ar.BETA1, ar.BETA2, ar.EPS, scale)
    ratios = tuple(ar.max_ratio(a, b, c) for a, b, c in ((l_p, p1, dp), (l_m, m1, dm), (l_v, v1, dv)))
    assert max(ratios) <= 1.0, f"{name}: the fp32 literal is at {ratios} of the bounds of p, m, v"
    rows = ar.untouched(m, v, g)
    assert ar.bits_equal(l_p[rows], p[rows]) and not l_m[rows].any() and not l_v[rows].any()
    return ratios, float(np.mean(dp > ar.VACUOUS * lr))


def test_fp32_literal_stays_inside_the_adam_bounds_and_the_bounds_say_something(sets):
    """On every Adam input set of the GPU tests: ratio <= 1 for p, m, v, and at most 1 % of the elements with a parameter bound above 1e-3 lr (a condition on the
    INPUTS; the family was chosen to meet it).  The dense sets also under opt_adam_dense_host's per-tensor learning rates."""
    worst, vac = np.zeros(3), 0.0
    for name, (p, m, v, g, scale, step) in sets.items():
        assert all(np.all((a == 0) | (np.abs(a) >= 2.0 ** -126)) for a in (p, m, v, g)), f"{name}: a subnormal input"
        ratios, frac = _literal_against_bound(name, p, m, v, g, scale, step, ar.LR)
        if p.size >= 1000:
            assert frac <= 0.01, f"{name}: {100 * frac:.2f} % of the parameter bounds are above 1e-3 lr"
        worst, vac = np.maximum(worst, ratios), max(vac, frac if p.size >= 1000 else 0.0)
    for list_name in ar.DENSE_LISTS:
        for i, (size, p, m, v, g, step) in enumerate(ar.dense_inputs(list_name)):
            ratios, frac = _literal_against_bound(f"{list_name}[{i}] host lr", p, m, v, g, ar.SCALE_DENSE, step, ar.host_lr(i))
            if p.size >= 1000:
                assert frac <= 0.01
            worst, vac = np.maximum(worst, ratios), max(vac, frac if p.size >= 1000 else 0.0)
    # tensors below 1000 elements: judged together (1 % of 3 elements is none)
    small = [(k, s) for k, s in sets.items() if s[0].size < 1000]
    total = sum(s[0].size for _, s in small)
    above = sum(_literal_against_bound(k, *s[:6], ar.LR)[1] * s[0].size for k, s in small)
    assert above <= 0.01 * total
    print(f"\nfp32 literal / bound over {len(sets)} input sets: p {worst[0]:.3f}, m {worst[1]:.3f}, v {worst[2]:.3f}; parameter bounds above 1e-3 lr: at most {100 * vac:.3f} % of a set")


def test_fp32_literal_stays_inside_the_bounds_where_g_squared_underflows():
    p, m, v, g = ar.tiny_inputs(77, 4096)
    with np.errstate(under="ignore"):
        ratios, _ = _literal_against_bound("tiny", p, m, v, g, ar.SCALE_DENSE, 11, ar.LR, tiny=ar.TINY)
    print(f"\n|g| ~ 1e-25: fp32 literal (gradual underflow) / bound with 2^-126 per operation: p {ratios[0]:.3f}, m {ratios[1]:.3f}, v {ratios[2]:.3f}")


@pytest.mark.parametrize("n,decay", ar.EMA_CASES)
def test_fp32_literal_stays_inside_the_ema_bound(n, decay):
    worst = 0.0
    for s, p in ar.ema_inputs():
        want, tol = ar.ema64(s, p, n, decay)
        worst = max(worst, ar.max_ratio(ar.ema32(s, p, n, decay), want, tol))
    assert worst <= 1.0
    print(f"\nema num_updates={n} decay={decay}: fp32 literal / bound {worst:.3f}")


@pytest.mark.parametrize("beta2", (ar.BETA2, ar.BETA2_ALT))
def test_step_scalars64_against_decimal_arithmetic(beta2):
    """pow() in float64 against 60-digit decimal powers of the SAME fp32-rounded betas.  pow is within an ulp of beta^t, which 1 - beta^t magnifies by
    beta^t / (1 - beta^t): 1e3 at step 1 of beta2 = 0.999."""
    decimal.getcontext().prec = 60
    D = decimal.Decimal
    lr, b1, b2 = D(ar.f32(ar.LR)), D(ar.f32(ar.BETA1)), D(ar.f32(beta2))
    for t in (1, 2, 13, 1000, 100000, 2 ** 24 - 1):
        ss, ib = ar.step_scalars64(t, ar.LR, ar.BETA1, beta2)
        want_ss, want_ib = lr / (1 - b1 ** t), 1 / (1 - b2 ** t).sqrt()
        cond1, cond2 = float(b1 ** t / (1 - b1 ** t)), float(b2 ** t / (1 - b2 ** t))
        assert abs(D(ss) / want_ss - 1) <= 4e-16 * (1 + cond1), (t, ss)
        assert abs(D(float(ib)) / want_ib - 1) <= 4e-16 * (1 + cond2), (t, ib)
        if t >= 100000:      # the saturated end: beta^t is below half an ulp of 1
            assert ss == ar.f32(ar.LR) and ib == 1.0
    # ... and the unrounded betas are NOT what the device reads: at step 1000 of beta2 = 0.999 the difference is 3e-5, far above one fp32 rounding
    if beta2 == ar.BETA2_ALT:
        assert abs(1.0 / np.sqrt(1.0 - 0.999 ** 1000) / ar.step_scalars64(1000, ar.LR, ar.BETA1, beta2)[1] - 1) > 1e-6
