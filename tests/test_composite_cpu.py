"""The float64 compositing reference (tests/composite_ref.py) and its error bound, proven without a GPU: the analytic backward against
float64 autograd, the oracle's serial fp32 loops and an fp32 restatement of the kernels' own association order inside the bound, six
mutants of that restatement outside it, and the margin that keeps every case away from a coin toss at T_thresh."""
import numpy as np
import pytest
import torch

import composite_ref as cr
from oracle import raymarch_ref as orm

F = np.float32


_ratio = cr.max_ratio


_REFS = {}


def _ref(case):
    """float64 forward, backward (plain and with the tail's adjoint) and the bounds of a case, computed once"""
    if case.name not in _REFS:
        a = (case.sigmas, case.rgbs, case.deltas, case.rays, case.T_thresh)
        fwd = cr.train_forward(*a)
        gs, gc = cr.train_backward(case.grad_weights_sum, case.grad_image, *a, fwd=fwd)
        _REFS[case.name] = cr.Bag(fwd=fwd, gs=gs, gc=gc, tol=cr.composite_tolerance(*a, fwd, case.grad_weights_sum, case.grad_image),
                                  tol_serial=cr.composite_tolerance(*a, fwd, case.grad_weights_sum, case.grad_image, serial=True))
    return _REFS[case.name]


def test_the_case_list_covers_what_it_claims():
    cases = cr.cases()
    assert len({c.name for c in cases}) == len(cases)
    counts = set(cr.COUNTS)
    assert {0, 1, 2, 63, 64, 65, 127, 128, 129, 192, 1024} <= counts and cr.COUNTS[0] == 0 and cr.COUNTS[-1] == 0 and 0 in cr.COUNTS[1:-1]
    assert {c.N for c in cases} >= {1, 2, 3, 4, 5, 8, 9, len(cr.COUNTS)}
    assert {c.T_thresh for c in cases} == {1e-4, 1e-2, 0.0, 1.0}
    assert any(c.M == c.total + 128 for c in cases) and any(c.M > c.total + 64 * 256 for c in cases)
    assert sum(c.M < c.total for c in cases) >= 2 and any(not c.in_order for c in cases)
    assert max(c.M for c in cases) < 40000
    for c in cases:                          # the marcher's contract, and no index past a buffer
        t = c.rays if c.in_order else c.rays[np.argsort(c.rays[:, 1], kind="stable")]
        if c.in_order:
            assert (c.rays[:, 0] == np.arange(c.N)).all()
        assert sorted(c.rays[:, 0]) == sorted(set(c.rays[:, 0])) and c.rays[:, 0].max() < c.N and c.rays.min() >= 0
        if c.in_order:
            assert (t[1:, 1] == t[:-1, 1] + t[:-1, 2]).all() and t[0, 1] == 0
        assert len(c.sigmas) == c.M and c.rgbs.shape == (c.M, 3) and c.deltas.shape == (c.M, 2)
        assert (c.deltas[:, 1] >= c.deltas[:, 0]).all() and (c.deltas[:, 0] > 0).all()
        for a in (c.nears, c.fars, c.gt, c.bg_rays, c.grad_image, c.grad_weights_sum):
            assert len(a) >= c.N


def test_no_case_rests_on_a_coin_toss():
    """No transmittance within a relative 1e-3 of T_thresh (zero exclusions; the cases at 0.0 and 1.0 compare exactly in fp32), and the bound on
    the kernel's transmittance is smaller than the distance that is left, so the kernel's live set is the reference's."""
    ends = 0
    for case in cr.cases() + [cr.poisoned_case()]:
        fwd = _ref(case).fwd
        assert cr.margin_violations(case, fwd) == 0, case.name
        owned = ~np.isnan(fwd.T_trace) if case.poison is None else np.zeros(case.M, bool)
        ends += int((owned & ~fwd.live).any())
        if case.exact or case.poison is not None:
            continue
        thr = float(F(case.T_thresh))
        assert (_ref(case).tol.T_trace[owned] < np.abs(fwd.T_trace[owned] - thr)).all(), case.name
    assert ends > 20


def _torch_grads(case, fwd, gws, gi, bg=None, seed=False):
    """float64 autograd through a plain restatement of the truncated sums (the live mask is data)"""
    s = torch.tensor(case.sigmas.astype(np.float64), requires_grad=True)
    c = torch.tensor(case.rgbs.astype(np.float64), requires_grad=True)
    dl = torch.tensor(case.deltas.astype(np.float64))
    N = case.N
    ws, img = [torch.zeros((), dtype=torch.float64)] * N, [torch.zeros(3, dtype=torch.float64)] * N
    for rid, off, cnt in case.rays:
        if cnt == 0 or off + cnt > case.M:
            continue
        q = torch.exp(-s[off:off + cnt] * dl[off:off + cnt, 0])
        T = torch.cat([torch.ones(1, dtype=torch.float64), torch.cumprod(q, 0)[:-1]])
        w = (1 - q) * T * torch.tensor(fwd.live[off:off + cnt].astype(np.float64))
        ws[rid], img[rid] = w.sum(), (w[:, None] * c[off:off + cnt]).sum(0)
    ws, img = torch.stack(ws), torch.stack(img)
    extra = None
    if bg is not None:
        b = torch.tensor(np.broadcast_to(bg, (N, 3)).astype(np.float64))
        out = img + (1 - ws)[:, None] * b
        if seed:
            out = out.detach().requires_grad_(True)
            loss = float(F(case.grad_scale)) * ((out - torch.tensor(case.gt[:N].astype(np.float64))) ** 2).sum() / case.n_values
            return torch.autograd.grad(loss, out)[0].numpy()
        ws_leaf, img_leaf = ws.detach().requires_grad_(True), img.detach().requires_grad_(True)
        out_leaf = img_leaf + (1 - ws_leaf)[:, None] * b
        extra = torch.autograd.grad((out_leaf * torch.tensor(gi[:N].astype(np.float64))).sum(), [ws_leaf, img_leaf])
        loss = (out * torch.tensor(gi[:N].astype(np.float64))).sum()
    else:
        loss = (img * torch.tensor(gi[:N].astype(np.float64))).sum()
    if gws is not None:
        loss = loss + (ws * torch.tensor(gws[:N].astype(np.float64))).sum()
    if not loss.requires_grad:                       # no ray of the table fits: the sums are constants
        return np.zeros(case.M), np.zeros((case.M, 3)), extra
    g = torch.autograd.grad(loss, [s, c])
    return g[0].numpy(), g[1].numpy(), extra


def _close12(got, want, what):
    scale = max(float(np.abs(want).max(initial=0.0)), 1e-300)
    assert np.abs(got - want).max(initial=0.0) <= 1e-12 * scale, what


def test_reference_backward_is_float64_autograd():
    """train_backward, finish_backward and mse_seed equal float64 torch.autograd of the restated forward, to 1e-12 of each gradient's scale."""
    for case in cr.cases():
        r = _ref(case)
        a = (case.sigmas, case.rgbs, case.deltas, case.rays, case.T_thresh)
        gs, gc, _ = _torch_grads(case, r.fwd, case.grad_weights_sum, case.grad_image)
        _close12(r.gs, gs, case.name), _close12(r.gc, gc, case.name)
        for bg in (case.bg, case.bg_rays[:case.N]):
            gws_adj, gi = cr.finish_backward(case.grad_image[:case.N], bg, case.grad_weights_sum[:case.N])
            gs1, gc1 = cr.train_backward(gws_adj, gi, *a, fwd=r.fwd)
            gs, gc, extra = _torch_grads(case, r.fwd, case.grad_weights_sum, case.grad_image, bg=bg)
            _close12(gs1, gs, case.name), _close12(gc1, gc, case.name)
            _close12(gws_adj - case.grad_weights_sum[:case.N], extra[0].numpy(), case.name), _close12(gi, extra[1].numpy(), case.name)
        out, _ = cr.finish(r.fwd.weights_sum, r.fwd.image, r.fwd.depth, case.nears[:case.N], case.fars[:case.N], case.bg)
        _close12(cr.mse_seed(out, case.gt[:case.N], case.grad_scale, case.n_values), _torch_grads(case, r.fwd, None, None, bg=case.bg, seed=True), case.name)


def test_oracle_serial_loops_lie_within_the_bound():
    worst = {}
    for case in cr.cases():
        r = _ref(case)
        ws, dep, img = orm.composite_rays_train_forward(case.sigmas, case.rgbs, case.deltas, case.rays, case.T_thresh)
        gs, gc = orm.composite_rays_train_backward(case.grad_weights_sum, case.grad_image, case.sigmas, case.rgbs, case.deltas, case.rays, ws, img,
                                                   case.T_thresh)
        t = r.tol_serial
        for k, got, want, tol in (("weights_sum", ws, r.fwd.weights_sum, t.weights_sum), ("image", img, r.fwd.image, t.image),
                                  ("depth", dep, r.fwd.depth, t.depth), ("grad_sigmas", gs, r.gs, t.grad_sigmas), ("grad_rgbs", gc, r.gc, t.grad_rgbs)):
            ratio = _ratio(got, want, tol)
            assert ratio <= 1.0, (case.name, k, ratio)
            worst[k] = max(worst.get(k, 0.0), ratio)
        assert (gs[~r.fwd.live] == 0).all() and (gc[~r.fwd.live] == 0).all()
    print("oracle serial loops, largest |fp32 - fp64| / bound:", {k: round(v, 4) for k, v in worst.items()})


# ---- the kernels' association order in fp32 numpy: one wave per ray, 64 lanes per chunk (k_composite_fwd / k_composite_bwd)

_LANES = np.arange(64)


def _scan(v, op):       # Hillis-Steele inclusive scan: lane l takes lane l - d for d = 1, 2, .. 32
    v = v.copy()
    d = 1
    while d < 64:
        v[d:] = op(v[d:], v[:-d])
        d *= 2
    return v


def _wave_sum(v):       # xor tree: every lane ends with the total
    for d in (32, 16, 8, 4, 2, 1):
        v = v + v[_LANES ^ d]
    return v[0]


def _chunk(case, off, base, cnt, T_carry, thr, mutant):
    valid = base + _LANES < cnt
    m = np.minimum(off + base + _LANES, off + cnt - 1)
    sig = np.where(valid, case.sigmas[m], F(0))
    dt, dreal = np.where(valid, case.deltas[m, 0], F(0)), np.where(valid, case.deltas[m, 1], F(0))
    c = np.where(valid[:, None], case.rgbs[m], F(0))
    with np.errstate(all="ignore"):
        alpha = np.where(valid, F(1) - np.exp(-sig * dt, dtype=F), F(0)).astype(F)
        P = _scan(F(1) - alpha, np.multiply)
        P_excl = np.concatenate(([F(1)], P[:-1]))
        T_before = T_carry * (P if mutant == "inclusive_T" else P_excl)
        T_after = T_carry * P
        live = valid & ((T_before > thr) if mutant == "gt_for_ge" else (T_before >= thr))
        w = np.where(live, alpha * T_before, F(0)).astype(F)
    return cr.Bag(alpha=alpha, w=w, T_after=T_after.astype(F), c=c.astype(F), dt=dt.astype(F), dreal=dreal.astype(F), live=live, m=off + base + _LANES)


def kernel_order_fp32(case, mutant=None):
    """-> weights_sum, depth, image, grad_sigmas, grad_rgbs as k_composite_fwd and k_composite_bwd associate them (rm_composite_train_fwd / _bwd)"""
    N, M, thr = case.N, case.M, F(case.T_thresh)
    ws_o, dep_o, img_o = np.zeros(N, F), np.zeros(N, F), np.zeros((N, 3), F)
    gs, gc = np.zeros(M, F), np.zeros((M, 3), F)
    with np.errstate(all="ignore"):
        for rid, off, cnt in case.rays:
            if cnt == 0 or off + cnt > M:
                continue
            acc, ws, d, T, tt = np.zeros((64, 3), F), np.zeros(64, F), np.zeros(64, F), F(1), F(0)
            for base in range(0, cnt, 64):
                k = _chunk(case, off, base, cnt, T, thr, mutant)
                t_incl = tt + _scan(k.dreal, np.add)
                acc, ws, d = acc + k.w[:, None] * k.c, ws + k.w, d + k.w * t_incl
                T, tt = k.T_after[63], t_incl[63]
                if mutant == "T_carry_dropped":
                    T = F(1)
                if mutant == "depth_carry_dropped":
                    tt = F(0)
                if T < thr:
                    break
            ws_o[rid], dep_o[rid] = _wave_sum(ws), _wave_sum(d)
            img_o[rid] = [_wave_sum(acc[:, 0]), _wave_sum(acc[:, 1]), _wave_sum(acc[:, 2])]
            g, rf = case.grad_image[rid], img_o[rid]
            tail = F(0) if mutant == "tail_omitted" else case.grad_weights_sum[rid] * (F(1) - ws_o[rid])
            T, run = F(1), np.zeros(3, F)
            for base in range(0, cnt, 64):
                k = _chunk(case, off, base, cnt, T, thr, mutant)
                incl = run + np.stack([_scan(k.w * k.c[:, i], np.add) for i in range(3)], 1)
                inner = k.T_after[:, None] * k.c - (rf - incl)
                row = k.dt * (g[0] * inner[:, 0] + g[1] * inner[:, 1] + g[2] * inner[:, 2] + tail)
                gs[k.m[k.live]], gc[k.m[k.live]] = row[k.live], g * k.w[k.live, None]
                T, run = k.T_after[63], incl[63]
                if mutant == "T_carry_dropped":
                    T = F(1)
                if mutant == "colour_carry_dropped":
                    run = np.zeros(3, F)
                if T < thr:
                    break
    return cr.Bag(weights_sum=ws_o, depth=dep_o, image=img_o, grad_sigmas=gs, grad_rgbs=gc)


def _ratios(case, got):
    r = _ref(case)
    want = dict(weights_sum=r.fwd.weights_sum, depth=r.fwd.depth, image=r.fwd.image, grad_sigmas=r.gs, grad_rgbs=r.gc)
    return {k: _ratio(got[k], want[k], r.tol[k]) for k in want}


def test_kernel_order_in_fp32_lies_within_the_bound():
    """The kernels' arithmetic alone (same scans, carries and tree, numpy fp32, libm exp) stays inside the bar: the bar is reachable."""
    worst = {}
    for case in cr.cases():
        got = kernel_order_fp32(case)
        for k, v in _ratios(case, got).items():
            assert v <= 1.0, (case.name, k, v)
            worst[k] = max(worst.get(k, 0.0), v)
        live = _ref(case).fwd.live
        assert (got.grad_sigmas[~live] == 0).all() and (got.grad_rgbs[~live] == 0).all()
    print("kernel order in fp32, largest |fp32 - fp64| / bound:", {k: round(v, 4) for k, v in worst.items()})
    assert max(worst.values()) > 0.02          # a bar fifty times above the arithmetic it bounds would discriminate nothing


MUTANTS = ("T_carry_dropped", "colour_carry_dropped", "gt_for_ge", "inclusive_T", "tail_omitted", "depth_carry_dropped")


@pytest.mark.parametrize("mutant", MUTANTS)
def test_the_bound_kills_the_mutant(mutant):
    """One defect at a time in the restatement; each must leave the bound on at least one case of the list."""
    killed = [case.name for case in cr.cases() if max(_ratios(case, kernel_order_fp32(case, mutant)).values()) > 1.0]
    assert killed, mutant


# ---- the evaluation form

_run_burst = cr.run_burst


@pytest.mark.parametrize("n_alive0", cr.BURST_ALIVE)
def test_burst_reference_against_the_oracle_loop(n_alive0):
    N = cr.BURST_RAYS
    scene = cr.burst_scene()
    o = cr.Bag(t=scene.rays_t0.copy(), ws=np.zeros(N, F), d=np.zeros(N, F), im=np.zeros((N, 3), F))

    def fp32(rd):
        alive = rd.rays_alive.copy()
        orm.composite_rays(rd.n_alive, rd.n_step, alive, o.t, rd.sigmas, rd.rgbs, rd.deltas, o.ws, o.d, o.im, 1e-2)
        return alive
    st, log = _run_burst(n_alive0, 1 + n_alive0 % 8, 1e-2, fp32=fp32)
    np.testing.assert_array_equal(o.t.astype(np.float64), st.t)            # dyadic deltas: rays_t is exact
    for got, want, tol in ((o.ws, st.ws, st.bound.weights_sum), (o.d, st.d, st.bound.depth), (o.im, st.im, st.bound.image)):
        assert _ratio(got, want, tol) <= 1.0
    T = np.array(log.trace)
    assert (np.abs(T - float(F(1e-2))) > cr.MARGIN * 1e-2).all()
    assert log.rounds > 1
    if n_alive0 >= 63:
        assert log.first > 0 and log.last > 0 and log.zero_first > 0 and log.zero_mid > 0 and log.steps == set(range(1, 9))
