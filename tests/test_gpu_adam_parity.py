"""Every optimiser pass of csrc/optim.hip against an independent float64 statement of the same operation (tests/adam_ref.py), element by element.

The bit-for-bit chain between the passes that share adam_update (test_gpu_codebook_adam_pipeline.py, test_gpu_adam_fused_dense.py) cannot see an error they have
in common; this file anchors each of them: p, exp_avg and exp_avg_sq of every element within adam_ref's derived bound of float64, exp_avg and exp_avg_sq
also EQUAL to the fp32 literal (multiplies, adds and subtracts without contraction are determinate), rows no ray ever touched handed back bit for bit, the device's
step scalars within one rounding of pow() in float64 -- at step counts that differ per table and per tensor, from the first step to the saturated end.  The EMA the same way,
through its vector and its scalar branch.  The bounds are judged against the reference's own fp32 literal in test_adam_ref_cpu.py, never against these kernels.

The table size is the library's compile-time 2^19 x 2, so "small" means few tables: float64 comparisons at D = 1 and D = 5 only, references computed once and shared."""
import ctypes

import numpy as np
import pytest
import torch

import adam_ref as ar

pytestmark = pytest.mark.gpu

T = ar.T_ROWS
B1, B2, EPS, LR = ar.BETA1, ar.BETA2, ar.EPS, ar.LR
# D: (message, next message), both bit values in each (D = 1: across the two).  The selected tables 0, 2, 5, 7, 8 are at steps 1, 1000, 6, 8 and 19 after the call
MESSAGES = {1: ((0,), (1,)), 5: ((0, 0, 1, 1, 0), (1, 0, 0, 1, 1))}
SCALAR_RTOL = 2.0 ** -24 + 1e-12      # one rounding to float + exp(t log beta)'s stated error
F32, F64 = np.float32, np.float64


class _Worst(dict):
    def check(self, label, what, got, want, tol):
        ratio = ar.max_ratio(got, want, tol)
        self[what] = max(self.get(what, 0.0), ratio)
        assert ratio <= 1.0, f"{label}: {what} is {ratio:.3g} x its bound"

    def show(self, title):
        print(f"\n{title}: largest |kernel - float64| / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in self.items()))


def _dev(a, shape=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t.view(*shape) if shape else t


def _host(t):
    return t.detach().cpu().numpy().reshape(-1)


def _f32s(pair):
    return ar.f32(pair[0]), ar.f32(pair[1])


def _reference(src, ss, ib, scale, tiny=0.0):
    p, m, v, g = src
    want, tol = ar.adam_step64(p, m, v, g, ss, ib, B1, B2, EPS, scale, tiny=tiny)
    return {"want": want, "tol": tol, "lit": ar.adam_step32(p, m, v, g, ss, ib, B1, B2, EPS, scale)}


def _judge(worst, label, got, src, ref, bitwise=True):
    """got = (p, m, v) as the pass left them (flat fp32 arrays), src = (p, m, v, g) as it found them.  Where float64 says finite: within the bound, and m, v equal
    to the literal; where it does not, the same kind of non-finite value; rows no ray ever touched: bit-identical."""
    for name, x, want, tol, lit in zip(("p", "exp_avg", "exp_avg_sq"), got, ref["want"], ref["tol"], ref["lit"]):
        fin = np.isfinite(want)
        assert np.array_equal(np.isnan(x), np.isnan(want)) and np.array_equal(np.isinf(x), np.isinf(want)), f"{label}: {name} is non-finite elsewhere than float64 says"
        if not fin.all():
            assert np.array_equal(x[np.isinf(want)], want[np.isinf(want)].astype(F32))      # (the sign too)
            x, want, tol, lit = x[fin], want[fin], tol[fin], lit[fin]
        worst.check(label, name, x, want, tol)
        if bitwise and name != "p":
            assert ar.bits_equal(x, lit), f"{label}: {name} differs from the fp32 literal in {int(np.sum(x.view(np.uint32) != lit.view(np.uint32)))} elements"
    rows = ar.untouched(*src[1:])
    for x, before in zip(got, src[:3]):
        assert ar.bits_equal(x[rows], before[rows]), f"{label}: a row no ray ever touched was changed"


def _check_scalars(label, got_ss, got_ib, step, lr=LR, beta2=B2):
    want_ss, want_ib = ar.step_scalars64(step, lr, B1, beta2)
    assert abs(float(got_ss) / want_ss - 1.0) <= SCALAR_RTOL, f"{label}: step {step}: step size {float(got_ss)!r} against {want_ss!r}"
    assert abs(float(got_ib) / want_ib - 1.0) <= SCALAR_RTOL, f"{label}: step {step}: 1 / sqrt(1 - beta2^t) {float(got_ib)!r} against {want_ib!r}"


# ------------------------------------------------------------------------------------------------------------------------------------------ the codebook
@pytest.fixture(scope="module")
def book():
    """CODEBOOK_TABLES tables under one gradient, on the host and on the device.  Computed once, never modified: every case works on clones."""
    G, ps, ms, vs = ar.codebook_inputs()
    b = {"G": G, "p": ps, "m": ms, "v": vs, "steps": [ar.step_before(t) for t in range(ar.CODEBOOK_TABLES)], "ref": {}}
    b["dG"] = _dev(G, (T, 2))
    for k in "pmv":
        b["d" + k] = [_dev(a, (T, 2)) for a in b[k]]
    torch.cuda.synchronize()
    return b


def _table_ref(book, t, ss, ib, G=None):
    """float64, bound and literal of table t stepped with the fp32 scalars ss, ib: computed once per (table, scalars) and shared; G: another gradient (not kept)"""
    src = (book["p"][t], book["m"][t], book["v"][t], book["G"] if G is None else G)
    if G is not None:
        return src, _reference(src, ss, ib, ar.SCALE_CODEBOOK)
    key = (t, F32(ss).tobytes(), F32(ib).tobytes())
    if key not in book["ref"]:
        book["ref"][key] = _reference(src, ss, ib, ar.SCALE_CODEBOOK)
    return src, book["ref"][key]


def _selected(D):
    return [2 * i + b for i, b in enumerate(MESSAGES[D][0])]


@pytest.mark.parametrize("D", (1, 5))
def test_codebook_adam_host_selected_pass_against_float64(book, D):
    """opt_codebook_adam, the anchor of the bit-for-bit chain: D tables, each with the scalars of its own step count, handed over by the host."""
    from nerf_signature_amd import _native as nv
    sel = _selected(D)
    scal = [_f32s(ar.step_scalars64(book["steps"][t] + 1, LR, B1, B2)) for t in sel]
    assert len({s for s in scal}) == D
    p, m, v = ([book["d" + k][t].clone() for t in sel] for k in "pmv")
    fl = ctypes.c_float * D
    nv.call("opt_codebook_adam", nv.ptr(book["dG"]), nv.ptr_array(p), nv.ptr_array(m), nv.ptr_array(v), D, B1, B2, EPS, fl(*[s[0] for s in scal]), fl(*[s[1] for s in scal]),
            ar.SCALE_CODEBOOK, nv.stream())
    torch.cuda.synchronize()
    assert torch.equal(book["dG"], _dev(book["G"], (T, 2)))
    worst = _Worst()
    for i, t in enumerate(sel):
        src, ref = _table_ref(book, t, *scal[i])
        _judge(worst, f"D={D}, table {t}", tuple(_host(x[i]) for x in (p, m, v)), src, ref)
    worst.show(f"opt_codebook_adam D={D}")


def _run_sel(nv, book, D, with_next, G=None):
    """opt_codebook_adam_sel[_next] over clones of tables 0 .. 2 D - 1 with MESSAGES[D]"""
    msg, nxt = (torch.tensor(b, dtype=torch.float32, device="cuda") for b in MESSAGES[D])
    n = 2 * D
    p, m, v = ([book["d" + k][t].clone() for t in range(n)] for k in "pmv")
    steps = [torch.tensor(book["steps"][t], device="cuda") for t in range(n)]
    lr, scratch, S = torch.tensor(LR, device="cuda"), torch.full((2 * D,), float("nan"), device="cuda"), torch.full((T, 2), float("nan"), device="cuda")
    head = (nv.ptr(book["dG"] if G is None else G), nv.ptr_array(p), nv.ptr_array(m), nv.ptr_array(v), nv.ptr_array(steps), nv.ptr(msg), D, nv.ptr(lr), B1, B2, EPS,
            ar.SCALE_CODEBOOK, nv.ptr(scratch))
    if with_next:
        nv.call("opt_codebook_adam_sel_next", *head, nv.ptr(nxt), nv.ptr(S), nv.stream())
    else:
        nv.call("opt_codebook_adam_sel", *head, nv.stream())
    torch.cuda.synchronize()
    return p, m, v, steps, scratch.cpu().numpy(), S


def _judge_sel(worst, book, D, p, m, v, steps, sc, S, with_next, G=None):
    sel = _selected(D)
    for t in range(2 * D):
        assert float(steps[t]) == book["steps"][t] + (1.0 if t in sel else 0.0)
        if t not in sel:
            assert all(torch.equal(x[t], book["d" + k][t]) for k, x in zip("pmv", (p, m, v))), f"D={D}: unselected table {t} was written"
    for i, t in enumerate(sel):
        _check_scalars(f"D={D}, table {t}", sc[i], sc[D + i], book["steps"][t] + 1)
        src, ref = _table_ref(book, t, sc[i], sc[D + i], G)
        _judge(worst, f"D={D}, table {t} (bit {i})", tuple(_host(x[t]) for x in (p, m, v)), src, ref)
    if with_next:      # S_next: the next message's tables as they are now, summed in table order
        acc = np.zeros(2 * T, F32)
        for i, b in enumerate(MESSAGES[D][1]):
            with np.errstate(invalid="ignore"):
                acc = acc + _host(p[2 * i + b])
        assert np.array_equal(_host(S), acc, equal_nan=True), f"D={D}: S_next is not the sum of the next message's tables"
    else:
        assert bool(torch.isnan(S).all())


@pytest.mark.parametrize("with_next", (False, True), ids=("plain", "next"))
@pytest.mark.parametrize("D", (1, 5))
def test_codebook_adam_device_selected_pass_against_float64(book, D, with_next):
    """opt_codebook_adam_sel / _sel_next: the selected tables against float64 under the scalars the device left in its scratch, those scalars against pow() in float64."""
    from nerf_signature_amd import _native as nv
    worst = _Worst()
    _judge_sel(worst, book, D, *_run_sel(nv, book, D, with_next), with_next)
    worst.show(f"opt_codebook_adam_sel{'_next' if with_next else ''} D={D}")


@pytest.mark.parametrize("beta2", (ar.BETA2, ar.BETA2_ALT))
def test_codebook_adam_step_scalars_from_the_first_step_to_the_saturated_end(beta2):
    """k_adam_prepare's two scalars at table step counts 0, 1, 12, 999, 99999 and 2^24 - 2 before the call (set by writing the step tensors).  At step 100000 both
    powers are below half an ulp of 1: the step size is lr and 1 / sqrt(1 - beta2^t) is 1.0f, exactly.  (All-zero tables and gradient: nothing else to judge, and
    they stay zero.)"""
    from nerf_signature_amd import _native as nv
    counts = (0, 1, 12, 999, 99999, 2 ** 24 - 2)
    bits = (1, 0, 1, 0, 1, 1)
    D = len(counts)
    p, m, v = ([torch.zeros(T, 2, device="cuda") for _ in range(2 * D)] for _ in range(3))
    before = [float(counts[t // 2]) if t % 2 == bits[t // 2] else 77.0 for t in range(2 * D)]
    steps = [torch.tensor(s, device="cuda") for s in before]
    msg, G = torch.tensor(bits, dtype=torch.float32, device="cuda"), torch.zeros(T, 2, device="cuda")
    lr, scratch = torch.tensor(LR, device="cuda"), torch.full((2 * D,), float("nan"), device="cuda")
    nv.call("opt_codebook_adam_sel", nv.ptr(G), nv.ptr_array(p), nv.ptr_array(m), nv.ptr_array(v), nv.ptr_array(steps), nv.ptr(msg), D, nv.ptr(lr), B1, beta2, EPS,
            ar.SCALE_CODEBOOK, nv.ptr(scratch), nv.stream())
    torch.cuda.synchronize()
    sc = scratch.cpu().numpy()
    for i, c in enumerate(counts):
        assert float(steps[2 * i + bits[i]]) == c + 1.0 and float(steps[2 * i + 1 - bits[i]]) == 77.0
        _check_scalars(f"beta2={beta2}", sc[i], sc[D + i], c + 1, beta2=beta2)
        print(f"\nbeta2={beta2} step {c + 1}: device {sc[i]!r} {sc[D + i]!r}, float64 {ar.step_scalars64(c + 1, LR, B1, beta2)}")
    assert sc[4] == F32(LR) and sc[D + 4] == F32(1.0) and sc[5] == F32(LR) and sc[D + 5] == F32(1.0)
    assert sc[D + 0] > 1.0 and sc[0] > F32(LR)
    assert not any(bool(x.any()) for x in p + m + v)


def test_codebook_adam_nonfinite_gradient_row(book):
    """One +inf and one NaN gradient element in the middle of a row range (opt_codebook_adam_sel_next, D = 5): exactly those elements of the selected tables turn
    non-finite, as float64 says (inf: exp_avg and exp_avg_sq +inf, p NaN; NaN: all three), every other element stays within its bound, unselected tables are untouched."""
    from nerf_signature_amd import _native as nv
    G = book["G"].copy()
    row = 2 * 123458
    assert G[row] != 0 and G[row + 1] != 0
    G[row], G[row + 1] = np.inf, np.nan
    worst = _Worst()
    D = 5
    out = _run_sel(nv, book, D, True, G=_dev(G, (T, 2)))
    _judge_sel(worst, book, D, *out, True, G=G)
    for t in _selected(D):
        x = [_host(a[t]) for a in out[:3]]
        assert all(int(np.sum(~np.isfinite(a))) == 2 for a in x)
        assert np.isnan(x[0][row]) and x[1][row] == np.inf and x[2][row] == np.inf and all(np.isnan(a[row + 1]) for a in x)
    worst.show("opt_codebook_adam_sel_next D=5, one +inf and one NaN gradient element")


# ------------------------------------------------------------------------------------------------------------------------------------------ the dense tensors
def _dense_dev(name, poison=()):
    """The list's tensors on the device: dicts of p, m, v, g (a negative size: a view 4 bytes off a 16-byte boundary), the step tensors, and the host's copies.
    poison: (tensor, element, value) written into the gradients."""
    src, dev = [], {k: [] for k in ("p", "m", "v", "g", "step", "base")}
    for i, (size, p, m, v, g, step) in enumerate(ar.dense_inputs(name)):
        g = g.copy()
        for t, e, val in poison:
            if t == i:
                assert g[e] != 0 and m[e] != 0
                g[e] = val
        src.append((p, m, v, g, step))
        for k, a in zip("pmvg", (p, m, v, g)):
            if size < 0:
                base = torch.full((a.size + 1,), 123.0, device="cuda")
                base[1:] = _dev(a)
                t_ = base[1:]
                assert t_.data_ptr() % 16 == 4 and t_.numel() % 4 == 0
                dev["base"].append(base)
            else:
                t_ = _dev(a)
            dev[k].append(t_)
        dev["step"].append(torch.tensor(step, device="cuda"))
    return src, dev


def _judge_dense(worst, label, src, dev, scalars, first=0, count=None):
    for i in range(first, first + (len(src) - first if count is None else count)):
        p, m, v, g, _ = src[i]
        ss, ib = scalars(i)
        _judge(worst, f"{label}: tensor {i} ({p.size} elements)", tuple(_host(dev[k][i]) for k in "pmv"), (p, m, v, g), _reference((p, m, v, g), ss, ib, ar.SCALE_DENSE))
        assert np.array_equal(_host(dev["g"][i]), g, equal_nan=True)
    assert all(float(b[0]) == 123.0 for b in dev["base"])      # the element in front of a misaligned view


def _arrays(nv, dev, n=None):
    n = len(dev["p"]) if n is None else n
    return n, [nv.ptr_array(dev[k][:n]) for k in ("p", "g", "m", "v")], (ctypes.c_uint32 * n)(*[t.numel() for t in dev["p"][:n]])


@pytest.mark.parametrize("name", sorted(ar.DENSE_LISTS))
def test_dense_adam_device_counted_pass_against_float64(name):
    """opt_adam_dense: every tensor at its own step count, so a tensor that read another's slot of the scratch shows.  "wide" mixes the float4 form (big tensors and
    their ride-alongs) with element-wise tensors in one group; "33" is two launch groups, the second at scratch + 64 with its slots starting again at 0."""
    from nerf_signature_amd import _native as nv
    src, dev = _dense_dev(name)
    n, (pp, pg, pm, pv), numel = _arrays(nv, dev)
    groups = (n + 31) // 32
    lr, scratch = torch.tensor(LR, device="cuda"), torch.full((64 * groups,), float("nan"), device="cuda")
    nv.call("opt_adam_dense", n, pp, pg, pm, pv, nv.ptr_array(dev["step"]), numel, nv.ptr(lr), B1, B2, EPS, ar.SCALE_DENSE, nv.ptr(scratch), nv.stream())
    torch.cuda.synchronize()
    sc = scratch.cpu().numpy()
    for i in range(n):
        assert float(dev["step"][i]) == src[i][4] + 1.0
        _check_scalars(f"{name}: tensor {i}", sc[64 * (i // 32) + i % 32], sc[64 * (i // 32) + 32 + i % 32], src[i][4] + 1)
    used = np.zeros(64 * groups, bool)
    for i in range(n):
        used[[64 * (i // 32) + i % 32, 64 * (i // 32) + 32 + i % 32]] = True
    assert np.isnan(sc[~used]).all() and np.isfinite(sc[used]).all()
    worst = _Worst()
    _judge_dense(worst, name, src, dev, lambda i: (sc[64 * (i // 32) + i % 32], sc[64 * (i // 32) + 32 + i % 32]))
    worst.show(f"opt_adam_dense {name}")


@pytest.mark.parametrize("name", sorted(ar.DENSE_LISTS))
def test_dense_adam_host_scalars_pass_against_float64(name):
    """opt_adam_dense_host: the two scalars of every tensor from the host, here with a learning rate per tensor."""
    from nerf_signature_amd import _native as nv
    src, dev = _dense_dev(name)
    n, (pp, pg, pm, pv), numel = _arrays(nv, dev)
    scal = [_f32s(ar.step_scalars64(src[i][4] + 1, ar.host_lr(i), B1, B2)) for i in range(n)]
    fl = ctypes.c_float * n
    nv.call("opt_adam_dense_host", n, pp, pg, pm, pv, numel, fl(*[s[0] for s in scal]), fl(*[s[1] for s in scal]), B1, B2, EPS, ar.SCALE_DENSE, nv.stream())
    torch.cuda.synchronize()
    worst = _Worst()
    _judge_dense(worst, name, src, dev, lambda i: scal[i])
    assert all(float(dev["step"][i]) == src[i][4] for i in range(n))      # (the host keeps the counts)
    worst.show(f"opt_adam_dense_host {name}")


@pytest.mark.parametrize("name", sorted(ar.DENSE_LISTS))
def test_dense_adam_inside_the_codebook_launch_against_float64(book, name):
    """opt_codebook_adam_sel_next_dense: the dense tensors (at most 32: the first 32 of "33") behind the walk of a D = 1 codebook, each kind under its own gradient
    scale; the scalars k_adam_prepare's second wave left in the dense scratch; the codebook's table as well."""
    from nerf_signature_amd import _native as nv
    src, dev = _dense_dev(name)
    n, (pp, pg, pm, pv), numel = _arrays(nv, dev, min(len(src), 32))
    D = 1
    msg, nxt = (torch.tensor(b, dtype=torch.float32, device="cuda") for b in MESSAGES[D])
    p, m, v = ([book["d" + k][t].clone() for t in range(2)] for k in "pmv")
    steps = [torch.tensor(book["steps"][t], device="cuda") for t in range(2)]
    lr, scratch, S = torch.tensor(LR, device="cuda"), torch.full((2 * D,), float("nan"), device="cuda"), torch.full((T, 2), float("nan"), device="cuda")
    dense_scratch = torch.zeros(2048, dtype=torch.uint8, device="cuda")      # NSIG_ADAM_DENSE_SCRATCH_BYTES
    nv.call("opt_codebook_adam_sel_next_dense", nv.ptr(book["dG"]), nv.ptr_array(p), nv.ptr_array(m), nv.ptr_array(v), nv.ptr_array(steps), nv.ptr(msg), D, nv.ptr(lr),
            B1, B2, EPS, ar.SCALE_CODEBOOK, nv.ptr(scratch), nv.ptr(nxt), nv.ptr(S), n, pp, pg, pm, pv, nv.ptr_array(dev["step"][:n]), numel, ar.SCALE_DENSE,
            nv.ptr(dense_scratch), nv.stream())
    torch.cuda.synchronize()
    worst = _Worst()
    _judge_sel(worst, book, D, p, m, v, steps, scratch.cpu().numpy(), S, True)
    sc = dense_scratch.cpu().numpy().view(F32)
    for i in range(n):
        assert float(dev["step"][i]) == src[i][4] + 1.0
        _check_scalars(f"{name}: tensor {i}", sc[i], sc[32 + i], src[i][4] + 1)
    _judge_dense(worst, name, src, dev, lambda i: (sc[i], sc[32 + i]), count=n)
    for i in range(n, len(src)):      # what did not ride: untouched
        assert all(ar.bits_equal(_host(dev[k][i]), a) for k, a in zip("pmv", src[i][:3])) and float(dev["step"][i]) == src[i][4]
    worst.show(f"opt_codebook_adam_sel_next_dense {name}")


def test_dense_adam_nonfinite_gradients():
    """One +inf and one NaN gradient element in the middle of a wide chunk (tensor 0 of "wide", its second 4096-chunk) and of an element-wise chunk (tensor 7, 1030
    elements): exactly those elements turn non-finite, as float64 says; every neighbour stays within its bound."""
    from nerf_signature_amd import _native as nv
    poison = ((0, 6100, np.inf), (0, 6101, np.nan), (7, 500, np.inf), (7, 502, np.nan))
    src, dev = _dense_dev("wide", poison)
    n, (pp, pg, pm, pv), numel = _arrays(nv, dev)
    lr, scratch = torch.tensor(LR, device="cuda"), torch.full((64,), float("nan"), device="cuda")
    nv.call("opt_adam_dense", n, pp, pg, pm, pv, nv.ptr_array(dev["step"]), numel, nv.ptr(lr), B1, B2, EPS, ar.SCALE_DENSE, nv.ptr(scratch), nv.stream())
    torch.cuda.synchronize()
    sc = scratch.cpu().numpy()
    worst = _Worst()
    _judge_dense(worst, "non-finite", src, dev, lambda i: (sc[i], sc[32 + i]))
    for i in range(n):
        bad = sorted(e for t, e, _ in poison if t == i)
        for k in "pmv":
            assert np.flatnonzero(~np.isfinite(_host(dev[k][i]))).tolist() == bad, (i, k)
    worst.show("opt_adam_dense wide, +inf and NaN gradient elements")


def test_dense_adam_where_the_squared_gradient_underflows():
    """|g| ~ 1e-25: (1 - beta2) (g s)^2 is below the smallest subnormal and v beta2 leaves the normal range.  Judged against float64 with 2^-126 per operation on top
    of the bounds, which covers a flush to zero as well as gradual underflow; what the device did is printed."""
    from nerf_signature_amd import _native as nv
    p, m, v, g = ar.tiny_inputs(77, 4096)
    step = 11.0
    d = {k: _dev(a) for k, a in zip("pmvg", (p, m, v, g))}
    st, lr, scratch = torch.tensor(step, device="cuda"), torch.tensor(LR, device="cuda"), torch.full((64,), float("nan"), device="cuda")
    nv.call("opt_adam_dense", 1, nv.ptr_array([d["p"]]), nv.ptr_array([d["g"]]), nv.ptr_array([d["m"]]), nv.ptr_array([d["v"]]), nv.ptr_array([st]),
            (ctypes.c_uint32 * 1)(4096), nv.ptr(lr), B1, B2, EPS, ar.SCALE_DENSE, nv.ptr(scratch), nv.stream())
    torch.cuda.synchronize()
    sc = scratch.cpu().numpy()
    _check_scalars("tiny", sc[0], sc[32], step + 1)
    got = tuple(_host(d[k]) for k in "pmv")
    with np.errstate(under="ignore"):
        ref = _reference((p, m, v, g), sc[0], sc[32], ar.SCALE_DENSE, tiny=ar.TINY)
    sub = (ref["lit"][2] != 0) & (np.abs(ref["lit"][2]) < ar.TINY)
    kept, flushed = int(np.sum(got[2][sub] == ref["lit"][2][sub])), int(np.sum(got[2][sub] == 0))
    print(f"\n|g| ~ 1e-25: {int(sub.sum())} of 4096 exp_avg_sq results are subnormal in the fp32 literal; the device kept {kept} of them to the bit and flushed {flushed} to zero; "
          f"elsewhere exp_avg_sq equals the literal: {ar.bits_equal(got[2][~sub], ref['lit'][2][~sub])}, exp_avg equals it: {ar.bits_equal(got[1], ref['lit'][1])}")
    assert sub.sum() > 500
    worst = _Worst()
    _judge(worst, "tiny", got, (p, m, v, g), ref, bitwise=False)
    worst.show("opt_adam_dense, |g| ~ 1e-25 (bounds + 2^-126 per operation)")


# ------------------------------------------------------------------------------------------------------------------------------------------ the EMA
@pytest.fixture(scope="module")
def ema_src():
    return ar.ema_inputs()


@pytest.mark.parametrize("num_updates,decay", ar.EMA_CASES)
def test_ema_update_against_float64_and_the_literal(ema_src, num_updates, decay):
    """opt_ema_update over 32 tensors in one launch: sizes around the 4096-element chunk, and a multiple of 4 viewed 4 bytes off as the parameter, as the shadow and as
    both (k_ema_dense's scalar branch).  The shadow: equal to s - (s - p) w in fp32 and within the bound of float64; the parameters untouched; the NaN fill behind
    (and, for a view, in front of) every shadow still there."""
    from nerf_signature_amd import _native as nv
    GUARD = 4
    ps, ss, bufs = [], [], []
    for (size, p_off, s_off), (s, p) in zip(ar.EMA_TENSORS, ema_src):
        pb, sb = torch.full((p_off + size + GUARD,), float("nan"), device="cuda"), torch.full((s_off + size + GUARD,), float("nan"), device="cuda")
        pb[p_off:p_off + size], sb[s_off:s_off + size] = _dev(p), _dev(s)
        ps.append(pb[p_off:p_off + size]), ss.append(sb[s_off:s_off + size]), bufs.append((pb, sb))
        assert ps[-1].data_ptr() % 16 == 4 * p_off and ss[-1].data_ptr() % 16 == 4 * s_off
    n = len(ps)
    count = torch.tensor([num_updates], dtype=torch.int32, device="cuda")
    nv.call("opt_ema_update", n, nv.ptr_array(ps), nv.ptr_array(ss), (ctypes.c_uint32 * n)(*[t.numel() for t in ps]), nv.ptr(count), float(decay), nv.stream())
    torch.cuda.synchronize()
    assert int(count) == num_updates
    worst = _Worst()
    for i, ((size, p_off, s_off), (s, p)) in enumerate(zip(ar.EMA_TENSORS, ema_src)):
        label = f"tensor {i} ({size} elements, offsets {p_off} {s_off})"
        got = _host(ss[i])
        want, tol = ar.ema64(s, p, num_updates, decay)
        worst.check(label, "shadow", got, want, tol)
        assert ar.bits_equal(got, ar.ema32(s, p, num_updates, decay)), f"{label}: differs from the fp32 literal"
        assert ar.bits_equal(_host(ps[i]), p), f"{label}: the parameter was written"
        pb, sb = (_host(b) for b in bufs[i])
        assert np.isnan(sb[:s_off]).all() and np.isnan(sb[s_off + size:]).all() and np.isnan(pb[:p_off]).all() and np.isnan(pb[p_off + size:]).all(), f"{label}: wrote past its end"
    worst.show(f"opt_ema_update num_updates={num_updates} decay={decay}")
