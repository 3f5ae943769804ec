"""k_codebook_adam_sel's rolling four-table pipeline (csrc/optim.hip) against the untouched host-selected pass, bit for bit.

The device-selected pass (opt_codebook_adam_sel / opt_codebook_adam_sel_next) resolves the message once per wave and walks the D selected tables through
four register slots, two columns half a table apart per thread; opt_codebook_adam (k_codebook_adam) takes the selected tables and their two scalars from the host and walks them one by one.  Both
apply adam_update4 to the same operands, so for the same tables and the same scalars every parameter and both moments must be EQUAL -- for every D % 4,
for D below one trip, at the workload's D = 32, for every shape of the walk's end (D = 9 .. 13: one full trip, then a tail that still issues requests and runs a
second tail trip; D = 12: two full trips) and above 32 up to the limit of 64, where the selection uses lanes 32 .. 63 of the ballot masks, readlane indices from 32
on and the upper half of the 64-bit masks; the unselected tables must not be touched, the step counts advance for the selected tables only, and
S_next must equal opt_codebook_presum_sel over the updated tables.  A disagreement is a bug in the pipeline's body, not a tolerance question."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

T = 1 << 19                      # NSIG_TABLE_ROWS: the table size is the library's compile-time constant, so "small" means few tables
D_MAX = 64                       # NSIG_MAX_MESSAGE_DIM
BETA1, BETA2, EPS, LR, GRAD_SCALE = 0.9, 0.99, 1e-15, 1e-2, 0.5
DS = (1, 2, 3, 4, 5, 7, 8, 32, 6, 9, 11, 12, 13, 33, 48, 63, 64)
KINDS = ("same", "complement", "alternating", "random")


def _scalars(step):
    return LR / (1.0 - BETA1 ** step), 1.0 / np.sqrt(1.0 - BETA2 ** step)


def _host_adam(nv, G, p, m, v, ss, ib, grad_scale):
    """The untouched host-selected pass over the tables p (moments m, v) with the scalars ss / ib."""
    n = len(p)
    fl = ctypes.c_float * n
    nv.call("opt_codebook_adam", nv.ptr(G), nv.ptr_array(p), nv.ptr_array(m), nv.ptr_array(v), n, BETA1, BETA2, EPS, fl(*ss), fl(*ib), float(grad_scale), nv.stream())


@pytest.fixture(scope="module")
def state():
    """2 * D_MAX tables with random parameters and the moments two earlier steps (other gradients, the host-selected pass) left; per-table step counts; this
    step's gradient.  Computed once, never modified: every case works on clones."""
    from nerf_signature_amd import _native as nv
    gen = torch.Generator(device="cuda").manual_seed(1234)
    n = 2 * D_MAX
    p = [torch.randn(T, 2, device="cuda", generator=gen) * 0.05 for _ in range(n)]
    m = [torch.zeros(T, 2, device="cuda") for _ in range(n)]
    v = [torch.zeros(T, 2, device="cuda") for _ in range(n)]
    for it in (1, 2):
        G = torch.randn(T, 2, device="cuda", generator=gen) * (0.1 ** it)
        G[::5] = 0                                        # rows no ray touched
        for first in range(0, n, D_MAX):                  # (the host-selected pass takes at most D_MAX tables)
            ss, ib = zip(*(_scalars(it) for _ in range(D_MAX)))
            _host_adam(nv, G, p[first:first + D_MAX], m[first:first + D_MAX], v[first:first + D_MAX], ss, ib, 1.0)
    steps = [float(2 + (7 * t) % 11) for t in range(n)]   # the counts differ per table
    G = torch.randn(T, 2, device="cuda", generator=gen) * 1e-3
    G[::3] = 0
    torch.cuda.synchronize()
    return {"p": p, "m": m, "v": v, "steps": steps, "G": G}


def _messages(D, kind):
    if kind == "random":
        rs = np.random.RandomState(100 + D)
        cur, nxt = rs.randint(0, 2, D), rs.randint(0, 2, D)
    else:
        cur = np.arange(D) % 2 if kind == "alternating" else np.random.RandomState(7 * D).randint(0, 2, D)
        if D > 32:
            cur[32] = 1                                   # (D = 33: the one bit of the masks' upper half is set)
        nxt = {"same": cur, "complement": 1 - cur, "alternating": (np.arange(D) // 2) % 2}[kind]     # alternating: 0101.. then 0011..: partner rows at bits 1, 2 of every 4
    return cur.astype(np.float32), nxt.astype(np.float32)


@pytest.mark.parametrize("with_next", (False, True), ids=("plain", "next"))
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("D", DS)
def test_device_selected_pipeline_equals_host_selected_pass(state, D, kind, with_next):
    from nerf_signature_amd import _native as nv
    from nerf_signature_amd import fieldops as fo
    n = 2 * D
    cur, nxt = _messages(D, kind)
    if D > 32:
        assert cur[32:].any(), "no selected bit in the upper half of the 64-bit masks"
    p, m, v = ([t.clone() for t in state[k][:n]] for k in ("p", "m", "v"))
    steps = [torch.tensor(s, device="cuda") for s in state["steps"][:n]]
    msg, nmsg = torch.from_numpy(cur).cuda(), torch.from_numpy(nxt).cuda()
    lr, scratch, S = torch.tensor(LR, device="cuda"), torch.full((2 * D,), float("nan"), device="cuda"), torch.full((T, 2), float("nan"), device="cuda")
    head = (nv.ptr(state["G"]), nv.ptr_array(p), nv.ptr_array(m), nv.ptr_array(v), nv.ptr_array(steps), nv.ptr(msg), D, nv.ptr(lr), BETA1, BETA2, EPS, GRAD_SCALE,
            nv.ptr(scratch))
    if with_next:
        nv.call("opt_codebook_adam_sel_next", *head, nv.ptr(nmsg), nv.ptr(S), nv.stream())
    else:
        nv.call("opt_codebook_adam_sel", *head, nv.stream())
    sel = [2 * i + int(cur[i]) for i in range(D)]

    # the step counts: + 1 for the selected tables only
    got_steps = [float(s) for s in steps]
    assert got_steps == [state["steps"][t] + (1.0 if t in sel else 0.0) for t in range(n)]
    # the unselected tables and their moments: untouched
    for t in set(range(n)) - set(sel):
        assert torch.equal(p[t], state["p"][t]) and torch.equal(m[t], state["m"][t]) and torch.equal(v[t], state["v"][t]), f"unselected table {t} was written"
    # the selected ones: what the host-selected pass leaves, given the same tables and the same two scalars per table (the ones the device derived)
    sc = scratch.cpu().numpy()
    assert np.isfinite(sc).all()
    np.testing.assert_allclose(sc[:D], [_scalars(got_steps[t])[0] for t in sel], rtol=1e-6)
    np.testing.assert_allclose(sc[D:], [_scalars(got_steps[t])[1] for t in sel], rtol=1e-6)
    rp, rm, rv = ([state[k][t].clone() for t in sel] for k in ("p", "m", "v"))
    _host_adam(nv, state["G"], rp, rm, rv, sc[:D].tolist(), sc[D:].tolist(), GRAD_SCALE)
    for i, t in enumerate(sel):
        assert not torch.equal(p[t], state["p"][t])      # (it was updated at all)
        assert torch.equal(p[t], rp[i]), f"D={D}: parameters of table {t} (bit {i}) differ"
        assert torch.equal(m[t], rm[i]), f"D={D}: exp_avg of table {t} (bit {i}) differs"
        assert torch.equal(v[t], rv[i]), f"D={D}: exp_avg_sq of table {t} (bit {i}) differs"
    # S_next: the stand-alone pre-sum of the next message over the tables as updated
    if with_next:
        assert torch.equal(S, fo.codebook_presum_sel(p, nmsg))
    else:
        assert bool(torch.isnan(S).all())                # the plain form writes no S_next
