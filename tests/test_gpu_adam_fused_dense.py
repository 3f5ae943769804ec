"""opt_codebook_adam_sel_next_dense (csrc/optim.hip) against the two passes it folds into one launch, bit for bit.

The fused launch's first 512 workgroups run opt_codebook_adam_sel[_next]'s walk, the ones behind them opt_adam_dense's chunk bodies over the dense tensors, and its one
prepare launch advances both kinds of step counts.  Same adam_update / adam_update4 calls on the same operands with the same device scalars: every selected and
unselected table, both moments, every step count, S_next, and every dense tensor with its moments must be EQUAL to what opt_codebook_adam_sel[_next] followed by
opt_adam_dense leave.  The two gradient scales differ (as in trainer._optimise), so a swapped scale shows.

Dense sizes straddle the scalar form's chunk (kDenseChunk = 1024 elements) and the wide form's (kDenseChunk4 = 4096); a tensor of 65 540 elements makes the group
a wide one (kDenseBigNumel), in which aligned multiple-of-4 tensors from 1024 elements on take the float4 form and the others -- odd sizes, a misaligned view --
the scalar form, all in ONE chunk table; without it every tensor takes the scalar form.  An empty list is the plain launch."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

T = 1 << 19                      # NSIG_TABLE_ROWS
D_MAX = 32
K, K4 = 1024, 4096               # kDenseChunk, kDenseChunk4
BETA1, BETA2, EPS, LR = 0.9, 0.99, 1e-15, 1e-2
SCALE_CODEBOOK, SCALE_DENSE = 0.5, 0.25
DENSE_SCRATCH_BYTES = 2048       # NSIG_ADAM_DENSE_SCRATCH_BYTES
SCALAR_SIZES = (1, 3, 4, K - 1, K, K + 1, 2 * K + 1)
# with the 65 540-element tensor in the group: 1024 / 1028 / 4096 / 4100 / 8192 ride along in the wide form, the odd sizes and the misaligned view (below) do not
WIDE_SIZES = (65540, 1, 3, 4, K - 1, K, K + 1, K + 4, 2 * K + 1, K4 - 4, K4, K4 + 4, 2 * K4)
DENSE_LISTS = {"scalar": SCALAR_SIZES, "wide": WIDE_SIZES}


@pytest.fixture(scope="module")
def state():
    """2 * D_MAX tables, their moments and step counts, a gradient; dense tensors of every size in DENSE_LISTS with gradients, moments and step counts.  Computed once,
    never modified: every case works on clones."""
    gen = torch.Generator(device="cuda").manual_seed(4321)
    n = 2 * D_MAX
    rnd = lambda *shape, s=1.0: torch.randn(*shape, device="cuda", generator=gen) * s
    st = {"p": [rnd(T, 2, s=0.05) for _ in range(n)], "m": [rnd(T, 2, s=1e-3) for _ in range(n)], "v": [rnd(T, 2, s=1e-3) ** 2 for _ in range(n)],
          "steps": [float(2 + (7 * t) % 11) for t in range(n)], "G": rnd(T, 2, s=1e-3)}
    st["G"][::3] = 0
    sizes = sorted(set(SCALAR_SIZES) | set(WIDE_SIZES))
    st["dense"] = {s: {"p": rnd(s, s=0.1), "g": rnd(s, s=1e-2), "m": rnd(s, s=1e-3), "v": rnd(s, s=1e-3) ** 2, "step": float(1 + s % 5)} for s in sizes}
    # a multiple of 4 elements, 4 bytes off a 16-byte boundary: the scalar form whatever the group (key -1)
    st["dense"][-1] = {"p": rnd(K4 + 1, s=0.1), "g": rnd(K4 + 1, s=1e-2), "m": rnd(K4 + 1, s=1e-3), "v": rnd(K4 + 1, s=1e-3) ** 2, "step": 3.0}
    torch.cuda.synchronize()
    return st


def _dense_clones(state, sizes):
    """Clones of the dense tensors of `sizes` (+ the misaligned view when the list is not empty): lists p, g, m, v, steps."""
    out = {k: [] for k in ("p", "g", "m", "v", "step")}
    for s in sizes:
        d = state["dense"][s]
        for k in ("p", "g", "m", "v"):
            out[k].append(d[k].clone())
        out["step"].append(torch.tensor(d["step"], device="cuda"))
    if sizes:
        d = state["dense"][-1]
        for k in ("p", "g", "m", "v"):
            t = d[k].clone()[1:]
            assert t.data_ptr() % 16 == 4 and t.numel() % 4 == 0
            out[k].append(t)
        out["step"].append(torch.tensor(d["step"], device="cuda"))
    return out


def _codebook_clones(state, D):
    n = 2 * D
    p, m, v = ([t.clone() for t in state[k][:n]] for k in ("p", "m", "v"))
    return p, m, v, [torch.tensor(s, device="cuda") for s in state["steps"][:n]]


def _run(nv, state, D, msg, nmsg, sizes, fused, with_next):
    """One optimiser step from the fixture's state: the fused launch, or the two separate passes.  Returns everything the step may write."""
    p, m, v, steps = _codebook_clones(state, D)
    dn = _dense_clones(state, sizes)
    n_dense = len(dn["p"])
    lr = torch.tensor(LR, device="cuda")
    scratch, S = torch.full((2 * D,), float("nan"), device="cuda"), torch.full((T, 2), float("nan"), device="cuda")
    head = (nv.ptr(state["G"]), nv.ptr_array(p), nv.ptr_array(m), nv.ptr_array(v), nv.ptr_array(steps), nv.ptr(msg), D, nv.ptr(lr), BETA1, BETA2, EPS, SCALE_CODEBOOK,
            nv.ptr(scratch))
    numel = (ctypes.c_uint32 * max(n_dense, 1))(*[t.numel() for t in dn["p"]])
    lists = [nv.ptr_array(dn[k]) for k in ("p", "g", "m", "v", "step")]
    if fused:
        dense_scratch = torch.zeros(DENSE_SCRATCH_BYTES, dtype=torch.uint8, device="cuda")
        nv.call("opt_codebook_adam_sel_next_dense", *head, nv.ptr(nmsg) if with_next else None, nv.ptr(S) if with_next else None, n_dense, *lists, numel, SCALE_DENSE,
                nv.ptr(dense_scratch), nv.stream())
    else:
        if with_next:
            nv.call("opt_codebook_adam_sel_next", *head, nv.ptr(nmsg), nv.ptr(S), nv.stream())
        else:
            nv.call("opt_codebook_adam_sel", *head, nv.stream())
        if n_dense:
            dscratch = torch.zeros(64, device="cuda")
            nv.call("opt_adam_dense", n_dense, lists[0], lists[1], lists[2], lists[3], lists[4], numel, nv.ptr(lr), BETA1, BETA2, EPS, SCALE_DENSE, nv.ptr(dscratch),
                    nv.stream())
    torch.cuda.synchronize()
    return {"p": p, "m": m, "v": v, "steps": steps, "S": S, "dp": dn["p"], "dm": dn["m"], "dv": dn["v"], "dsteps": dn["step"], "dg": dn["g"]}


def _messages(D):
    gen = torch.Generator().manual_seed(10 + D)
    return (torch.randint(0, 2, (D,), generator=gen).float().cuda(), torch.randint(0, 2, (D,), generator=gen).float().cuda())


def _assert_equal(got, want, what):
    for key in ("p", "m", "v", "steps", "dp", "dm", "dv", "dsteps", "dg"):
        assert len(got[key]) == len(want[key])
        for i, (a, b) in enumerate(zip(got[key], want[key])):
            assert torch.equal(a, b), f"{what}: {key}[{i}] differs"
    assert torch.equal(got["S"].view(torch.int32), want["S"].view(torch.int32)), f"{what}: S_next differs"      # (as bits: the plain form leaves the NaN fill)


@pytest.mark.parametrize("with_next", (False, True), ids=("plain", "next"))
@pytest.mark.parametrize("dense", sorted(DENSE_LISTS))
@pytest.mark.parametrize("D", (1, 3, 4, 5, 32))
def test_fused_launch_equals_the_two_separate_passes(state, D, dense, with_next):
    from nerf_signature_amd import _native as nv
    msg, nmsg = _messages(D)
    sizes = DENSE_LISTS[dense]
    got = _run(nv, state, D, msg, nmsg, sizes, True, with_next)
    want = _run(nv, state, D, msg, nmsg, sizes, False, with_next)
    _assert_equal(got, want, f"D={D}, {dense}")
    # ... and the step did something: every dense tensor moved, its count advanced once, the selected tables moved, the others did not
    srcs = [state["dense"][s] for s in sizes] + [state["dense"][-1]]
    for i, src in enumerate(srcs):
        ref = src["p"] if i < len(sizes) else src["p"][1:]
        assert not torch.equal(got["dp"][i], ref) and float(got["dsteps"][i]) == src["step"] + 1.0
    sel = {2 * i + int(msg[i]) for i in range(D)}
    for t in range(2 * D):
        assert torch.equal(got["p"][t], state["p"][t]) == (t not in sel)
        assert float(got["steps"][t]) == state["steps"][t] + (1.0 if t in sel else 0.0)


@pytest.mark.parametrize("with_next", (False, True), ids=("plain", "next"))
def test_an_empty_dense_list_is_the_plain_launch(state, with_next):
    from nerf_signature_amd import _native as nv
    msg, nmsg = _messages(5)
    _assert_equal(_run(nv, state, 5, msg, nmsg, (), True, with_next), _run(nv, state, 5, msg, nmsg, (), False, with_next), "no dense tensors")


def test_refusals_keep_the_existing_wording(state):
    """A null or misaligned table, a null dense tensor, an empty one, too many of them, next_message without S_next: refused before anything is launched."""
    from nerf_signature_amd import _native as nv
    D = 2
    p, m, v, steps = _codebook_clones(state, D)
    dn = _dense_clones(state, (4, K))
    n_dense = len(dn["p"])
    msg, nmsg = _messages(D)
    lr, scratch, S = torch.tensor(LR, device="cuda"), torch.zeros(2 * D, device="cuda"), torch.zeros(T, 2, device="cuda")
    dense_scratch = torch.zeros(DENSE_SCRATCH_BYTES, dtype=torch.uint8, device="cuda")
    numel = (ctypes.c_uint32 * n_dense)(*[t.numel() for t in dn["p"]])
    name = "opt_codebook_adam_sel_next_dense"

    def call(tables=None, dense_p=None, numel_=numel, n=n_dense, S_next=S):
        nv.call(name, nv.ptr(state["G"]), tables or nv.ptr_array(p), nv.ptr_array(m), nv.ptr_array(v), nv.ptr_array(steps), nv.ptr(msg), D, nv.ptr(lr), BETA1, BETA2, EPS,
                SCALE_CODEBOOK, nv.ptr(scratch), nv.ptr(nmsg), nv.ptr(S_next) if S_next is not None else None, n, dense_p or nv.ptr_array(dn["p"]), nv.ptr_array(dn["g"]),
                nv.ptr_array(dn["m"]), nv.ptr_array(dn["v"]), nv.ptr_array(dn["step"]), numel_, SCALE_DENSE, nv.ptr(dense_scratch), nv.stream())

    def refused(message, **kw):
        with pytest.raises(ValueError) as e:
            call(**kw)
        assert str(e.value) == f"{name} failed (code 1): {name}: {message}"

    ptrs = [t.data_ptr() for t in p]
    refused("table 1 has a null pointer", tables=(ctypes.c_void_p * 4)(ptrs[0], None, ptrs[2], ptrs[3]))
    refused("table 2 is not 16-byte aligned", tables=(ctypes.c_void_p * 4)(ptrs[0], ptrs[1], ptrs[2] + 8, ptrs[3]))
    dptrs = [t.data_ptr() for t in dn["p"]]
    refused("tensor 1 has a null pointer or no elements", dense_p=(ctypes.c_void_p * n_dense)(dptrs[0], None, dptrs[2]))
    refused("tensor 0 has a null pointer or no elements", numel_=(ctypes.c_uint32 * n_dense)(0, K, K4))
    refused("at most 32 dense tensors ride in the launch", n=33)
    refused("next_message / S_next go together and S_next is 16-byte aligned", S_next=None)
    torch.cuda.synchronize()
    # nothing was launched: tables, dense tensors and every step count are what they were
    assert all(torch.equal(a, b) for a, b in zip(p, state["p"])) and [float(s) for s in steps] == state["steps"][:2 * D]
    assert torch.equal(dn["p"][0], state["dense"][4]["p"]) and float(dn["step"][0]) == state["dense"][4]["step"]
