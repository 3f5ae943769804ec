"""The tampering kernels (csrc/tamper.hip) against their host restatement (tests/tamper_ref.py) at the smallest shapes where each can go wrong: one element,
sizes around the wave (63, 64, 65) and the workgroup (255, 256, 257), an empty tensor inside a list, 33 tensors (two launch groups), and 2^20 + 3 elements
(258 chunks: more than the select's 256 workgroups, so a workgroup walks more than one chunk, and a ragged last chunk)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tamper_ref as tr  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = {"one": [1], "wave": [63, 64, 65], "group": [255, 256, 257], "empty-inside": [1025, 0, 7], "33-tensors": [5] * 33, "258-chunks": [(1 << 20) + 3, 5]}
VALUES = ("normal", "equal", "two", "low-byte", "special")


def make(sizes, values, seed=0):
    """The host arrays of one case (float32)."""
    rng = np.random.RandomState(seed)
    out, at = [], 0
    for t, n in enumerate(sizes):
        if values == "normal":
            a = (rng.randn(n) * 10.0 ** ((t % 5) - 2)).astype(np.float32)
        elif values == "equal":
            a = np.full(n, 1.5, np.float32)
        elif values == "two":
            a = rng.choice(np.array([0.25, -3.0], np.float32), n)
        elif values == "low-byte":
            bits = (np.uint32(0x3F800000) + ((np.arange(at, at + n) % 256).astype(np.uint32))) | (rng.randint(0, 2, n).astype(np.uint32) << np.uint32(31))
            a = bits.view(np.float32)
        else:
            a = rng.randn(n).astype(np.float32)
            special = np.array([0.0, -0.0, 1e-45, -1e-40, np.inf, -np.inf, 3e-39], np.float32)
            where = rng.rand(n) < 0.3
            a[where] = special[rng.randint(0, len(special), int(where.sum()))]
            if at == 0 and n:
                a[0] = np.nan                                    # exactly one NaN in the whole list
        out.append(a)
        at += n
    return out


def device(arrays):
    return [torch.from_numpy(a.copy()).cuda() for a in arrays]


def bits_of(t):
    return t.detach().cpu().numpy().view(np.uint32)


def same_bits(tensors, arrays):
    return all(np.array_equal(bits_of(t), np.asarray(a, np.float32).view(np.uint32)) for t, a in zip(tensors, arrays))


def ranks(total):
    return sorted({k for k in (1, 2, total // 2, total - 1, total) if 1 <= k <= total})


CASES = [pytest.param(s, v, id=f"{s}-{v}") for s in SIZES for v in VALUES]


@pytest.mark.parametrize("sizes,values", CASES)
def test_select_is_exact(sizes, values):
    from nerf_signature_amd import tamper
    arrays = make(SIZES[sizes], values)
    launch = tamper._Launch(device(arrays))
    got = [launch.abs_kth(k, out=(torch.empty(1, dtype=torch.int32, device="cuda"), torch.empty(1, dtype=torch.int64, device="cuda"))) for k in ranks(launch.total)]
    for k, (thr, le) in zip(ranks(launch.total), got):                       # (all enqueued first: one scratch, stream-ordered)
        want = tr.abs_kth(arrays, k)
        have = (int(thr.cpu().numpy().view(np.uint32)[0]), int(le.item()))
        print(f"k={k}: threshold_bits {have[0]:#010x} count_le {have[1]} (restatement {want[0]:#010x} {want[1]})")
        assert have == want


@pytest.mark.parametrize("sizes,values", CASES)
def test_prune(sizes, values):
    from nerf_signature_amd import tamper
    arrays = make(SIZES[sizes], values, seed=1)
    live = device(arrays)
    tm = tamper.Tamper(live)
    for p in (0.5, 0.3):
        tm.apply("prune", p)
        assert same_bits(live, tr.prune_fraction(arrays, p)), p
    tm.apply("prune", 0.5)
    once = [t.clone() for t in live]
    tm.apply("prune", 0.5)                                                    # from the pristine copy again: calls never accumulate
    assert same_bits(live, [bits_of(t).view(np.float32) for t in once])
    k = int(round(0.5 * tm.total))
    if k:                                                                     # ... and on its own result, in place, with its own threshold: nothing more goes
        thr, _ = tamper.abs_kth(live, k)
        tamper.apply(live, live, "prune", threshold=thr)
        assert same_bits(live, tr.prune_fraction(arrays, 0.5))
    tm.apply("prune", 0.0)
    assert same_bits(live, arrays)
    tm.apply("prune", 1.0)
    assert all(not bits_of(t).any() for t in live)                            # +0.0 everywhere, the NaN and -0.0 included
    tm.restore()
    assert same_bits(live, arrays)


@pytest.mark.parametrize("sizes", list(SIZES))
def test_quantise_and_half(sizes):
    from nerf_signature_amd import tamper
    arrays = make(SIZES[sizes], "normal", seed=2)
    if arrays[0].size > 4:
        arrays[0][1], arrays[0][3] = np.inf, np.nan                           # pass through, and do not enter min / max
    arrays[-1][...] = -0.75                                                   # a constant tensor: unchanged
    arrays[0][0] = 70000.0                                                    # above 65504
    live = device(arrays)
    tm = tamper.Tamper(live)
    for b in (2, 8, 16):
        tm.apply("quantize", b)
        assert same_bits(live, tr.quantize(arrays, b)), b
        assert same_bits(live[-1:], arrays[-1:])
    tm.apply("half")
    assert same_bits(live, tr.half(arrays))
    assert same_bits(live, [t.half().float().cpu().numpy() for t in device(arrays)])
    assert np.isinf(live[0][0].item())


@pytest.mark.parametrize("sizes", list(SIZES))
def test_statistics(sizes):
    from nerf_signature_amd import tamper
    arrays = make(SIZES[sizes], "normal", seed=3)
    if arrays[0].size > 4:
        arrays[0][2], arrays[0][4] = -np.inf, np.nan
    launch = tamper._Launch(device(arrays))
    got = launch.stats()
    again = launch.stats()
    assert torch.equal(got, again)                                            # fixed reduction shape
    got = got.cpu().numpy()
    for a, g in zip(arrays, got):
        lo, hi, mean, std = tr.finite_stats(a)
        e_mean, e_std = tr.stats_bound(a)
        print(f"n={a.size}: mean err {abs(g[2] - mean):.3e} (bound {e_mean:.3e}), deviation err {abs(g[3] - std):.3e} (bound {e_std:.3e})")
        assert (g[0], g[1]) == (lo, hi)
        assert abs(g[2] - mean) <= e_mean and abs(g[3] - std) <= e_std


@pytest.mark.parametrize("sizes", list(SIZES))
def test_noise(sizes):
    from nerf_signature_amd import tamper
    arrays = make(SIZES[sizes], "normal", seed=4)
    live = device(arrays)
    tm = tamper.Tamper(live)
    for strength, seed in ((0.5, 0), (1.0, 12345678901234567), (0.01, 3)):
        tm.apply("noise", strength, seed=seed)
        got = [t.cpu().numpy() for t in live]
        worst = 0.0
        for a, y, (want, s, z) in zip(arrays, got, tr.noise64(arrays, strength, seed)):
            err, bound = np.abs(y.astype(np.float64) - want), tr.noise_bound(a, s, z, tr.EPS_Z)
            if a.size:
                worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
            assert np.all(err <= bound)
        print(f"strength {strength} seed {seed}: largest error / bound = {worst:.3f}")
    tm.apply("noise", 0.5, seed=0)
    first = [t.clone() for t in live]
    tm.apply("noise", 0.5, seed=0)
    assert all(torch.equal(a, b) for a, b in zip(first, live))                # two runs: the same bits
    tm.apply("noise", 0.5, seed=1)
    assert sum(a.numel() for a in live) < 4 or any(not torch.equal(a, b) for a, b in zip(first, live))
    tm.apply("noise", 0.0, seed=0)
    assert all(torch.equal(a, b) for a, b in zip(tm.pristine, live))          # x + 0 z
    # src == dst gives what the out-of-place pass gives
    inplace = device(arrays)
    st = tamper.stats(inplace)
    tamper.apply(inplace, inplace, "noise", strength=0.5, stats=st, seed=0)
    assert all(torch.equal(a, b) for a, b in zip(first, inplace))
