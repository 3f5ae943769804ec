"""The occupancy walk against the C oracle, bit for bit, on the inputs of tests/march_scenes.py: rays of all eight sign octants and the degenerate
ones (axis-parallel, signed zeros, through cell corners, along cell faces, grazing a box face, from inside the box), sparse and alternating
occupancy, grid sizes 8 to 256, the sample cap inside a chunk, a constant step that ties in fp32 (the closed-form chunk's fallback) and starts
below t = 0.25, and the last cell of a grid with more than 2^24 bits (whose float bit index, raymarching.cu:339,378, rounds to one past the bitfield).  tests/test_march_scenes_cpu.py asserts, with the oracle alone, that every case really holds what it is named for.

Both launch routes of the training march run on every case -- count + scan + write, and count_nf (which computes near / far itself) + scan_write
-- for all four instantiations of the walk kernel, and the eval burst runs through rm_march and rm_eval_march.  No tolerance anywhere: the oracle
is sequential fp32 C (oracle/raymarch_ref.c) and the kernels claim the sequential walk's rounding."""
import numpy as np
import pytest
import torch

import march_scenes as ms
from oracle import raymarch_ref as orm

pytestmark = pytest.mark.gpu

_FILL = 7.0          # every output buffer starts with it: a row nobody wrote is seen


@pytest.fixture(scope="module")
def nv():
    from nerf_signature_amd import _native
    return _native


def _cuda(a):
    return None if a is None else torch.from_numpy(np.array(a, order="C")).cuda()       # (a copy: the shared references are read-only)


def _same_bits(got, want, what):
    """value-equal (the readable message) and then bit-equal: signed zeros and NaN payloads count"""
    got = got.cpu().numpy()
    np.testing.assert_array_equal(got, want, err_msg=what)
    assert np.array_equal(got.view(np.int32), np.ascontiguousarray(want).view(np.int32)), f"{what}: equal values, different bits (a signed zero)"


def _device(case):
    bits, o, d, nz, aabb = ms.inputs(case)
    return _cuda(bits), _cuda(o), _cuda(d), _cuda(nz), _cuda(aabb)


def _train_march(nv, case, dev, ref, route, M):
    """one training march into M rows by one of the two launch routes: (nears, fars, counts, rays, counter, xyzs, dirs, deltas)"""
    bits, o, d, nz, aabb = dev
    N = o.shape[0]
    geom = (float(case.bound), float(case.dt_gamma), case.max_steps)
    i32, f32 = dict(dtype=torch.int32, device="cuda"), dict(dtype=torch.float32, device="cuda")
    counts, rays, ctr = torch.full((N,), -3, **i32), torch.full((N, 3), -9, **i32), torch.full((2,), -5, **i32)
    t_rec = torch.full((N * case.max_steps,), float("nan"), **f32)
    x, dd, dl = torch.full((M, 3), _FILL, **f32), torch.full((M, 3), _FILL, **f32), torch.full((M, 2), _FILL, **f32)
    if route == "count+scan+write":
        nears, fars = _cuda(ref.nears), _cuda(ref.fars)
        nv.call("rm_march_train_count", nv.ptr(o), nv.ptr(d), nv.ptr(bits), *geom, N, case.C, case.H, nv.ptr(nears), nv.ptr(fars), nv.ptr(nz), nv.ptr(counts),
                nv.ptr(t_rec), nv.stream())
        nv.call("rm_march_train_scan", nv.ptr(counts), N, nv.ptr(rays), nv.ptr(ctr), nv.stream())
        nv.call("rm_march_train_write", nv.ptr(o), nv.ptr(d), *geom, N, case.C, case.H, M, nv.ptr(nears), nv.ptr(nz), nv.ptr(t_rec), nv.ptr(rays), nv.ptr(ctr),
                nv.ptr(x), nv.ptr(dd), nv.ptr(dl), nv.stream())
    else:
        nears, fars = torch.full((N,), -1.0, **f32), torch.full((N,), -1.0, **f32)
        nv.call("rm_march_train_count_nf", nv.ptr(o), nv.ptr(d), nv.ptr(aabb), float(case.min_near), nv.ptr(bits), *geom, N, case.C, case.H, nv.ptr(nz),
                nv.ptr(nears), nv.ptr(fars), nv.ptr(counts), nv.ptr(t_rec), nv.stream())
        nv.call("rm_march_train_scan_write", nv.ptr(o), nv.ptr(d), *geom, N, case.C, case.H, M, nv.ptr(nears), nv.ptr(nz), nv.ptr(t_rec), nv.ptr(counts),
                nv.ptr(rays), nv.ptr(ctr), nv.ptr(x), nv.ptr(dd), nv.ptr(dl), nv.stream())
    return nears, fars, counts, rays, ctr, x, dd, dl


ROUTES = ("count+scan+write", "count_nf+scan_write")


_TRAIN_CASES = ms.CASES + (ms.BORDER,)


@pytest.mark.parametrize("case", _TRAIN_CASES, ids=[c.name for c in _TRAIN_CASES])
def test_training_walk_equals_the_oracle(nv, case):
    """The (id, offset, count) table, the counter and every row of xyzs / dirs / deltas with the zero padding, by both routes; on the second the walk's
    own near / far as well.  Cases marked half_capacity run again with room for half the samples: the same rays are dropped (raymarching.cu:416).
    The last case (march_scenes.BORDER) is built so that a step lands exactly on a cell's exit at the first index of a chunk."""
    ref = ms.reference(case)
    dev = _device(case)
    total = int(ref.counter[0])
    rooms = [(ref.xyzs.shape[0], ref.xyzs, ref.dirs, ref.deltas)]
    if case.half_capacity:
        bits, o, d, nz, _ = ms.inputs(case)
        M = max(128, (total // 2) // 128 * 128)
        x, dd, dl, table = orm.march_rays_train(o, d, case.bound, bits, case.C, case.H, ref.nears, ref.fars, None, M, case.noise, -1, False, case.dt_gamma,
                                                case.max_steps, noises=nz)
        np.testing.assert_array_equal(table, ref.rays)
        fits = ref.rays[:, 1] + ref.rays[:, 2] <= M
        assert x.shape[0] == M < total and (~fits & (ref.rays[:, 2] > 0)).any() and (fits & (ref.rays[:, 2] > 0)).any()       # some rays dropped, some kept
        rooms.append((M, x, dd, dl))
    for M, want_x, want_d, want_dl in rooms:
        for route in ROUTES:
            what = f"{case.name} {route} M={M}"
            nears, fars, counts, rays, ctr, x, dd, dl = _train_march(nv, case, dev, ref, route, M)
            np.testing.assert_array_equal(counts.cpu().numpy(), ref.rays[:, 2], err_msg=f"{what}: counts")
            np.testing.assert_array_equal(rays.cpu().numpy(), ref.rays, err_msg=f"{what}: (id, offset, count)")
            np.testing.assert_array_equal(ctr.cpu().numpy(), ref.counter, err_msg=f"{what}: counter")
            if route == "count_nf+scan_write":
                _same_bits(nears, ref.nears, f"{what}: nears")
                _same_bits(fars, ref.fars, f"{what}: fars")
            _same_bits(x, want_x, f"{what}: xyzs")
            _same_bits(dd, want_d, f"{what}: dirs")
            _same_bits(dl, want_dl, f"{what}: deltas")


N = ms.N_RAYS


def _burst_starts(ref, rng):
    """rays_t [N]: the nears; a parameter uniform in [near, far]; a value >= far (far itself and the next float above it, alternating)"""
    with np.errstate(over="ignore", invalid="ignore"):
        inside = (ref.nears + rng.rand(N).astype(np.float32) * (ref.fars - ref.nears)).astype(np.float32)
        inside = np.where(np.isfinite(inside), inside, ref.nears)
        beyond = np.where(np.arange(N) % 2 == 0, ref.fars, np.nextafter(ref.fars, np.float32(np.inf))).astype(np.float32)
    return (("near", ref.nears), ("inside", inside), ("beyond", beyond))


@pytest.mark.parametrize("case", ms.EVAL_CASES, ids=[c.name for c in ms.EVAL_CASES])
def test_eval_burst_equals_the_oracle(nv, case):
    """rm_march and rm_eval_march (control words written here) on a shuffled subset of the rays: n_step 1, 3, 8, 64 from three kinds of rays_t; the rows of
    a ray that ends inside its burst are zero, rows behind the burst keep what the buffer held (rm_eval_march) or are zero (rm_march's padding)."""
    ref = ms.reference(case)
    host_bits, ho, hd, _, _ = ms.inputs(case)
    bits, o, d, _, _ = _device(case)
    rng = np.random.RandomState(500 + case.seed)
    n_alive = 150
    alive = rng.permutation(N)[:n_alive].astype(np.int32)
    noises = ms.noises(n_alive, 3000 + case.seed) if case.noise else None
    fars, nears, alive_d, noises_d = _cuda(ref.fars), _cuda(ref.nears), _cuda(alive), _cuda(noises)
    geom = (float(case.bound), float(case.dt_gamma), case.max_steps, case.C, case.H)
    f32 = dict(dtype=torch.float32, device="cuda")
    some_rows = False
    for which, t in _burst_starts(ref, rng):
        t_d = _cuda(t)
        for n_step in (1, 3, 8, 64):
            what = f"{case.name} rays_t={which} n_step={n_step}"
            rows = n_alive * n_step
            want = orm.march_rays(n_alive, n_step, alive, t, ho, hd, case.bound, host_bits, case.C, case.H, ref.nears, ref.fars, 128, False, case.dt_gamma,
                                  case.max_steps, noises=noises if noises is not None else np.zeros(n_alive, np.float32))
            M = want[0].shape[0]
            assert M % 128 == 0 and M > rows
            if which == "beyond":
                assert not want[2].any()            # no ray takes a step
            else:
                some_rows = some_rows or bool(want[2].any())
            got = [torch.full((M, k), _FILL, **f32) for k in (3, 3, 2)]
            nv.call("rm_march", n_alive, n_step, nv.ptr(alive_d), nv.ptr(t_d), nv.ptr(o), nv.ptr(d), *geom, nv.ptr(bits), nv.ptr(nears), nv.ptr(fars),
                    *(nv.ptr(g) for g in got), nv.ptr(noises_d), M, nv.stream())
            for g, w, name in zip(got, want, ("xyzs", "dirs", "deltas")):
                _same_bits(g, w, f"{what}: rm_march {name}")
            # the launch of rm_eval_march covers a capacity larger than the burst; the counts are on the device
            cap = rows + 37
            ctl = _cuda(np.array([n_alive, n_step, rows, 0], np.uint32).view(np.int32))
            got = [torch.full((cap, k), _FILL, **f32) for k in (3, 3, 2)]
            nv.call("rm_eval_march", nv.ptr(ctl), cap, nv.ptr(alive_d), nv.ptr(t_d), nv.ptr(o), nv.ptr(d), *geom, nv.ptr(bits), nv.ptr(fars),
                    *(nv.ptr(g) for g in got), nv.ptr(noises_d), nv.stream())
            for g, w, name in zip(got, want, ("xyzs", "dirs", "deltas")):
                _same_bits(g[:rows], w[:rows], f"{what}: rm_eval_march {name}")
                assert bool((g[rows:] == _FILL).all()), f"{what}: rm_eval_march wrote {name} behind the burst"
            assert ctl.cpu().numpy().view(np.uint32).tolist() == [n_alive, n_step, rows, 0]
    assert some_rows or case.kind in ("empty", "specks")
