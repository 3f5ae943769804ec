"""The planned codebook scatter over buffers with more rows than points (hg_scatter_plan_rows, field_bwd_planned_rows, hg_scatter_planned_rows: the device row
count of a captured loop's padded sample buffers) and the single-owner form of its slice owners, against the existing entry points at the exact size, against
the float64 sum, and in one captured step.  G and the slice counts are compared; the order of the queue entries inside a chunk is not defined."""
import numpy as np
import pytest
import torch

import closed_form as cf
from oracle import field_ref as fr

pytestmark = pytest.mark.gpu
T_ROWS = 1 << 19
CB_RES = fr.level_resolutions(64, 2048, 2048)[0]
PRIME_Y, PRIME_Z = 2654435761, 805459861
ROWS = [0, 1, 31, 32, 33, 1023, 1024, 1025, 3000]
SETS = ["uniform", "cell", "n2048", "n2049"]      # cell: every point in one cell (a hot row pair, 60 slices without an entry); n2048 / n2049: a slice at fixed_scale's threshold


@pytest.fixture(scope="module")
def fo():
    from nerf_signature_amd import fieldops
    return fieldops


@pytest.fixture(scope="module")
def field(fo):
    """Base tables, a codebook pre-sum and packed MLP weights of the closed-form model, on the device."""
    base = [torch.from_numpy(cf.table(l)).cuda() for l in range(16)]
    cb = [torch.from_numpy(cf.table(100 + l, scale=0.05)).cuda() for l in range(64)]
    packed = fo.pack_weights(torch.from_numpy(cf.mlp_params(3072, 1337)).cuda(), torch.from_numpy(cf.mlp_params(7168, 1338)).cuda())
    S = fo.codebook_presum(fo.select_tables(cb, fo.message_bits(torch.from_numpy(cf.messages(32)[2]))))
    return base, S, packed


def padded(m):
    return m + 128 - m % 128      # raymarching.padded_point_count


def cell_slices(iy, iz):
    """The slices of the four (dy, dz) pairs of a cell (csrc/hashgrid.h pair_hash, pair_slice)."""
    return [((((iy + (q >> 1)) * PRIME_Y) ^ ((iz + (q & 1)) * PRIME_Z)) >> 13) & 63 for q in range(4)]


def slice_counts(pts, bound=1.0):
    """Entries per slice of world points [M,3] (fp32, CPU): four per point, by the kernels' fp32 cell arithmetic."""
    v01 = (pts + bound) / (2.0 * bound)
    cell = torch.floor(v01.clamp(0, 1) * 2048.0).long()
    counts = np.zeros(64, np.int64)
    for iy, iz in zip(cell[:, 1].tolist(), cell[:, 2].tolist()):
        for s in cell_slices(iy, iz):
            counts[s] += 1
    return counts


def _two_cells():
    """Two cells (iy, iz) with four distinct slices each and no slice in common."""
    found = []
    for iy in range(1249, 1400):
        s = cell_slices(iy, 389)
        if len(set(s)) == 4 and all(not set(s) & set(cell_slices(*c)) for c in found):
            found.append((iy, 389))
            if len(found) == 2:
                return found
    raise AssertionError("no such cells")


def points(name, rows, seed=0):
    """World points [rows, 3] in [-1, 1] (fp32, CPU) of one point set."""
    rng = np.random.RandomState(seed + rows)
    if name == "uniform":
        x01 = rng.rand(rows, 3).astype(np.float32)
    elif name == "cell":
        x01 = np.repeat(np.array([[0.37, 0.61, 0.19]], np.float32), rows, 0)
    else:      # n points inside cell A, the rest inside cell B (anywhere inside: different rows of the same slices)
        n = min(int(name[1:]), rows)
        (ay, az), (by, bz) = _two_cells()
        x01 = rng.rand(rows, 3).astype(np.float32)
        frac = 0.05 + 0.9 * rng.rand(rows, 2).astype(np.float32)
        x01[:n, 1:] = (np.array([ay, az], np.float32) + frac[:n]) / np.float32(2048)
        x01[n:, 1:] = (np.array([by, bz], np.float32) + frac[n:]) / np.float32(2048)
    return torch.from_numpy(x01 * np.float32(2) - np.float32(1))


def padded_inputs(pts, capacity, seed=1, inf_at=None):
    """(xyzs, dirs, g_sigma, g_rgb) with `capacity` rows on the device: the points and random upstream gradients, then the zero fill the march and the compositing
    backward leave behind them."""
    rows = pts.shape[0]
    rng = np.random.RandomState(seed)
    x, d = torch.zeros(capacity, 3), torch.zeros(capacity, 3)
    gs, gc = torch.zeros(capacity), torch.zeros(capacity, 3)
    x[:rows] = pts
    if rows:
        d[:rows] = torch.from_numpy(cf.unit_dirs(max(rows, 8), seed=8)[:rows])
        gs[:rows] = torch.from_numpy(rng.randn(rows).astype(np.float32))
        gc[:rows] = torch.from_numpy(rng.randn(rows, 3).astype(np.float32))
    if inf_at is not None:
        gs[inf_at] = float("inf")
    return x.cuda(), d.cuda(), gs.cuda(), gc.cuda()


def plan_counts(plan):
    return plan.buf[:256].view(torch.int32).cpu().numpy().astype(np.int64)      # BinHeader.counts


def plan_gmax_bits(plan):
    return int(plan.buf[256:260].view(torch.int32).item())


_PREFILL = None


def prefill():
    global _PREFILL
    if _PREFILL is None:
        _PREFILL = torch.from_numpy(np.random.RandomState(1).randn(T_ROWS, 2).astype(np.float32))
    return _PREFILL


def exact_launch(fo, field, pts):
    """(G, slice counts, d feature [rows, 2]) of the existing entry points sized for exactly these points, accumulated into the pre-filled G."""
    base, S, packed = field
    rows = pts.shape[0]
    x, d, gs, gc = padded_inputs(pts, rows)
    s, c, _, masks = fo.field_forward(x, d, 1.0, base, S, packed, want_masks=True)
    plan = fo.ScatterPlan(x, 1.0)
    G = fo.field_backward_planned(x, 1.0, gs, gc, s, c, masks, packed, plan, prefill().cuda())
    dfeat = fo.field_backward(x, 1.0, gs, gc, s, c, masks, packed, want_dfeat=True)
    return G.cpu(), plan_counts(plan), dfeat.cpu()


@pytest.fixture(scope="module")
def exact(fo, field):
    cache = {}

    def get(name, rows):
        if (name, rows) not in cache:
            cache[name, rows] = exact_launch(fo, field, points(name, rows))
        return cache[name, rows]

    return get


def rows_launch(fo, field, pts, capacity, rows_value=None, owners=None, G=None, inf_at=None):
    """The same through the row-aware entry points over buffers of `capacity` rows (the forward pass over all of them, as the training step runs it)."""
    base, S, packed = field
    x, d, gs, gc = padded_inputs(pts, capacity, inf_at=inf_at)
    s, c, _, masks = fo.field_forward(x, d, 1.0, base, S, packed, want_masks=True)
    rows_dev = torch.tensor([pts.shape[0] if rows_value is None else rows_value, 0], dtype=torch.int32, device="cuda")
    plan = fo.ScatterPlan(x, 1.0, rows_dev)
    G = fo.field_backward_planned(x, 1.0, gs, gc, s, c, masks, packed, plan, prefill().cuda() if G is None else G, owners=owners)
    return G, plan


@pytest.mark.parametrize("name,rows", [(name, rows) for rows in ROWS for name in SETS if name in ("uniform", "cell") or rows >= int(name[1:])])
def test_row_aware_launches_equal_the_exact_size_launch_and_lie_within_the_fixed_point_bound(fo, field, exact, name, rows):
    """Plan + backward + scatter with a device row count, over buffers of exactly the padded row count and of 1.25 times that, against the existing entry points
    at M = rows: G and the slice counts bit for bit; the counts against the cells' slices computed here; G against the float64 sum of the same feature
    gradients within the fixed-point bound of the existing scatter tests (oracle.field_ref.scatter_tolerance, quantum from the launch's largest gradient and
    4 * rows entries).  rows = 0: G stays the pre-filled one."""
    pts = points(name, rows)
    if rows:
        G_exact, counts_exact, dfeat = exact(name, rows)
        want_counts = slice_counts(pts)
        np.testing.assert_array_equal(counts_exact, want_counts)
        if name != "uniform":
            assert int((want_counts == 0).sum()) >= 56
        if name in ("n2048", "n2049"):
            assert sorted(want_counts[want_counts > 0].tolist()) == sorted([int(name[1:])] * 4 + [rows - int(name[1:])] * 4)
    else:
        G_exact, want_counts = prefill(), np.zeros(64, np.int64)
    for capacity in (padded(rows), padded(int(padded(rows) * 1.25))):
        for owners in (None, "single", "replicas"):
            G, plan = rows_launch(fo, field, pts, capacity, owners=owners)
            np.testing.assert_array_equal(plan_counts(plan), want_counts, err_msg=f"capacity {capacity} {owners}")
            np.testing.assert_array_equal(G.cpu().numpy(), G_exact.numpy(), err_msg=f"capacity {capacity} {owners}")
    if rows:
        x01 = (pts + 1.0) / 2.0
        fr.assert_scatter_close(G, prefill().double() + fr.scatter_ref(x01, dfeat, CB_RES), fr.scatter_row_stats(x01, dfeat, CB_RES), True, prefill=prefill(),
                                quantum=fr.fixed_quantum(float(dfeat.abs().max()), 4 * rows), what=f"{name} rows={rows}")


@pytest.mark.parametrize("name,rows", [("uniform", 3000), ("cell", 3000), ("n2049", 3000), ("uniform", 100000)])
def test_single_owner_equals_replicas_and_merge_on_the_same_queue(fo, field, name, rows):
    """One queue (one plan, one MLP backward), the owners in both forms: the same bits in a pre-filled G, after one launch and after a second one into the same G
    (accumulation).  100000 points: ~6250 entries per slice, two rounds of a single owner's queue walk, the last one partial."""
    base, S, packed = field
    nv = fo.nv
    pts, capacity = points(name, rows), padded(int(rows * 1.25))
    x, d, gs, gc = padded_inputs(pts, capacity)
    s, c, _, masks = fo.field_forward(x, d, 1.0, base, S, packed, want_masks=True)
    rows_dev = torch.tensor([rows, 0], dtype=torch.int32, device="cuda")
    plan = fo.ScatterPlan(x, 1.0, rows_dev)
    nv.call("field_bwd_planned_rows", nv.ptr(x), capacity, nv.ptr(rows_dev), 1.0, nv.ptr(gs), nv.ptr(gc), nv.ptr(s), nv.ptr(c), nv.ptr(masks), nv.ptr(packed), nv.ptr(plan.buf),
            nv.stream())
    got = {}
    for owners in ("single", "replicas"):
        G = prefill().cuda()
        once = None
        for _ in range(2):
            nv.call("hg_scatter_planned_rows", nv.ptr(plan.buf), capacity, nv.ptr(rows_dev), nv.ptr(G), fo.OWNERS[owners], nv.stream())
            once = G.clone() if once is None else once
        got[owners] = (once.cpu().numpy(), G.cpu().numpy())
    np.testing.assert_array_equal(got["single"][0], got["replicas"][0])
    np.testing.assert_array_equal(got["single"][1], got["replicas"][1])
    assert int((got["single"][0] != prefill().numpy()).sum()) > 0 and int((got["single"][1] != got["single"][0]).sum()) > 0


@pytest.mark.parametrize("owners", ["single", "replicas"])
def test_one_inf_gradient_poisons_every_row_in_both_forms(fo, field, owners):
    pts = points("uniform", 3000)
    G, _ = rows_launch(fo, field, pts, padded(3750), owners=owners, inf_at=1234)
    assert bool(torch.isnan(G).all())


def test_a_row_count_of_zero_leaves_G_and_the_reset_header(fo, field):
    """*rows_dev == 0 over buffers that hold points: no entries, the largest-gradient word as the plan's reset leaves it, G untouched -- also where the plan buffer
    held another launch's counts before."""
    pts = points("uniform", 3000)
    G, plan = rows_launch(fo, field, pts, padded(3000))
    assert plan_counts(plan).sum() == 12000 and plan_gmax_bits(plan) != 0
    base, S, packed = field
    x, d, gs, gc = padded_inputs(pts, padded(3000))
    s, c, _, masks = fo.field_forward(x, d, 1.0, base, S, packed, want_masks=True)
    plan.rows_dev, plan.xyzs, plan.launched = torch.zeros(2, dtype=torch.int32, device="cuda"), x, False      # the same buffer, planned again
    plan.launch()
    for owners in (None, "single", "replicas"):
        G = fo.field_backward_planned(x, 1.0, gs, gc, s, c, masks, packed, plan, prefill().cuda(), owners=owners)
        assert torch.equal(G.cpu(), prefill())
        assert plan_counts(plan).sum() == 0 and plan_gmax_bits(plan) == 0


def test_captured_step_does_not_depend_on_the_content_headroom(monkeypatch):
    """One captured watermark step over 256 content rays and 32 blocks of 4 x 4 rays, with content_headroom 0.25 and with 0 on the same rays: G and every codebook
    table bit for bit the same (every launch through the planned fixed-point scatter: NERFSIG_DETERMINISTIC=1; no overflow)."""
    monkeypatch.setenv("NERFSIG_DETERMINISTIC", "1")
    from nerf_signature_amd import trainer
    from nerf_signature_amd.optim import CodebookAdam
    from test_gpu_render import _data, _model
    bo, bd, co, cd, gt = _data(n_content=256, block=4)
    data = {"watermark": {"rays_o_block": bo.cuda(), "rays_d_block": bd.cuda()}, "content": {"rays_o": co.cuda(), "rays_d": cd.cuda(), "images": gt.cuda()}}
    msg = torch.from_numpy(np.random.RandomState(0).randint(0, 2, 32).astype(np.float32))
    runs = []
    for headroom in (0.25, 0.0):
        torch.manual_seed(0)
        m, _, _ = _model()
        opt = CodebookAdam(m.get_params(1e-2), betas=(0.9, 0.99), eps=1e-15, capturable=True)
        loop = trainer.GraphedWatermarkLoop(m, opt, dict(dt_gamma=0, max_steps=1024), data, content_headroom=headroom)
        loop.step(msg)
        torch.cuda.synchronize()
        assert not loop.overflowed()
        assert m.point_headroom == ((256,) if headroom else ())
        runs.append((loop.sink.G.detach().cpu().numpy().copy(), [e.weight.detach().cpu().numpy().copy() for e in m.msg_encoder.embeddings]))
    assert np.abs(runs[0][0]).sum() > 0
    np.testing.assert_array_equal(runs[0][0], runs[1][0])
    for a, b in zip(runs[0][1], runs[1][1]):
        np.testing.assert_array_equal(a, b)
