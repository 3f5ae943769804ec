"""SURVEY.md 8(a) R11 on the GPU: NeRFRenderer.mark_untrained_grid / update_extra_state against
  (1) golden G11 -- the reference's own methods (renderer_wtmk.py:380-538) run on a 32^3 two-cascade grid with a closed-form density
      field and closed-form draws (tests/golden/make_golden.py::grid_maintenance), and
  (2) the oracle's restatement at the production size (128^3) with the real field network behind `density()`.
The draws the reference makes on its device generator (torch.rand_like / torch.randint) are patched with closed_form.PatchedDraws on
every side, so jitter and cell choice are identical."""
import os

import numpy as np
import pytest
import torch

import closed_form as cf
from oracle import field_ref as fr

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _bits(b, shape):
    return np.unpackbits(np.asarray(b), bitorder="little").reshape(shape).astype(bool)


def test_grid_maintenance_matches_reference_golden():
    from nerf_signature_amd.renderer import NeRFRenderer

    class Field(NeRFRenderer):
        def density(self, x, message=None):
            return cf.grid_density(x, message)

    g = np.load(os.path.join(G, "g11_grid_maintenance.npz"))
    n = int(g["grid_size"])
    r = Field(bound=2, cuda_ray=True, density_scale=1, min_near=0.2, density_thresh=0.6, bg_radius=-1).cuda()
    r.grid_size = n
    r.density_grid = torch.zeros(r.cascade, n ** 3, device="cuda")
    r.density_bitfield = torch.zeros(r.cascade * n ** 3 // 8, dtype=torch.uint8, device="cuda")
    r.mark_untrained_grid(g["poses"], g["intrinsics"], S=16)
    got, want = r.density_grid.cpu().numpy(), g["grid_marked"]
    # the frustum test is a batched 3x3 matrix product: rocBLAS and the CPU may round a coordinate that sits on a frustum plane
    # differently, so a handful of cells may flip; everything else must agree
    assert int((got != want).sum()) <= 8 and int((want < 0).sum()) > 1000
    r.density_grid.copy_(torch.from_numpy(want))
    r.iter_density, r.local_step = 14, 5
    r.step_counter[:5, 0] = torch.tensor([1000, 1203, 990, 1500, 20], dtype=torch.int32, device="cuda")
    # the oracle runs alongside only to learn which cells the partial update draws more than once (unspecified winner)
    st = {"density_grid": torch.from_numpy(want.copy()), "density_bitfield": None, "bound": 2, "grid_size": n, "density_scale": 1, "density_thresh": 0.6,
          "iter_density": 14, "mean_density": 0, "step_counter": torch.zeros(16, 2, dtype=torch.int32), "local_step": 0, "mean_count": 0}
    calls = 0
    for k in range(3):
        if k == 2:
            r.local_step = 20
            r.step_counter[:, 0] = (torch.arange(16, dtype=torch.int32) * 100 + 7).cuda()
        with cf.PatchedDraws() as draws:
            draws.calls = calls
            r.update_extra_state(message=None, decay=0.95, S=16)
            assert draws.calls == int(g[f"draw_calls_{k}"])
        with cf.PatchedDraws() as draws:
            draws.calls = calls
            _, hits = fr.update_extra_state(st, cf.grid_density, None, 0.95, 16, rand_like=torch.rand_like, randint=torch.randint)
            calls = draws.calls
        once = (hits <= 1).numpy()
        got, want = r.density_grid.cpu().numpy(), g[f"grid_{k}"]
        # not bit-equal to the CPU capture: torch's GPU kernels divide by a scalar as a multiplication by its reciprocal
        # (`2 * coords / (G - 1)`, renderer_wtmk.py:473), so probe positions differ from the CPU's in the last bit -- on the GPU the
        # reference's own code does the same.  The closed-form field turns one ulp of position into <= 4e-4 relative in sigma.
        np.testing.assert_allclose(got[once], want[once], rtol=2e-3, atol=2e-5)
        np.testing.assert_array_equal(got < 0, want < 0)
        near = np.abs(want - min(float(g[f"mean_density_{k}"]), 0.6)) <= 2e-3 * 0.6
        differ = _bits(r.density_bitfield.cpu().numpy(), once.shape) != _bits(g[f"bitfield_{k}"], once.shape)
        assert not bool((differ & once & ~near).any()) and float(near.mean()) < 0.01
        np.testing.assert_allclose(r.mean_density, float(g[f"mean_density_{k}"]), rtol=1e-4 if k < 2 else 1e-3)
        assert r.mean_count == int(g[f"mean_count_{k}"]) and r.local_step == 0
        # the device bitfield is exactly packbits(grid, min(mean, thresh)) of the device grid (kernel_packbits, raymarching.cu:268-289)
        thresh = min(r.mean_density, r.density_thresh)
        np.testing.assert_array_equal(_bits(r.density_bitfield.cpu().numpy(), got.shape), got > thresh)
    assert r.iter_density == 17


def test_grid_update_with_field_network_matches_oracle():
    """Production size: 128^3 cells probed through NeRFNetwork.density (hash encoders + sigma MLP through the C ABI) with a message,
    against the oracle's update_extra_state with the oracle's fp32 field: grid values within 1e-3 (relative to the density scale),
    bitfield identical except for cells within that tolerance of the threshold."""
    from nerf_signature_amd.network import NeRFNetwork
    D = 32
    m = NeRFNetwork(bound=1.0, cuda_ray=True, density_scale=1, min_near=0.2, density_thresh=10, bg_radius=-1, message_dim=D, n_views=1)
    with torch.no_grad():
        for l in range(16):
            m.encoder.embeddings[l].weight.copy_(torch.from_numpy(cf.table(l)))
        for l in range(2 * D):
            m.msg_encoder.embeddings[l].weight.copy_(torch.from_numpy(cf.table(100 + l, scale=0.05)))
        m.sigma_net.params.copy_(torch.from_numpy(cf.mlp_params(3072, 1337)))
        m.color_net.params.copy_(torch.from_numpy(cf.mlp_params(7168, 1338)))
    m = m.cuda().train()
    msg = torch.from_numpy(cf.messages(D)[2])
    P = {"bound": 1.0, "base_tables": [e.weight.detach().cpu() for e in m.encoder.embeddings],
         "cb_tables": [e.weight.detach().cpu() for e in m.msg_encoder.embeddings],
         "sigma_params": m.sigma_net.params.detach().cpu(), "color_params": m.color_net.params.detach().cpu()}
    st = {"density_grid": torch.zeros(1, 128 ** 3), "density_bitfield": None, "bound": 1.0, "grid_size": 128, "density_scale": 1, "density_thresh": 10,
          "iter_density": 0, "mean_density": 0, "step_counter": torch.zeros(16, 2, dtype=torch.int32), "local_step": 0, "mean_count": 0}
    with torch.no_grad(), cf.PatchedDraws():
        fr.update_extra_state(st, lambda x, message: fr.density(x, message, P), msg, 0.95, 128, rand_like=torch.rand_like, randint=torch.randint)
    with cf.PatchedDraws():
        m.update_extra_state(message=msg.cuda(), decay=0.95, S=128)
    got, want = m.density_grid.cpu().numpy(), st["density_grid"].numpy()
    scale = float(np.abs(want).max())
    assert scale > 0.1
    np.testing.assert_allclose(got, want, rtol=1e-3, atol=1e-3 * scale)
    np.testing.assert_allclose(m.mean_density, st["mean_density"], rtol=1e-4)
    thresh = min(st["mean_density"], 10)
    near = np.abs(want - thresh) <= 2e-3 * scale
    differ = _bits(m.density_bitfield.cpu().numpy(), want.shape) != _bits(st["density_bitfield"].numpy(), want.shape)
    assert not bool((differ & ~near).any()) and float(near.mean()) < 0.05


def test_refresh_probe_order_changes_nothing_but_the_time():
    """update_extra_state queries its full-grid probe x fastest (the cached block's transposed view) and the partial refresh's scattered probe sorted on
    (y, z, x) -- an order the hash gather likes -- and hands the densities back in the order the reference draws its jitter in: the same grid / the same
    densities bit for bit as the plain order, with the real field network behind density()."""
    from nerf_signature_amd import synthetic
    from nerf_signature_amd.stage1 import CleanNeRFNetwork
    m = CleanNeRFNetwork(bound=1.0, cuda_ray=True, density_scale=1, min_near=0.2, density_thresh=10, bg_radius=-1)
    with torch.no_grad():
        for l, e in enumerate(m.encoder.embeddings):
            e.weight.copy_(torch.from_numpy(synthetic.table_values(l, 0.5)))
    m = m.cuda().train()
    plain_blocks = type(m)._grid_blocks.__get__(m)

    def unordered(S):      # the same blocks without the attributes _probe_density keys its reordering on
        for c, i in plain_blocks(S):
            yield c.clone(), i

    grids = []
    for reorder in (True, False):
        m._grid_blocks = plain_blocks if reorder else unordered
        m.density_grid.zero_()
        m.density_bitfield.zero_()
        m.iter_density = 0
        torch.manual_seed(0)
        m.update_extra_state()
        grids.append(m.density_grid.clone())
    assert torch.equal(grids[0], grids[1]) and float(grids[0].max()) > 0
    m._grid_blocks = plain_blocks
    n = m.grid_size ** 3 // 4
    torch.manual_seed(5)
    coords = torch.randint(0, m.grid_size, (2 * n, 3), device="cuda")
    out = []
    for thresh in (type(m).PROBE_SORT_MIN, 1 << 40):
        m.PROBE_SORT_MIN = thresh
        torch.manual_seed(7)
        out.append(m._probe_density(coords, 0, None))
    assert torch.equal(out[0], out[1]) and float(out[0].max()) > 0


def _refresh_model(bound=2.0):
    from nerf_signature_amd import synthetic
    from nerf_signature_amd.stage1 import CleanNeRFNetwork
    m = CleanNeRFNetwork(bound=bound, cuda_ray=True, density_scale=1, min_near=0.2, density_thresh=10, bg_radius=-1)
    with torch.no_grad():
        for l, e in enumerate(m.encoder.embeddings):
            e.weight.copy_(torch.from_numpy(synthetic.table_values(l, 0.5)))
        grid = synthetic.density_grid(bound)
        grid[:, ::97] = -1.0                                          # some cells no camera sees (mark_untrained_grid): they must stay -1
        bits, _ = synthetic.pack_bits_np(grid, 10.0)
        m.density_grid.copy_(torch.from_numpy(grid))
        m.density_bitfield.copy_(torch.from_numpy(bits))
    return m.cuda().train()


def test_device_side_refresh_restates_update_extra_state_step_by_step():
    """gridrefresh.DeviceGridRefresh (csrc/gridrefresh.hip) against renderer_wtmk.py:445-538 piece by piece, on two cascades at the production size, with the real field
    behind it: probe points inside their cells with the reference's centre arithmetic and a uniform jitter; densities = the model's density() there (and the CPU
    oracle's on a sample); the partial form's draws (uniform cells + occupied cells only, grouped by grid row); the scatter (largest candidate per cell); the EMA where
    both sides are >= 0, untouched and unseen (-1) cells left alone; mean, threshold, bitfield, refresh count, mean sample count of the window; the same bits from the
    same seed, other draws from another."""
    from nerf_signature_amd import fieldops as fo, raymarching
    from nerf_signature_amd.gridrefresh import DeviceGridRefresh
    m = _refresh_model(2.0)
    C, H = m.cascade, m.grid_size
    assert C == 2
    packed = fo.pack_weights(m.sigma_net.params, m.color_net.params)
    P = {"bound": 2.0, "base_tables": [e.weight.detach().cpu() for e in m.encoder.embeddings], "cb_tables": [],
         "sigma_params": m.sigma_net.params.detach().cpu(), "color_params": m.color_net.params.detach().cpu()}
    ring = torch.zeros(16, 2, dtype=torch.int32, device="cuda")
    ring[:, 0] = (torch.arange(16, dtype=torch.int32) * 1000 + 13).cuda()
    step_dev = torch.tensor([21], dtype=torch.int32, device="cuda")

    def check_common(r, old, cas, n):
        xyz, cell, sigma = r.xyz[:n], r.cell_index[:n].long(), r.sigma[:n]
        coords = raymarching.morton3D_invert(cell.int()).float()
        extent, half = m._cascade_extent(cas)
        centre = (2 * coords / (H - 1) - 1) * (extent - half)
        off = (xyz - centre) / half
        assert float(off.abs().max()) <= 1.0 + 1e-4 and abs(float(off.mean())) < 5e-3 and abs(float(off.std()) - 3 ** -0.5) < 5e-3      # U(-1, 1) inside the cell
        want = m.density(xyz)["sigma"]
        assert torch.equal(sigma, want)                                                        # the density query IS the model's density()
        pick = torch.arange(0, n, n // 1500, device="cuda")
        with torch.no_grad():
            cpu = fr.density(xyz[pick].cpu(), None, P)["sigma"].reshape(-1)
        np.testing.assert_allclose(sigma[pick].cpu().numpy(), cpu.numpy(), rtol=2e-3, atol=1e-4)
        best = torch.full((H ** 3,), -1.0, device="cuda").scatter_reduce(0, cell, sigma * m.density_scale, reduce="amax", include_self=True)
        assert torch.equal(r.fresh[cas], best)                                                 # repeated cells: the largest candidate
        both = (old[cas] >= 0) & (best >= 0)
        assert torch.equal(m.density_grid[cas], torch.where(both, torch.maximum(old[cas] * 0.95, best), old[cas]))
        assert bool((m.density_grid[cas][old[cas] < 0] == -1).all()) and int((old[cas] < 0).sum()) > 1000
        return cell

    def check_books(r, iter_before):
        mean = float(m.density_grid.clamp(min=0).double().mean())
        assert m.mean_density == pytest.approx(mean, rel=1e-6) and int(r.iter_dev) == m.iter_density == iter_before + 1
        assert torch.equal(m.density_bitfield, raymarching.packbits(m.density_grid, min(m.mean_density, m.density_thresh)))
        assert m.mean_count == int(sum(int(ring[(21 - 5 + i) % 16, 0]) for i in range(5)) / 5) and m.local_step == 0

    # ---- the full form (iter_density < 16): every cell of every cascade once
    r = DeviceGridRefresh(m, seed=3, capture=False)
    old = m.density_grid.clone()
    r.run(packed, ring, step_dev, window=5)
    cell = check_common(r, old, C - 1, H ** 3)
    assert torch.equal(torch.sort(cell).values, torch.arange(H ** 3, device="cuda"))
    check_books(r, 0)
    # ---- the partial form: N uniform cells + N occupied cells per cascade
    m.iter_density = 16
    r.iter_dev.fill_(16)
    old = m.density_grid.clone()
    r.run(packed, ring, step_dev, window=5)
    N = H ** 3 // 4
    check_common(r, old, C - 1, 2 * N)
    keys, ids = r.keys.long(), r.ids.long()
    assert torch.equal(torch.sort(ids).values, torch.arange(2 * N, device="cuda"))           # every draw placed exactly once ...
    rows = keys // H
    assert bool((rows[1:] >= rows[:-1]).all())                                                # ... grouped by grid row (z, y)
    x, y, z = keys % H, (keys // H) % H, keys // (H * H)
    morton = raymarching.morton3D(torch.stack([x, y, z], -1).int()).long()
    assert torch.equal(morton, r.cell_index[:2 * N].long())
    uniform, occupied = ids < N, ids >= N
    for axis in (x, y, z):                                                                    # 524 288 uniform draws per axis: mean (H - 1) / 2 +- 0.051 (1 sigma)
        assert abs(float(axis[uniform].float().mean()) - (H - 1) / 2) < 0.3
    assert float(torch.unique(morton[uniform]).numel()) / N > 0.85                            # (with repetition: 1 - (1 - 1/M)^N of M = 4 N cells ~ 0.885 of N distinct)
    assert bool((old[C - 1][morton[occupied]] > 0).all())                                     # the second half: occupied cells only (renderer_wtmk.py:493-496)
    n_occ = int((old[C - 1] > 0).sum())
    assert torch.unique(morton[occupied]).numel() > 0.9 * min(n_occ, N * (1 - np.exp(-1)))   # ... spread over them
    untouched = torch.ones(H ** 3, dtype=torch.bool, device="cuda")
    untouched[morton] = False
    assert torch.equal(m.density_grid[C - 1][untouched], old[C - 1][untouched]) and int(untouched.sum()) > H ** 3 // 2
    check_books(r, 16)
    # ---- a pure function of (grid, parameters, seed, refresh count); captured == eager
    finals = []
    for seed, capture in ((3, False), (3, True), (4, False)):
        m2 = _refresh_model(2.0)
        r2 = DeviceGridRefresh(m2, seed=seed, capture=capture)
        m2.iter_density = 14
        r2.iter_dev.fill_(14)
        for _ in range(6):                                                                    # two full (eager, captured) + four partial (eager, captured, replay, replay)
            r2.run(packed, ring, step_dev, window=5)
        torch.cuda.synchronize()
        assert (len(r2.graphs) == 2) == capture
        finals.append((m2.density_grid.clone(), m2.density_bitfield.clone(), m2.mean_density))
    assert torch.equal(finals[0][0], finals[1][0]) and torch.equal(finals[0][1], finals[1][1]) and finals[0][2] == finals[1][2]
    assert not torch.equal(finals[0][0], finals[2][0])


def test_captured_refresh_follows_a_reallocated_step_count():
    """DeviceGridRefresh.run keys its captured graphs on the addresses the refresh reads: a step count handed over in a new tensor of the same value is not
    read through the graph captured with the old one (whose memory now holds another value) -- the next run is a new key, eager and then captured, and grid,
    bitfield and mean sample count stay those of an uncaptured twin."""
    from nerf_signature_amd import fieldops as fo
    from nerf_signature_amd.gridrefresh import DeviceGridRefresh
    m, twin = _refresh_model(2.0), _refresh_model(2.0)
    packed = fo.pack_weights(m.sigma_net.params, m.color_net.params)
    ring = torch.zeros(16, 2, dtype=torch.int32, device="cuda")
    ring[:, 0] = (torch.arange(16, dtype=torch.int32) * 1000 + 13).cuda()
    r, r_twin = DeviceGridRefresh(m, seed=3, capture=True), DeviceGridRefresh(twin, seed=3, capture=False)
    old = torch.tensor([21], dtype=torch.int32, device="cuda")
    for _ in range(2):                                                                        # eager, captured
        r.run(packed, ring, old, window=5)
        r_twin.run(packed, ring, old, window=5)
    assert len(r.graphs) == 1
    new = old.clone()
    assert new.data_ptr() != old.data_ptr()
    old.fill_(3)                                                                              # (the caller let it go: its memory holds something else now)
    seen = len(r.seen)
    for k in range(2):
        r.run(packed, ring, new, window=5)
        r_twin.run(packed, ring, new, window=5)
        assert len(r.seen) == seen + 1 and len(r.graphs) == 1 + k                             # not the old graph: a new key, eager, then captured
    torch.cuda.synchronize()
    assert torch.equal(m.density_grid, twin.density_grid) and torch.equal(m.density_bitfield, twin.density_bitfield)
    assert m.mean_count == twin.mean_count and m.mean_density == twin.mean_density


# ---- csrc/gridrefresh.hip entry point by entry point through the C ABI, against tests/grid_refresh_ref.py (the tests above reach it through DeviceGridRefresh, at one shape)

GUARD = 256      # bytes of 0xA5 in front of and behind every buffer handed to a call


class _Guarded:
    """n_bytes of device memory between two guard regions of a known pattern; `.t` views them as dtype.  shift: extra guard bytes in front (a misaligned pointer).
    The buffer itself starts out as the pattern too: nothing a call reads before writing it is zero by luck."""

    def __init__(self, n_bytes, dtype=torch.uint8, shift=0):
        self.front, self.n = GUARD + shift, int(n_bytes)
        self.raw = torch.full((self.front + self.n + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        self.t = self.raw[self.front:self.front + self.n].view(dtype)

    def put(self, array):
        self.t.copy_(torch.from_numpy(np.ascontiguousarray(array)).view(self.t.dtype).reshape(self.t.shape))
        return self

    def intact(self):
        return bool((self.raw[:self.front] == 0xA5).all()) and bool((self.raw[self.front + self.n:] == 0xA5).all())

    def get(self):
        return self.t.cpu().numpy()


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


class _Draw:
    """The buffers of rg_refresh_draw at one (H, N), each sized exactly as the header says, and one call on them."""

    def __init__(self, H, N):
        from nerf_signature_amd import _native as nv
        self.nv, self.H, self.N = nv, H, N
        self.grid = _Guarded(4 * H ** 3, torch.float32)
        self.scratch_bytes = int(nv.fn("rg_refresh_draw_scratch_bytes")(N, H))
        self.it = _Guarded(4, torch.int32)

    def run(self, grid_np, seed, it, cas):
        nv, N, H = self.nv, self.N, self.H
        self.grid.put(grid_np)
        self.it.t.fill_(it)
        scratch, keys, ids = _Guarded(self.scratch_bytes, torch.int32), _Guarded(8 * N, torch.int32), _Guarded(8 * N, torch.int32)      # (fresh: the pattern, not the last run)
        nv.call("rg_refresh_draw", nv.ptr(keys.t), nv.ptr(ids.t), N, H, nv.ptr(self.grid.t), nv.ptr(scratch.t), seed, nv.ptr(self.it.t), cas, nv.stream())
        torch.cuda.synchronize()
        assert scratch.intact() and keys.intact() and ids.intact() and self.grid.intact() and self.it.intact()
        assert int(self.it.t) == it and _same_bits(self.grid.get(), grid_np)
        self.keys, self.ids = keys, ids
        return keys.get().astype(np.int64), ids.get().astype(np.int64)


_OCCUPANCY = ("none", "first", "last", "seam", "all", "sparse")


def _occupancy(kind, cells, rng):
    """One cascade's grid in morton order.  The background is zeros and -1: `occupied` is strictly `> 0`."""
    g = np.where(np.arange(cells) % 3 == 0, -1.0, 0.0).astype(np.float32)
    if kind == "first":
        g[0] = 0.5
    elif kind == "last":
        g[cells - 1] = 2.0
    elif kind == "seam":      # the last cell of one 4096-cell occupancy workgroup and the first of the next (8^3 has one workgroup: the middle of it)
        a = 4095 if cells > 4096 else cells // 2 - 1
        g[a] = g[a + 1] = 1.0
    elif kind == "all":
        g = np.where(np.arange(cells) % 2 == 0, 1e-30, 3.0).astype(np.float32)
    elif kind == "sparse":
        r = rng.randint(0, 10, cells)
        g = np.where(r == 0, rng.uniform(0.01, 5.0, cells), np.where(r < 5, 0.0, -1.0)).astype(np.float32)
    return g


def _check_draw(keys, ids, want, H, N):
    assert np.array_equal(np.sort(ids), np.arange(2 * N))                      # every draw placed exactly once
    assert np.array_equal(keys, want[ids])                                     # ... with the key the reference gives that draw
    rows = keys // H
    assert (rows[1:] >= rows[:-1]).all()                                       # ... grouped by grid row
    by_key, by_id = np.lexsort((keys, rows)), np.lexsort((ids, rows))
    return keys[by_key], ids[by_id]                                            # the multiset of every row, rows in order


_DRAW_CASES = [(8, 1), (8, 4096), (8, 4097), (32, 1), (32, 4096), (32, 4097), (64, 1), (64, 4096), (64, 4097), (64, 64 ** 3 // 4), (256, 4097)]


@pytest.mark.parametrize("H,N", _DRAW_CASES)
def test_rg_refresh_draw_matches_the_reference_draw_for_draw(H, N):
    """rg_refresh_draw against grid_refresh_ref.draw_keys, exactly, on six occupancy patterns (nothing occupied -> cell 0; one cell at morton 0, at cells - 1;
    two at a 4095 / 4096 workgroup seam; everything; a sparse mix of positives, zeros and -1).  H = 8: one occupancy workgroup, 64 rows; 32: 1024 rows, exactly
    one trip of the scan; 64: 4096 rows and 64 occupancy workgroups (the scan's carry on the rows); 256: the global-atomic sort, 65 536 rows and 4096 block sums
    (the carry on both).  2N = 2: below one 8192-draw chunk; 8192: exactly one; 8194: one draw past it."""
    import grid_refresh_ref as gr
    rng = np.random.RandomState(H + N)
    d = _Draw(H, N)
    seed = 0xD1CEBA5EBA11AD55 + H
    for kind in _OCCUPANCY:
        grid = _occupancy(kind, H ** 3, rng)
        want = gr.draw_keys(grid, N, H, seed, 16, 1)
        first = _check_draw(*d.run(grid, seed, 16, 1), want, H, N)
        again = _check_draw(*d.run(grid, seed, 16, 1), want, H, N)
        assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1]), kind
        occupied = want[N:]
        x, y, z = occupied % H, (occupied // H) % H, occupied // (H * H)
        assert (kind == "none") == bool((grid > 0).sum() == 0) and (grid[gr.morton(x, y, z)] > 0).all() == (kind != "none")


def test_rg_refresh_draw_cascade_and_refresh_count():
    """The same grid under other cascades and refresh counts (the streams' counters, the largest int32 among them): each the reference's draws, each different."""
    import grid_refresh_ref as gr
    H, N, seed = 32, 4097, 3
    d = _Draw(H, N)
    grid = _occupancy("sparse", H ** 3, np.random.RandomState(1))
    seen = []
    for cas, it in ((0, 16), (7, 16), (1, 0), (1, 16), (1, (1 << 31) - 1)):
        want = gr.draw_keys(grid, N, H, seed, it, cas)
        _check_draw(*d.run(grid, seed, it, cas), want, H, N)
        seen.append(want)
    assert all((seen[a][:N] != seen[b][:N]).mean() > 0.9 and (seen[a][N:] != seen[b][N:]).mean() > 0.9 for a in range(5) for b in range(a))


@pytest.mark.parametrize("form", ["full", "partial"])
@pytest.mark.parametrize("H", [8, 64])
def test_rg_refresh_points_against_float64(H, form):
    """rg_refresh_points, full form (keys = ids = NULL, n = H^3) and partial form (the keys and ids of a draw): the morton index exactly, the point within
    8 * 2^-24 * extent of the float64 reference.  The kernel's roundings (the library is built without contraction, so none is fused): the division 2c / (H - 1)
    (<= 2^-24 absolute; the subtraction of 1 behind it is exact or rounds to a finer grid than that error), extent - half_cell (<= 2^-24 extent), the product
    of the two (<= 2^-24 extent, and it carries the first two: 2^-24 (extent - half) + 2^-24 extent), the jitter's product with half_cell (<= 2^-24 half_cell;
    u * 2 - 1 is exact on the 2^-23 grid) and the final sum (<= 2^-24 extent): five roundings, together below 5 * 2^-24 * extent; the bound keeps the issue's 8.
    No tolerance on u: the jitter's draw is an integer, taken for the draw's id and not for its position."""
    import grid_refresh_ref as gr
    from nerf_signature_amd import _native as nv
    extent = np.float32(2.0 if H == 8 else 1.5)
    half = np.float32(extent / np.float32(H))
    seed, it, cas = 11, 16, 1
    it_dev = _Guarded(4, torch.int32)
    it_dev.t.fill_(it)
    if form == "full":
        n, keys_ptr, ids_ptr = H ** 3, None, None
        keys = ids = np.arange(n)
    else:
        N = 4097
        d = _Draw(H, N)
        keys, ids = d.run(_occupancy("sparse", H ** 3, np.random.RandomState(H)), seed, it, cas)
        n, keys_ptr, ids_ptr = 2 * N, nv.ptr(d.keys.t), nv.ptr(d.ids.t)
        assert (ids != np.arange(n)).mean() > 0.9
    xyz, cells = _Guarded(12 * n, torch.float32), _Guarded(4 * n, torch.int32)
    nv.call("rg_refresh_points", keys_ptr, ids_ptr, n, H, float(extent), float(half), seed, nv.ptr(it_dev.t), cas, nv.ptr(xyz.t), nv.ptr(cells.t), nv.stream())
    torch.cuda.synchronize()
    assert xyz.intact() and cells.intact() and it_dev.intact() and int(it_dev.t) == it
    want_xyz, want_cells = gr.points(keys, ids, H, extent, half, seed, it, cas)
    assert np.array_equal(cells.get().astype(np.int64), want_cells)
    err = np.abs(xyz.get().reshape(n, 3).astype(np.float64) - want_xyz)
    print(f"points H={H} {form}: max error {err.max() / (2.0 ** -24 * float(extent)):.3f} x 2^-24 extent")
    assert err.max() <= 8 * 2.0 ** -24 * float(extent)
    centre = (2.0 * np.stack([keys % H, (keys // H) % H, keys // (H * H)], -1) / (H - 1) - 1.0) * (float(extent) - float(half))
    off = (want_xyz - centre) / float(half)
    assert np.abs(off).max() < 1 and abs(off.mean()) < 0.08 and np.unique(off).size > min(n, 1000)      # (the reference itself: a jitter inside the cell)


@pytest.mark.parametrize("n_cells", [1, 255, 257, 2048 * 256 + 1])
def test_rg_refresh_begin_fills_exactly_its_cells(n_cells):
    """-1 in every cell and nothing behind: one thread, a partial workgroup, one cell into the second, and one cell more than 2048 workgroups reach in one stride."""
    from nerf_signature_amd import _native as nv
    fresh = _Guarded(4 * n_cells, torch.float32)
    nv.call("rg_refresh_begin", nv.ptr(fresh.t), n_cells, nv.stream())
    torch.cuda.synchronize()
    assert fresh.intact() and bool((fresh.t == -1.0).all())


def _finish(grid_np, fresh_np, decay, thresh, shift=0, ring=None, window=0, steps=None, it=16, fresh_dev=None):
    """One rg_refresh_finish on guarded buffers sized as the header says; the bitfield `shift` bytes off its alignment.  steps None: step_dev = NULL."""
    from nerf_signature_amd import _native as nv
    n = grid_np.size
    grid = _Guarded(4 * n, torch.float32).put(grid_np)
    fresh = fresh_dev if fresh_dev is not None else _Guarded(4 * n, torch.float32).put(fresh_np)
    partials = _Guarded(int(nv.fn("rg_refresh_partials_bytes")(n)), torch.float64)
    bits = _Guarded(n // 8, torch.uint8, shift=shift)
    assert nv.ptr(bits.t) % 4 == shift % 4
    mean, it_dev, count = _Guarded(4, torch.float32), _Guarded(4, torch.int32), _Guarded(4, torch.int32)
    it_dev.t.fill_(it)
    count.t.fill_(-12345)
    ring_dev = None if ring is None else _Guarded(128, torch.int32).put(np.asarray(ring, np.int32))
    step_dev = None if steps is None else _Guarded(4, torch.int32).put(np.array([steps], np.uint32).view(np.int32))
    fresh_before = fresh.get().copy()
    nv.call("rg_refresh_finish", nv.ptr(grid.t), nv.ptr(fresh.t), n, decay, nv.ptr(partials.t), thresh, nv.ptr(bits.t), nv.ptr(mean.t), nv.ptr(it_dev.t),
            None if ring_dev is None else nv.ptr(ring_dev.t), window, None if step_dev is None else nv.ptr(step_dev.t), nv.ptr(count.t), nv.stream())
    torch.cuda.synchronize()
    for b in (grid, fresh, partials, bits, mean, it_dev, count, ring_dev, step_dev):
        assert b is None or b.intact()
    assert _same_bits(fresh.get(), fresh_before)
    assert ring_dev is None or np.array_equal(ring_dev.get().reshape(16, 2), np.asarray(ring, np.int32))
    return {"grid": grid.get(), "bits": bits.get(), "mean": mean.get()[0], "iter": int(it_dev.t), "count": int(count.t)}


def _f32_ulps(a, b):
    a, b = np.float32(a), np.float32(b)
    return 0 if a == b else abs(int(a.view(np.int32)) - int(b.view(np.int32))) if np.isfinite(a) and np.isfinite(b) else 1 << 30


T_PLANT = np.float32(0.3)


def _finish_inputs(n, rng):
    """An old grid of -1, 0 and positives and a fresh grid of -1, 0, positives, NaN and (where the old grid is -1, so that the mean stays finite) +inf; cells 0-2
    planted to come out at exactly T_PLANT (kept; reached by the maximum) and one ulp above it, cell 3 large enough to hold the mean above T_PLANT at any n."""
    r = rng.randint(0, 20, n)
    grid = np.where(r < 3, -1.0, np.where(r < 6, 0.0, rng.uniform(0.01, 3.0, n))).astype(np.float32)
    r = rng.randint(0, 20, n)
    fresh = np.where(r < 5, -1.0, np.where(r < 7, 0.0, np.where(r < 8, np.nan, rng.uniform(0.0, 4.0, n)))).astype(np.float32)
    fresh[(grid < 0) & (rng.randint(0, 2, n) == 0)] = np.inf
    grid[:4] = [T_PLANT, 0.1, np.nextafter(T_PLANT, np.float32(1)), 3.0]
    fresh[:4] = [-1.0, T_PLANT, np.nan, 5.0]
    return grid, fresh


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("n_cells", [8, 40, 4096, 4104, 2 * 32 ** 3])
def test_rg_refresh_finish_matches_the_reference_bit_for_bit(n_cells, shift):
    """rg_refresh_finish against grid_refresh_ref.finish: the grid bit for bit (one multiply, one maximum, no contraction), the refresh count advanced by one, the
    mean within one fp32 ulp of the float32 of the float64 mean (the device sums doubles in another order), the bitfield exactly in three regimes --
    density_thresh below the mean (the level is exact; the planted cells equal to it give bit 0, one ulp above it bit 1), density_thresh above the mean (the
    level is the device's own mean: no cell of the reference's grid within 2 ulp of the reference's mean, asserted on the reference alone), and an infinite
    mean (+inf in fresh over a probed cell).  n_cells: one byte, a partial word, one EMA workgroup, one byte-group into the second, a two-cascade 32^3 grid;
    the bitfield 4-byte aligned and one byte off."""
    import grid_refresh_ref as gr
    grid, fresh = _finish_inputs(n_cells, np.random.RandomState(n_cells))
    for regime in ("below", "above", "infinite"):
        thresh = 1e9 if regime == "above" else float(T_PLANT)
        f = fresh.copy()
        if regime == "infinite":
            f[3] = np.inf
        want_grid, want_mean, want_bits, _ = gr.finish(grid, f, 0.95, thresh)
        mean32 = np.float32(want_mean)
        if regime == "below":
            assert want_mean > 1.01 * float(T_PLANT) and (want_grid == T_PLANT).sum() >= 2
        elif regime == "above":
            positive = want_grid[np.isfinite(want_grid) & (want_grid > 0)]
            assert np.abs(positive.view(np.int32).astype(np.int64) - int(mean32.view(np.int32))).min() > 2 and thresh > want_mean
        else:
            assert np.isinf(want_mean)
        got = _finish(grid, f, 0.95, thresh, shift=shift)
        assert _same_bits(got["grid"], want_grid) and got["iter"] == 17 and got["count"] == -12345
        assert not _same_bits(want_grid, grid)
        print(f"finish n={n_cells} shift={shift} {regime}: mean {got['mean']!r} against {mean32!r}")
        assert _f32_ulps(got["mean"], mean32) <= 1
        assert np.array_equal(got["bits"], want_bits)
        if regime != "above":
            assert [int(got["bits"][0] >> b) & 1 for b in range(4)] == [0, 0, 1, 1]
        if n_cells > 8:
            assert 0.05 < np.unpackbits(want_bits).mean() < 0.95


def test_rg_refresh_finish_mean_sample_count():
    """*mean_count = int(sum / window) of column 0 of the ring rows (steps - window + i) mod 2^32 mod 16: every window in {0, 1, 5, 16} (0 leaves it alone) with every
    step count in {0, 3, 21, 2^32 - 1} (below the window the row index wraps through 2^32) and with step_dev = NULL (steps = window); totals of 2^30 per row, whose
    sum leaves int32; column 1 holds noise that must not matter."""
    import grid_refresh_ref as gr
    rng = np.random.RandomState(7)
    grid, fresh = _finish_inputs(40, rng)
    ring = np.zeros((16, 2), np.int32)
    ring[:, 0] = (1 << 30) + 37 * np.arange(16) ** 2
    ring[:, 1] = rng.randint(-(1 << 31), 1 << 31, 16, dtype=np.int64).astype(np.int32)
    seen = set()
    for window in (0, 1, 5, 16):
        for steps in (0, 3, 21, (1 << 32) - 1, None):
            got = _finish(grid, fresh, 0.95, 0.3, ring=ring, window=window, steps=steps)
            want = gr.finish(grid, fresh, 0.95, 0.3, ring, window, steps)[3]
            assert got["count"] == (-12345 if window == 0 else want) and got["iter"] == 17, (window, steps)
            seen.add(want)
    assert len(seen) >= 10 and int(ring[:5, 0].astype(np.int64).sum()) > (1 << 31)
    other = ring.copy()
    other[:, 1] = rng.randint(-(1 << 31), 1 << 31, 16, dtype=np.int64).astype(np.int32)
    assert _finish(grid, fresh, 0.95, 0.3, ring=other, window=16, steps=21)["count"] == gr.finish(grid, fresh, 0.95, 0.3, ring, 16, 21)[3]


@pytest.mark.parametrize("scale", [1.0, 0.5])
@pytest.mark.parametrize("n", [1, 257])
def test_rg_refresh_scatter_keeps_what_the_reference_keeps(n, scale):
    """rg_refresh_begin + rg_refresh_scatter against grid_refresh_ref.scatter (the largest candidate of a cell; cells 0 and n_cells - 1), and judged through
    rg_refresh_finish on an old grid of 1.0 as the reference's `valid = (grid >= 0) & (tmp >= 0)` judges it: a cell whose only candidates are negative stays 1.0,
    a +0 or -0.0 cell decays to 0.95, a NaN cell stays 1.0 and the NaN stays visible in fresh."""
    import grid_refresh_ref as gr
    from nerf_signature_amd import _native as nv
    n_cells, nan, inf = 264, np.float32(np.nan), np.float32(np.inf)
    if n == 1:
        runs = [([c], [v]) for c, v in ((0, 3.0), (n_cells - 1, 0.25), (0, 0.0), (n_cells - 1, -0.0), (0, -2.0), (n_cells - 1, inf), (0, nan), (5, -inf))]
    else:
        planted = [(0, 3.0), (n_cells - 1, 0.5), (10, -1.0), (10, -3.0), (11, -0.0), (12, 0.0), (13, nan), (14, -2.0), (14, -0.0), (15, 2.0), (15, nan), (15, 7.0),
                   (16, inf), (16, 5.0), (17, 0.25), (17, 4.0), (17, -1.0), (18, -inf)]
        rng = np.random.RandomState(n)
        more = n - len(planted)
        values = np.where(rng.randint(0, 3, more) == 0, rng.choice(np.array([-0.0, 0.0, -1.5, 1e-30], np.float32), more), rng.uniform(0.0, 6.0, more))
        runs = [([c for c, _ in planted] + rng.randint(20, 60, more).tolist(), [v for _, v in planted] + values.tolist())]
    for cells, sigmas in runs:
        cells, sigmas = np.asarray(cells, np.int32), np.asarray(sigmas, np.float32)
        assert cells.size == n
        fresh, sig_dev, cell_dev = _Guarded(4 * n_cells, torch.float32), _Guarded(4 * n, torch.float32).put(sigmas), _Guarded(4 * n, torch.int32).put(cells)
        nv.call("rg_refresh_begin", nv.ptr(fresh.t), n_cells, nv.stream())
        nv.call("rg_refresh_scatter", nv.ptr(sig_dev.t), nv.ptr(cell_dev.t), n, scale, nv.ptr(fresh.t), nv.stream())
        torch.cuda.synchronize()
        assert fresh.intact() and sig_dev.intact() and cell_dev.intact()
        want, got = gr.scatter(sigmas, cells, scale, n_cells), fresh.get()
        assert np.array_equal(np.isnan(got), np.isnan(want)) and _same_bits(np.nan_to_num(got, nan=9.0), np.nan_to_num(want, nan=9.0)), (cells[:1], sigmas[:1])
        old = np.ones(n_cells, np.float32)
        after = _finish(old, None, 0.95, 0.5, fresh_dev=fresh)["grid"]
        assert _same_bits(after, gr.finish(old, want, 0.95, 0.5)[0])
        decayed = np.float32(0.95)
        if n == 1:
            v = sigmas[0] * np.float32(scale)
            expect = 1.0 if np.isnan(v) or (v < 0) else max(decayed, v)
            assert after[cells[0]] == expect and (np.delete(after, cells[0]) == 1.0).all()
        else:
            assert after[[10, 13, 15, 18]].tolist() == [1.0] * 4 and after[[11, 12, 14]].tolist() == [decayed] * 3 and after[16] == inf
            assert after[17] == max(decayed, np.float32(4.0 * scale)) and after[0] == 3.0 * scale and after[n_cells - 1] == max(decayed, np.float32(0.5 * scale))
            assert np.isnan(got[[13, 15]]).all() and (got[[10, 18]] == -1).all() and not np.signbit(got[[11, 12, 14]]).any() and (after[60:n_cells - 1] == 1.0).all()
