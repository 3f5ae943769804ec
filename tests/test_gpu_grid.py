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
