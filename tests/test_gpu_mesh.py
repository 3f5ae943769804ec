"""Mesh extraction on the GPU: the marching-cubes kernels against the numpy restatement (tests/mc_ref.py), element for element; the
density lattice against the reference's extract_fields loop, bit for bit; extract_geometry and save_mesh end to end."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mc_ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _march(u, thr):
    from nerf_signature_amd import mesh
    v, t = mesh.marching_cubes(torch.from_numpy(np.ascontiguousarray(u)).to(DEV), thr)
    return v.cpu().numpy(), t.cpu().numpy()


def _same(u, thr):
    """GPU == restatement: triangles equal, vertices bit-equal (the build has -ffp-contract=off and correctly rounded fp32 division)."""
    v, t = _march(u, thr)
    rv, rt = mc_ref.marching_cubes(u, thr)
    assert v.dtype == np.float32 and t.dtype == np.int32 and v.shape == rv.shape and t.shape == rt.shape, (v.shape, rv.shape, t.shape, rt.shape)
    assert np.array_equal(t, rt)
    assert np.array_equal(v.view(np.int32), rv.view(np.int32))
    return v, t


def test_all_256_single_cell_cases():
    rng = np.random.default_rng(0)
    for case in range(256):
        mag = rng.uniform(0.1, 3.0, 8).astype(np.float32)
        u = np.empty((2, 2, 2), np.float32)
        for c in range(8):
            x, y, z = c & 1, (c >> 1) & 1, (c >> 2) & 1
            u[x, y, z] = 0.5 + (mag[c] if (case >> c) & 1 else -mag[c])
        v, t = _same(u, 0.5)
        assert len(t) == mc_ref.TRI_COUNT[case]


@pytest.mark.parametrize("shape", [(2, 2, 2), (3, 3, 3), (17, 17, 17), (129, 129, 129), (257, 257, 257), (5, 40, 33)])
def test_sizes(shape):
    """Smooth fields with several components and a little noise: many crossings, all cell cases, every boundary of the lattice."""
    rng = np.random.default_rng(sum(shape))
    g = [np.linspace(0, 1, n, dtype=np.float64) for n in shape]
    X, Y, Z = np.meshgrid(*g, indexing="ij")
    u = np.sin(7.1 * X + 1.3) * np.cos(5.3 * Y - 0.4) + np.sin(6.7 * Z + 2.0 * X) + 0.05 * rng.standard_normal(shape)
    v, t = _same(u.astype(np.float32), 0.1)
    assert len(t) > 0


def test_sphere_256():
    p = np.arange(256, dtype=np.float64) - 127.5
    X, Y, Z = np.meshgrid(p, p, p, indexing="ij")
    u = (100.0 - np.sqrt(X * X + Y * Y + Z * Z)).astype(np.float32)
    v, t = _same(u, 0.0)
    assert mc_ref.euler_characteristic(len(v), t) == 2 and mc_ref.is_closed_oriented(t)


@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_noise(sign):
    u = (sign * np.random.default_rng(3).standard_normal((48, 31, 64))).astype(np.float32)
    v, t = _same(u, 0.0)
    assert len(t) > 10000


def test_threshold_ties_nan_and_infinities():
    rng = np.random.default_rng(4)
    u = rng.standard_normal((24, 20, 28)).astype(np.float32)
    pick = rng.integers(0, 8, u.shape)
    u[pick == 0] = 0.25          # equal to the threshold: outside
    u[pick == 1] = np.nan        # outside
    u[pick == 2] = np.inf
    u[pick == 3] = -np.inf
    _same(u, 0.25)


def test_empty_and_full_lattices_give_zero_outputs():
    for val in (-1.0, 2.0, np.nan):
        v, t = _march(np.full((9, 7, 5), val, np.float32), 0.0)
        assert v.shape == (0, 3) and t.shape == (0, 3)


def test_refusals():
    from nerf_signature_amd import mesh
    big = torch.zeros(1, device=DEV).expand(2, 2, (1 << 26) + 1)     # above the 2^28-node limit, nothing allocated
    with pytest.raises(ValueError, match="limit"):
        mesh.marching_cubes(big, 0.0)
    with pytest.raises(ValueError, match="float32"):
        mesh.marching_cubes(torch.zeros(4, 4, 4, device=DEV, dtype=torch.float64), 0.0)
    with pytest.raises(ValueError, match="3-D"):
        mesh.marching_cubes(torch.zeros(4, 4, device=DEV), 0.0)
    with pytest.raises(ValueError, match="at least 2"):
        mesh.marching_cubes(torch.zeros(4, 1, 4, device=DEV), 0.0)


# ---- the density lattice --------------------------------------------------------------------------------------------------------------------------------

def _nerf(opaque=False):
    from nerf_signature_amd import synthetic
    from nerf_signature_amd.network import NeRFNetwork
    m = NeRFNetwork(bound=1.0, cuda_ray=True, density_scale=1, min_near=0.2, density_thresh=10, bg_radius=-1, message_dim=32, n_views=1)
    synthetic.init_model(m, "hotdog", opaque=opaque)
    return m.to(DEV).eval()


def _clean():
    from nerf_signature_amd import synthetic
    from nerf_signature_amd.stage1 import CleanNeRFNetwork
    m = CleanNeRFNetwork(bound=1.0, cuda_ray=True, density_scale=1, min_near=0.2, density_thresh=10, bg_radius=-1)
    with torch.no_grad():
        for l, e in enumerate(m.encoder.embeddings):
            e.weight.copy_(torch.from_numpy(synthetic.table_values(l, 0.5)))
    return m.to(DEV).eval()


def extract_fields_restated(bound_min, bound_max, resolution, query_func, S=128):
    """The reference's extract_fields (nerf/utils.py:174-189): CPU linspace, 128^3 chunks in z-fastest point order, one query per chunk."""
    X = torch.linspace(float(bound_min[0]), float(bound_max[0]), resolution).split(S)
    Y = torch.linspace(float(bound_min[1]), float(bound_max[1]), resolution).split(S)
    Z = torch.linspace(float(bound_min[2]), float(bound_max[2]), resolution).split(S)
    u = torch.zeros(resolution, resolution, resolution, dtype=torch.float32, device=DEV)
    with torch.no_grad():
        for xi, xs in enumerate(X):
            for yi, ys in enumerate(Y):
                for zi, zs in enumerate(Z):
                    xx, yy, zz = torch.meshgrid(xs, ys, zs, indexing="ij")
                    pts = torch.cat([xx.reshape(-1, 1), yy.reshape(-1, 1), zz.reshape(-1, 1)], dim=-1).to(DEV)
                    u[xi * S:xi * S + len(xs), yi * S:yi * S + len(ys), zi * S:zi * S + len(zs)] = query_func(pts).reshape(len(xs), len(ys), len(zs))
    return u


@pytest.mark.parametrize("kind", ["nerf", "nerf_message", "clean"])
@pytest.mark.parametrize("R", [200, 256])
def test_lattice_is_bit_identical_to_extract_fields(kind, R, mlp_prec):
    from nerf_signature_amd import mesh
    m = _clean() if kind == "clean" else _nerf()
    msg = torch.randint(0, 2, (32,), generator=torch.Generator().manual_seed(R)).float().to(DEV) if kind == "nerf_message" else None
    lo, hi = m.aabb_infer[:3], m.aabb_infer[3:]
    got = mesh.lattice(m, lo, hi, R, message=msg)
    want = extract_fields_restated(lo, hi, R, (lambda p: m.density(p, msg)["sigma"]) if msg is not None else (lambda p: m.density(p)["sigma"]))
    assert got.shape == (R, R, R) and got.dtype == torch.float32 and got.is_contiguous()
    assert torch.equal(got, want)


def test_extract_geometry_with_an_analytic_query():
    from nerf_signature_amd import mesh
    lo, hi = torch.tensor([-1.0, -0.8, -1.2], device=DEV), torch.tensor([1.0, 1.1, 0.9], device=DEV)
    R = 150

    def query(p):
        return 0.7 - torch.sqrt((p * p * torch.tensor([1.0, 1.5, 0.8], device=p.device)).sum(-1))

    v, t = mesh.extract_geometry(lo, hi, R, 0.0, query)
    u = extract_fields_restated(lo, hi, R, query).cpu().numpy()
    rv, rt = mc_ref.marching_cubes(u, 0.0)
    want_v = mc_ref.to_world(rv, lo.cpu().numpy(), hi.cpu().numpy(), R)
    assert v.dtype == np.float64 and t.dtype == np.int64 and len(t) > 1000
    assert np.array_equal(v, want_v) and np.array_equal(t, rt.astype(np.int64))


def test_save_mesh_writes_what_extract_geometry_returns(tmp_path):
    from nerf_signature_amd import mesh
    m = _nerf(opaque=True)
    path = str(tmp_path / "meshes" / "hotdog.ply")
    V, T = mesh.save_mesh(m, path, resolution=128, threshold=10)
    v, t = mesh.extract_geometry(m.aabb_infer[:3], m.aabb_infer[3:], 128, 10, lambda p: m.density(p)["sigma"])
    rv, rt = mc_ref.read_ply(path)
    assert (V, T) == (len(v), len(t)) and T > 100
    assert np.array_equal(rv, v) and np.array_equal(rt, t)
