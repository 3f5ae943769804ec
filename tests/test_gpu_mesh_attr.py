"""Mesh attributes and cleaning on the GPU: mc_vertex_normals and mesh_components against the numpy restatement (tests/mesh_attr_ref.py), bit for bit;
mesh.clean against the restated filter and compaction; vertex colours against the model's own forward; save_mesh with every option end to end."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mc_ref  # noqa: E402
import mesh_attr_ref as mar  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


# ---- normals ----------------------------------------------------------------------------------------------------------------------------------------------

def _normals_same(u, thr, scale=(1.0, 1.0, 1.0)):
    """GPU == restatement: gradients bit-equal wherever they are numbers (a NaN's sign and payload are the hardware's), NaN in the same places;
    unit normals bit-equal (-ffp-contract=off, correctly rounded fp32 sqrtf and division); both routes to the scratch; mc_emit's outputs untouched."""
    from nerf_signature_amd import mesh
    ud = _dev(u)
    rv, rt = mc_ref.marching_cubes(u, thr)
    rn, rg = mar.vertex_normals(u, thr, scale)
    v, t, n = mesh.marching_cubes(ud, thr, normals=True, scale=scale)            # the scratch of this very call
    n2, g = mesh.vertex_normals(ud, thr, scale=scale, gradients=True)            # recomputed
    assert n.dtype == torch.float32 and tuple(n.shape) == rn.shape and tuple(g.shape) == rg.shape
    assert torch.equal(n.view(torch.int32), n2.view(torch.int32))
    n, g = n.cpu().numpy(), g.cpu().numpy()
    num = ~np.isnan(rg)
    assert np.array_equal(np.isnan(g), ~num)
    assert np.array_equal(_bits(g)[num], _bits(rg)[num])
    assert np.array_equal(_bits(n), _bits(rn))
    assert np.array_equal(_bits(v.cpu().numpy()), _bits(rv)) and np.array_equal(t.cpu().numpy(), rt)       # after the normals: unchanged
    return rn, rg


def test_normals_of_all_256_single_cell_cases():
    """(2, 2, 2): every difference is one-sided."""
    rng = np.random.default_rng(0)
    for case in range(256):
        mag = rng.uniform(0.1, 3.0, 8).astype(np.float32)
        u = np.empty((2, 2, 2), np.float32)
        for c in range(8):
            x, y, z = c & 1, (c >> 1) & 1, (c >> 2) & 1
            u[x, y, z] = 0.5 + (mag[c] if (case >> c) & 1 else -mag[c])
        rn, _ = _normals_same(u, 0.5)
        assert (len(rn) > 0) == (case not in (0, 255))


def _smooth(shape):
    rng = np.random.default_rng(sum(shape))
    g = [np.linspace(0, 1, n, dtype=np.float64) for n in shape]
    X, Y, Z = np.meshgrid(*g, indexing="ij")
    return (np.sin(7.1 * X + 1.3) * np.cos(5.3 * Y - 0.4) + np.sin(6.7 * Z + 2.0 * X) + 0.05 * rng.standard_normal(shape)).astype(np.float32)


@pytest.mark.parametrize("shape", [(3, 3, 3), (5, 40, 33), (17, 17, 17), (129, 129, 129)])
def test_normals_sizes(shape):
    """More than one workgroup, vertex bases that cross workgroups, every border of the lattice (one-sided differences beside central ones)."""
    rn, _ = _normals_same(_smooth(shape), 0.1)
    assert len(rn) > 0 and np.abs(np.linalg.norm(rn.astype(np.float64), axis=1) - 1).max() < 2e-7


def test_normals_with_threshold_ties_nan_and_infinities():
    rng = np.random.default_rng(4)
    u = rng.standard_normal((24, 20, 28)).astype(np.float32)
    pick = rng.integers(0, 64, u.shape)
    u[pick < 6] = 0.25           # equal to the threshold (outside): t = 0 or 1 on the edges to inside nodes
    u[pick == 6] = np.nan
    u[pick == 7] = np.inf
    u[pick == 8] = -np.inf
    rn, rg = _normals_same(u, 0.25)
    zero = ~rn.any(axis=1)
    assert zero.sum() > 1000 and (~zero).sum() > 1000                      # both kinds are there
    assert not np.isfinite(rg[zero]).all(axis=1).all() and np.isfinite(rn).all()


def test_normals_with_an_anisotropic_scale():
    rn, rg = _normals_same(_smooth((5, 40, 33)), 0.1, scale=(63.0 / 2.0, 63.0 / 2.3, 63.0 / 1.7))
    assert np.abs(np.linalg.norm(rn.astype(np.float64), axis=1) - 1).max() < 2e-7


def test_normals_of_an_empty_mesh():
    from nerf_signature_amd import mesh
    v, t, n = mesh.marching_cubes(torch.full((9, 7, 5), -1.0, device=DEV), 0.0, normals=True)
    assert v.shape == (0, 3) and t.shape == (0, 3) and n.shape == (0, 3)


# ---- components -------------------------------------------------------------------------------------------------------------------------------------------

def _strip(n, order):
    t = np.arange(n)[:, None] + np.arange(3)[None, :]
    V = n + 2
    perm = {"ascending": np.arange(V), "descending": np.arange(V)[::-1], "random": np.random.default_rng(7).permutation(V)}[order]
    return perm[t].astype(np.int32), V


def _tetrahedra(n):
    rng = np.random.default_rng(8)
    faces = np.array([[0, 1, 2], [0, 3, 1], [1, 3, 2], [2, 3, 0]])
    t = (4 * np.arange(n)[:, None, None] + faces[None]).reshape(-1, 3)
    return rng.permutation(4 * n)[t][rng.permutation(len(t))].astype(np.int32), 4 * n


def _fan(n):
    i = np.arange(1, n + 1)
    return np.stack([np.zeros(n, np.int64), i, i + 1], -1).astype(np.int32), n + 2


@functools.lru_cache(maxsize=None)
def _mesh(name):
    """(vertices, triangles, V) on the host."""
    if name == "noise":
        u, thr = mar.noise_lattice()
    else:
        u, thr = mar.two_spheres_and_specks(), 0.0
    v, t = mc_ref.marching_cubes(u, thr)
    return v, t, len(v)


def _case(name):
    if name == "one_triangle":
        return np.array([[2, 0, 1]], np.int32), 3
    if name == "two_disjoint_triangles":
        return np.array([[5, 3, 4], [1, 2, 0]], np.int32), 6
    if name.startswith("strip_"):
        return _strip(4097, name[6:])
    if name == "tetrahedra":
        return _tetrahedra(3000)
    if name == "fan":
        return _fan(5000)
    if name == "isolated_vertices":
        t, V = _strip(4097, "random")
        return t, V + 1000
    _, t, V = _mesh(name)
    return t, V


CASES = ["one_triangle", "two_disjoint_triangles", "strip_ascending", "strip_descending", "strip_random", "tetrahedra", "fan", "isolated_vertices",
         "noise", "spheres"]


@pytest.mark.parametrize("name", CASES)
def test_components_equal_the_union_find(name):
    from nerf_signature_amd import mesh
    t, V = _case(name)
    want = mar.components(t, V)
    td = _dev(t)
    a = mesh.components(td, V)
    b = mesh.components(td, V)
    assert a.dtype == torch.int32 and tuple(a.shape) == (V,)
    assert np.array_equal(a.cpu().numpy(), want) and torch.equal(a, b)
    if name == "noise":
        assert len(np.unique(want)) >= 200
    if name == "isolated_vertices":
        assert np.array_equal(want[-1000:], np.arange(V - 1000, V))


def test_components_without_triangles_or_vertices():
    from nerf_signature_amd import mesh
    none = torch.zeros(0, 3, dtype=torch.int32, device=DEV)
    assert mesh.components(none, 5).tolist() == [0, 1, 2, 3, 4] and mesh.components(none, 0).shape == (0,)


def test_ids_out_of_range_are_refused_not_dereferenced():
    from nerf_signature_amd import mesh
    t = np.array([[0, 1, 2], [2, 3, 7], [4, 5, 6], [-1, 0, 1], [3, 4, 2 ** 31 - 1]], np.int32)
    with pytest.raises(ValueError, match=r"triangle 1 has a vertex id outside \[0, 7\)"):
        mesh.components(_dev(t), 7)
    with pytest.raises(ValueError, match="triangle 3 "):
        mesh.components(_dev(t), 8)
    with pytest.raises(ValueError, match="triangle 1 "):
        mesh.clean(torch.zeros(7, 3, device=DEV), _dev(t))
    with pytest.raises(ValueError, match="int32"):
        mesh.components(_dev(t.astype(np.int64)), 8)
    assert mesh.components(_dev(t[:3]), 8).tolist() == [0, 0, 0, 0, 4, 4, 4, 0]    # and the device is fine afterwards


# ---- clean --------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("options", [{"min_triangles": 8}, {"keep_largest": 1}], ids=["min_triangles_8", "keep_largest_1"])
@pytest.mark.parametrize("name", ["noise", "spheres"])
def test_clean_equals_the_restated_filter(name, options):
    from nerf_signature_amd import mesh
    v, t, V = _mesh(name)
    normals = mar.vertex_normals(*((mar.noise_lattice()) if name == "noise" else (mar.two_spheres_and_specks(), 0.0)))[0]
    ids = np.arange(V, dtype=np.int64)
    wv, wt, wn, wi = mar.clean(v, t, attributes=(normals, ids), **options)
    gv, gt, gn, gi = mesh.clean(_dev(v), _dev(t), attributes=(_dev(normals), _dev(ids)), **options)
    assert gv.dtype == torch.float32 and gt.dtype == torch.int32 and 0 < len(wt) < len(t)
    assert np.array_equal(_bits(gv.cpu().numpy()), _bits(wv)) and np.array_equal(gt.cpu().numpy(), wt)
    assert np.array_equal(_bits(gn.cpu().numpy()), _bits(wn)) and np.array_equal(gi.cpu().numpy(), wi)
    assert (mc_ref.undirected_edge_counts(gt.cpu().numpy()) == 2).all() and mc_ref.is_closed_oriented(gt.cpu().numpy())
    if "keep_largest" in options:
        assert len(np.unique(mar.components(wt, len(wv)))) == 1


def test_clean_with_defaults_and_with_nothing_left():
    from nerf_signature_amd import mesh
    v, t, V = _mesh("spheres")
    gv, gt = mesh.clean(_dev(v), _dev(t))
    assert np.array_equal(gv.cpu().numpy(), v) and np.array_equal(gt.cpu().numpy(), t)
    gv, gt, ga = mesh.clean(_dev(v), _dev(t), min_triangles=10 ** 6, attributes=(_dev(v),))
    assert gv.shape == (0, 3) and gt.shape == (0, 3) and ga.shape == (0, 3)
    none = torch.zeros(0, 3, dtype=torch.int32, device=DEV)
    gv, gt = mesh.clean(torch.zeros(0, 3, device=DEV), none, keep_largest=3)
    assert gv.shape == (0, 3) and gt.shape == (0, 3)


# ---- colours and end to end -----------------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _nerf():
    from nerf_signature_amd import synthetic
    from nerf_signature_amd.network import NeRFNetwork
    m = NeRFNetwork(bound=1.0, cuda_ray=True, density_scale=1, min_near=0.2, density_thresh=10, bg_radius=-1, message_dim=32, n_views=1)
    synthetic.init_model(m, "hotdog", opaque=True)
    return m.to(DEV).eval()


R = 64


@pytest.mark.parametrize("with_message", [False, True], ids=["clean", "message"])
def test_colours_and_save_mesh_with_every_option(with_message, mlp_prec, tmp_path):
    from nerf_signature_amd import mesh
    m = _nerf()
    msg = torch.randint(0, 2, (32,), generator=torch.Generator().manual_seed(5)).float().to(DEV) if with_message else None
    lo, hi = m.aabb_infer[:3], m.aabb_infer[3:]
    u = mesh.lattice(m, lo, hi, R, msg)
    v, t, n = mesh.marching_cubes(u, 10, normals=True, scale=mesh.lattice_scale(lo, hi, R))
    rn, _ = mar.vertex_normals(u.cpu().numpy(), 10, mesh.lattice_scale(lo, hi, R))
    assert len(t) > 100 and np.array_equal(_bits(n.cpu().numpy()), _bits(rn))
    cv, ct, cn = mesh.clean(v, t, min_triangles=8, attributes=(n,))
    assert 0 < len(ct) <= len(t)

    world, _ = mesh.to_world(cv, ct, lo, hi, R)
    wd = mesh.world_vertices(cv, lo, hi, R)
    assert wd.dtype == torch.float64 and np.array_equal(wd.cpu().numpy(), world)
    x = wd.float()
    rgb = mesh.vertex_colors(m, x, cn, msg)
    d = torch.where((cn == 0).all(dim=-1, keepdim=True), torch.tensor([0.0, 0.0, 1.0], device=DEV), -cn)
    with torch.no_grad():
        _, want = m(x, d, msg)
    assert rgb.dtype == torch.float32 and torch.equal(rgb, want)
    assert torch.equal(mesh.vertex_colors(m, wd, cn, msg), want)                         # float64 positions are rounded to float32

    path = str(tmp_path / "meshes" / "coloured.ply")
    assert mesh.save_mesh(m, path, resolution=R, threshold=10, message=msg, normals=True, colors=True, min_triangles=8) == (len(cv), len(ct))
    got = mar.read_ply(path)
    assert np.array_equal(got["vertices"], world) and np.array_equal(got["faces"], ct.cpu().numpy())
    assert np.array_equal(_bits(got["normals"]), _bits(cn.cpu().numpy()))
    q = mar.quantize_colors(rgb.cpu().numpy())
    assert np.array_equal(got["colors"], q) and q.std() > 0

    only = str(tmp_path / "colours_only.ply")                                            # colours imply normals are computed, not written
    mesh.save_mesh(m, only, resolution=R, threshold=10, message=msg, colors=True, min_triangles=8)
    got = mar.read_ply(only)
    assert "normals" not in got and np.array_equal(got["colors"], q) and np.array_equal(got["vertices"], world)


def test_save_mesh_with_defaults_writes_the_same_bytes_as_before(tmp_path):
    from nerf_signature_amd import mesh
    m = _nerf()
    lo, hi = m.aabb_infer[:3], m.aabb_infer[3:]
    a, b = str(tmp_path / "a.ply"), str(tmp_path / "b.ply")
    V, T = mesh.save_mesh(m, a, resolution=R, threshold=10)
    v, t = mesh.marching_cubes(mesh.lattice(m, lo, hi, R), 10)
    mar.write_ply_before_attributes(b, *mesh.to_world(v, t, lo, hi, R))
    assert (V, T) == (len(v), len(t)) and T > 100 and open(a, "rb").read() == open(b, "rb").read()
