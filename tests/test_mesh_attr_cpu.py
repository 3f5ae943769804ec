"""Mesh attributes and cleaning without a GPU: the numpy restatement (tests/mesh_attr_ref.py) proved against scipy and analytic lattices, the PLY
writer's attribute records and its unchanged default, and the argument checks of the new C entry points."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mc_ref  # noqa: E402
import mesh_attr_ref as mar  # noqa: E402


# ---- components -------------------------------------------------------------------------------------------------------------------------------------------

def _scipy_labels(tris, V):
    """scipy's components relabelled to the smallest vertex id of each."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    t = np.asarray(tris, np.int64).reshape(-1, 3)
    r = np.concatenate([t[:, 0], t[:, 1], t[:, 2]])
    c = np.concatenate([t[:, 1], t[:, 2], t[:, 0]])
    _, lab = connected_components(coo_matrix((np.ones(r.size, np.int8), (r, c)), shape=(V, V)), directed=False)
    smallest = np.full(lab.max() + 1 if V else 0, V, np.int64)
    np.minimum.at(smallest, lab, np.arange(V))
    return smallest[lab].astype(np.int32)


@pytest.mark.parametrize("V,T,seed", [(1, 0, 0), (7, 1, 1), (50, 20, 2), (400, 150, 3), (3000, 2500, 4), (5000, 900, 5)])
def test_components_equal_scipy_on_triangle_soups(V, T, seed):
    tris = np.random.default_rng(seed).integers(0, V, (T, 3)).astype(np.int32)       # degenerate triangles (repeated ids) included
    got = mar.components(tris, V)
    assert got.dtype == np.int32 and np.array_equal(got, _scipy_labels(tris, V))
    assert (got <= np.arange(V)).all() and np.array_equal(got[got], got)


def test_components_equal_scipy_on_marching_cubes_meshes():
    u, level = mar.noise_lattice()
    for lattice, thr in ((u, level), (mar.two_spheres_and_specks(), 0.0)):
        v, t = mc_ref.marching_cubes(lattice, thr)
        got = mar.components(t, len(v))
        assert np.array_equal(got, _scipy_labels(t, len(v)))
    u, level = mar.noise_lattice()
    v, t = mc_ref.marching_cubes(u, level)
    assert len(np.unique(mar.components(t, len(v)))) >= 200              # the lattice the GPU test uses: hundreds of components
    v, t = mc_ref.marching_cubes(mar.two_spheres_and_specks(), 0.0)
    lab = mar.components(t, len(v))
    assert sorted(np.bincount(lab[t[:, 0]])[np.unique(lab)].tolist())[:2] == [1, 8] and len(np.unique(lab)) == 4


# ---- normals ----------------------------------------------------------------------------------------------------------------------------------------------

def _angle(a, b):
    """Angle between unit-ish vectors through the cross product (well conditioned near zero), float64."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.arctan2(np.linalg.norm(np.cross(a, b), axis=1), np.einsum("ij,ij->i", a, b))


def test_normals_of_a_sphere_are_radial_to_the_finite_difference_error():
    """The float32 lattice 100 - r of a sphere of radius 20.5 in 64^3, threshold 79.5.  Measured here: the float64 evaluation of the formula deviates
    from the radial direction by at most 5.04e-4 rad (0.029 degrees).  That is the formula's error, not the kernel's: central differences of r
    truncate at (h^2 / 6) times the third derivative of r, at most 1 / (3 r^2) = 7.9e-4 per component for h = 1, and the edge interpolation stays
    inside that; asserted below 1e-3.  The fp32 restatement may add, per vertex, no more than 1.2e-6 rad: each gradient component (magnitude <= 1)
    goes through at most 8 roundings of 2^-24 relative (difference, halving, the interpolation's three operations, t's three) and the normalisation
    through 3 more that are not common to all components, so the direction moves by less than sqrt(3) * 11 * 2^-24 = 1.14e-6.  Measured: 6.5e-8 rad."""
    c, r = 31.5, 20.5
    u = mar.ball((64, 64, 64), (c, c, c), 100.0)             # 100 - distance
    thr = np.float32(100.0 - r)
    v, _ = mc_ref.marching_cubes(u, thr)
    n32, _ = mar.vertex_normals(u, thr)
    n64, _ = mar.vertex_normals(u, thr, dtype=np.float64)
    assert n32.dtype == np.float32 and n32.shape == v.shape and len(v) > 5000
    radial = v.astype(np.float64) - c
    radial /= np.linalg.norm(radial, axis=1, keepdims=True)
    e64, e32, step = _angle(n64, radial), _angle(n32, radial), _angle(n32, n64)
    print(f"formula error {e64.max():.3e} rad, fp32 restatement {e32.max():.3e} rad, fp32 against fp64 {step.max():.3e} rad")
    assert e64.max() < 1e-3
    assert (e32 <= e64 + 1.2e-6).all() and step.max() <= 1.2e-6
    assert np.abs(np.linalg.norm(n32.astype(np.float64), axis=1) - 1).max() < 2e-7
    assert (np.einsum("ij,ij->i", n32, radial) > 0.999).all()                # outwards


def test_normals_are_zero_where_the_gradient_is_not_finite_or_zero():
    u = np.zeros((4, 4, 4), np.float32)
    u[1, 1, 1] = np.inf                         # every vertex touches the infinite node: inf - inf or inf gradients
    n, g = mar.vertex_normals(u, 0.5)
    assert len(n) == 6 and not n.any() and not np.isfinite(g).all()
    flat = np.zeros((3, 3, 3), np.float32)
    flat[1, 1, 1] = 1.0                         # central differences across the bump cancel at t = 0.5 ... but not one-sided ones: check against the rule itself
    n, g = mar.vertex_normals(flat, 0.5)
    length = np.sqrt((g.astype(np.float64) ** 2).sum(1))
    assert np.array_equal(~n.any(axis=1), length == 0)


def test_anisotropic_scale_is_applied_per_axis():
    u = mar.ball((20, 22, 24), (9.3, 10.1, 11.7), 6.0)
    _, g1 = mar.vertex_normals(u, 0.0)
    n, g = mar.vertex_normals(u, 0.0, scale=(2.0, 0.5, 3.0))
    assert np.array_equal(g, g1 * np.array([2.0, 0.5, 3.0], np.float32))
    assert np.abs(np.linalg.norm(n.astype(np.float64), axis=1) - 1).max() < 2e-7


# ---- filter and compaction ----------------------------------------------------------------------------------------------------------------------------------

def _closed(t):
    return len(t) > 0 and bool((mc_ref.undirected_edge_counts(t) == 2).all()) and mc_ref.is_closed_oriented(t)


def test_clean_keeps_closed_meshes_closed_and_carries_attributes():
    u, level = mar.noise_lattice()
    v, t = mc_ref.marching_cubes(u, level)
    ids = np.arange(len(v))
    cv, ct, cid = mar.clean(v, t, min_triangles=9, attributes=(ids,))
    assert 0 < len(ct) < len(t) and not _closed(t) and _closed(ct)          # the open border pieces (1 and 4 triangles) are gone too
    assert np.array_equal(cv, v[cid]) and (np.diff(cid) > 0).all()                    # stable, attributes carried
    assert np.array_equal(cv[ct], v[t][np.isin(t[:, 0], cid)])                        # the surviving triangles, in order, with the same corners
    sizes = np.bincount(mar.components(ct, len(cv))[ct[:, 0]])
    assert sizes[sizes > 0].min() >= 9
    same = mar.clean(v, t)
    assert np.array_equal(same[0], v) and np.array_equal(same[1], t)                  # defaults: nothing to remove (every vertex is used)


def test_keep_largest_keeps_the_larger_sphere():
    u = mar.two_spheres_and_specks()
    v, t = mc_ref.marching_cubes(u, 0.0)
    cv, ct = mar.clean(v, t, keep_largest=1)
    assert _closed(ct) and mc_ref.euler_characteristic(len(cv), ct) == 2
    assert np.abs(cv - np.array([13.2, 14.1, 15.3])).max() < 9.5 and np.linalg.norm(cv - np.array([13.2, 14.1, 15.3]), axis=1).min() > 8.5
    cv2, ct2 = mar.clean(v, t, keep_largest=2)
    assert len(np.unique(mar.components(ct2, len(cv2)))) == 2 and _closed(ct2)
    u, level = mar.noise_lattice()
    nv_, nt_ = mc_ref.marching_cubes(u, level)
    n8 = mar.clean(nv_, nt_, min_triangles=8)
    assert len(nt_) - len(n8[1]) == 3 * 1 + 4 and _closed(n8[1])                       # exactly the four open pieces
    cv8, ct8 = mar.clean(v, t, min_triangles=8)                                       # the open corner triangle goes, the octahedron (8) stays
    assert len(np.unique(mar.components(ct8, len(cv8)))) == 3 and _closed(ct8)
    none = mar.clean(v, t, min_triangles=10 ** 6)
    assert none[0].shape == (0, 3) and none[1].shape == (0, 3)


def test_ties_go_to_the_smaller_label_and_unreferenced_vertices_are_dropped():
    # vertex 0 unused; three components of 2 triangles (labels 1, 5, 9) and one of 1 triangle (label 13)
    t = np.array([[9, 10, 11], [5, 6, 7], [1, 2, 3], [13, 14, 15], [2, 3, 4], [10, 11, 12], [6, 7, 8]], np.int32)
    v = np.arange(17 * 3, dtype=np.float32).reshape(17, 3)
    lab = mar.components(t, 17)
    assert lab.tolist() == [0, 1, 1, 1, 1, 5, 5, 5, 5, 9, 9, 9, 9, 13, 13, 13, 16]
    cv, ct = mar.clean(v, t, keep_largest=2)
    assert np.array_equal(cv, v[1:9]) and ct.tolist() == [[4, 5, 6], [0, 1, 2], [1, 2, 3], [5, 6, 7]]
    cv, ct = mar.clean(v, t, keep_largest=4, min_triangles=2)
    assert np.array_equal(cv, v[1:13]) and len(ct) == 6
    cv, ct = mar.clean(v, t)
    assert np.array_equal(cv, v[1:16]) and np.array_equal(ct, t - 1)


# ---- PLY --------------------------------------------------------------------------------------------------------------------------------------------------

def _small_mesh():
    verts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0.25, -1e-300, 7.5]], np.float64)
    tris = np.array([[0, 1, 2], [2, 1, 3]], np.int64)
    normals = np.array([[0, 0, 1], [0, -0.0, -1], [0.6, 0.8, 0], [0, 0, 0]], np.float32)
    colors = np.array([[0.0, 1.0, 0.5], [-3.0, 7.0, 0.49803922], [0.001, 0.002, 0.999], [np.float32(0.5 / 255), 0.25, 0.75]], np.float32)
    return verts, tris, normals, colors


def test_ply_with_normals_and_colours_round_trips(tmp_path):
    from nerf_signature_amd import mesh
    verts, tris, normals, colors = _small_mesh()
    q = mar.quantize_colors(colors)
    assert q.tolist()[:2] == [[0, 255, 128], [0, 255, 127]] and np.array_equal(mesh.quantize_colors(colors), q)
    for kw in ({"normals": normals, "colors": colors}, {"normals": normals}, {"colors": colors}, {"colors": q}, {}):
        path = str(tmp_path / ("_".join(sorted(kw)) + "x.ply"))
        mesh.write_ply(path, verts, tris, **kw)
        got = mar.read_ply(path)
        assert np.array_equal(got["vertices"], verts) and np.array_equal(got["faces"], tris)
        assert ("normals" in got) == ("normals" in kw) and ("colors" in got) == ("colors" in kw)
        if "normals" in kw:
            assert np.array_equal(got["normals"].view(np.int32), normals.view(np.int32))
        if "colors" in kw:
            assert np.array_equal(got["colors"], q)


def test_ply_without_attributes_is_byte_equal_to_the_writer_before_them(tmp_path):
    from nerf_signature_amd import mesh
    verts, tris, _, _ = _small_mesh()
    v, t = mc_ref.marching_cubes(mar.two_spheres_and_specks(), 0.0)
    for k, (vv, tt) in enumerate(((verts, tris), (v, t), (np.zeros((0, 3)), np.zeros((0, 3), np.int64)))):
        a, b = str(tmp_path / f"a{k}.ply"), str(tmp_path / f"b{k}.ply")
        mesh.write_ply(a, vv, tt)
        mesh.write_ply(b, vv, tt, normals=None, colors=None)
        mar.write_ply_before_attributes(str(tmp_path / f"c{k}.ply"), vv, tt)
        want = open(str(tmp_path / f"c{k}.ply"), "rb").read()
        assert open(a, "rb").read() == want and open(b, "rb").read() == want
        rv, rt = mc_ref.read_ply(a)
        assert np.array_equal(rv, np.asarray(vv, np.float64)) and np.array_equal(rt, tt)


# ---- argument checks --------------------------------------------------------------------------------------------------------------------------------------

def test_python_entry_points_refuse_what_they_cannot_take():
    import torch
    from nerf_signature_amd import mesh
    with pytest.raises(ValueError, match="GPU"):
        mesh.vertex_normals(torch.zeros(4, 4, 4), 0.0)
    with pytest.raises(ValueError, match="GPU"):
        mesh.components(torch.zeros(2, 3, dtype=torch.int32), 4)
    with pytest.raises(ValueError, match="GPU"):
        mesh.clean(torch.zeros(4, 3), torch.zeros(2, 3, dtype=torch.int32))
    with pytest.raises(ValueError, match="GPU"):
        mesh.marching_cubes(torch.zeros(4, 4, 4), 0.0, normals=True)


def test_c_entry_points_check_their_arguments():
    from nerf_signature_amd import build, _native as nv
    build.build()
    d, off = nv._vp(256), nv._vp(264)
    normals = lambda u=d, dims=(4, 4, 4), s=d, V=5, n=d: ("mc_vertex_normals", u, *dims, 0.0, s, V, 1.0, 1.0, 1.0, n, None, None)
    for args, msg in ((normals(u=None), "null pointer"), (normals(s=None), "null pointer"), (normals(n=None), "null pointer"),
                      (normals(dims=(4, 1, 4)), "at least 2"), (normals(dims=(1 << 10, 1 << 10, (1 << 8) + 1)), "out of range"),
                      (normals(s=off), "16-byte aligned"), (normals(V=3 * 64 + 1), "out of range")):
        with pytest.raises(ValueError, match=msg):
            nv.call(*args)
    nv.call(*normals(V=0, n=None))                                   # an empty mesh: accepted, nothing launched
    size = nv.fn("mesh_components_scratch_bytes")
    assert size(1 << 31, 0) == 0 and size(0, 1 << 31) == 0 and size(0, 0) >= 4 and size((1 << 31) - 1, (1 << 31) - 1) >= 4
    comps = lambda t=d, T=2, V=4, lab=d, s=d: ("mesh_components", t, T, V, lab, s, None)
    for args, msg in ((comps(t=None), "null pointer"), (comps(lab=None), "null pointer"), (comps(s=None), "null pointer"),
                      (comps(V=1 << 31), "out of range"), (comps(T=1 << 31), "out of range"), (comps(s=off), "16-byte aligned")):
        with pytest.raises(ValueError, match=msg):
            nv.call(*args)
