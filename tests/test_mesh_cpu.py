"""Mesh extraction without a GPU: the generated triangulation table, the numpy restatement of the kernels on analytic lattices, the PLY
writer and the argument checks of the Python and C entry points."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mc_ref  # noqa: E402
from nerf_signature_amd import mc_table as mt  # noqa: E402


# ---- the table ----------------------------------------------------------------------------------------------------------------------------------------

def test_generator_reproduces_the_committed_header():
    text, mx = mt.render()
    with open(mt.HEADER, "rb") as f:
        assert f.read() == text.encode("utf-8")
    assert mx == 5 and mt.main([]) == 0


def _crossing(case):
    inside = [(case >> c) & 1 for c in range(8)]
    return {e for e, (a, b) in enumerate(mt.EDGE_CORNERS) if inside[a] != inside[b]}


def _mid(e):
    a, b = mt.EDGE_CORNERS[e]
    return (np.array(mt.CORNERS[a], float) + np.array(mt.CORNERS[b], float)) / 2


@pytest.mark.parametrize("case", range(256))
def test_every_case_follows_the_rule(case):
    tris = mt.triangles(case)
    assert len(tris) <= 5
    used = {e for t in tris for e in t}
    assert used == _crossing(case)                                   # only crossing edges, and all of them
    directed = [(t[i], t[(i + 1) % 3]) for t in tris for i in range(3)]
    assert len(set(directed)) == len(directed)                        # no directed edge twice
    boundary = {d for d in directed if (d[1], d[0]) not in directed}
    assert boundary == set(mt.face_segments(case))                   # the boundary is exactly what the face rule draws, in its direction
    segs = {frozenset(s) for s in mt.face_segments(case)}
    for p, q in directed:
        if frozenset((p, q)) not in segs:                            # an interior (fan) diagonal: once each way, never inside one face
            assert (q, p) in directed
            assert not (mt.EDGE_FACES[p] & mt.EDGE_FACES[q]), (case, p, q)
    assert (len(tris) > 0) == (case not in (0, 255))


@pytest.mark.parametrize("corner", range(8))
@pytest.mark.parametrize("flip", [False, True])
def test_normals_point_from_inside_to_outside(corner, flip):
    """One corner inside (flip: one corner outside): every normal points away from (towards) that corner."""
    case = (1 << corner) ^ (0xFF if flip else 0)
    tris = mt.triangles(case)
    assert len(tris) == 1
    a, b, c = (_mid(e) for e in tris[0])
    n = np.cross(b - a, c - a)
    away = (a + b + c) / 3 - np.array(mt.CORNERS[corner], float)
    assert np.dot(n, away) * (-1 if flip else 1) > 0


def test_face_rule_depends_on_the_face_alone():
    """Two cells sharing a face draw the same segments on it, in opposite directions (seen from each cell's outside)."""
    for case in range(256):
        segs = mt.face_segments(case)
        for axis in range(3):
            # the +axis face of this cell is the -axis face of its neighbour with the same 4 corner signs
            nb = 0
            for c in range(8):
                x = list(mt.CORNERS[c])
                if x[axis] == 1:
                    x[axis] = 0
                    nb |= ((case >> c) & 1) << (x[0] + 2 * x[1] + 4 * x[2])
            _, edges_hi, _ = mt.FACES[2 * axis + 1]
            _, edges_lo, _ = mt.FACES[2 * axis]
            shift = {e: next(f for f in edges_lo if mt.EDGES[f] == (mt.EDGES[e][0], mt.EDGES[e][1] - (1 << axis))) for e in edges_hi}
            mine = {(shift[p], shift[q]) for p, q in segs if p in edges_hi and q in edges_hi}
            theirs = {(q, p) for p, q in mt.face_segments(nb) if p in edges_lo and q in edges_lo}
            assert mine == theirs, (case, axis)


# ---- the restatement on analytic lattices -------------------------------------------------------------------------------------------------------------

def _grid(n):
    return np.stack(np.meshgrid(*(np.arange(n, dtype=np.float64),) * 3, indexing="ij"), axis=-1) - (n - 1) / 2


def test_sphere_is_closed_with_euler_characteristic_two_and_the_right_volume():
    r = 24.0
    u = (r - np.linalg.norm(_grid(64), axis=-1)).astype(np.float32)
    v, t = mc_ref.marching_cubes(u, 0.0)
    assert (mc_ref.undirected_edge_counts(t) == 2).all() and mc_ref.is_closed_oriented(t)
    assert mc_ref.euler_characteristic(len(v), t) == 2
    vol = mc_ref.signed_volume(v, t)
    assert abs(vol / (4 / 3 * np.pi * r ** 3) - 1) < 0.01, vol     # positive: the normals point out of the sphere


def test_torus_has_euler_characteristic_zero():
    p = _grid(48)
    q = np.sqrt(p[..., 0] ** 2 + p[..., 1] ** 2) - 14.0
    u = (6.0 - np.sqrt(q ** 2 + p[..., 2] ** 2)).astype(np.float32)
    v, t = mc_ref.marching_cubes(u, 0.0)
    assert (mc_ref.undirected_edge_counts(t) == 2).all() and mc_ref.is_closed_oriented(t)
    assert mc_ref.euler_characteristic(len(v), t) == 0


@pytest.mark.parametrize("n", [16, 23, 32])
@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_noise_gives_closed_consistently_oriented_meshes(n, sign):
    u = (sign * np.random.default_rng(n).standard_normal((n, n, n))).astype(np.float32)
    u[[0, -1], :, :] = u[:, [0, -1], :] = u[:, :, [0, -1]] = -1.0       # padded: the surface stays off the border
    v, t = mc_ref.marching_cubes(u, 0.0)
    assert len(t) > 100
    assert (mc_ref.undirected_edge_counts(t) == 2).all() and mc_ref.is_closed_oriented(t)


def test_every_vertex_interpolates_to_the_threshold():
    rng = np.random.default_rng(5)
    u = (rng.standard_normal((20, 17, 9)) * 10).astype(np.float32)
    thr = np.float32(0.7)
    v, t = mc_ref.marching_cubes(u, thr)
    frac = v - np.floor(v)
    ax = np.argmax(frac, axis=1)
    inner = frac.max(axis=1) > 0                                      # vertices strictly inside their edge (t in (0, 1))
    assert inner.mean() > 0.95
    lo = np.floor(v[inner]).astype(np.int64)
    a = u[lo[:, 0], lo[:, 1], lo[:, 2]].astype(np.float64)
    hi = lo.copy()
    hi[np.arange(len(hi)), ax[inner]] += 1
    b = u[hi[:, 0], hi[:, 1], hi[:, 2]].astype(np.float64)
    tt = frac[inner].max(axis=1).astype(np.float64)
    err = np.abs(a + tt * (b - a) - thr)
    # the vertex is float(i) + t in fp32: |t| rounding (2^-24 relative) plus the coordinate's rounding (ulp of i + t) times |b - a|
    bound = (np.spacing(np.float32(lo[np.arange(len(lo)), ax[inner]] + 1)).astype(np.float64) + 2 ** -23) * np.abs(b - a) + 4 * np.spacing(np.float32(np.abs(a) + np.abs(thr)))
    assert (err <= bound).all(), float(np.max(err / bound))


def test_empty_and_full_lattices_give_nothing():
    for val in (-1.0, 1.0):
        v, t = mc_ref.marching_cubes(np.full((5, 4, 3), val, np.float32), 0.0)
        assert v.shape == (0, 3) and t.shape == (0, 3)


# ---- the PLY writer ------------------------------------------------------------------------------------------------------------------------------------

def test_ply_round_trip(tmp_path):
    from nerf_signature_amd import mesh
    verts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0.25, -1e-300, 7.5]], np.float64)
    tris = np.array([[0, 1, 2], [2, 1, 3]], np.int64)
    path = str(tmp_path / "two.ply")
    mesh.write_ply(path, verts, tris)
    v, t = mc_ref.read_ply(path)
    assert np.array_equal(v, verts) and np.array_equal(t, tris)


# ---- argument checks ----------------------------------------------------------------------------------------------------------------------------------

def test_marching_cubes_refuses_what_it_cannot_march():
    import torch
    from nerf_signature_amd import mesh
    with pytest.raises(ValueError, match="GPU"):
        mesh.marching_cubes(torch.zeros(4, 4, 4), 0.0)
    with pytest.raises(ValueError, match="GPU"):
        mesh.marching_cubes(np.zeros((4, 4, 4), np.float32), 0.0)


def test_c_entry_points_check_their_arguments():
    from nerf_signature_amd import build, _native as nv
    build.build()
    d = nv._vp(256)
    assert nv.fn("mc_scratch_bytes")(1, 4, 4) == 0 and nv.fn("mc_scratch_bytes")(1 << 10, 1 << 10, 1 << 9) == 0
    assert nv.fn("mc_scratch_bytes")(256, 256, 256) >= 6 * 256 ** 3
    with pytest.raises(ValueError, match="null pointer"):
        nv.call("mc_count", None, 4, 4, 4, 0.0, d, d, None)
    with pytest.raises(ValueError, match="at least 2"):
        nv.call("mc_count", d, 4, 1, 4, 0.0, d, d, None)
    with pytest.raises(ValueError, match="out of range"):
        nv.call("mc_count", d, 1 << 10, 1 << 10, (1 << 8) + 1, 0.0, d, d, None)
    with pytest.raises(ValueError, match="16-byte aligned"):
        nv.call("mc_emit", d, 4, 4, 4, 0.0, nv._vp(264), 3, 1, d, d, None)
    with pytest.raises(ValueError, match="not the totals"):
        nv.call("mc_emit", d, 4, 4, 4, 0.0, d, 3, 0, d, d, None)
    nv.call("mc_emit", d, 4, 4, 4, 0.0, d, 0, 0, None, None, None)      # an empty mesh: accepted, nothing launched
