"""The mesh rasteriser without a GPU: tests/raster_ref.py (the numpy restatement of include/nerfsig.h's "mesh rasteriser") against an exact, independent scan
conversion in fractions.Fraction, its watertightness, order independence and perspective correction, four mutants that each of those catches, every refusal and
byte-size query of the rs_* entry points word for word against the built library, and mesh.read_ply against mesh.write_ply."""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import raster_cases as rc  # noqa: E402
import raster_ref as rr  # noqa: E402


def _render(vertices, tris, colors=None, H=16, W=16, **kw):
    colors = np.zeros_like(vertices) if colors is None else colors
    return rr.render(vertices, tris, colors, rc.IDENTITY, rc.INTR16, H, W, **kw)


# ---- an independent, exact scan conversion ----------------------------------------------------------------------------------------------------------

def _cross(ux, uy, vx, vy):
    return ux * vy - uy * vx


def _lex_positive(v, gx, gy):
    """Is v + eps gx + eps^2 gy positive for every small enough eps > 0?"""
    return v > 0 or (v == 0 and (gx > 0 or (gx == 0 and gy > 0)))


def fraction_scan(xy, z, tris, H, W):
    """Per pixel the (exact depth, index) minimum over the triangles that contain the pixel centre nudged by (eps, eps^2): barycentric coordinates by Cramer's rule
    in exact rationals, whatever the winding; a centre exactly on an edge or a vertex thereby belongs to whichever triangle lies just right of it and, on a
    horizontal edge, just below.  Nothing here is shared with raster_ref: no edge functions, no swap, no fill-rule table, no floating point."""
    ids = np.full((H, W), -1, np.int64)
    depth = {}
    for j in range(H):
        for i in range(W):
            px, py = Fraction(256 * i + 128), Fraction(256 * j + 128)
            best = None
            for t, (a, b, c) in enumerate(np.asarray(tris).tolist()):
                ax, ay = (Fraction(int(v)) for v in xy[a])
                e1x, e1y = int(xy[b][0]) - ax, int(xy[b][1]) - ay
                e2x, e2y = int(xy[c][0]) - ax, int(xy[c][1]) - ay
                det = _cross(e1x, e1y, e2x, e2y)
                if det == 0:
                    continue
                l1, l2 = _cross(px - ax, py - ay, e2x, e2y) / det, _cross(e1x, e1y, px - ax, py - ay) / det
                g1, g2 = (e2y / det, -e2x / det), (-e1y / det, e1x / det)
                lam = (1 - l1 - l2, l1, l2)
                grad = ((-g1[0] - g2[0], -g1[1] - g2[1]), g1, g2)
                if all(_lex_positive(lam[k], *grad[k]) for k in range(3)):
                    q = sum(lam[k] / Fraction(z[v]) for k, v in enumerate((a, b, c)))
                    cand = (1 / q, t)
                    best = cand if best is None or cand < best else best
            if best is not None:
                ids[j, i] = best[1]
                depth[(j, i)] = best[0]
    return ids, depth


def _within_one_ulp(got, exact):
    """got (float32) against an exact rational: float64 arithmetic in a handful of operations is within 2^-50 of exact, so its float32 rounding is the exact value's
    rounding or, when that sits within 2^-50 of a rounding boundary, the neighbour."""
    want = np.float32(float(exact))
    return got == want or got == np.nextafter(want, np.float32(np.inf)) or got == np.nextafter(want, np.float32(-np.inf))


def test_projection_reproduces_the_screen_mesh_exactly():
    xy, z, verts, tris, colors = rc.exact_mesh()
    rec = rr.project(verts, rc.IDENTITY, rc.INTR16, 0.05)
    assert np.array_equal(rec[:, :2], xy) and (rec[:, 3] == 0).all()
    assert np.array_equal(rec[:, 2].copy().view(np.float32), (1.0 / z).astype(np.float32))


def test_reference_agrees_with_the_exact_scan_conversion_on_every_pixel():
    xy, z, verts, tris, colors = rc.exact_mesh()
    assert len(tris) == 21
    got = _render(verts, tris, colors)
    ids, depth = fraction_scan(xy, z, tris, 16, 16)
    assert np.array_equal(got["triangle"], ids)                                   # no pixel left out: the background too
    covered = ids >= 0
    assert 60 < covered.sum() < 256 and len(np.unique(ids[covered])) >= 8 and (got["coverage"].max() >= 3)
    assert np.isinf(got["depth"][~covered]).all() and (got["image"][~covered] == 1).all()
    for (j, i), d in depth.items():
        assert _within_one_ulp(got["depth"][j, i], d), (j, i)
    # the triangle with corners on pixel centres owns its top-left corner and neither of the other two (seen through whatever lies in front: by coverage)
    alone = _render(verts, tris[:1])["triangle"]
    assert alone[1, 2] == 0 and alone[1, 12] == -1 and alone[11, 2] == -1 and alone[1, 11] == 0 and alone[10, 2] == 0
    assert np.array_equal(alone, fraction_scan(xy, z, tris[:1], 16, 16)[0])


# ---- watertightness --------------------------------------------------------------------------------------------------------------------------------------

def test_fan_and_strip_cover_every_centre_exactly_once():
    xy, z, verts, tris = rc.fan()
    got = _render(verts, tris)
    assert np.array_equal(got["records"][:, :2], xy)
    assert (got["coverage"] == 1).all()                                                       # counted without the depth test
    assert got["coverage"][8, 8] == 1 and len(np.unique(got["triangle"])) == 8                # the hub is a pixel centre
    assert np.array_equal(got["triangle"], fraction_scan(xy, z, tris, 16, 16)[0])
    xy, z, verts, tris, want = rc.strip()
    got = _render(verts, tris)
    assert np.array_equal(got["coverage"], want) and np.array_equal(got["triangle"] >= 0, want == 1)
    assert np.array_equal(got["triangle"], fraction_scan(xy, z, tris, 16, 16)[0])
    # both windings are drawn: the strip with every triangle turned over covers the same centres
    assert np.array_equal(_render(verts, tris[:, ::-1].copy())["coverage"], want)


# ---- order independence --------------------------------------------------------------------------------------------------------------------------------

def test_permuting_the_triangles_permutes_the_ids_and_nothing_else():
    xy, z, verts, tris, colors = rc.exact_mesh()
    base = _render(verts, tris[:-1], colors)                                                  # (without the repeated triangle: its two copies tie everywhere)
    perm = np.random.RandomState(3).permutation(len(tris) - 1)
    got = _render(verts, tris[:-1][perm], colors)
    assert np.array_equal(got["image"], base["image"]) and np.array_equal(got["depth"], base["depth"])
    covered = base["triangle"] >= 0
    assert np.array_equal(got["triangle"] >= 0, covered) and np.array_equal(perm[got["triangle"][covered]], base["triangle"][covered])
    assert not np.array_equal(got["triangle"], base["triangle"])


def test_a_repeated_triangle_loses_to_its_lower_index():
    xy, z, verts, tris, colors = rc.exact_mesh()
    base, dup = _render(verts, tris[:-1], colors), _render(verts, tris, colors)
    assert (base["triangle"] == 3).sum() > 0
    assert np.array_equal(dup["triangle"], base["triangle"]) and np.array_equal(dup["depth"], base["depth"]) and np.array_equal(dup["image"], base["image"])
    assert dup["coverage"].sum() == base["coverage"].sum() + _render(verts, tris[3:4])["coverage"].sum()


# ---- perspective ---------------------------------------------------------------------------------------------------------------------------------------------

def test_colours_are_perspective_correct():
    xy, z, verts, tris, colors = rc.slanted_quad()
    got = _render(verts, tris, colors)
    c = got["image"][8, 8]
    exact = (Fraction(1, 2) * Fraction(1, 4)) / (Fraction(1, 2) + Fraction(1, 2) * Fraction(1, 4))
    assert exact == Fraction(1, 5)
    assert all(_within_one_ulp(v, exact) for v in c)
    assert abs(float(c[0]) - 0.5) > 0.25 > float(np.spacing(np.float32(0.5)))                # far from the screen-affine value
    assert _within_one_ulp(got["depth"][8, 8], 1 / (Fraction(1, 2) + Fraction(1, 8)))
    assert all(_within_one_ulp(v, Fraction(1, 2)) for v in _render(verts, tris, colors, affine=True)["image"][8, 8])


# ---- the snap ------------------------------------------------------------------------------------------------------------------------------------------------

def test_snap_rounds_half_to_even():
    # u * 256 = 640.5, 641.5, -2.5, 640.75 at depth 1 under the identity pose: the fixed-point grid is 1/256 pixel, these lie between its points
    u = np.array([640.5, 641.5, -2.5, 640.75]) / 256.0
    verts = np.stack([(u - 8) / 16, np.zeros(4), np.ones(4)], axis=1).astype(np.float32)
    rec = rr.project(verts, rc.IDENTITY, rc.INTR16, 0.05)
    assert rec[:, 0].tolist() == [640, 642, -2, 641] and (rec[:, 1] == 2048).all()


def test_projection_flags():
    verts = np.array([[0, 0, 1], [0, 0, 0.05], [0, 0, 0.04], [0, 0, -1], [np.nan, 0, 1], [0, 0, np.nan], [1023.5, 0, 1], [1024.5, 0, 1], [0, -1025, 1], [3e38, 0, 0.06]], np.float32)
    rec = rr.project(verts, rc.IDENTITY, rc.INTR16, 0.05)
    # a NaN anywhere in the position reaches Zc (0 * NaN); 16 * 1023.5 + 8 = 16384 is still inside the guard band; 3e38 / 0.06 overflows
    assert rec[:, 3].tolist() == [0, 0, 1, 1, 1, 1, 0, 2, 2, 2]
    assert (rec[rec[:, 3] != 0, :3] == 0).all() and rec[6, 0] == 16384 * 256


# ---- mutants: each is caught by one of the properties above -----------------------------------------------------------------------------------------------

def test_mutants_are_caught():
    xy, z, verts, tris = rc.fan()
    assert (_render(verts, tris, fill_rule=False)["coverage"] > 1).any()                      # fill rule dropped: shared spokes are drawn twice
    xy, z, verts, tris, colors = rc.exact_mesh()
    assert (_render(verts, tris, colors, tie="high")["triangle"] == len(tris) - 1).any()      # tie-break reversed: the repeated triangle wins
    xy, z, verts, tris, colors = rc.slanted_quad()
    assert not _within_one_ulp(_render(verts, tris, colors, affine=True)["image"][8, 8, 0], Fraction(1, 5))
    u = np.array([640.5, 641.5, -2.5, 640.75]) / 256.0
    verts = np.stack([(u - 8) / 16, np.zeros(4), np.ones(4)], axis=1).astype(np.float32)
    assert rr.project(verts, rc.IDENTITY, rc.INTR16, 0.05, snap="trunc")[:, 0].tolist() != [640, 642, -2, 641]


# ---- refusals and byte sizes of the built library -----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def native():
    from nerf_signature_amd import build, _native
    build.build()
    return _native


def _refused(native, text, name, *args):
    with pytest.raises(ValueError) as e:
        native.call(name, *args)
    assert str(e.value) == f"{name} failed (code 1): {name}: {text}"


def test_scratch_bytes(native):
    """include/nerfsig.h: 256 status bytes, then 16 V, 8 H W and 4 T bytes, each rounded up to a multiple of 256; 0 = out of range."""
    q = native.fn("rs_scratch_bytes")
    a = lambda n: (n + 255) // 256 * 256
    for V, T, H, W in ((0, 0, 1, 1), (1, 1, 1, 1), (16, 64, 16, 16), (17, 65, 48, 64), (1000, 4097, 400, 400), ((1 << 31) - 1, (1 << 31) - 1, 4096, 4096)):
        assert q(V, T, H, W) == 256 + a(16 * V) + a(8 * H * W) + a(4 * T)
    for V, T, H, W in ((1 << 31, 1, 8, 8), (1, 1 << 31, 8, 8), (1, 1, 0, 8), (1, 1, 8, 0), (1, 1, 4097, 8), (1, 1, 8, 4097)):
        assert q(V, T, H, W) == 0
    from nerf_signature_amd import raster
    assert raster.STATUS_BYTES == 256 and raster.MAX_SIDE == 4096 and raster._align(257) == 512


def test_project_refusals(native):
    d, name = native._vp(256), "rs_project"
    ok = [d, 8, d, 16.0, 16.0, 8.0, 8.0, 0.05, 16, 16, d, None]      # vertices, V, pose, fx, fy, cx, cy, near, H, W, scratch, stream
    sub = lambda i, v: ok[:i] + [v] + ok[i + 1:]
    for i, v in ((8, 0), (8, 4097), (9, 0), (9, 4097)):
        H, W = sub(i, v)[8:10]
        _refused(native, f"image of {H} x {W} pixels is out of range (1 .. 4096 each way)", name, *sub(i, v))
    _refused(native, f"V={1 << 31}, T=0 out of range (each below 2^31)", name, *sub(1, 1 << 31))
    for i in (0, 2, 10):
        _refused(native, "null pointer", name, *sub(i, None))
    _refused(native, "scratch must be 16-byte aligned", name, *sub(10, native._vp(264)))
    for i in (3, 4, 5, 6):
        for bad in (float("inf"), float("nan")):
            _refused(native, "the intrinsics must be finite", name, *sub(i, bad))
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        _refused(native, "the near plane must be a finite number > 0", name, *sub(7, bad))


def test_raster_and_shade_refusals(native):
    d, off = native._vp(256), native._vp(264)
    ok = [d, 8, 8, 16, 16, d, None]                                   # triangles, T, V, H, W, scratch, stream
    sub = lambda i, v: ok[:i] + [v] + ok[i + 1:]
    _refused(native, "image of 0 x 16 pixels is out of range (1 .. 4096 each way)", "rs_raster", *sub(3, 0))
    _refused(native, "image of 16 x 5000 pixels is out of range (1 .. 4096 each way)", "rs_raster", *sub(4, 5000))
    _refused(native, f"V=8, T={1 << 31} out of range (each below 2^31)", "rs_raster", *sub(1, 1 << 31))
    _refused(native, f"V={(1 << 32) - 1}, T=8 out of range (each below 2^31)", "rs_raster", *sub(2, (1 << 32) - 1))
    _refused(native, "null pointer", "rs_raster", *sub(0, None))
    _refused(native, "null pointer", "rs_raster", *sub(5, None))
    _refused(native, "scratch must be 16-byte aligned", "rs_raster", *sub(5, off))
    native.call("rs_raster", None, 0, 8, 16, 16, d, None)               # no triangles: nothing to launch, no error
    native.call("rs_raster", d, 8, 0, 16, 16, d, None)                  # no vertices: the same
    ok = [d, 8, 8, d, d, 16, 16, d, d, d, d, None]                   # triangles, T, V, colors, bg, H, W, scratch, image, depth, triangle, stream
    _refused(native, "image of 4097 x 16 pixels is out of range (1 .. 4096 each way)", "rs_shade", *sub(5, 4097))
    _refused(native, "image of 16 x 0 pixels is out of range (1 .. 4096 each way)", "rs_shade", *sub(6, 0))
    _refused(native, f"V=8, T={1 << 31} out of range (each below 2^31)", "rs_shade", *sub(1, 1 << 31))
    _refused(native, f"V={1 << 31}, T=8 out of range (each below 2^31)", "rs_shade", *sub(2, 1 << 31))
    for i in (0, 3, 4, 7, 8, 9, 10):
        _refused(native, "null pointer", "rs_shade", *sub(i, None))
    _refused(native, "scratch must be 16-byte aligned", "rs_shade", *sub(7, off))


def test_python_layer_has_no_cpu_path(native):
    import torch
    from nerf_signature_amd import raster
    v, t, c = torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32), torch.zeros(3, 3)
    with pytest.raises(ValueError, match=r"render_mesh: the vertices must be a tensor on the GPU \(there is no CPU path\)"):
        raster.render_mesh(v, t, c, rc.IDENTITY, rc.INTR16, 16, 16)
    with pytest.raises(ValueError, match="RasterScratch: V=1, T=1, 0 x 8 out of range"):
        raster.RasterScratch(1, 1, 0, 8, "cpu")


# ---- PLY round trip --------------------------------------------------------------------------------------------------------------------------------------------

def test_read_ply_round_trip_and_refusals(tmp_path):
    from nerf_signature_amd import mesh
    rng = np.random.RandomState(0)
    v, t = rng.randn(7, 3), rng.randint(0, 7, size=(5, 3)).astype(np.int32)
    n, c = rng.randn(7, 3).astype(np.float32), rng.randint(0, 256, size=(7, 3)).astype(np.uint8)
    for k, (normals, colors) in enumerate(((None, None), (n, None), (None, c), (n, c))):
        path = str(tmp_path / f"m{k}.ply")
        mesh.write_ply(path, v, t, normals=normals, colors=colors)
        got = mesh.read_ply(path)
        assert np.array_equal(got["vertices"], v) and got["vertices"].dtype == np.float64 and np.array_equal(got["triangles"], t) and got["triangles"].dtype == np.int32
        assert (got["normals"] is None) == (normals is None) and (got["colors"] is None) == (colors is None)
        assert normals is None or np.array_equal(got["normals"], n)
        assert colors is None or (np.array_equal(got["colors"], c) and got["colors"].dtype == np.uint8)
    mesh.write_ply(str(tmp_path / "f.ply"), v, t, colors=rng.rand(7, 3))                      # float colours are stored as bytes
    assert np.array_equal(mesh.read_ply(str(tmp_path / "f.ply"))["colors"].shape, (7, 3))
    mesh.write_ply(str(tmp_path / "e.ply"), np.zeros((0, 3)), np.zeros((0, 3), np.int32))
    empty = mesh.read_ply(str(tmp_path / "e.ply"))
    assert empty["vertices"].shape == (0, 3) and empty["triangles"].shape == (0, 3)

    whole = open(str(tmp_path / "m3.ply"), "rb").read()

    def refused(data, text):
        p = str(tmp_path / "bad.ply")
        with open(p, "wb") as f:
            f.write(data)
        with pytest.raises(ValueError) as e:
            mesh.read_ply(p)
        assert text in str(e.value), str(e.value)

    refused(b"PLY\n" + whole[4:], "is not a PLY file")
    refused(whole.replace(b"end_header\n", b"end\n"), "is not a PLY file")
    refused(whole.replace(b"binary_little_endian", b"ascii"), "unsupported layout: 'format ascii 1.0' where write_ply has 'format binary_little_endian 1.0'")
    refused(whole.replace(b"property double x", b"property float x"), "unsupported layout: 'property float x / property double y / property double z'")
    refused(whole.replace(b"property uchar red", b"property uchar alpha\nproperty uchar red"), "'property uchar alpha' is no vertex property write_ply writes")
    refused(whole.replace(b"list uchar int vertex_indices", b"list uchar uint vertex_indices"), "'property list uchar uint vertex_indices' where write_ply has")
    refused(whole.replace(b"element face 5", b"element edge 5"), "'element edge 5' where write_ply has 'element face <count>'")
    refused(whole[:-1], "bytes after the header")
    refused(whole + b"\0", "bytes after the header")
    head = whole.index(b"end_header\n") + len(b"end_header\n")
    quad = bytearray(whole)
    quad[head + 7 * (24 + 12 + 3) + 13] = 4                                                   # the count byte of the second face
    refused(bytes(quad), "face 1 is not a triangle")
