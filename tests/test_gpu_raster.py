"""The rasteriser kernels (csrc/raster.hip) against their host restatement (tests/raster_ref.py, itself proven in tests/test_raster_cpu.py) at the smallest shapes
where each thing can go wrong.  Every comparison is an equality -- records, id image, depth bits, image, status words -- and every device buffer is exactly
sized and sits between guard bytes that must come back untouched."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import raster_cases as rc  # noqa: E402
import raster_ref as rr  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GUARD, FILL = 256, 0xA5
H2, W2, INTR2 = 64, 48, (60.0, 60.0, 24.0, 32.0)      # non-square, W no multiple of the wave


class Guarded:
    """A device buffer of exactly n bytes between two runs of guard bytes."""

    def __init__(self, data=None, nbytes=None, dtype=None):
        if data is not None:
            data = np.ascontiguousarray(data)
            nbytes, dtype = data.nbytes, {np.dtype(np.float32): torch.float32, np.dtype(np.int32): torch.int32}[data.dtype]
        self.raw = torch.full((nbytes + 2 * GUARD,), FILL, dtype=torch.uint8, device=DEV)
        self.bytes = self.raw[GUARD:GUARD + nbytes]
        self.t = self.bytes.view(dtype) if dtype is not None else self.bytes
        if data is not None and nbytes:
            self.t.copy_(torch.from_numpy(data.reshape(-1)).to(DEV))

    def intact(self):
        return bool((self.raw[:GUARD] == FILL).all()) and bool((self.raw[GUARD + self.bytes.numel():] == FILL).all())


def device_render(vertices, tris, colors, pose, intr, H, W, bg=(1.0, 1.0, 1.0), near=0.05):
    """The three entry points on guarded buffers -> raster_ref.render's dict (numpy) plus "status" (the four words) and "zbuf"."""
    from nerf_signature_amd import raster
    vertices, tris, colors = (np.asarray(a, d).reshape(-1, 3) for a, d in ((vertices, np.float32), (tris, np.int32), (colors, np.float32)))
    V, T = len(vertices), len(tris)
    gv, gt, gc = Guarded(vertices), Guarded(tris), Guarded(colors)
    gp, gb = Guarded(np.asarray(pose, np.float32).reshape(16)), Guarded(np.asarray(bg, np.float32).reshape(3))
    image, depth, winner = Guarded(nbytes=12 * H * W, dtype=torch.float32), Guarded(nbytes=4 * H * W, dtype=torch.float32), Guarded(nbytes=4 * H * W, dtype=torch.int32)
    sc = raster.RasterScratch(V, T, H, W, DEV)
    gs = Guarded(nbytes=sc.buf.numel())
    sc.buf = gs.bytes
    raster.launch(gv.t.view(V, 3), gt.t.view(T, 3), gc.t.view(V, 3), gp.t.view(4, 4), intr, H, W, gb.t, near, sc, image.t, depth.t, winner.t)
    torch.cuda.synchronize()
    assert all(g.intact() for g in (gv, gt, gc, gp, gb, image, depth, winner, gs))
    status = sc.status.tolist()
    return {"records": sc.records.cpu().numpy(), "image": image.t.view(H, W, 3).cpu().numpy(), "depth": depth.t.view(H, W).cpu().numpy(),
            "triangle": winner.t.view(H, W).cpu().numpy(), "culled": (status[1], status[2]), "bad": None if status[0] == raster.RS_OK else status[0],
            "status": status, "zbuf": sc.zbuf.cpu().numpy()}


def same(got, want):
    """Bit equality of everything the reference states."""
    assert np.array_equal(got["records"], want["records"])
    assert np.array_equal(got["triangle"], want["triangle"])
    assert np.array_equal(got["depth"].view(np.uint32), want["depth"].view(np.uint32))
    assert np.array_equal(got["image"].view(np.uint32), want["image"].view(np.uint32))
    assert got["culled"] == want["culled"] and got["bad"] == want["bad"]
    # the z-buffer is the same statement once more: all ones, or depth bits above the winner's index
    z = np.where(want["triangle"] >= 0, (want["depth"].view(np.uint32).astype(np.int64) << 32) | want["triangle"].astype(np.int64), -1)
    assert np.array_equal(got["zbuf"], z)


def n_large(ref, H, W):
    """How many triangles the header sends the large route: drawable, with more than NSIG_RASTER_SMALL_BOX pixel centres in the clamped box."""
    rec, n = ref["records"], 0
    for a, b, c in ref["tris"].tolist():
        if not all(0 <= k < len(rec) for k in (a, b, c)) or rec[[a, b, c], 3].any():
            continue
        x, y = rec[[a, b, c], 0].astype(np.int64), rec[[a, b, c], 1].astype(np.int64)
        if (x[1] - x[0]) * (y[2] - y[0]) - (y[1] - y[0]) * (x[2] - x[0]) == 0:
            continue
        i0, i1 = max(-((128 - x.min()) // 256), 0), min((x.max() - 128) // 256, W - 1)
        j0, j1 = max(-((128 - y.min()) // 256), 0), min((y.max() - 128) // 256, H - 1)
        n += i0 <= i1 and j0 <= j1 and (i1 - i0 + 1) * (j1 - j0 + 1) > 64
    return n


def reference(vertices, tris, colors, pose, intr, H, W, **kw):
    out = rr.render(vertices, tris, colors, pose, intr, H, W, **kw)
    out["tris"] = np.asarray(tris, np.int64).reshape(-1, 3)
    return out


# ---- the exact mesh ------------------------------------------------------------------------------------------------------------------------------------------

def test_exact_screen_space_mesh():
    xy, z, verts, tris, colors = rc.exact_mesh()
    want = reference(verts, tris, colors, rc.IDENTITY, rc.INTR16, 16, 16)
    got = device_render(verts, tris, colors, rc.IDENTITY, rc.INTR16, 16, 16)
    same(got, want)
    assert np.array_equal(got["records"][:, :2], xy)
    assert got["status"][3] == n_large(want, 16, 16) > 0 and (got["triangle"] == 3).any() and not (got["triangle"] == len(tris) - 1).any()
    for case in (rc.fan(), rc.strip()[:4]):
        _, _, v, t = case
        same(device_render(v, t, np.ones_like(v), rc.IDENTITY, rc.INTR16, 16, 16), reference(v, t, np.ones_like(v), rc.IDENTITY, rc.INTR16, 16, 16))
    _, _, v, t, c = rc.slanted_quad()
    same(device_render(v, t, c, rc.IDENTITY, rc.INTR16, 16, 16, bg=(0.25, 0.5, 2.0)), reference(v, t, c, rc.IDENTITY, rc.INTR16, 16, 16, bg=(0.25, 0.5, 2.0)))


# ---- a marching-cubes ball from rotated poses --------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ball():
    """Marching cubes of a ball on a 24^3 lattice (this library's own mc kernels), in world units [-1, 1]^3, with seeded vertex colours."""
    from nerf_signature_amd import mesh
    g = torch.arange(24, dtype=torch.float32, device=DEV)
    x, y, zz = torch.meshgrid(g, g, g, indexing="ij")
    u = 8.6 - torch.sqrt((x - 11.3) ** 2 + (y - 11.6) ** 2 + (zz - 11.4) ** 2)
    v, t = mesh.marching_cubes(u.contiguous(), 0.0)
    verts = (v.cpu().numpy().astype(np.float32) / np.float32(23.0) * np.float32(2.0) - np.float32(1.0)).astype(np.float32)
    tris = t.cpu().numpy().astype(np.int32)
    assert 1500 < len(tris) < 3000
    colors = np.random.RandomState(5).rand(len(verts), 3).astype(np.float32)
    return verts, tris, colors


POSES = [(1.1, 0.7, 2.5), (0.5, 2.5, 2.2), (2.2, 4.0, 3.0)]


@pytest.mark.parametrize("view", range(3))
def test_ball_from_rotated_poses(ball, view):
    from nerf_signature_amd import synthetic
    verts, tris, colors = ball
    pose = synthetic.orbit_pose(*POSES[view])
    want = reference(verts, tris, colors, pose, INTR2, H2, W2)
    got = device_render(verts, tris, colors, pose, INTR2, H2, W2)
    same(got, want)
    covered = (want["triangle"] >= 0).mean()
    assert 0.1 < covered < 0.9 and want["culled"] == (0, 0) and len(np.unique(want["triangle"])) > 300
    assert not np.array_equal(want["triangle"], want["triangle"][::-1]) and got["status"][3] == n_large(want, H2, W2)


CLOSE, NEAR, WIDE = (1.1, 0.7, 0.85), 0.12, (20.0, 20.0, 24.0, 32.0)      # a tenth of a unit above the ball's surface, through a wide lens


def test_culling_close_to_the_surface(ball):
    """A camera so close that the cap of the ball under it lies nearer than `near`: its vertices are flagged, their triangles skipped and counted, the hole sits
    where the reference puts it, and the triangles around the hole are tens of pixels wide (the large route)."""
    from nerf_signature_amd import synthetic
    verts, tris, colors = ball
    pose = synthetic.orbit_pose(*CLOSE)
    want = reference(verts, tris, colors, pose, WIDE, H2, W2, near=NEAR)
    got = device_render(verts, tris, colors, pose, WIDE, H2, W2, near=NEAR)
    same(got, want)
    assert want["culled"][0] > 10 and (want["records"][:, 3] == 1).sum() > 3 and (want["depth"] < 0.5).sum() > 500
    assert 1.4 < want["depth"][H2 // 2, W2 // 2] < 1.7                                        # the hole, straight ahead: the far side of the ball shows through it
    assert got["status"][3] == n_large(want, H2, W2) > 10
    # the guard band: the same view through a lens long enough to throw the ball's limb past 16384 pixels
    long_lens = (12000.0, 12000.0, 24.0, 32.0)
    want = reference(verts, tris, colors, pose, long_lens, H2, W2, near=NEAR)
    assert want["culled"][1] > 0 and (want["records"][:, 3] == 2).sum() > 0
    same(device_render(verts, tris, colors, pose, long_lens, H2, W2, near=NEAR), want)


# ---- the large route -------------------------------------------------------------------------------------------------------------------------------------------

def test_large_route_and_the_same_triangles_through_the_small_route():
    """Two triangles that take the large route at 16 x 16 -- one just covering the image, one with all three vertices off screen inside the guard band -- and the
    same two at 8 x 8, where the clamped box holds 64 centres and the small route draws them: the same pixels, as the image is the larger one's corner."""
    xy = np.array([[-40 * 256, -40 * 256 + 3], [300 * 256 + 77, -38 * 256], [-39 * 256, 290 * 256 + 5],
                   [-9000 * 256 + 1, -7000 * 256], [12000 * 256, -6500 * 256 + 9], [100 * 256, 15000 * 256 + 128]], np.int64)
    z = np.array([2.0, 4.0, 2.0, 1.0, 1.0, 2.0])
    verts = rc.unproject(xy, z)
    colors = np.random.RandomState(2).rand(6, 3).astype(np.float32)
    tris = np.array([[0, 1, 2], [3, 5, 4]], np.int32)
    for k in (0, 1):                                                                          # each alone, so that each one's pixels are seen
        alone = device_render(verts, tris[k:k + 1], colors, rc.IDENTITY, rc.INTR16, 16, 16)
        same(alone, reference(verts, tris[k:k + 1], colors, rc.IDENTITY, rc.INTR16, 16, 16))
        assert (alone["triangle"] == 0).all() and alone["status"][3] == 1
    big = device_render(verts, tris, colors, rc.IDENTITY, rc.INTR16, 16, 16)
    want = reference(verts, tris, colors, rc.IDENTITY, rc.INTR16, 16, 16)
    same(big, want)
    assert np.array_equal(big["records"][:, :2], xy) and (big["triangle"] >= 0).all() and big["status"][3] == 2
    small = device_render(verts, tris, colors, rc.IDENTITY, rc.INTR16, 8, 8)
    same(small, reference(verts, tris, colors, rc.IDENTITY, rc.INTR16, 8, 8))
    assert small["status"][3] == 0
    for k in ("triangle", "depth", "image"):
        assert np.array_equal(small[k], big[k][:8, :8])
    edge = device_render(verts, tris, colors, rc.IDENTITY, rc.INTR16, 5, 13)                  # 65 centres: the first size past the threshold
    same(edge, reference(verts, tris, colors, rc.IDENTITY, rc.INTR16, 5, 13))
    assert edge["status"][3] == 2 and np.array_equal(edge["image"], big["image"][:5, :13])


# ---- tail edges ------------------------------------------------------------------------------------------------------------------------------------------------

def small_triangles(T, seed, specials=True):
    """T triangles of a few pixels each under the identity pose with INTR2, three vertices apiece; with `specials` (T >= 63) a triangle fully off screen at
    index 3, one of zero area at 10, one with a guard-band vertex at 20, and out-of-range ids at 30 (negative) and T - 1 (V itself)."""
    rng = np.random.RandomState(seed)
    fx, fy, cx, cy = INTR2
    zc = rng.choice([1.0, 1.5, 2.0, 3.0], size=T)
    u, v = rng.uniform(-2, W2 + 2, size=T), rng.uniform(-2, H2 + 2, size=T)
    du, dv = rng.uniform(-2.5, 2.5, size=(T, 3)), rng.uniform(-2.5, 2.5, size=(T, 3))
    dz = rng.uniform(-0.05, 0.05, size=(T, 3))
    u[0], v[0], du[0], dv[0] = 20.3, 30.6, [-2.2, 2.4, 0.3], [-1.9, -0.4, 2.3]                  # triangle 0 is on screen and holds a few centres
    if specials:
        u[3], v[3] = -60.0, 20.0
        du[10], dv[10], dz[10] = [0.0, 0.0, 1.0], [0.0, 0.0, 1.0], 0.0                        # two corners coincide: the area is exactly zero
        du[20, 1] = 400.0 * fx
    zz = zc[:, None] + dz
    verts = np.stack([((u[:, None] + du) - cx) / fx * zz, ((v[:, None] + dv) - cy) / fy * zz, zz], axis=-1).reshape(-1, 3).astype(np.float32)
    tris = np.arange(3 * T, dtype=np.int32).reshape(T, 3)
    if specials:
        tris[30, 1] = -1
        tris[T - 1, 2] = 3 * T
    return verts, tris, rng.rand(3 * T, 3).astype(np.float32)


@pytest.mark.parametrize("T", [1, 63, 64, 65, 4097])
def test_tail_edges(T):
    verts, tris, colors = small_triangles(T, seed=T, specials=T >= 63)
    want = reference(verts, tris, colors, rc.IDENTITY, INTR2, H2, W2)
    got = device_render(verts, tris, colors, rc.IDENTITY, INTR2, H2, W2)                      # (its guards: nothing was written through an id out of range)
    same(got, want)
    if T >= 63:
        assert got["bad"] == 30 and got["status"][0] == 30 and got["culled"] == (0, 1)
        for t in (3, 10, 20, 30, T - 1):
            assert not (got["triangle"] == t).any()
        assert want["records"][3 * 20 + 1, 3] == 2 and (want["records"][:, 3] != 0).sum() == 1
    else:
        assert got["bad"] is None and (got["triangle"] == 0).sum() >= 1
    assert (got["triangle"] >= 0).sum() >= min(T, 30)


def test_a_single_triangle_with_a_bad_id_draws_nothing():
    from nerf_signature_amd import raster
    verts, tris, colors = small_triangles(1, seed=1, specials=False)
    for bad in (3, -1, -(1 << 31), (1 << 31) - 1):
        t = tris.copy()
        t[0, 0] = bad
        got = device_render(verts, t, colors, rc.IDENTITY, INTR2, H2, W2)
        same(got, reference(verts, t, colors, rc.IDENTITY, INTR2, H2, W2))
        assert got["status"] == [0, 0, 0, 0] and (got["triangle"] == -1).all() and np.isinf(got["depth"]).all() and (got["image"] == 1).all()
    d = lambda a, dt: torch.from_numpy(np.asarray(a)).to(DEV, dt)
    with pytest.raises(ValueError, match=r"render_mesh: triangle 0 has a vertex id outside \[0, 3\)"):
        raster.render_mesh(d(verts, torch.float32), d(t, torch.int32), d(colors, torch.float32), rc.IDENTITY, INTR2, H2, W2)


# ---- empty inputs ----------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("V,T", [(0, 0), (5, 0), (0, 3)])
def test_empty_inputs_give_the_background(V, T):
    rng = np.random.RandomState(V + T)
    verts, colors = rng.rand(V, 3).astype(np.float32) + np.float32([0, 0, 2]), rng.rand(V, 3).astype(np.float32)
    tris = np.zeros((T, 3), np.int32)
    got = device_render(verts, tris, colors, rc.IDENTITY, INTR2, 7, 5, bg=(0.1, 0.2, 0.3))
    same(got, reference(verts, tris, colors, rc.IDENTITY, INTR2, 7, 5, bg=(0.1, 0.2, 0.3)))
    assert (got["triangle"] == -1).all() and np.isposinf(got["depth"]).all() and np.array_equal(got["image"], np.broadcast_to(np.float32([0.1, 0.2, 0.3]), (7, 5, 3)))
    assert got["status"] == [0xFFFFFFFF, 0, 0, 0]


# ---- reproducibility -------------------------------------------------------------------------------------------------------------------------------------------

def test_two_runs_give_the_same_bits_and_a_shuffle_the_same_picture(ball):
    from nerf_signature_amd import synthetic
    verts, tris, colors = ball
    pose = synthetic.orbit_pose(*POSES[0])
    a, b = (device_render(verts, tris, colors, pose, INTR2, H2, W2) for _ in range(2))
    for k in ("records", "triangle", "depth", "image", "zbuf"):
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8))
    perm = np.random.RandomState(9).permutation(len(tris))
    c = device_render(verts, tris[perm], colors, pose, INTR2, H2, W2)
    assert np.array_equal(c["image"].view(np.uint32), a["image"].view(np.uint32)) and np.array_equal(c["depth"].view(np.uint32), a["depth"].view(np.uint32))
    covered = a["triangle"] >= 0
    assert np.array_equal(c["triangle"] >= 0, covered) and np.array_equal(perm[c["triangle"][covered]], a["triangle"][covered])


# ---- the Python layer --------------------------------------------------------------------------------------------------------------------------------------------

def test_render_mesh_returns_what_the_entry_points_wrote(ball):
    from nerf_signature_amd import raster, synthetic
    verts, tris, colors = ball
    d = lambda a, dt: torch.from_numpy(np.asarray(a)).to(DEV, dt)
    v, t, c = d(verts, torch.float32), d(tris, torch.int32), d(colors, torch.float32)
    pose = synthetic.orbit_pose(*CLOSE)
    want = device_render(verts, tris, colors, pose, WIDE, H2, W2, bg=(0.5, 0.5, 0.5), near=NEAR)
    scratch = raster.RasterScratch(len(verts), len(tris), H2, W2, DEV)
    for sc in (None, scratch, scratch):                                                       # a scratch is reusable: the second view through it sees nothing of the first
        got = raster.render_mesh(v, t, c, torch.from_numpy(pose), WIDE, H2, W2, bg_color=0.5, near=NEAR, scratch=sc)
        assert got["image"].is_cuda and got["depth"].is_cuda and got["triangle"].dtype == torch.int32 and got["image"].shape == (H2, W2, 3)
        assert got["culled"] == want["culled"] and got["culled"][0] > 0
        for k in ("image", "depth", "triangle"):
            assert np.array_equal(got[k].cpu().numpy().view(np.uint32), want[k].view(np.uint32))
    with pytest.raises(ValueError, match="the scratch was sized for another mesh, image or device"):
        raster.render_mesh(v, t, c, pose, INTR2, H2, W2 + 1, scratch=scratch)
    with pytest.raises(ValueError, match=r"render_mesh: the triangles must be int32 \[T,3\], got torch.int64 "):
        raster.render_mesh(v, t.long(), c, pose, INTR2, H2, W2)
    with pytest.raises(ValueError, match=r"render_mesh: the triangles must be a tensor on the GPU \(there is no CPU path\)"):
        raster.render_mesh(v, t.cpu(), c, pose, INTR2, H2, W2)
    with pytest.raises(ValueError, match="image of 0 x 48 pixels is out of range"):
        raster.render_mesh(v, t, c, pose, INTR2, 0, W2)
