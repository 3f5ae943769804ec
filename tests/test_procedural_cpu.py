"""tests/procedural_ref.py -- the restatement of ps_render_u8 (include/nerfsig.h, "procedural scenes") that the GPU tests compare the kernel with -- held to an
exact check in fractions.Fraction, to closed forms and to its own mutants; every refusal of the entry point through the built library; the directory round
trip of procedural.write_scene.  No GPU."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import procedural_ref as pr  # noqa: E402

from nerf_signature_amd import procedural as ps  # noqa: E402
from nerf_signature_amd.synthetic import orbit_pose  # noqa: E402

LIGHT, AMBIENT = (0.4, 1.0, 0.5), 0.25
THREE = np.array([ps.sphere((0.0, 0.1, 0.0), 0.3, (0.9, 0.35, 0.2), (0.95, 0.85, 0.3), 8.0),
                  ps.box((-0.6, -0.5, -0.6), (0.6, -0.2, 0.6), (0.85, 0.82, 0.75), (0.25, 0.3, 0.45), 5.0),
                  ps.sphere((0.36, -0.08, 0.3), 0.12, (0.2, 0.65, 0.4))], np.float32)


def look_z(distance):
    """The identity rotation at (0, 0, -distance): looking down +z, x right, y down."""
    pose = np.eye(4, dtype=np.float32)
    pose[2, 3] = -distance
    return pose


def test_exact_check_at_every_subsample():
    """16 x 16, S = 2, three primitives, two poses: hit or miss and the winner of the float64 restatement equal those of exact arithmetic on the same float32
    rays at all 2 x 1024 sub-samples; the exact side decides every one of them (no interval overlaps)."""
    H = W = 16
    intr = (18.0, 18.0, 8.0, 8.0)
    hits, seen = 0, set()
    for theta, phi in ((1.0, 0.4), (0.7, 3.9)):
        pose = orbit_pose(theta, phi, 2.2)
        u, v = pr.subsample_positions(H, W, 2)
        o, d = pr.pixel_rays(pose, intr, u, v)
        win = pr.cast(o, d, THREE)[0]
        exact = [pr.exact_winner(o, ray, THREE) for ray in d.reshape(-1, 3)]
        assert None not in exact
        assert np.array_equal(win, np.array(exact))
        hits += int((win >= 0).sum())
        seen |= set(np.unique(win).tolist())
    assert hits > 500 and seen == {-1, 0, 1, 2}          # every primitive and the background are seen


def test_sphere_seen_from_its_axis_is_a_disc():
    """A sphere of radius r at distance D on the optical axis covers the pixels within f r / sqrt(D^2 - r^2) of the principal point, to within one pixel."""
    H = W = 65
    f, r, D = 60.0, 0.4, 2.5
    prims = [ps.sphere((0, 0, 0), r, (1, 1, 1))]
    img = pr.render(look_z(D)[None], (f, f, W / 2, H / 2), H, W, prims, LIGHT, AMBIENT, S=1, C=4)[0]
    R = f * r / math.sqrt(D * D - r * r)
    jj, ii = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij")
    dist = np.hypot(ii - W / 2, jj - H / 2)
    assert (img[..., 3][dist < R - 1] == 255).all() and (img[..., 3][dist > R + 1] == 0).all()
    assert set(np.unique(img[..., 3])) == {0, 255} and abs(np.sqrt((img[..., 3] == 255).sum() / math.pi) - R) < 1


def test_box_face_on_has_the_lambert_code():
    """The -z face of a box seen along +z, light (0, 3, -4) / 5: n.L = 0.8, so every channel is rint(255 albedo (ambient + (1 - ambient) 0.8))."""
    H = W = 9
    albedo = (0.5, 0.25, 1.0)
    img = pr.render(look_z(2.0)[None], (9.0, 9.0, 4.5, 4.5), H, W, [ps.box((-0.5, -0.5, -0.5), (0.5, 0.5, 0.5), albedo)], (0.0, 3.0, -4.0), 0.25, S=1, C=4)[0]
    want = [int(np.rint(255.0 * (np.float64(np.float32(a)) * (0.25 + 0.75 * (4.0 / 5.0))))) for a in albedo]
    assert want == [108, 54, 217]
    assert img[4, 4].tolist() == want + [255] and img[0, 0].tolist() == [0, 0, 0, 0]


def test_box_special_cases():
    cube = np.array([ps.box((-1, -1, -1), (1, 1, 1), (1, 1, 1))], np.float32)
    # d_k == 0: the axis divides nothing; inside its slab (the boundary included) it does not constrain, outside it is a miss
    for ox, hit in ((0.0, True), (1.0, True), (-1.0, True), (1.0000001, False), (-1.5, False)):
        win, t, n, _ = pr.cast(np.float32([ox, 0, -3]), np.float32([[0, 0, 1]]), cube)
        assert (win[0] == 0) == hit
        if hit:
            assert t[0] == 2.0 and n[0].tolist() == [0.0, 0.0, -1.0]
    # ... and the pixel column with u == cx of an identity camera really has d_0 == 0
    u, v = pr.subsample_positions(5, 7, 1)
    o, d = pr.pixel_rays(look_z(3.0), (6.0, 6.0, 3.5, 2.5), u, v)
    assert (d[:, 3, 0, 0, 0] == 0.0).all() and (d[2, :, 0, 0, 1] == 0.0).all() and (d[:, 2, 0, 0, 0] != 0.0).all()
    # the camera inside the box: the exit face, its normal turned towards the camera
    win, t, n, _ = pr.cast(np.float32([0.25, 0, 0]), np.float32([[1, 0.5, 0.25], [-1, 0, 0], [0, 0, -2]]), cube)
    assert win.tolist() == [0, 0, 0] and t.tolist() == [0.75, 1.25, 0.5]
    assert n.tolist() == [[-1.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]
    # a ray through an edge: both axes enter at t = 1, the lower axis keeps the face
    win, t, n, _ = pr.cast(np.float32([-2, -2, 0]), np.float32([[1, 1, 0]]), cube)
    assert win[0] == 0 and t[0] == 1.0 and n[0].tolist() == [-1.0, 0.0, 0.0]
    win, t, n, _ = pr.cast(np.float32([0, -2, -2]), np.float32([[0, 1, 1]]), cube)
    assert t[0] == 1.0 and n[0].tolist() == [0.0, -1.0, 0.0]


def index_tie(mutant=None):
    """A sphere and a box met at the same t = 2: the lower index wins, whichever kind it is."""
    s, b = ps.sphere((0, 0, 2), 1.0, (1, 0, 0)), ps.box((-1, -1, 1), (1, 1, 3), (0, 1, 0))
    o, d = np.float32([0, 0, -1]), np.float32([[0, 0, 1]])
    first = pr.cast(o, d, np.array([s, b], np.float32), mutant)
    second = pr.cast(o, d, np.array([b, s], np.float32), mutant)
    return first[1][0] == 2.0 and second[1][0] == 2.0 and first[0][0] == 0 and second[0][0] == 0


def near_root(mutant=None):
    """From outside, a sphere is met at its near root; from inside (the near root behind t_min) at the far one."""
    ball = np.array([ps.sphere((0, 0, 0), 1.0, (1, 1, 1))], np.float32)
    win, t, n, _ = pr.cast(np.float32([0, 0, -3]), np.float32([[0, 0, 1]]), ball, mutant)
    inside = pr.cast(np.float32([0, 0, 0.5]), np.float32([[0, 0, 1]]), ball, mutant)
    return win[0] == 0 and t[0] == 2.0 and n[0].tolist() == [0.0, 0.0, -1.0] and inside[1][0] == 0.5 and inside[2][0].tolist() == [0.0, 0.0, 1.0]


def straight_alpha(mutant=None):
    """S = 2, two of four sub-samples hit: alpha is rint(127.5) = 128 and the colour is the mean of the two HIT colours, not of four."""
    colour = np.zeros((1, 1, 2, 2, 3))
    hit = np.zeros((1, 1, 2, 2), bool)
    colour[0, 0, 0, 1], colour[0, 0, 1, 1] = (0.25, 0.5, 1.0), (0.75, 0.5, 0.0)
    hit[0, 0, 0, 1] = hit[0, 0, 1, 1] = True
    rgba = pr.resolve(colour, hit, 2, 4, (1, 1, 1), mutant)[0, 0].tolist()
    rgb = pr.resolve(colour, hit, 2, 3, (1.0, 0.0, 0.5), mutant)[0, 0].tolist()
    return rgba == [128, 128, 128, 128] and rgb == [int(np.rint(255 * (0.5 * 0.5 + b * 0.5))) for b in (1.0, 0.0, 0.5)]


def checker_floor(mutant=None):
    """The top of a slab at p = (0.7, 0, 0.2), f = 1: floor gives cells (0, 0, 0), even, colour A; rounded coordinates (1, 0, 0) would give colour B.  And at
    p = (-0.3, 0, 0.2) floor gives (-1, 0, 0): odd, colour B."""
    slab = np.array([ps.box((-2, -1, -2), (2, 0, 2), (1, 1, 1), (0, 0, 0), 1.0)], np.float32)
    d = np.float32([[0, -1, 0]])
    out = []
    for x in (0.7, -0.3):
        o = np.float32([x, 1, 0.2])
        win, t, n, _ = pr.cast(o, d, slab, mutant)
        out.append(pr.shade(o, d, slab, (0, 1, 0), 0.0, win, t, n, mutant)[0].tolist())
    return out == [[1.0, 1.0, 1.0], [0.0, 0.0, 0.0]]


CHECKS = {"wrong_root": near_root, "tie_high": index_tie, "premultiplied": straight_alpha, "checker_round": checker_floor}


def test_every_rule_holds_and_every_mutant_is_caught():
    assert set(CHECKS) == set(pr.MUTANTS) and len(pr.MUTANTS) >= 4
    for name, check in CHECKS.items():
        assert check(None), name
        assert not check(name), f"the mutant '{name}' passes its rule's check"
    # each mutant also changes the picture of a scene that has all four features in view
    pose = orbit_pose(1.0, 0.4, 2.2)[None]
    prims = np.concatenate([THREE, np.array([ps.box((-0.6, -0.5, -0.6), (0.6, -0.2, 0.6), (0, 0, 1)), ps.sphere((0, 0.1, 0), 0.1, (1, 1, 1))], np.float32)])
    args = (pose, (40.0, 40.0, 16.0, 16.0), 32, 32, prims, LIGHT, AMBIENT)
    base = pr.render(*args, S=2, C=4)
    for name in pr.MUTANTS:
        assert not np.array_equal(pr.render(*args, S=2, C=4, mutant=name), base), name


def test_rounding_is_half_to_even():
    """Codes at exact halves: 0.5 -> 0, 1.5 -> 2, 2.5 -> 2 (rounding half up gives 1, 2, 3), and alpha 2 / 4 -> rint(127.5) = 128."""
    for half, code in ((0.5, 0), (1.5, 2), (2.5, 2), (126.5, 126)):
        c = next(x for x in (half / 255.0, np.nextafter(half / 255.0, 0), np.nextafter(half / 255.0, 1)) if 255.0 * x == half)      # a double whose product IS the half
        colour, hit = np.full((1, 1, 1, 1, 3), c), np.ones((1, 1, 1, 1), bool)
        assert pr.resolve(colour, hit, 1, 4, (1, 1, 1))[0, 0].tolist() == [code] * 3 + [255]
    # out-of-range colours are clamped, not wrapped
    colour = np.array([1.7, -0.2, 1.0]).reshape(1, 1, 1, 1, 3)
    assert pr.resolve(colour, np.ones((1, 1, 1, 1), bool), 1, 4, (1, 1, 1))[0, 0].tolist() == [255, 0, 255, 255]


def test_straight_alpha_on_an_edge_pixel_of_a_render():
    """A flat sphere under full ambient light has ONE colour: at S = 2 its partly covered edge pixels keep that colour's code and carry the coverage in alpha;
    against a background (C = 3) the same pixels are the blend."""
    H = W = 24
    prims, intr = [ps.sphere((0, 0, 0), 0.5, (0.8, 0.4, 0.2))], (20.0, 20.0, 12.0, 12.0)
    rgba = pr.render(look_z(2.0)[None], intr, H, W, prims, LIGHT, 1.0, S=2, C=4)[0]
    edge = (rgba[..., 3] > 0) & (rgba[..., 3] < 255)
    assert edge.sum() >= 8 and set(np.unique(rgba[..., 3])) <= {0, 64, 128, 191, 255}
    assert (rgba[rgba[..., 3] > 0][:, :3] == np.array([204, 102, 51])).all()
    rgb = pr.render(look_z(2.0)[None], intr, H, W, prims, LIGHT, 1.0, S=2, C=3, bg=(0.0, 0.0, 1.0))[0]
    j, i = np.argwhere(rgba[..., 3] == 128)[0]
    col = np.float32([0.8, 0.4, 0.2]).astype(np.float64)
    assert rgb[j, i].tolist() == [int(np.rint(255 * (c * 0.5 + b * 0.5))) for c, b in zip(col, (0.0, 0.0, 1.0))]
    assert rgb[0, 0].tolist() == [0, 0, 255]


def test_plinth_is_inside_bound_one_and_textured():
    scene = ps.SCENES["plinth"]
    assert scene.prims.shape == (4, 16) and scene.prims.dtype == np.float32
    for q in scene.prims:
        lo, hi = (q[4:7] - q[7], q[4:7] + q[7]) if q[0] == ps.SPHERE else (q[4:7], q[7:10])
        assert (lo >= -1).all() and (hi <= 1).all()
    assert sorted(scene.prims[:, 0].tolist()) == [0, 0, 1, 1] and scene.prims[0, 1] == ps.CHECKER
    assert scene.prims[1, 5] - scene.prims[1, 7] == pytest.approx(scene.prims[0, 8])          # the sphere rests on the slab
    poses = np.stack([orbit_pose(1.0, 0.7, 2.2), orbit_pose(0.8, 3.8, 2.2)])
    img, win = pr.render(poses, (58.0, 58.0, 24.0, 24.0), 48, 48, scene.prims, scene.light, scene.ambient, S=1, C=4, details=True)
    assert set(np.unique(win).tolist()) == {-1, 0, 1, 2, 3}
    assert len(np.unique(img[0].reshape(-1, 4), axis=0)) > 100


def test_scene_validation():
    with pytest.raises(ValueError, match="at most 16"):
        ps.ProceduralScene([ps.sphere((0, 0, 0), 0.1, (1, 1, 1))] * 17)
    with pytest.raises(ValueError, match="radius 0 is not > 0"):
        ps.ProceduralScene([ps.sphere((0, 0, 0), 0.0, (1, 1, 1))])
    with pytest.raises(ValueError, match="box lo > hi"):
        ps.ProceduralScene([ps.box((0, 0, 0), (1, -1, 1), (1, 1, 1))])
    with pytest.raises(ValueError, match="must be finite"):
        ps.ProceduralScene([ps.box((0, 0, 0), (1, math.inf, 1), (1, 1, 1))])
    with pytest.raises(ValueError, match="kind 2"):
        ps.ProceduralScene([[2.0] + [0.0] * 15])
    with pytest.raises(ValueError, match="light"):
        ps.ProceduralScene([], light=(0, 0, 0))
    with pytest.raises(ValueError, match="ambient"):
        ps.ProceduralScene([], ambient=1.5)
    assert ps.ProceduralScene([]).prims.shape == (0, 16)
    with pytest.raises(ValueError, match="on the GPU"):
        ps.render(ps.SCENES["plinth"], torch.eye(4)[None], (10, 10, 4, 4), 8, 8)


def test_every_refusal_word_for_word():
    """ps_render_u8 checks everything before it launches: each refusal by its whole message, through the built library, with addresses that are never used."""
    from nerf_signature_amd import _native as nv, build
    build.build()
    d = nv._vp(256)
    ball, cube = ps.sphere((0, 0, 0), 0.5, (1, 1, 1)), ps.box((0, 0, 0), (1, 1, 1), (1, 1, 1))

    def refused(message, **kw):
        a = dict(poses=d, P=1, intr=(10.0, 10.0, 4.0, 4.0), H=8, W=8, prims=[ball, cube], K=None, light=(0.0, 1.0, 0.0), ambient=0.25, S=2, C=4, bg=(1.0, 1.0, 1.0), image=d)
        a.update(kw)
        table = np.ascontiguousarray(np.asarray(a["prims"], np.float32).reshape(-1, 16))
        K = len(table) if a["K"] is None else a["K"]
        host = table.ctypes.data_as(nv._vp) if a["prims"] is not None and len(table) else None
        with pytest.raises(ValueError) as e:
            nv.call("ps_render_u8", a["poses"], a["P"], *a["intr"], a["H"], a["W"], host, K, *a["light"], a["ambient"], a["S"], a["C"], *a["bg"], a["image"], None)
        assert str(e.value) == f"ps_render_u8 failed (code 1): ps_render_u8: {message}"

    def changed(row, word, value):
        row = list(row)
        row[word] = value
        return row

    refused("image of 0 x 8 pixels is out of range (1 .. 4096 each way)", H=0)
    refused("image of 8 x 4097 pixels is out of range (1 .. 4096 each way)", W=4097)
    refused("P=0 views of 8 x 8 pixels out of range (P >= 1, P H W < 2^32)", P=0)
    refused("P=256 views of 4096 x 4096 pixels out of range (P >= 1, P H W < 2^32)", P=256, H=4096, W=4096)
    refused("K=17 primitives out of range (0 .. 16)", prims=[ball] * 17)
    for s in (0, 3, 8):
        refused(f"samples={s} is not 1, 2 or 4", S=s)
    for c in (1, 2, 5):
        refused(f"channels={c} is not 3 or 4", C=c)
    refused("null pointer", poses=None)
    refused("null pointer", image=None)
    refused("null pointer", prims=[], K=2)
    refused("the intrinsics must be finite and the focal lengths non-zero", intr=(0.0, 10.0, 4.0, 4.0))
    refused("the intrinsics must be finite and the focal lengths non-zero", intr=(10.0, 10.0, math.nan, 4.0))
    refused("the intrinsics must be finite and the focal lengths non-zero", intr=(10.0, math.inf, 4.0, 4.0))
    refused("the light must be a finite vector other than zero", light=(0.0, 0.0, 0.0))
    refused("the light must be a finite vector other than zero", light=(0.0, math.inf, 0.0))
    refused("ambient=-0.5 outside [0, 1]", ambient=-0.5)
    refused("ambient=1.5 outside [0, 1]", ambient=1.5)
    refused("ambient=nan outside [0, 1]", ambient=math.nan)
    refused("the background must be finite", bg=(1.0, math.nan, 1.0))
    refused("primitive 1: word 3 is not finite", prims=[ball, changed(cube, 3, math.inf)])
    refused("primitive 0: word 15 is not finite", prims=[changed(ball, 15, math.nan)])
    refused("primitive 0: kind 2 is neither 0 (sphere) nor 1 (box)", prims=[changed(ball, 0, 2.0)])
    refused("primitive 1: texture 0.5 is neither 0 (flat) nor 1 (checker)", prims=[ball, changed(cube, 1, 0.5)])
    refused("primitive 0: radius 0 is not > 0", prims=[changed(ball, 7, 0.0)])
    refused("primitive 1: radius -1 is not > 0", prims=[ball, changed(ball, 7, -1.0)])
    refused("primitive 1: box lo > hi on axis 2", prims=[ball, changed(cube, 6, 1.5)])
    assert nv.SIGNATURES["ps_render_u8"] == [nv._vp, nv._u32] + [nv._fl] * 4 + [nv._u32] * 2 + [nv._vp, nv._u32] + [nv._fl] * 4 + [nv._u32] * 2 + [nv._fl] * 3 + [nv._vp, nv._vp]
    assert ctypes.sizeof(ctypes.c_float) * 16 * ps.MAX_PRIMS == 1024


@pytest.mark.parametrize("channels", [3, 4])
def test_write_scene_load_scene_round_trip(tmp_path, channels):
    """What write_scene wrote, load_scene(scale=1, offset=0) reads back: the same bytes, the same poses, the same intrinsics, H, W and radius."""
    from nerf_signature_amd import dataset as ds
    H, W, P = 10, 12, 3
    intr = (17.25, 17.25, W / 2, H / 2)
    poses = ps.orbit_poses(P, 2.2, (0.6, 1.5), seed=5)
    images = pr.render(poses, intr, H, W, ps.SCENES["plinth"].prims, LIGHT, AMBIENT, S=2, C=channels)
    assert 0 < images[..., :3].min() + 1 and len(np.unique(images)) > 20
    centres = torch.from_numpy(poses)[:, :3, 3].double()
    radius = sum(float(v) for v in (centres * centres).sum(-1).sqrt()) / P
    store = ds.Scene(torch.from_numpy(poses), torch.from_numpy(images), intr, H, W, radius, "procedural", [])
    for split in ("train", "test"):
        path = ps.write_scene(store, str(tmp_path), split)
        assert os.path.basename(path) == f"transforms_{split}.json"
    back = ds.load_scene(str(tmp_path), "train", scale=1, offset=(0, 0, 0), device="cpu")
    assert back.mode == "blender" and len(back.files) == P and (back.H, back.W) == (H, W)
    assert back.images.dtype == torch.uint8 and torch.equal(back.images, store.images)
    assert torch.equal(back.poses, store.poses)
    assert back.intrinsics == intr and back.radius == radius
    import json
    t = json.load(open(os.path.join(str(tmp_path), "transforms_train.json")))
    assert W / (2 * math.tan(t["camera_angle_x"] / 2)) == pytest.approx(intr[0], rel=1e-12)
    for p in range(P):          # the inverse mapping is exact
        assert np.array_equal(ds.ngp_pose(ps.file_matrix(poses[p]), 1, (0, 0, 0)), poses[p])
