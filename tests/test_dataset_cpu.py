"""The u8 image store and the scene loader without a GPU: the shared case list reaches the pixels and byte phases the GPU suite relies on; the decode is an IEEE
division, not a multiplication; load_scene(device="cpu") against its numpy restatement (tests/dataset_ref.py) on scene directories written into tmp_path; every
refusal word for word; the two u8 entry points are declared, exported and check their arguments."""
import json
import os
import re

import numpy as np
import pytest
import torch

import dataset_ref as dr
import orbit_ref
import store_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rg_sample_rays_u8", "rg_sample_rays_weighted_u8")


# ---- the case list
def test_case_list_is_the_documented_one():
    assert (sc.SEED, sc.STEPS, sc.STRIDE, sc.OFFSET) == (7, (0, 1, 2), 1, 0)
    assert sc.CASES == ((1, 1, 1, 1), (3, 3, 3, 65), (3, 5, 7, 130))
    assert sc.WEIGHTED == {2: (1, 4), 4: (1, 7, 16)}


def test_draws_reach_the_first_and_last_pixel_of_every_pose_and_every_byte_phase():
    """A condition of tests/test_gpu_store_u8.py, not a hope: over steps 0, 1, 2 (stride 1: pose = step mod P, each pose once) the uniform draws of the two larger
    cases hit pixel 0 and pixel H*W - 1 of every pose -- so the first and the last byte of the store -- and all four values of 3 * ind mod 4; the three image bases
    of the 5 x 7 case sit at byte phases 0, 1, 2."""
    for P, H, W, N in sc.CASES[1:]:
        assert P == len(sc.STEPS)
        for step in sc.STEPS:
            inds = orbit_ref.pixel_indices(sc.SEED, step, N, H, W)
            assert inds.min() == 0 and inds.max() == H * W - 1, (H, W, step)
            assert set((3 * inds % 4).tolist()) == {0, 1, 2, 3}, (H, W, step)
    P, H, W, _ = sc.CASES[2]
    assert H * W * 3 == 105 and [(p * H * W * 3) % 4 for p in range(P)] == [0, 1, 2]
    P, H, W, N = sc.ALL_CODES
    assert set(orbit_ref.pixel_indices(sc.SEED, 0, N, H, W).tolist()) == set(range(H * W))


def test_stores_hold_every_code():
    for C in (3, 4):
        P, H, W, _ = sc.CASES[2]
        s = sc.store(P, H, W, C)
        assert s.dtype == np.uint8 and s.shape == (P, H * W, C) and set(s.reshape(-1).tolist()) == set(range(256))
        a = sc.every_code_store(C)
        assert a.shape == (1, 256, C)
        for c in range(C):
            assert sorted(a[0, :, c].tolist()) == list(range(256))
        assert np.array_equal(sc.store(P, H, W, C), s)
    # the smaller stores: as many distinct codes as they have bytes
    assert len(set(sc.store(3, 3, 3, 3).reshape(-1).tolist())) == 81 and sc.store(1, 1, 1, 4).shape == (1, 1, 4)


def test_decode_is_the_ieee_division():
    """np.uint8 -> float32 / 255 (nerf/provider.py:221) equals torch's uint8.float() / 255 for all 256 codes; q * (1/255) does not -- 126 codes differ, which is why the
    stores hold every code."""
    q = np.arange(256, dtype=np.uint8)
    want = q.astype(np.float32) / 255
    assert want.dtype == np.float32
    assert np.array_equal(want, (torch.from_numpy(q).float() / 255).numpy())
    assert np.array_equal(want, (torch.arange(256) / 255).numpy())
    mutant = q.astype(np.float32) * np.float32(1.0 / 255.0)
    assert int((mutant != want).sum()) == 126
    assert want[0] == 0.0 and want[255] == 1.0


# ---- the loader
def _same(scene, want):
    assert scene.mode == want["mode"] and (scene.H, scene.W) == (want["H"], want["W"])
    assert scene.poses.dtype == torch.float32 and np.array_equal(scene.poses.numpy(), want["poses"])
    assert scene.images.dtype == torch.uint8 and np.array_equal(scene.images.numpy(), want["images"])
    assert scene.intrinsics == tuple(float(v) for v in want["intrinsics"]) and all(type(v) is float for v in scene.intrinsics)
    assert scene.radius == want["radius"]
    assert scene.files == want["files"]


@pytest.mark.parametrize("C", [3, 4])
@pytest.mark.parametrize("mode", ["colmap", "blender"])
def test_loader_equals_the_restatement(tmp_path, mode, C):
    from nerf_signature_amd.dataset import load_scene
    root = str(tmp_path / "scene")
    written = dr.write_scene(root, mode, C=C, suffix=False)
    splits = {"colmap": {"train": [1, 2], "val": [0], "trainval": [0, 1, 2], "all": [0, 1, 2]},
              "blender": {"train": [0, 1, 2], "val": [3, 4, 5], "test": [6, 7, 8], "trainval": [0, 1, 2, 3, 4, 5], "all": [6, 7, 8, 0, 1, 2, 3, 4, 5]}}[mode]
    for split, numbers in splits.items():
        s = load_scene(root, split=split, device="cpu")
        _same(s, dr.expected(root, split=split))
        assert (s.H, s.W) == (5, 7) and tuple(s.images.shape) == (len(numbers), 5, 7, C)
        for i, k in enumerate(numbers):      # the files themselves, in the split's order (all: the json files in sorted order -- test, train, val)
            assert np.array_equal(s.images[i].numpy(), written[k]), (split, k)
            assert s.files[i] == os.path.join(root, f"images/r_{k}.png")
    # poses: the row permutation, the signs, scale and offset -- against the formula written out on frame 0 of the file
    frame = json.load(open(os.path.join(root, "transforms.json" if mode == "colmap" else "transforms_train.json")))["frames"][0]
    m = np.array(frame["transform_matrix"], dtype=np.float32)
    s = load_scene(root, split="all", scale=0.8, offset=(0.5, -0.25, 2.0), device="cpu")
    _same(s, dr.expected(root, split="all", scale=0.8, offset=(0.5, -0.25, 2.0)))
    got = s.poses[s.files.index(os.path.join(root, "images/r_0.png"))].numpy()
    for row, src, off in ((0, 1, 0.5), (1, 2, -0.25), (2, 0, 2.0)):
        assert got[row, 0] == m[src, 0] and got[row, 1] == -m[src, 1] and got[row, 2] == -m[src, 2]
        assert got[row, 3] == np.float32(float(m[src, 3]) * 0.8 + off)
    assert got[3].tolist() == [0, 0, 0, 1]
    assert s.radius == pytest.approx(float(np.linalg.norm(s.poses[:, :3, 3].numpy().astype(np.float64), axis=-1).mean()), rel=1e-6)


def test_intrinsics_by_every_focal_route(tmp_path):
    from nerf_signature_amd.dataset import load_scene
    h, w = 10, 14
    tan = lambda a: float(np.tan(a / 2))
    # focal keys -> (fl_x, fl_y) as functions of the downscale f and the downscaled size: fl_* are divided by f, an angle is taken on H / W (one stands in for the other)
    routes = (({"fl_x": 21.5, "fl_y": 19.25}, lambda f, H, W: (21.5 / f, 19.25 / f)), ({"fl_x": 21.5}, lambda f, H, W: (21.5 / f, 21.5 / f)),
              ({"fl_y": 19.25}, lambda f, H, W: (19.25 / f, 19.25 / f)),
              ({"camera_angle_x": 0.8}, lambda f, H, W: (W / (2 * tan(0.8)), W / (2 * tan(0.8)))), ({"camera_angle_y": 0.6}, lambda f, H, W: (H / (2 * tan(0.6)), H / (2 * tan(0.6)))),
              ({"camera_angle_x": 0.8, "camera_angle_y": 0.6}, lambda f, H, W: (W / (2 * tan(0.8)), H / (2 * tan(0.6)))))
    for n, (focal, want) in enumerate(routes):
        for centre in (False, True):
            root = str(tmp_path / f"s{n}{int(centre)}")
            dr.write_scene(root, "colmap", h=h, w=w, focal=focal, centre=centre)
            for f in (1, 2):
                s = load_scene(root, split="all", downscale=f, device="cpu")
                _same(s, dr.expected(root, split="all", downscale=f))
                H, W = h // f, w // f
                assert s.intrinsics[:2] == want(f, H, W), (focal, f)
                assert s.intrinsics[2:] == (((w / 2 + 0.25) / f, (h / 2 - 0.5) / f) if centre else (W / 2, H / 2))
    root = str(tmp_path / "nofocal")
    dr.write_scene(root, "colmap", focal={})
    with pytest.raises(RuntimeError, match=re.escape("Failed to load focal length, please check the transforms.json!")):
        load_scene(root, device="cpu")


@pytest.mark.parametrize("C", [3, 4])
def test_downscale_is_the_exact_integer_box_mean(tmp_path, C):
    from nerf_signature_amd.dataset import box_downscale, load_scene
    root = str(tmp_path / "scene")
    written = dr.write_scene(root, "blender", C=C, h=10, w=14)
    for size_keys in (True, False):
        if not size_keys:       # the size from the first image
            root = str(tmp_path / "nosize")
            written = dr.write_scene(root, "blender", C=C, h=10, w=14, size_keys=False)
        full, half = load_scene(root, device="cpu"), load_scene(root, downscale=2, device="cpu")
        _same(full, dr.expected(root))
        _same(half, dr.expected(root, downscale=2))
        assert (full.H, full.W, half.H, half.W) == (10, 14, 5, 7)
        ties = 0
        for i in range(3):
            img = written[i].astype(np.int64)
            s = img[0::2, 0::2] + img[0::2, 1::2] + img[1::2, 0::2] + img[1::2, 1::2]
            assert np.array_equal(half.images[i].numpy(), (s + 2) // 4)
            ties += int((s % 4 == 2).sum())
        assert ties > 0         # exact ties round up
    img = np.full((6, 3, 3), 255, dtype=np.uint8)
    assert np.array_equal(box_downscale(img, 3), np.full((2, 1, 3), 255, dtype=np.uint8)) and box_downscale(img, 1) is img


def test_missing_files_are_skipped_and_the_suffix_rule_is_blenders(tmp_path):
    from nerf_signature_amd.dataset import load_scene
    root = str(tmp_path / "fox")
    written = dr.write_scene(root, "colmap", missing=(1,))
    s = load_scene(root, split="all", device="cpu")
    _same(s, dr.expected(root, split="all"))
    assert s.files == [os.path.join(root, "images/r_0.png"), os.path.join(root, "images/r_2.png")] and np.array_equal(s.images[1].numpy(), written[2])
    # blender: 'images/r_0' means images/r_0.png; a name with a dot is taken as it is
    for suffix in (False, True):
        root = str(tmp_path / f"lego{int(suffix)}")
        dr.write_scene(root, "blender", suffix=suffix, missing=(2,))
        s = load_scene(root, device="cpu")
        _same(s, dr.expected(root))
        assert s.files == [os.path.join(root, f"images/r_{k}.png") for k in (0, 1)]
    # colmap has no suffix rule: the same entries name files that do not exist
    root = str(tmp_path / "nosuffix")
    dr.write_scene(root, "colmap")
    t = json.load(open(os.path.join(root, "transforms.json")))
    for f in t["frames"]:
        f["file_path"] = f["file_path"][:-4]
    json.dump(t, open(os.path.join(root, "transforms.json"), "w"))
    with pytest.raises(ValueError, match=re.escape(f"load_scene: none of the 3 frames of split 'all' under {root} has an image file")):
        load_scene(root, split="all", device="cpu")


def test_loader_refusals_word_for_word(tmp_path):
    from PIL import Image
    from nerf_signature_amd.dataset import load_scene
    empty = str(tmp_path / "empty")
    os.makedirs(empty)
    with pytest.raises(NotImplementedError, match=re.escape(f"[NeRFDataset] Cannot find transforms*.json under {empty}")):
        load_scene(empty, device="cpu")
    root = str(tmp_path / "colmap")
    dr.write_scene(root, "colmap")
    with pytest.raises(NotImplementedError, match=re.escape("load_scene: split 'test' of a colmap scene (poses interpolated between two randomly chosen frames) is not offered")):
        load_scene(root, split="test", device="cpu")
    with pytest.raises(ValueError, match=re.escape("load_scene: the splits are train, val, test, trainval and all, not 'dev'")):
        load_scene(root, split="dev", device="cpu")
    for bad in (0, -1, 1.5, "2", True):
        with pytest.raises(ValueError, match=re.escape(f"load_scene: downscale must be an integer >= 1, not {bad!r}")):
            load_scene(root, downscale=bad, device="cpu")
    # the image is 5 x 7: no multiple of 2
    with pytest.raises(ValueError, match=re.escape(f"load_scene: {root}/images/r_1.png is 5 x 7, not 4 x 6 (H x W = 2 x 3 times downscale = 2; a fractional resize is not offered)")):
        load_scene(root, downscale=2, device="cpu")
    # other PIL modes: palette, grey, 16-bit
    for mode, make in (("P", lambda: Image.new("P", (7, 5))), ("L", lambda: Image.new("L", (7, 5))), ("I;16", lambda: Image.fromarray(np.zeros((5, 7), dtype=np.uint16)))):
        bad = str(tmp_path / ("mode_" + mode.replace(";", "")))
        dr.write_scene(bad, "colmap")
        make().save(os.path.join(bad, "images/r_2.png"))
        got = Image.open(os.path.join(bad, "images/r_2.png")).mode
        with pytest.raises(ValueError, match=re.escape(f"load_scene: {bad}/images/r_2.png has PIL mode '{got}'; images must be 8-bit RGB or RGBA")):
            load_scene(bad, device="cpu")
    # one channel count
    mixed = str(tmp_path / "mixed")
    dr.write_scene(mixed, "colmap", C=3)
    Image.fromarray(dr.frame_image(2, 5, 7, 4), "RGBA").save(os.path.join(mixed, "images/r_2.png"))
    with pytest.raises(ValueError, match=re.escape(f"load_scene: {mixed}/images/r_2.png has 4 channels, the images before it 3")):
        load_scene(mixed, device="cpu")


def test_a_cpu_scene_has_no_sampler(tmp_path):
    """The samplers are device code: a scene loaded to the CPU is data only."""
    from nerf_signature_amd.dataset import load_scene
    root = str(tmp_path / "scene")
    dr.write_scene(root, "blender", C=4)
    s = load_scene(root, device="cpu")
    with pytest.raises(ValueError, match="poses must be on the GPU"):
        s.sampler(16)
    table = s.linear_decode()
    x = torch.arange(256) / 255
    assert table.dtype == torch.float32 and tuple(table.shape) == (256,)
    assert torch.equal(table, torch.where(x < 0.04045, x / 12.92, ((x + 0.055) / 1.055) ** 2.4))


# ---- the ABI
def test_u8_entry_points_are_declared_listed_and_exported():
    """Fails before the u8 store: the header declares neither name and the library exports neither."""
    from nerf_signature_amd import _native, build
    build.build()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nerfsig.h")).read(), flags=re.S)
    for name in SYMBOLS:
        args = re.search(r"^int\s+%s\s*\((.*?)\);" % name, header, flags=re.M | re.S).group(1)
        assert len(args.split(",")) == len(_native.SIGNATURES[name]), name
        _native.fn(name)
    # the RGBA entry points' arguments, plus channels and decode
    assert len(_native.SIGNATURES["rg_sample_rays_u8"]) == len(_native.SIGNATURES["rg_sample_rays_rgba"]) + 2
    assert len(_native.SIGNATURES["rg_sample_rays_weighted_u8"]) == len(_native.SIGNATURES["rg_sample_rays_weighted_rgba"]) + 2
    assert set(SYMBOLS) <= set(_native.verify_exports())


def test_u8_argument_checks_need_no_gpu():
    from nerf_signature_amd import _native as nv, build
    build.build()
    d, odd = nv._vp(256), nv._vp(258)
    head = lambda images, channels: (d, 3, images, channels, None, 70.0, 70.0, 40.0, 30.0, 60, 80)
    tail = (16, None, 1, 0, 0)
    for name, mid, end in (("rg_sample_rays_u8", (), (None, None, None)), ("rg_sample_rays_weighted_u8", (d, 4), (None, None, d, None, None))):
        with pytest.raises(ValueError, match=name + ": a u8 store holds 3 or 4 channels, not 2"):
            nv.call(name, *head(d, 2), *tail, *mid, d, d, d, None, *end)
        with pytest.raises(ValueError, match=name + ": bg_out belongs to a 4-channel store, and is required there"):
            nv.call(name, *head(d, 4), *tail, *mid, d, d, d, None, *end)
        with pytest.raises(ValueError, match=name + ": bg_out belongs to a 4-channel store, and is required there"):
            nv.call(name, *head(d, 3), *tail, *mid, d, d, d, d, *end)
        with pytest.raises(ValueError, match=name + ": the RGBA store must be 4-byte aligned"):
            nv.call(name, *head(odd, 4), *tail, *mid, d, d, d, d, *end)
        with pytest.raises(ValueError, match=name + ": null pointer"):
            nv.call(name, *head(None, 4), *tail, *mid, d, d, None, d, *end)
        with pytest.raises(ValueError, match=name + ": ground truth requested without an image store"):
            nv.call(name, *head(None, 3), *tail, *mid, d, d, d, None, *end)
    nv.call("rg_sample_rays_u8", *head(None, 3), 0, None, 1, 0, 0, None, None, None, None, None, None, None)      # no rays: nothing launched
    # the float entry points keep their message
    with pytest.raises(ValueError, match="rg_sample_rays_rgba: the RGBA store must be 16-byte aligned"):
        nv.call("rg_sample_rays_rgba", d, 3, nv._vp(264), 70.0, 70.0, 40.0, 30.0, 60, 80, *tail, d, d, d, d, None, None, None)
