"""The u8 image store on the device (rg_sample_rays_u8 / rg_sample_rays_weighted_u8; rays.DeviceRaySampler over a torch.uint8 tensor; dataset.load_scene): every
output of both samplers equal to the float sampler's over the decoded store (code / 255, the IEEE division) on the shared case list (tests/store_cases.py, whose reach test_dataset_cpu.py proves),
views at every byte phase between guard bytes, decode tables, the captured stage-1 loop fed from either store, and a scene directory read into a sampler.
Every comparison is an equality: the feature has no tolerance."""
import numpy as np
import pytest
import torch

import dataset_ref as dr
import store_cases as sc
import test_gpu_rgba as base        # its ball views' shapes, model and draw helper: the captured loops below are that file's, fed from a u8 store

pytestmark = pytest.mark.gpu
_draw = base._draw


def _decoded(u8):
    """The float twin of a u8 store: code / 255 in IEEE division (dataset.decode_u8; test_decode_u8_is_the_host_division holds it to numpy).  torch's
    `u8.float() / 255` ON THE DEVICE is not that: a Python-scalar divisor is multiplied in as 1/255 there, and 126 of the 256 codes differ (measured on an MI355X)."""
    from nerf_signature_amd.dataset import decode_u8
    return decode_u8(u8)


def test_decode_u8_is_the_host_division():
    q = torch.arange(256, dtype=torch.uint8, device="cuda")
    want = np.arange(256, dtype=np.uint8).astype(np.float32) / np.float32(255)
    assert np.array_equal(_decoded(q).cpu().numpy(), want) and _decoded(q).dtype == torch.float32


def _pair(P, H, W, N, C, G=None, decode=None, images=None, twin=None):
    """(u8 sampler, float twin) over one case: the twin's store is the decoded store, formed on the device (or `twin`)."""
    from nerf_signature_amd import rays
    u8 = torch.from_numpy(sc.store(P, H, W, C) if images is None else images).cuda()
    flt = _decoded(u8) if twin is None else twin
    poses = torch.from_numpy(sc.poses(P)).cuda()
    kw = dict(stride=sc.STRIDE, offset=sc.OFFSET, seed=sc.SEED)
    maps = lambda: {} if G is None else dict(error_map=torch.from_numpy(sc.error_map(P, G)).cuda(), error_grid=G)
    a = rays.DeviceRaySampler(poses, u8, sc.intrinsics(H, W), H, W, N, decode=decode, **kw, **maps())
    b = rays.DeviceRaySampler(poses, flt, sc.intrinsics(H, W), H, W, N, **kw, **maps())
    assert a.u8 and a.images.dtype == torch.uint8 and a.images.data_ptr() == u8.data_ptr() and not b.u8 and b.images.dtype == torch.float32
    assert a.channels == b.channels == C
    return a, b, u8


def _equal(a, b, C, G, where):
    assert a["pose"] == b["pose"], where
    for key in ("o", "d", "gt", "inds") + (("bg",) if C == 4 else ()) + (("coarse", "keys") if G is not None else ()):
        assert torch.equal(a[key], b[key]), (key, where)
    assert not torch.isnan(a["gt"]).any() and not torch.isnan(a["o"]).any() and int(a["inds"].min()) >= 0


@pytest.mark.parametrize("C", [3, 4])
@pytest.mark.parametrize("case", sc.CASES + (sc.ALL_CODES,), ids=lambda c: "x".join(map(str, c)))
def test_uniform_u8_sampler_equals_its_float_twin(case, C):
    P, H, W, N = case
    a, b, u8 = _pair(P, H, W, N, C, images=sc.every_code_store(C) if case == sc.ALL_CODES else None)
    for step in sc.STEPS:
        x, y = _draw(a, step), _draw(b, step)
        _equal(x, y, C, None, (case, step))
        assert x["pose"] == step % P and int(x["inds"].max()) < H * W
        if C == 3:      # the ground truth is the drawn pixel's codes over 255, by numpy on the host
            want = u8[x["pose"]][x["inds"]].cpu().numpy().astype(np.float32) / np.float32(255)
            assert np.array_equal(x["gt"].cpu().numpy(), want)


@pytest.mark.parametrize("C", [3, 4])
@pytest.mark.parametrize("G", sorted(sc.WEIGHTED))
@pytest.mark.parametrize("case", sc.CASES, ids=lambda c: "x".join(map(str, c)))
def test_weighted_u8_sampler_equals_its_float_twin(case, G, C):
    P, H, W, _ = case
    for N in sc.WEIGHTED[G]:
        a, b, _ = _pair(P, H, W, N, C, G=G)
        for step in sc.STEPS:
            x, y = _draw(a, step), _draw(b, step)
            _equal(x, y, C, G, (case, G, N, step))
            assert int(x["coarse"].min()) >= 0 and int(x["coarse"].max()) < G * G and not torch.isnan(x["keys"]).any()


def test_a_uint8_store_is_decoded_not_sampled_as_0_to_255():
    """Before the u8 store a uint8 tensor went through .float() and its ground truth came out as 0...255."""
    from nerf_signature_amd import rays
    P, H, W, N = sc.CASES[2]
    store = sc.store(P, H, W, 3)
    s = rays.DeviceRaySampler(torch.from_numpy(sc.poses(P)).cuda(), torch.from_numpy(store).cuda().view(P, H, W, 3), sc.intrinsics(H, W), H, W, N, seed=sc.SEED)
    for step in sc.STEPS:
        x = _draw(s, step)
        want = store[x["pose"]][x["inds"].cpu().numpy()].astype(np.float32) / np.float32(255)
        assert np.array_equal(x["gt"].cpu().numpy(), want)
        assert float(x["gt"].max()) <= 1.0


@pytest.mark.parametrize("G", [None, 4], ids=["uniform", "map4"])
def test_rgb_views_at_every_byte_phase_between_guard_bytes(G):
    """The RGB store as a view 1, 2 and 3 bytes into a buffer of 0xFF bytes: the results of the store at phase 0.  A fetch that read a byte before the view or behind it
    would read 255 where the pixel holds another code -- and the draws reach the first and the last pixel of every pose."""
    from nerf_signature_amd import rays
    P, H, W, N = sc.CASES[2]
    N = N if G is None else 16
    a, _, u8 = _pair(P, H, W, N, 3, G=G)
    want = [_draw(a, step) for step in sc.STEPS]
    n = u8.numel()
    for off in (1, 2, 3):
        buf = torch.full((n + 8,), 0xFF, dtype=torch.uint8, device="cuda")
        assert buf.data_ptr() % 4 == 0
        buf[off:off + n] = u8.reshape(-1)
        view = buf[off:off + n].view(P, H * W, 3)
        assert view.data_ptr() % 4 == off
        s = rays.DeviceRaySampler(a.poses, view, a.intr, H, W, N, seed=sc.SEED, **({} if G is None else dict(error_map=a.error_map, error_grid=G)))
        assert s.images.data_ptr() == view.data_ptr()
        for step, w in zip(sc.STEPS, want):
            _equal(_draw(s, step), w, 3, G, (off, step))
        assert bool((buf[:off] == 0xFF).all()) and bool((buf[off + n:] == 0xFF).all())


def test_an_rgba_store_at_an_odd_address_is_refused_before_any_launch():
    from nerf_signature_amd import _native as nv, rays
    P, H, W, N = sc.CASES[2]
    u8 = torch.from_numpy(sc.store(P, H, W, 4)).cuda()
    poses = torch.from_numpy(sc.poses(P)).cuda()
    for off in (1, 2, 3):
        buf = torch.full((u8.numel() + 8,), 0xFF, dtype=torch.uint8, device="cuda")
        view = buf[off:off + u8.numel()].view(P, H * W, 4)
        with pytest.raises(ValueError, match="4-byte aligned"):
            rays.DeviceRaySampler(poses, view, sc.intrinsics(H, W), H, W, N)
        # ... and by the entry point itself, whose outputs stay untouched
        o, d, gt, bg = (torch.full((N, 3), float("nan"), device="cuda") for _ in range(4))
        with pytest.raises(ValueError, match="rg_sample_rays_u8: the RGBA store must be 4-byte aligned"):
            nv.call("rg_sample_rays_u8", nv.ptr(poses), P, view.data_ptr(), 4, None, *sc.intrinsics(H, W), H, W, N, None, 1, 0, sc.SEED, nv.ptr(o), nv.ptr(d), nv.ptr(gt),
                    nv.ptr(bg), None, None, nv.stream())
        torch.cuda.synchronize()
        assert bool(torch.isnan(o).all()) and bool(torch.isnan(gt).all()) and bool(torch.isnan(bg).all())


def _table():
    """256 distinct arbitrary floats (negative, above 1 and tiny ones among them)."""
    t = torch.randn(256, generator=torch.Generator().manual_seed(256)) * 3
    assert len(set(t.tolist())) == 256
    return t.cuda()


@pytest.mark.parametrize("G", [None, 4], ids=["uniform", "map4"])
def test_decode_table(G):
    P, H, W, N = sc.CASES[2]
    N = N if G is None else 16
    table = _table()
    # RGB: the ground truth is the table's entry of every code
    a, _, u8 = _pair(P, H, W, N, 3, G=G, decode=table)
    for step in sc.STEPS:
        x = _draw(a, step)
        assert torch.equal(x["gt"], table[u8[x["pose"]][x["inds"]].long()]), step
    # RGBA: table colours under alpha code / 255 -- the float sampler over that decoded store
    store4 = torch.from_numpy(sc.store(P, H, W, 4)).cuda()
    decoded = torch.cat([table[store4[..., :3].long()], _decoded(store4[..., 3:])], dim=-1).contiguous()
    a, b, _ = _pair(P, H, W, N, 4, G=G, decode=table, twin=decoded)
    for step in sc.STEPS:
        _equal(_draw(a, step), _draw(b, step), 4, G, step)
    # no table is the table arange(256) / 255 (formed on the host: the IEEE division)
    for C in (3, 4):
        a, _, _ = _pair(P, H, W, N, C, G=G)
        b, _, _ = _pair(P, H, W, N, C, G=G, decode=(torch.arange(256) / 255).cuda())
        assert a.decode is None and b.decode is not None
        for step in sc.STEPS:
            _equal(_draw(a, step), _draw(b, step), C, G, (C, step))


def test_sampler_refusals():
    from nerf_signature_amd import rays
    P, H, W, N = sc.CASES[2]
    poses, u8 = torch.from_numpy(sc.poses(P)).cuda(), torch.from_numpy(sc.store(P, H, W, 3)).cuda()
    mk = lambda images, **kw: rays.DeviceRaySampler(poses, images, sc.intrinsics(H, W), H, W, N, **kw)
    table = (torch.arange(256) / 255).cuda()
    with pytest.raises(ValueError, match="decode= belongs to a uint8 store"):
        mk(_decoded(u8), decode=table)
    with pytest.raises(ValueError, match="decode= belongs to a uint8 store"):
        mk(None, decode=table)
    for bad in (table[:255], table.double(), table.cpu(), table.view(16, 16), list(range(256))):
        with pytest.raises(ValueError, match=r"decode must be a float32 tensor \[256\] on cuda"):
            mk(u8, decode=bad)
    for dtype in (torch.int32, torch.int8, torch.int64, torch.bool):
        with pytest.raises(ValueError, match="images must be a float or a uint8 tensor, not " + str(dtype)):
            mk(u8.to(dtype))
    assert mk(u8.half() / 255).images.dtype == torch.float32          # float stores of any width take the path they took: .float()
    with pytest.raises(ValueError, match="RGB or RGBA"):
        mk(u8[..., :2])
    # bg= goes with the channel count, whatever the store's dtype
    buf = lambda: torch.empty(N, 3, device="cuda")
    with pytest.raises(ValueError, match="RGBA store"):
        mk(u8).sample_into(None, buf(), buf(), buf(), bg=buf())
    with pytest.raises(ValueError, match="bg="):
        mk(torch.from_numpy(sc.store(P, H, W, 4)).cuda()).sample_into(None, buf(), buf(), buf())


# ---- the captured stage-1 loop, fed from either store
def _loop(images, error_map, n_rays=256):
    from nerf_signature_amd import rays
    from nerf_signature_amd.stage1 import GraphedCleanLoop
    v = base._rgba_ball_views()
    m = base._clean_model()
    s = rays.DeviceRaySampler(v["poses"], images, v["intr"], v["H"], v["W"], n_rays, seed=base.SEED, error_map=error_map, error_grid=32)
    torch.manual_seed(11)
    return m, s, GraphedCleanLoop(m, base._adam(m), base.KW, n_rays=n_rays, sampler=s, update_extra_interval=0, perturb=True, seed=3)


@pytest.mark.parametrize("variant", ["rgb", "rgba", "rgba_error_map"])
def test_captured_loop_from_a_u8_store_equals_the_loop_from_its_float_twin(variant):
    """20 captured steps of GraphedCleanLoop on test_gpu_rgba.py's ball views (24 poses of 64 x 64, 256 rays, error grid 32), quantised to uint8: every parameter, the
    loss ring and the error map torch.equal between the u8 sampler and the float sampler over the decoded store.  No change to the loop was needed."""
    v = base._rgba_ball_views()
    P, H, W = v["P"], v["H"], v["W"]
    u8 = (v["images"] * 255).round().to(torch.uint8).view(P, H, W, 4)
    assert u8.unique().numel() == 5         # 0, the three colour codes, 255
    if variant == "rgb":
        u8 = u8[..., :3].contiguous()
    got = {}
    for name, images in (("u8", u8), ("float", _decoded(u8))):
        m, s, loop = _loop(images, variant == "rgba_error_map")
        assert s.u8 == (name == "u8") and loop.rgba == (variant != "rgb")
        for _ in range(20):
            loop.step()
        torch.cuda.synchronize()
        assert not loop.overflowed() and len(loop.graph.segments) == 1
        got[name] = ([p.detach().clone() for p in m.trainable()], loop.losses(), None if s.error_map is None else s.error_map.clone(), int(loop.step_dev), loop.gt.clone())
        loop.close()
    a, b = got["u8"], got["float"]
    assert a[3] == b[3] == 20 and len(a[1]) == 20 and a[1] == b[1] and np.isfinite(a[1]).all()
    assert len(a[0]) == len(b[0]) == 18
    for x, y in zip(a[0], b[0]):
        assert torch.equal(x, y)
    assert torch.equal(a[4], b[4])
    if variant == "rgba_error_map":
        assert torch.equal(a[2], b[2]) and not torch.equal(a[2], torch.ones_like(a[2]))


def test_a_content_sampler_draw_from_a_u8_store():
    """trainer.GraphedWatermarkLoop(content_sampler=) calls sample_into(counter, rays_o, rays_d, images) and nothing else of the sampler: that call, over an RGB u8
    store and over its float twin."""
    v = base._rgba_ball_views()
    from nerf_signature_amd import rays
    P, H, W, N = v["P"], v["H"], v["W"], 256
    u8 = (v["images"][..., :3] * 255).round().to(torch.uint8).contiguous()
    out = []
    for images in (u8, _decoded(u8)):
        s = rays.DeviceRaySampler(v["poses"], images, v["intr"], H, W, N, seed=base.SEED)
        assert s.error_map is None and s.channels == 3
        ct = {k: torch.full((1, N, 3), float("nan"), device="cuda") for k in ("rays_o", "rays_d", "images")}
        s.sample_into(torch.full((1,), 5, dtype=torch.int32, device="cuda"), ct["rays_o"], ct["rays_d"], ct.get("images"))
        out.append(ct)
    for k in out[0]:
        assert torch.equal(out[0][k], out[1][k]) and not torch.isnan(out[0][k]).any(), k


# ---- a scene directory, end to end
@pytest.mark.parametrize("C", [3, 4])
def test_scene_directory_to_sampler_and_view(tmp_path, C):
    from nerf_signature_amd import stage1
    from nerf_signature_amd.dataset import load_scene
    root = str(tmp_path / "scene")
    dr.write_scene(root, "blender", C=C, h=10, w=14)
    want = dr.expected(root, downscale=2)
    scene = load_scene(root, downscale=2)
    assert scene.poses.is_cuda and scene.images.is_cuda and scene.images.dtype == torch.uint8 and tuple(scene.images.shape) == (3, 5, 7, C)
    assert np.array_equal(scene.images.cpu().numpy(), want["images"]) and np.array_equal(scene.poses.cpu().numpy(), want["poses"])
    N = 64
    s = scene.sampler(N, seed=sc.SEED)
    assert s.u8 and s.channels == C and s.decode is None
    for step in (0, 1, 4):
        x = _draw(s, step)
        p, inds, gt, bg = dr.expected_draw(want, sc.SEED, step, N)
        assert x["pose"] == p and np.array_equal(x["inds"].cpu().numpy(), inds)
        assert np.array_equal(x["gt"].cpu().numpy(), gt)
        assert C == 3 or np.array_equal(x["bg"].cpu().numpy(), bg)
    # the linear colour space as a table: the reference's srgb_to_linear on the decoded store
    lin = scene.sampler(N, seed=sc.SEED, decode=scene.linear_decode())
    x = _draw(lin, 0)
    p, inds, _, _ = dr.expected_draw(want, sc.SEED, 0, N)
    if C == 3:
        from nerf_signature_amd.trainer import srgb_to_linear
        assert torch.equal(x["gt"], srgb_to_linear(_decoded(scene.images[p].view(-1, 3)[torch.from_numpy(inds).cuda()])))
    # a view for eval_step
    view = scene.view(1)
    assert tuple(view["images"].shape) == (1, 5, 7, C) and view["images"].dtype == torch.float32 and tuple(view["rays_o"].shape) == (1, 35, 3)
    assert np.array_equal(view["images"].cpu().numpy(), want["images"][1:2].astype(np.float32) / np.float32(255))
    m = base._clean_model().eval()
    pred, depth, gt, loss = stage1.eval_step(m, view, base.KW)
    assert tuple(pred.shape) == (1, 5, 7, 3) and tuple(depth.shape) == (1, 5, 7) and tuple(gt.shape) == (1, 5, 7, 3) and bool(torch.isfinite(loss))
