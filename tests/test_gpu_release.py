"""release / SignatureKey / verify / Tamper / quality.model_robustness on a trained stage: one quality.watermark_stage() trained with the README schedule
through the captured loop (about a second), four messages of quality.messages."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def trained():
    from nerf_signature_amd import quality, rays
    stage = quality.watermark_stage()
    quality.train(stage, mode="graphed", log_every=0)
    msgs = [m.to(stage["device"]) for m in quality.messages(stage["D"], 4)]
    r = rays.get_rays(stage["test_poses"][:1], stage["intr"], stage["H"], stage["W"], -1)
    return stage, msgs, (r["rays_o"], r["rays_d"])


def _same(a, b):
    """Bit equality (a ray that misses the box has a NaN depth, as in the reference: torch.equal would call two such renders different)."""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _block_kw(stage):
    return dict(staged=False, bg_color=1, perturb=False, force_all_rays=True, **stage["render_kwargs"])


def _full_kw(stage):
    return dict(staged=True, bg_color=1, perturb=False, force_all_rays=True, **stage["render_kwargs"])


def _key(stage, message):
    from nerf_signature_amd.release import SignatureKey
    return SignatureKey.from_block_rays(message, stage["model"].msg_decoder, stage["block_o"], stage["block_d"], stage["render_kwargs"])


@pytest.mark.parametrize("which", range(4))
def test_release_renders_the_bits_of_the_source_model(trained, which):
    from nerf_signature_amd.release import release
    stage, msgs, (fo_, fd_) = trained
    model, m = stage["model"], msgs[which]
    bo, bd = stage["block_o"], stage["block_d"]
    with torch.no_grad():
        released = release(model, m)
        assert not [k for k in released.state_dict() if k.startswith(("msg_encoder.", "msg_decoder."))]
        want, got = model.render(bo, bd, m, **_block_kw(stage)), released.render(bo, bd, **_block_kw(stage))
        assert torch.equal(want["image"], got["image"]) and _same(want["depth"], got["depth"]) and torch.equal(want["weights_sum"], got["weights_sum"])
        assert not torch.equal(want["image"], model.render(bo, bd, None, **_block_kw(stage))["image"])      # (the message is visible in the bits at all)
        want, got = model.render(fo_, fd_, m, **_full_kw(stage)), released.render(fo_, fd_, **_full_kw(stage))
        assert torch.equal(want["image"], got["image"]) and _same(want["depth"], got["depth"])
        model.eval(), released.eval()
        try:
            want, got = model.render(bo, bd, m, **_block_kw(stage)), released.render(bo, bd, **_block_kw(stage))
        finally:
            model.train(), released.train()
        assert torch.equal(want["image"], got["image"]) and _same(want["depth"], got["depth"])
    with pytest.raises(RuntimeError, match="inference only"):
        released.render(bo, bd, **_block_kw(stage))


def test_checkpoint_round_trip_renders_the_same_bits(trained, tmp_path):
    from nerf_signature_amd.release import ReleasedModel, release
    stage, msgs, (fo_, fd_) = trained
    bo, bd = stage["block_o"], stage["block_d"]
    with torch.no_grad():
        released = release(stage["model"], msgs[0])
        back = ReleasedModel.load(released.save(str(tmp_path / "released.pth")), device=stage["device"])
        assert set(back.state_dict()) == set(released.state_dict()) and (back.mean_count, back.mean_density) == (released.mean_count, released.mean_density)
        a, b = released.render(bo, bd, **_block_kw(stage)), back.render(bo, bd, **_block_kw(stage))
        assert torch.equal(a["image"], b["image"]) and _same(a["depth"], b["depth"])
        a, b = released.render(fo_, fd_, **_full_kw(stage)), back.render(fo_, fd_, **_full_kw(stage))
        assert torch.equal(a["image"], b["image"])


def test_verify_finds_the_message_and_only_that_message(trained):
    from nerf_signature_amd.release import p_value, release, verify
    stage, msgs, _ = trained
    D = stage["D"]
    released = [release(stage["model"], m) for m in msgs]
    for m, r in zip(msgs, released):
        key = _key(stage, m)
        v = verify(r, key)
        print(f"matches {v['matches']} of {D}, p = {v['p_value']:.3e}")
        assert v["matches"] >= D - 1 and v["bit_accuracy"] == v["matches"] / D and v["p_value"] == p_value(D, v["matches"]) <= 7.7e-9
        assert v["bits"] == [int(b > 0) for b in m.tolist()] or v["matches"] == D - 1
        assert verify(r, key.with_message(1 - m))["matches"] == D - v["matches"]
        # black box: any callable (rays_o, rays_d) -> image
        kw = dict(staged=False, bg_color=1, perturb=False, force_all_rays=True, **stage["render_kwargs"])
        assert verify(lambda o, d: stage["model"].render(o, d, m, **kw)["image"], key) == v
    agree = int((msgs[0] == msgs[1]).sum())
    assert verify(released[1], _key(stage, msgs[0]))["matches"] <= agree + 1
    assert verify(released[1], _key(stage, msgs[0]))["matches"] >= agree - 1


def test_key_of_pose_and_blocks_rebuilds_its_rays(trained, tmp_path):
    """A key in the reference's form (pose file + block-coordinate file): block_rays() are the pixels' rays of those rectangles, before and after save / load,
    and verify runs on them."""
    import numpy as np
    from nerf_signature_amd import synthetic
    from nerf_signature_amd.release import SignatureKey, release, verify
    stage, msgs, _ = trained
    D, H, W = stage["D"], stage["H"], stage["W"]
    cfg = synthetic.SCENES[stage["scene"]]
    bh, bw = H // cfg["rows"], W // cfg["cols"]
    pose = synthetic.orbit_pose(1.1, 0.7, cfg["radius"])[None]
    cells = [(10 + k // 8, 12 + k % 8) for k in range(D)]
    coords = np.array([[r * bh, c * bw, (r + 1) * bh, (c + 1) * bw] for r, c in cells], np.int64)
    key = SignatureKey(msgs[0], stage["model"].msg_decoder.state_dict(), stage["intr"], H, W, pose, coords, stage["render_kwargs"])
    o, d = key.block_rays(stage["device"])
    assert o.shape == d.shape == (D, bh, bw, 3) and o.is_contiguous() and d.is_contiguous()
    ro, rd = synthetic.get_rays(torch.from_numpy(pose), stage["intr"], H, W)                  # the host statement of the same pinhole rays
    ro, rd = ro.view(H, W, 3), rd.view(H, W, 3)
    for k, (r0, c0, r1, c1) in enumerate(coords.tolist()):
        assert torch.allclose(o[k].cpu(), ro[r0:r1, c0:c1], atol=1e-5) and torch.allclose(d[k].cpu(), rd[r0:r1, c0:c1], atol=1e-5), k
    back = SignatureKey.load(key.save(str(tmp_path / "key")))
    bo, bd = back.block_rays(stage["device"])
    assert torch.equal(bo, o) and torch.equal(bd, d)
    v = verify(release(stage["model"], msgs[0]), back)
    assert len(v["bits"]) == D and v["matches"] == sum(int(b == int(m)) for b, m in zip(v["bits"], msgs[0].tolist()))


def test_tamper_drops_the_caches_and_strength_zero_changes_nothing(trained):
    from nerf_signature_amd.release import release, verify
    stage, msgs, _ = trained
    bo, bd = stage["block_o"], stage["block_d"]
    released = release(stage["model"], msgs[2], copy=True)
    key = _key(stage, msgs[2])
    with torch.no_grad():
        render = lambda: released.render(bo, bd, **_block_kw(stage))["image"]
        want, matches = render(), verify(released, key)["matches"]
        tm = released.tamper()
        assert tm.total == 17 * (1 << 20) + 10240
        for kind in ("prune", "noise"):
            tm.apply(kind, 0.0)
            assert torch.equal(render(), want) and verify(released, key)["matches"] == matches
        tm.apply("prune", 0.5)
        pruned = render()
        assert not torch.equal(pruned, want)                       # the MLP image was re-packed and the tables re-read: the caches are really dropped
        zeros = sum(int((t == 0).sum()) for t in released.tampered_tensors())
        assert zeros >= round(0.5 * tm.total)
        tm.apply("half")
        assert not torch.equal(render(), pruned) and not torch.equal(render(), want)
        tm.restore()
        assert torch.equal(render(), want) and verify(released, key)["matches"] == matches
        assert all(torch.equal(a, b) for a, b in zip(tm.pristine, released.tampered_tensors()))
        # the source model was released as a copy: it never saw any of this
        assert torch.equal(stage["model"].render(bo, bd, msgs[2], **_block_kw(stage))["image"], want)


def test_model_robustness_returns_one_record_per_grid_point(trained):
    from nerf_signature_amd import quality
    stage, msgs, _ = trained
    before = [t.clone() for t in (stage["model"].sigma_net.params, stage["model"].encoder.tables()[0])]
    out = quality.model_robustness(stage, msgs[3], seeds=(0, 1))
    want = [(k, s, seed) for k, s in quality.MODEL_ATTACKS for seed in ((0, 1) if k == "noise" else (0,))]
    assert list(out) == want and len(want) == 5 + 10 + 4 + 1
    for point, rec in out.items():
        print(point, rec)
        assert set(rec) == {"bit_accuracy", "matches", "p_value", "psnr"}
        assert 0 <= rec["matches"] <= stage["D"] and rec["bit_accuracy"] == rec["matches"] / stage["D"] and 0 < rec["p_value"] <= 1
        assert math.isfinite(rec["psnr"]) or rec["psnr"] == math.inf           # (+inf: the tampered render is bit-equal)
    assert all(torch.equal(a, b) for a, b in zip(before, (stage["model"].sigma_net.params, stage["model"].encoder.tables()[0])))
