"""Verifying a signature through an exported mesh (raster.verify_mesh, quality.mesh_survival) on the synthetic stage, untrained: the path and its bookkeeping are
checked, what survives is not (DESIGN.md section 24 reports it)."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
R = 48


@pytest.fixture(scope="module")
def stage():
    from nerf_signature_amd import quality
    return quality.watermark_stage(device=DEV, n_poses=1, n_test_poses=1, opaque=True)      # the ball opaque by accumulation, as tools/raster_bench.py measures it


@pytest.fixture(scope="module")
def message(stage):
    from nerf_signature_amd import quality
    return quality.messages(stage["D"], 1, seed=11)[0].to(DEV)


@pytest.fixture(scope="module")
def key(stage, message):
    from nerf_signature_amd import quality
    return quality.stage_key(stage, message)


@pytest.fixture(scope="module")
def coloured(stage, message):
    """(world vertices float32, triangles, normals, colours) of the stage's model at 48^3, cleaned, as mesh.save_mesh would write them."""
    from nerf_signature_amd import mesh
    m = stage["model"]
    lo, hi = m.aabb_infer[:3], m.aabb_infer[3:]
    u = mesh.lattice(m, lo, hi, R, message)
    occ = mesh.occupied(m, lo, hi, R)
    assert 0.03 < occ.float().mean() < 0.1 and bool(occ[R // 2, R // 2, R // 2]) and not bool(occ[0, 0, 0])      # the ball of radius 0.5 in the box [-1, 1]^3: pi / 48 of it
    thr = float(u[occ].median())                                                              # the random density head has no surface of its own: cut it at its median
    u = torch.where(occ, u, torch.full_like(u, -1.0))                                         # ... inside the occupied cells, as mesh_survival does
    v, t, n = mesh.marching_cubes(u, thr, normals=True, scale=mesh.lattice_scale(lo, hi, R))
    rgb = mesh.vertex_colors(m, mesh.world_vertices(v, lo, hi, R), n, message)
    v, t, n, rgb = mesh.clean(v, t, 8, attributes=(n, rgb))
    assert len(t) > 100
    return mesh.world_vertices(v, lo, hi, R).float().contiguous(), t, n, rgb.contiguous()


def test_occupied_marks_the_nodes_in_the_balls_cells(stage):
    """mesh.occupied against the scene's own statement (synthetic.density_grid): a node is occupied when the centre of its 128^3 cell lies inside the ball of radius 0.5."""
    from nerf_signature_amd import mesh
    m = stage["model"]
    occ = mesh.occupied(m, m.aabb_infer[:3], m.aabb_infer[3:], R).cpu().numpy()
    ax = torch.linspace(-1.0, 1.0, R).numpy()
    cell = np.clip(np.floor((ax / np.float32(1.0) + np.float32(1.0)) * np.float32(64.0)), 0, 127)
    centre = 2.0 * (cell + 0.5) / 128.0 - 1.0
    want = np.sqrt(centre[:, None, None] ** 2 + centre[None, :, None] ** 2 + centre[None, None, :] ** 2) < 0.5
    assert occ.shape == (R, R, R) and np.array_equal(occ, want) and 3000 < want.sum() < 12000


def test_the_pose_and_blocks_key_reproduces_the_stages_block_rays(stage, key):
    from nerf_signature_amd import synthetic
    o, d = key.block_rays(DEV)
    assert o.shape == stage["block_o"].shape == (stage["D"], 12, 12, 3)
    assert torch.equal(o, stage["block_o"]) and torch.equal(d, stage["block_d"])
    assert key.poses.shape == (1, 4, 4) and np.array_equal(key.poses[0], synthetic.orbit_pose(1.1, 0.7, synthetic.SCENES["hotdog"]["radius"]))
    b = key.blocks
    assert b.shape == (32, 4) and ((b[:, 2] - b[:, 0]) == 12).all() and ((b[:, 3] - b[:, 1]) == 12).all() and (b % 12 == 0).all() and len({tuple(r) for r in b.tolist()}) == 32


def test_verify_mesh_is_verify_on_the_key_views_blocks(stage, key, coloured):
    from nerf_signature_amd import raster, release as rel
    verts, tris, _, rgb = coloured
    got, view = raster.verify_mesh(verts, tris, rgb, key, details=True)
    assert got == raster.verify_mesh(verts, tris, rgb, key)
    by_hand = raster.render_mesh(verts, tris, rgb, key.poses[0], key.intrinsics, key.H, key.W, bg_color=1.0, near=0.05)
    for k in ("image", "depth", "triangle"):
        assert torch.equal(by_hand[k], view[k])
    assert by_hand["culled"] == view["culled"] and (by_hand["triangle"] >= 0).sum() > 100
    blocks = raster.key_blocks(by_hand["image"], key)
    assert blocks.shape == (key.D, 12, 12, 3) and blocks.is_contiguous()
    for k, (r0, c0, r1, c1) in enumerate(key.blocks.tolist()):
        assert torch.equal(blocks[k], by_hand["image"][r0:r1, c0:c1])
    with torch.no_grad():
        image = torch.clamp(blocks.float(), min=0, max=1)
        logits = key.decoder(DEV)(key.normalize(image.permute(0, 3, 1, 2))).reshape(-1)
    want = rel.verdict((logits > 0).to(torch.uint8).cpu(), key.message)
    assert got == want and len(got["bits"]) == key.D and got["p_value"] == rel.p_value(key.D, got["matches"])


def test_vertex_colors_along_given_directions(stage, message, key, coloured):
    from nerf_signature_amd import mesh, raster
    m = stage["model"]
    verts, _, normals, rgb = coloured
    dirs = raster.view_directions(verts, key.poses[0])
    c = torch.from_numpy(key.poses[0][:3, 3]).to(DEV)
    assert dirs.shape == verts.shape and dirs.dtype == torch.float32 and torch.equal(dirs, (verts - c) / torch.norm(verts - c, dim=-1, keepdim=True))
    assert torch.allclose(dirs.norm(dim=-1), torch.ones(len(dirs), device=DEV), atol=1e-6)
    got = mesh.vertex_colors(m, verts, None, message, directions=dirs)
    with torch.no_grad():
        _, want = m(verts, dirs, message)
    assert torch.equal(got, want) and not torch.equal(got, rgb)
    assert torch.equal(mesh.vertex_colors(m, verts.double(), normals, message, directions=dirs), want)      # the normals are not looked at
    # the default path is what it was: against the normal
    zero = (normals == 0).all(dim=-1, keepdim=True)
    against = torch.where(zero, torch.tensor([0.0, 0.0, 1.0], device=DEV), -normals).contiguous()
    assert torch.equal(mesh.vertex_colors(m, verts, normals, message), mesh.vertex_colors(m, verts, None, message, directions=against))
    with pytest.raises(ValueError, match="vertices with 3 directions"):
        mesh.vertex_colors(m, verts, None, message, directions=dirs[:3])


def test_refused_keys(stage, message, key, coloured):
    from nerf_signature_amd import raster, release as rel
    verts, tris, _, rgb = coloured
    ready = rel.SignatureKey.from_block_rays(message, stage["model"].msg_decoder, stage["block_o"], stage["block_d"], stage["render_kwargs"])
    with pytest.raises(ValueError, match=r"verify_mesh: the key needs its pose and block coordinates; one built from ready block rays \(from_block_rays\) has no view to render"):
        raster.verify_mesh(verts, tris, rgb, ready)
    with pytest.raises(ValueError, match="key_blocks: the key has no block coordinates"):
        raster.key_blocks(torch.zeros(key.H, key.W, 3, device=DEV), ready)
    two = rel.SignatureKey(message, key.decoder_state, key.intrinsics, key.H, key.W, np.concatenate([key.poses, key.poses]), key.blocks, key.render_kwargs)
    sentence = r"block rays of more than one key pose: the reference reshapes the key view to \[1, H, W, 3\] \(provider_wtmk.py:465\)"
    with pytest.raises(NotImplementedError, match=sentence):
        two.block_rays(DEV)
    with pytest.raises(NotImplementedError, match=sentence):
        raster.verify_mesh(verts, tris, rgb, two)
    with pytest.raises(ValueError, match=r"key_blocks: expected the key view \[400, 400, 3\]"):
        raster.key_blocks(torch.zeros(400, 399, 3, device=DEV), key)


def test_mesh_survival_loop(stage, message, coloured):
    from nerf_signature_amd import quality, release as rel
    out = quality.mesh_survival(stage, message, resolutions=(R,), colors=("normal", "view"), threshold="median")
    D = stage["D"]
    assert set(out) == {"field", "cells"} and len(out["field"]["bits"]) == D and len(out["cells"]) == 2
    a, b = out["cells"]
    assert (a["resolution"], a["colors"], b["resolution"], b["colors"]) == (R, "normal", R, "view")
    assert (a["V"], a["T"]) == (b["V"], b["T"]) == (len(coloured[0]), len(coloured[1]))             # the colouring changes no geometry
    for c in out["cells"]:
        assert math.isfinite(c["psnr_db"]) and math.isfinite(c["ssim"]) and -1.0 <= c["ssim"] <= 1.0 and c["psnr_db"] > 0
        assert 0 <= c["matches"] <= D and c["bit_accuracy"] == c["matches"] / D and c["p_value"] == rel.p_value(D, c["matches"])
        near, guard = c["culled"]
        assert 0 <= near <= c["T"] and 0 <= guard <= c["T"] - near
    with pytest.raises(ValueError, match="neither 'normal' nor 'view'"):
        quality.mesh_survival(stage, message, resolutions=(R,), colors=("flat",))
