"""The oracle's Python restatement vs golden vectors captured from the real reference
(tests/golden/make_golden.py).  CPU only."""
import os

import numpy as np
import torch

import closed_form as cf
from oracle import field_ref as fr

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _load(name):
    return np.load(os.path.join(G, name), allow_pickle=False)


def test_g1_base_encoder_rows_bit_exact_and_features():
    g = _load("g1_base_encoder.npz")
    x = torch.from_numpy(cf.points())
    res = fr.level_resolutions()
    assert [float(r) for r in res] == [16, 22, 30, 42, 58, 80, 111, 153, 212, 294, 406, 561, 776, 1072, 1482, 2047]
    np.testing.assert_array_equal(np.array([float(r) for r in res], np.float32), g["resolutions"])
    for l, r in enumerate(res):
        rows, w, _ = fr.voxel_lookup(x, r)
        np.testing.assert_array_equal(rows.numpy().astype(np.int32), g["rows"][l])
        np.testing.assert_array_equal(w.numpy(), g["weights"][l])
    feats = fr.base_encode(x, [torch.from_numpy(cf.table(l)) for l in range(16)])
    np.testing.assert_array_equal(feats.numpy(), g["features"])


def test_scatter_ref_equals_float64_autograd_of_the_lookup():
    """oracle.field_ref.scatter_ref (the float64 table gradient the GPU scatter routes are held to) against float64 autograd of
    trilerp(table[rows], w) at the codebook resolution and at all 16 base-level resolutions, on cf.points()' edge points (exact 0 and 1,
    cell boundaries and their neighbours) plus points repeated on one row; gradients of mixed sign and scale."""
    x = torch.from_numpy(cf.points())
    x = torch.cat([x, x[4:10].repeat(5, 1)])                    # the same cell corners hit again (rows that accumulate)
    rng = np.random.RandomState(5)
    g = torch.from_numpy((rng.randn(x.shape[0], 2) * np.exp2(rng.randint(-20, 20, (x.shape[0], 1)))).astype(np.float32))
    cb_res = fr.level_resolutions(64, 2048, 2048)[0]
    assert float(cb_res) == 2048.0
    for res in [cb_res] + fr.level_resolutions():
        rows, w, _ = fr.voxel_lookup(x, res)
        table = torch.zeros(1 << 19, 2, dtype=torch.float64, requires_grad=True)
        (fr.trilerp(table[rows], w.double()) * g.double()).sum().backward()
        got = fr.scatter_ref(x, g, res)
        assert got.dtype == torch.float64 and got.shape == (1 << 19, 2)
        assert torch.equal(got != 0, table.grad != 0), float(res)
        # two float64 evaluations of the same products and sums (another association order): a few ulp of the row's sum of magnitudes
        np.testing.assert_allclose(got.numpy(), table.grad.numpy(), rtol=1e-13, atol=1e-13 * float(table.grad.abs().max()))
    # a non-finite gradient reaches its rows and only them
    g[0, 0] = float("nan")
    got = fr.scatter_ref(x, g, cb_res)
    rows, _, _ = fr.voxel_lookup(x[:1], cb_res)
    assert torch.isnan(got[rows[0], 0]).all() and int(torch.isnan(got).sum()) == 8


def test_g2_codebook_forward_and_shared_gradient():
    g = _load("g2_codebook.npz")
    x = torch.from_numpy(cf.points())
    rvec = torch.from_numpy(g["rvec"])
    for D in (32, 48):
        assert float(g[f"resolution_D{D}"]) == 2048.0
        tables = [torch.from_numpy(cf.table(100 + l, scale=0.05)).requires_grad_(True) for l in range(2 * D)]
        for k, msg in enumerate(cf.messages(D)):
            for t in tables:
                t.grad = None
            out = fr.codebook_encode(x, torch.from_numpy(msg), tables, faithful=(k == 2))
            np.testing.assert_allclose(out.detach().numpy(), g[f"out_D{D}_m{k}"], rtol=0, atol=2e-7)
            (out * rvec).sum().backward()
            sel = [2 * i + int(msg[i]) for i in range(D)]
            assert all(tables[2 * i + 1 - int(msg[i])].grad is None for i in range(D))
            g0 = tables[sel[0]].grad
            nz = torch.nonzero(g0.abs().sum(-1)).squeeze(-1)
            np.testing.assert_array_equal(nz.numpy().astype(np.int32), g[f"grad_rows_D{D}_m{k}"])
            np.testing.assert_allclose(g0[nz].numpy(), g[f"grad_vals_D{D}_m{k}"], rtol=1e-5, atol=1e-7)
            # the identity the HIP path relies on: every selected table receives the same gradient
            assert float(g[f"grad_maxdiff_D{D}_m{k}"]) == 0.0
            assert max(float((tables[j].grad - g0).abs().max()) for j in sel) == 0.0


def test_g3_g4_sh_and_trunc_exp():
    g = _load("g3_g4_sh_truncexp.npz")
    sh = fr.sh4(torch.from_numpy(cf.unit_dirs()))
    np.testing.assert_allclose(sh.numpy(), g["sh"], rtol=0, atol=1e-6)
    v = torch.from_numpy(g["te_x"]).requires_grad_(True)
    y = fr.trunc_exp(v)
    y.backward(torch.ones_like(y))
    np.testing.assert_array_equal(y.detach().numpy(), g["te_y"])
    np.testing.assert_array_equal(v.grad.numpy(), g["te_grad"])


def test_g5_g6_normalize_loss_meters():
    g = _load("g5_g6_decoder_meters.npz")
    img = torch.from_numpy(g["img"])
    np.testing.assert_allclose(fr.normalize_img(img.permute(0, 3, 1, 2)).numpy(), g["normalized"], rtol=0, atol=1e-6)
    decoded, msg = torch.from_numpy(g["decoded"]), torch.from_numpy(g["msg"])
    lossw = torch.nn.functional.binary_cross_entropy_with_logits(decoded * 10.0, msg.unsqueeze(-1), reduction="mean")
    np.testing.assert_allclose(float(lossw), float(g["lossw"]), rtol=1e-6)
    acc = fr.bit_accuracy(decoded.permute(1, 0), msg[None])
    np.testing.assert_allclose(float(acc), float(g["bit_acc"]), rtol=0, atol=1e-7)
    np.testing.assert_allclose(fr.psnr(g["img"], g["img"] * 0.9 + 0.02), float(g["psnr"]), rtol=1e-5)


def test_g7_get_rays():
    g = _load("g7_get_rays.npz")
    inds = torch.from_numpy(g["inds"])[None]
    o, d = fr.get_rays(torch.from_numpy(g["pose"])[None], g["intrinsics"], 400, 400, inds)
    np.testing.assert_allclose(o[0].numpy(), g["rays_o"], rtol=0, atol=0)
    np.testing.assert_allclose(d[0].numpy(), g["rays_d"], rtol=0, atol=1e-7)


def _glue_setup():
    g = _load("g8_g9_glue.npz")
    D = 32
    grid, bitfield, C = cf.ball_scene()
    P = {"bound": 1.0,
         "base_tables": [torch.from_numpy(cf.table(l)) for l in range(16)],
         "cb_tables": [torch.from_numpy(cf.table(100 + l, scale=0.05)).requires_grad_(True) for l in range(2 * D)],
         "sigma_params": torch.from_numpy(cf.mlp_params(3072, 1337)),
         "color_params": torch.from_numpy(cf.mlp_params(7168, 1338))}
    S = {"bound": 1.0, "cascade": C, "grid_size": 128, "density_bitfield": bitfield,
         "aabb": np.array([-1, -1, -1, 1, 1, 1], np.float32), "min_near": 0.2, "density_scale": 1}
    return g, P, S


def test_g8_network_forward_glue():
    g, P, S = _glue_setup()
    pts, dirs, msg = (torch.from_numpy(g[k]) for k in ("pts", "dirs", "msg"))
    s_m, c_m = fr.field_forward(pts, dirs, msg, P)
    s_0, c_0 = fr.field_forward(pts, dirs, None, P)
    np.testing.assert_allclose(s_m.detach().numpy(), g["sigma_msg"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(c_m.detach().numpy(), g["rgb_msg"], rtol=0, atol=1e-6)
    np.testing.assert_allclose(s_0.detach().numpy(), g["sigma_clean"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(c_0.detach().numpy(), g["rgb_clean"], rtol=0, atol=1e-6)
    assert not np.allclose(g["sigma_msg"], g["sigma_clean"])


def test_g9_render_glue_train_staged_clean_eval_and_grads():
    g, P, S = _glue_setup()
    o, d, msg = (torch.from_numpy(g[k]) for k in ("rays_o", "rays_d", "msg"))
    kw = dict(bg_color=1, dt_gamma=0.0, max_steps=1024)
    out = fr.render(o, d, msg, P, S, staged=False, **kw)
    np.testing.assert_allclose(out["image"].detach().numpy(), g["image"], rtol=0, atol=2e-6)
    np.testing.assert_allclose(out["weights_sum"].detach().numpy(), g["weights_sum"], rtol=0, atol=2e-6)
    np.testing.assert_allclose(out["depth"].detach().numpy(), g["depth"], rtol=0, atol=2e-6, equal_nan=True)
    (out["image"] * torch.from_numpy(g["gvec"])).sum().backward()
    g0 = P["cb_tables"][int(msg[0])].grad
    nz = torch.nonzero(g0.abs().sum(-1)).squeeze(-1)
    np.testing.assert_array_equal(nz.numpy().astype(np.int32), g["cb_grad_rows"])
    np.testing.assert_allclose(g0[nz].numpy(), g["cb_grad_vals"], rtol=1e-4, atol=1e-9)
    st = fr.render(o, d, msg, P, S, staged=True, max_ray_batch=24, **kw)
    np.testing.assert_allclose(st["image"].numpy(), g["image_staged"], rtol=0, atol=2e-6)
    cl = fr.render(o, d, None, P, S, staged=False, **kw)
    np.testing.assert_allclose(cl["image"].detach().numpy(), g["image_clean"], rtol=0, atol=2e-6)
    ev = fr.render(o, d, msg, P, S, staged=False, training=False, **kw)
    np.testing.assert_allclose(ev["image"].numpy(), g["image_eval"], rtol=0, atol=2e-6)
    np.testing.assert_allclose(ev["depth"].numpy(), g["depth_eval"], rtol=0, atol=2e-6, equal_nan=True)
    # the staged training image equals the unstaged one; eval-mode compositing differs slightly (T = 1 - sum w)
    np.testing.assert_allclose(g["image_staged"], g["image"], rtol=0, atol=1e-6)


def test_state_dict_contract_matches_reference():
    g = _load("g8_g9_glue.npz")
    keys = list(g["state_dict_keys"])
    assert "encoder.embeddings.0.weight" in keys and "msg_encoder.embeddings.63.weight" in keys
    assert "sigma_net.params" in keys and "color_net.params" in keys and "density_bitfield" in keys


def _grid_state():
    g = _load("g11_grid_maintenance.npz")
    G = int(g["grid_size"])
    state = {"density_grid": torch.zeros(2, G ** 3), "density_bitfield": None, "bound": 2, "grid_size": G, "density_scale": 1, "density_thresh": 0.6,
             "iter_density": 0, "mean_density": 0, "step_counter": torch.zeros(16, 2, dtype=torch.int32), "local_step": 0, "mean_count": 0}
    return g, state


def test_g11_density_grid_maintenance_matches_reference():
    """The oracle's mark_untrained_grid / update_extra_state against the reference's own NeRFRenderer methods (golden G11:
    renderer_wtmk.py:380-538 run on a 32^3 two-cascade grid with closed-form density and draws): grid values, -1 marks, bitfield,
    mean density and mean count identical after the marking, two full updates and one partial update."""
    import closed_form as cf
    g, st = _grid_state()
    n_marked = fr.mark_untrained_grid(st, g["poses"], g["intrinsics"], S=16)
    np.testing.assert_array_equal(st["density_grid"].numpy(), g["grid_marked"])
    assert n_marked == int((g["grid_marked"] < 0).sum()) > 0
    st["iter_density"], st["local_step"] = 14, 5
    st["step_counter"][:5, 0] = torch.tensor([1000, 1203, 990, 1500, 20], dtype=torch.int32)
    with cf.PatchedDraws() as draws:
        for k in range(3):
            if k == 2:
                st["local_step"] = 20
                st["step_counter"][:, 0] = torch.arange(16, dtype=torch.int32) * 100 + 7
            _, hits = fr.update_extra_state(st, cf.grid_density, None, 0.95, 16, rand_like=torch.rand_like, randint=torch.randint)
            # a cell the partial update draws more than once keeps one of its probes, unspecified which (index_put_ with duplicate
            # indices, renderer_wtmk.py:520): those cells are compared by bounds only
            once = (hits <= 1).numpy()
            assert once.all() == (k < 2) and once.mean() > 0.85
            got, want = st["density_grid"].numpy(), g[f"grid_{k}"]
            np.testing.assert_array_equal(got[once], want[once])
            np.testing.assert_array_equal((got < 0), (want < 0))
            bits = lambda b: np.unpackbits(b, bitorder="little").reshape(once.shape).astype(bool)
            np.testing.assert_array_equal(bits(st["density_bitfield"].numpy())[once], bits(g[f"bitfield_{k}"])[once])
            if k < 2:
                assert st["mean_density"] == float(g[f"mean_density_{k}"])
            else:
                assert abs(st["mean_density"] - float(g[f"mean_density_{k}"])) < 1e-3 * float(g[f"mean_density_{k}"])
            assert st["mean_count"] == int(g[f"mean_count_{k}"])
            assert draws.calls == int(g[f"draw_calls_{k}"])
    assert st["iter_density"] == 17 and st["local_step"] == 0
