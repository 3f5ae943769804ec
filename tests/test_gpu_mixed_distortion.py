"""The mixed distortion layer on the device (distortion code 6: the step's kind is a word in device memory): the selector against its host statement, every
selectable kind bit for bit against the existing single-kind path (the layer alone and fused into the decoder, forward and backward), the captured loop
against the eager step fed the same draws, and one model trained against all five kinds against one trained against none."""
import copy
import math

import numpy as np
import pytest
import torch

import mixed_distortion_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"      # (spelled with its index: the layer compares its buffers' device with the one it is handed)
SHAPES = [(32, 12, 12, 3), (48, 11, 15, 3), (4, 2, 2, 3), (5, 9, 14, 3)]
FUSED_ONLY = ("none", "noise", "brightness", "blurring")      # no geometric member: no resampling launch in front of the decoder


def _step_tensor(step):
    return torch.tensor([step if step < 2 ** 31 else step - 2 ** 32], dtype=torch.int32, device=DEV)


def test_device_selector_is_the_host_selector_and_the_selected_draw_is_the_single_kinds():
    """wm_distort_draw(6) at steps {0, 1, 2, 255, 256, 65535, 2^31 - 1, 2^32 - 1}, three sets, four seeds: the selector word equals host_selector; the selected
    kind's parameter / noise is bit for bit what wm_distort_draw(kind) writes at the same (seed, step) (scaling: float32(host_uniform)); an unselected rotation
    is (1, 0) per image; the noise tensor is written only when noise is selected."""
    from nerf_signature_amd.distortion import NAMES, DistortionLayer, host_selector, host_uniform
    shape = (5, 9, 14, 3)
    checked = set()
    for which, names in R.SETS.items():
        for seed in (0, 1, 2, 2 ** 32 + 5):
            mixed = DistortionLayer(names, seed)
            for step in (0, 1, 2, 255, 256, 65535, 2 ** 31 - 1, 2 ** 32 - 1):
                counter = _step_tensor(step)
                mixed._buffers(shape, torch.device(DEV))
                mixed.noise.fill_(-7.0)
                mixed.draw_on_device(counter, shape, torch.device(DEV))
                block = mixed.param.cpu()
                kind = int(block[:1].view(torch.int32))
                assert kind == host_selector(seed, step, mixed.mask) == mixed.select_on_host(step), (which, seed, step)
                name = NAMES[kind]
                checked.add(name)
                if name in ("noise", "brightness", "blurring", "rotation"):
                    single = DistortionLayer(name, seed)
                    single.draw_on_device(counter, shape, torch.device(DEV))
                if name == "noise":
                    assert torch.equal(mixed.noise, single.noise) and float(mixed.noise.abs().max()) < 6.0
                else:
                    assert bool((mixed.noise == -7.0).all())                                   # written only when selected
                if name == "brightness":
                    assert torch.equal(block[1:2], single.param.cpu())
                if name == "blurring":
                    assert torch.equal(block[2:3], single.param.cpu())
                if name == "scaling":
                    assert float(block[3]) == float(torch.tensor(host_uniform(seed, step, 0.75, 1.25), dtype=torch.float32)) and mixed.out_width(14) in range(10, 18)
                if name == "rotation":
                    assert torch.equal(block[4:], single.param.cpu())
                else:
                    assert torch.equal(block[4:].reshape(-1, 2), torch.tensor([[1.0, 0.0]]).expand(shape[0], 2))
    assert checked == set(R.SETS["six"])


def _raw(shape, seed=1):
    """Rendered blocks with pixels below 0, above 1, and at exactly 0 and 1."""
    rng = np.random.RandomState(seed)
    raw = rng.uniform(-0.25, 1.25, shape).astype(np.float32)
    flat = raw.reshape(-1)
    flat[::7], flat[3::11], flat[5::13] = 0.0, 1.0, -0.0
    return torch.from_numpy(raw)


def _mixed_layer(names, kind, shape, noise):
    from nerf_signature_amd.distortion import DistortionLayer
    layer = DistortionLayer(names, 3)
    layer._buffers(shape, torch.device(DEV))
    params = R.forced_parameters(kind, shape[0])
    layer.set_mixed(kind, noise=noise if kind == "noise" else None, **params)
    return layer, params


@pytest.mark.parametrize("names", [R.SETS["six"], FUSED_ONLY], ids=["six", "fused_only"])
@pytest.mark.parametrize("shape", SHAPES)
def test_layer_alone_is_bit_equal_to_the_single_kind(shape, names):
    """wm_distort_fwd / _bwd (and the resampling launch of a set that holds a geometric kind) under code 6 with every member forced in turn, against the
    existing single-kind operators holding the same parameters: values and the gradient with respect to the unclamped render, torch.equal."""
    raw = _raw(shape)
    noise = torch.from_numpy(np.random.RandomState(2).normal(0, math.sqrt(0.1), shape).astype(np.float32)).to(DEV)
    for kind in names:
        layer, params = _mixed_layer(names, kind, shape, noise)
        single = R.single_layer(kind, shape, torch.device(DEV), params, noise)
        a = raw.to(DEV).requires_grad_(True)
        out1 = layer(a.detach().clamp(0, 1), raw=a)
        b = raw.to(DEV).requires_grad_(True)
        out0 = torch.clamp(b, 0, 1) if single is None else single(b.detach().clamp(0, 1), raw=b)
        assert out1.shape == out0.shape and torch.equal(out1, out0), kind
        r = torch.from_numpy(np.random.RandomState(3).randn(*out0.shape).astype(np.float32)).to(DEV)
        (out1 * r).sum().backward()
        (out0 * r).sum().backward()
        assert float(b.grad.abs().max()) > 0 and torch.equal(a.grad, b.grad), kind


@pytest.mark.parametrize("names", [R.SETS["six"], FUSED_ONLY], ids=["six", "fused_only"])
@pytest.mark.parametrize("shape", SHAPES)
def test_fused_into_the_decoder_is_bit_equal_to_the_single_kind(shape, names):
    """decode_rendered forward + backward under code 6 with every member forced in turn, against the same call with the existing single-kind layer: decoded
    values, the clamped blocks, the image gradient and all 29 parameter gradients, torch.equal."""
    from nerf_signature_amd.hidden_models import get_hidden_decoder_multi_views
    torch.manual_seed(5)
    dec = get_hidden_decoder_multi_views(num_bits=1, redundancy=1, num_blocks=8, input_ch=3, channels=64).to(DEV)
    raw = _raw(shape)
    noise = torch.from_numpy(np.random.RandomState(2).normal(0, math.sqrt(0.1), shape).astype(np.float32)).to(DEV)
    msg = torch.from_numpy(np.random.RandomState(4).randint(0, 2, (shape[0], 1)).astype(np.float32)).to(DEV)

    def run(layer):
        for p in dec.parameters():
            p.grad = None
        a = raw.to(DEV).requires_grad_(True)
        decoded, pred = dec.decode_rendered(a, layer)
        torch.nn.functional.binary_cross_entropy_with_logits(decoded * 10.0, msg).backward()
        grads = [None if p.grad is None else p.grad.clone() for p in dec.parameters()]
        return decoded.detach().clone(), pred.detach().clone(), a.grad.clone(), grads

    for kind in names:
        layer, params = _mixed_layer(names, kind, shape, noise)
        single = R.single_layer(kind, shape, torch.device(DEV), params, noise)
        d1, p1, g1, w1 = run(layer)
        d0, p0, g0, w0 = run(single)
        assert torch.equal(p1, raw.to(DEV).clamp(0, 1)) and torch.equal(p1, p0), kind
        assert torch.equal(d1, d0), kind
        assert float(g0.abs().max()) > 0 and torch.equal(g1, g0), kind
        given = [w for w in w0 if w is not None]
        assert len(given) == 29 and len(w1) == len(w0)
        for x, y in zip(w1, w0):
            assert (x is None) == (y is None) and (x is None or torch.equal(x, y)), kind


@pytest.mark.parametrize("names", [("noise", "brightness", "blurring", "rotation"), R.FIVE], ids=["four", "five_with_scaling"])
def test_captured_loop_draws_the_kind_on_the_device_and_matches_the_eager_step(names):
    """GraphedWatermarkLoop(distortion=<set>), 12 replays with seed 69: by host_selector / host_uniform its first 12 selectors cover every member of both sets,
    every blur step draws a sigma of 0.30 or more (side tap 0.004 or more: a blur float32 can see -- a sigma under ~0.17 is the identity to it, and two such steps
    would share the undistorted loss whatever the code does) and the scaling steps of the 5-set replay two widths other than W.  Every replay's device-side selector
    is the host's; consecutive replays used different draws and (same message, learning rate zero) EVERY replay gave a different loss, as the single kinds are
    held to; an eager train_step fed each replay's draws reproduces
    its loss to the tolerance the single kinds are held to.  One capture serves every kind -- one per decoder width when the set holds scaling, the replayed
    width following the host selector -- and the captured step has the same number of graph nodes whichever kind the host last saw."""
    import test_gpu_render as T
    import test_gpu_twin as TW
    from nerf_signature_amd import trainer
    from nerf_signature_amd.distortion import KINDS, host_selector, kinds_mask, scaled_width, host_uniform
    from nerf_signature_amd.optim import CodebookAdam
    seed, steps = 69, 12
    expected = [host_selector(seed, k + 1, kinds_mask(names)) for k in range(steps)]      # (the opening kernel counts the replay before the step draws)
    assert set(expected) == {KINDS[n] for n in names}
    assert all(0.01 + 0.49 * host_uniform(seed, k + 1, 0.0, 1.0) >= 0.3 for k in range(steps) if expected[k] == 3)
    bo, bd, co, cd, gt = T._data(n_content=300)
    data = {"watermark": {"rays_o_block": bo.cuda(), "rays_d_block": bd.cuda()}, "content": {"rays_o": co.cuda(), "rays_d": cd.cuda(), "images": gt.cuda()}}
    torch.manual_seed(0)
    m, _, _ = T._model()
    opt = CodebookAdam(m.get_params(0.0), betas=(0.9, 0.99), eps=1e-15, fused=True, capturable=True)
    kw = dict(dt_gamma=0, max_steps=1024)
    loop = trainer.GraphedWatermarkLoop(m, opt, kw, data, distortion=names, distortion_seed=seed)
    msg = torch.from_numpy(np.random.RandomState(3).randint(0, 2, 32).astype(np.float32))
    W = bo.shape[2]
    losses, draws, captures, widths = [], [], set(), set()
    for k in range(steps):
        out = loop.step(msg)
        torch.cuda.synchronize()
        layer = loop.distortion
        losses.append(float(out[4].detach()))
        assert int(layer.param[:1].cpu().view(torch.int32)) == expected[k] == layer.selected
        width = layer.out_width(W)
        if expected[k] == 5:
            assert width == scaled_width(W, host_uniform(seed, k + 1, 0.75, 1.25)) and float(layer.param[3].cpu()) == float(torch.tensor(layer.factor, dtype=torch.float32))
        else:
            assert width == W
        assert loop.selected is loop.variants[width if "scaling" in names else None]["capture"]      # the replayed width follows the host selector
        captures.add(id(loop.selected))
        draws.append((layer.selected, layer.factor, layer.param.clone(), layer.noise.clone()))
        widths.add(width)
        assert not loop.overflowed()
    if "scaling" in names:
        assert sorted(loop.variants) == list(range(int(0.75 * W), int(1.25 * W - 1e-9) + 1)) and len(widths - {W}) == 2 and len(captures) == 3
    else:
        assert list(loop.variants) == [None] and len(captures) == 1
    assert all(not (torch.equal(draws[i][2], draws[i + 1][2]) and torch.equal(draws[i][3], draws[i + 1][3])) for i in range(steps - 1))
    # same message, same weights, different distortion: different loss -- every replay, no allowance (no scaling step of this seed has the width W)
    print("\nkinds", expected, "losses", [round(l, 6) for l in losses], "sigmas", {k: round(float(draws[k][2][2]), 4) for k in range(steps) if expected[k] == 3})
    assert len(set(round(l, 6) for l in losses)) == steps
    layer = loop.distortion
    nodes = []
    for seen in (None, KINDS["noise"], KINDS["rotation"]):       # the kind the host last saw changes nothing about what a step enqueues
        layer.selected = seen
        nodes.append(TW._graph_nodes(loop))
    assert len(set(nodes)) == 1, nodes
    loop.close()
    for k in range(steps):
        layer.selected, layer.factor = draws[k][0], draws[k][1]
        layer.param.copy_(draws[k][2])
        layer.noise.copy_(draws[k][3])
        eager = trainer.train_step(m, data, msg, kw, distortion=layer)
        np.testing.assert_allclose(float(eager[4].detach()), losses[k], rtol=1e-4, atol=1e-5, err_msg=f"replay {k}, kind {expected[k]}")


def test_robustness_training_one_mixed_model_against_the_undistorted_baseline():
    """Scene S0, the README schedule (1000 captured steps): one model trained with "none", one with "mixed", both evaluated by quality.robustness (the
    baseline twice, evaluation seeds 4321 and 4322).  For every kind the baseline reads under 0.99 -- the standing criterion for a trained distortion -- the
    mixed model must beat the baseline's better figure, and there must be such a kind.  Every other accuracy is a measurement."""
    from nerf_signature_amd import quality
    stage = quality.watermark_stage("hotdog")
    base_rec = quality.train(stage, None, "graphed", distortion="none")
    base = [quality.robustness(stage, seed=s, message_batch=16) for s in (4321, 4322)]
    del stage
    torch.cuda.empty_cache()
    stage = quality.watermark_stage("hotdog")
    mixed_rec = quality.train(stage, None, "graphed", distortion="mixed")
    mixed = quality.robustness(stage, seed=4321, message_batch=16)
    print("\nbaseline (none), evaluation seed 4321:", {k: round(v, 4) for k, v in base[0].items()})
    print("baseline (none), evaluation seed 4322:", {k: round(v, 4) for k, v in base[1].items()})
    print("mixed, evaluation seed 4321:           ", {k: round(v, 4) for k, v in mixed.items()})
    print(f"ms/step: none {base_rec['ms_per_step']:.3f}, mixed {mixed_rec['ms_per_step']:.3f}")
    assert not base_rec["overflowed"] and not mixed_rec["overflowed"]
    weak = [k for k in base[0] if min(base[0][k], base[1][k]) < 0.99]
    assert weak, "the undistorted baseline reads every kind at 0.99 or better: nothing to beat"
    for k in weak:
        assert mixed[k] > max(base[0][k], base[1][k]), (k, mixed[k], base[0][k], base[1][k])
