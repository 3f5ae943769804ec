"""The mixed distortion layer without a GPU: the host's statement of the device-side selector as a pure function, the layer on the CPU against the stock
operators of the selected kind, the accepted spellings of a set, and the native refusals word for word (they are raised before any launch)."""
import ctypes
import math

import pytest
import torch

import mixed_distortion_ref as R


@pytest.mark.parametrize("which", ["five", "two", "six"])
def test_host_selector_is_uniform_over_the_set_and_never_leaves_it(which):
    """Seeds 0, 1 and 2^32 + 5, steps 0 .. 3999: every member within 5 sigma of Binomial(4000, 1 / n) of its expected count (the function is deterministic: these
    seeds were checked to lie inside the bound), nothing outside the mask ever, and the same answer when asked again."""
    from nerf_signature_amd.distortion import KINDS, host_selector, kinds_mask
    names = R.SETS[which]
    mask = kinds_mask(names)
    expected, bound = R.count_bound(len(names))
    assert bound == {"five": 127, "two": 159, "six": 118}[which]
    for seed in R.SEEDS:
        picks = [host_selector(seed, step, mask) for step in range(R.STEPS)]
        counts = {KINDS[n]: picks.count(KINDS[n]) for n in names}
        print(which, seed, counts)
        assert sum(counts.values()) == R.STEPS                                   # a kind outside the mask is never selected
        assert all(abs(c - expected) <= bound for c in counts.values()), counts
        assert picks[:64] == [host_selector(seed, step, mask) for step in range(64)]
    assert [host_selector(0, s, mask) for s in range(32)] != [host_selector(1, s, mask) for s in range(32)]
    for bad in (0, 64, 1 << 8):
        with pytest.raises(ValueError):
            host_selector(0, 0, bad)


def test_host_selector_is_independent_of_the_parameter_word():
    """The selector comes from a sequence of its own: over the steps that select brightness in a 5-set, the brightness factor (host_uniform of the same key) still
    covers its whole range -- not the fifth of it a selector cut from the same word would leave."""
    from nerf_signature_amd.distortion import host_selector, host_uniform, kinds_mask
    mask = kinds_mask(R.FIVE)
    u = [host_uniform(0, s, 0.0, 1.0) for s in range(R.STEPS) if host_selector(0, s, mask) == 2]
    assert min(u) < 0.02 and max(u) > 0.98 and abs(sum(u) / len(u) - 0.5) < 0.05


def test_spellings_of_a_set():
    from nerf_signature_amd.distortion import DistortionLayer
    a, b, c = DistortionLayer(("blurring", "noise")), DistortionLayer("noise+blurring"), DistortionLayer(["noise", "blurring"])
    assert a.mixed and a.kinds == b.kinds == c.kinds == ("noise", "blurring") and a.mask == b.mask == 0b1010 and a.kind == 6
    m = DistortionLayer("mixed", 5)
    assert m.kinds == R.FIVE and m.mask == 0b111110 and m.name == "mixed" and m.seed == 5
    assert DistortionLayer(("none", "rotation")).mask == 0b10001
    for bad in ((), ("noise", "noise"), "noise+jpeg", ("crop",)):
        with pytest.raises(ValueError):
            DistortionLayer(bad)
    single = DistortionLayer("blurring")                                          # single names keep what they were
    assert not single.mixed and single.kind == 3 and single.code == 3 and single.fused and not single.geometric


@pytest.mark.parametrize("shape", [(5, 9, 14, 3), (4, 2, 2, 3)])
def test_mixed_layer_on_the_cpu_is_the_selected_kinds_stock_operators(shape):
    from nerf_signature_amd.distortion import KINDS, DistortionLayer, reference_ops
    torch.manual_seed(0)
    x = torch.rand(shape)
    noise = 0.3 * torch.randn(shape)
    layer = DistortionLayer(R.SETS["six"], 3)
    layer._buffers(shape, x.device)
    for kind in R.SETS["six"]:
        p = R.forced_parameters(kind, shape[0])
        layer.set_mixed(kind, noise=noise if kind == "noise" else None, **p)
        assert layer.selected == KINDS[kind] and int(layer.param[:1].view(torch.int32)) == KINDS[kind]
        out = layer(x)
        single = R.single_layer(kind, shape, x.device, p, noise)
        want = x if kind == "none" else reference_ops(x, kind, single.param if kind != "scaling" else single.factor, single.noise)
        assert torch.equal(out, want), kind
        assert layer.out_width(shape[2]) == (single.out_width(shape[2]) if single is not None else shape[2])
        assert layer.fused == (kind != "scaling") and layer.geometric          # (the set holds rotation: its launch is always there)
        if kind != "rotation":                                                    # an unselected rotation is exactly (1, 0) per image
            assert torch.equal(layer.param[4:].reshape(-1, 2), torch.tensor([[1.0, 0.0]]).expand(shape[0], 2))
    other = DistortionLayer(("noise", "blurring"))
    other._buffers(shape, x.device)
    with pytest.raises(ValueError):
        other.set_mixed("rotation", radians=[0.0] * shape[0])                     # no member of that set


def test_the_eager_draw_picks_with_one_randint_then_draws_like_the_single_kind():
    """draw(): torch.randint from the layer's host generator picks the kind; the kind's own draw follows from the same generator -- replayed here by hand."""
    from nerf_signature_amd.distortion import DistortionLayer, NAMES
    shape = (3, 5, 6, 3)
    layer = DistortionLayer(("brightness", "blurring", "scaling", "none"), 9)
    gen = torch.Generator(device="cpu").manual_seed(9)
    seen = set()
    for _ in range(24):
        layer.draw(shape, torch.device("cpu"))
        kind = layer.kinds[int(torch.randint(4, (1,), generator=gen))]
        assert NAMES[layer.selected] == kind
        seen.add(kind)
        if kind == "brightness":
            assert float(layer.param[1]) == float(torch.tensor(float(torch.empty(1).uniform_(0.5, 1.5, generator=gen))))
        elif kind == "blurring":
            assert float(layer.param[2]) == float(torch.tensor(float(torch.empty(1).uniform_(0.01, 0.5, generator=gen))))
        elif kind == "scaling":
            assert layer.factor == torch.empty(1).uniform_(0.75, 1.25, generator=gen).item()
    assert seen == set(layer.kinds)


@pytest.mark.parametrize("spec", [("brightness", "blurring", "none"), ["brightness", "blurring", "none"], "brightness+blurring+none"])
def test_the_bound_train_step_keeps_one_layer_and_one_generator_across_steps(spec, monkeypatch):
    """reference_trainer_train_step with self.distortion a tuple, a list (rebuilt by value every step) or a string: consecutive steps hand train_step the SAME
    layer, whose draws continue one generator's sequence -- replayed here by hand -- and do not restart it."""
    import types
    from nerf_signature_amd import trainer
    from nerf_signature_amd.distortion import NAMES
    handed = []
    monkeypatch.setattr(trainer, "train_step", lambda *a, distortion=None, **k: handed.append((distortion, distortion.selected, distortion.param.clone())))
    me = types.SimpleNamespace(model=types.SimpleNamespace(bg_radius=0), opt=types.SimpleNamespace(), lambda_w=1.0, lambda_i=1.0, distortion=spec)
    data = {"watermark": {"rays_o_block": torch.zeros(3, 4, 5, 3), "rays_d_block": torch.zeros(3, 4, 5, 3)}}
    for _ in range(16):
        if isinstance(spec, list):
            me.distortion = list(spec)                                            # an equal list, another object
        trainer.reference_trainer_train_step(me, data, torch.zeros(4))
    assert all(h[0] is handed[0][0] for h in handed)
    gen = torch.Generator(device="cpu").manual_seed(0)
    kinds = handed[0][0].kinds
    for _, selected, block in handed:
        kind = kinds[int(torch.randint(len(kinds), (1,), generator=gen))]
        assert NAMES[selected] == kind
        if kind == "brightness":
            assert float(block[1]) == float(torch.tensor(float(torch.empty(1).uniform_(0.5, 1.5, generator=gen))))
        elif kind == "blurring":
            assert float(block[2]) == float(torch.tensor(float(torch.empty(1).uniform_(0.01, 0.5, generator=gen))))
    assert len({h[1] for h in handed}) == 3                                       # (not one kind for ever)
    me.distortion = ("brightness", "none")                                        # another set: another layer
    trainer.reference_trainer_train_step(me, data, torch.zeros(4))
    assert handed[-1][0] is not handed[0][0] and handed[-1][0].kinds == ("none", "brightness")


def _fake(n=1):
    return ctypes.c_void_p(4096 * n)      # a non-null address nobody reads: every refusal below comes before a launch


def test_native_refusals_word_for_word():
    from nerf_signature_amd import _native as nv
    from nerf_signature_amd.distortion import kinds_mask
    code = lambda names, n=4: 6 | kinds_mask(names) << 8 | n << 16
    mean, std = (ctypes.c_float * 3)(0.5, 0.5, 0.5), (ctypes.c_float * 3)(0.2, 0.2, 0.2)

    def refused(name, *args):
        with pytest.raises(ValueError) as e:
            nv.call(name, *args)
        return str(e.value).split(": ", 1)[1]

    empty = "the mixed distortion's set is empty or holds bits beyond the kinds 0..5"
    block = "the mixed distortion needs its parameter block (dist_param)"
    noise = "the mixed distortion's set holds noise: it needs the noise tensor (dist_noise)"
    blur = "the mixed distortion's set holds the blur: H and W must be at least 2"
    fwd = lambda c, p, n, H=4, W=4: refused("dec_forward_train", _fake(), mean, std, _fake(2), 4, 3, H, W, 1e-3, _fake(3), _fake(4), _fake(5), c, p, n, None, 0.0, 0.0, None, None)
    bwd = lambda c, p, n, s, H=4, W=4: refused("dec_backward_train", _fake(), _fake(2), mean, std, _fake(3), 4, 3, H, W, _fake(4), _fake(5), _fake(6), c, p, n, s, None, None)
    lone = lambda f, c, p, n, H=4, W=4: refused(f, _fake(), *((_fake(2),) if f == "wm_distort_bwd" else ()), 4, H, W, 3, c, p, n, _fake(3), None)
    for who, call in (("dec_forward_train", fwd), ("dec_backward_train", lambda c, p, n, **k: bwd(c, p, n, _fake(7), **k)),
                      ("wm_distort_fwd", lambda c, p, n, **k: lone("wm_distort_fwd", c, p, n, **k)), ("wm_distort_bwd", lambda c, p, n, **k: lone("wm_distort_bwd", c, p, n, **k))):
        assert call(6, _fake(8), _fake(9)) == f"{who}: {empty}"                                  # an empty mask
        assert call(6 | 0x40 << 8, _fake(8), _fake(9)) == f"{who}: {empty}"                      # a bit beyond the six kinds
        assert call(code(("brightness", "blurring")), None, None) == f"{who}: {block}"
        assert call(code(("noise", "brightness")), _fake(8), None) == f"{who}: {noise}"
        assert call(code(("noise", "blurring")), _fake(8), _fake(9), H=1, W=7) == f"{who}: {blur}"
        assert call(code(("noise", "blurring")), _fake(8), _fake(9), H=7, W=1) == f"{who}: {blur}"
    assert bwd(code(("brightness", "rotation")), _fake(8), None, None) == "dec_backward_train: the mixed distortion's image gradient goes through the scratch image (grad_scratch)"
    draw = lambda c, n_noise, p, n: refused("wm_distort_draw", c, 7, None, n_noise, p, n, None)
    assert draw(6 | 4 << 16, 0, _fake(), None) == f"wm_distort_draw: {empty}"
    assert draw(6 | 0x80 << 8 | 4 << 16, 0, _fake(), None) == f"wm_distort_draw: {empty}"
    assert draw(code(("brightness",)), 0, None, None) == f"wm_distort_draw: {block}"
    assert draw(code(("noise", "brightness")), 16, _fake(), None) == f"wm_distort_draw: {noise}"
    assert draw(code(("noise", "brightness")), 0, _fake(), _fake(2)) == "wm_distort_draw: the mixed distortion's set holds noise: n_noise = the noise tensor's element count"
    assert draw(code(("rotation",), 0), 0, _fake(), None) == "wm_distort_draw: the mixed distortion's set holds rotation: the code carries the number of images (NSIG_DISTORT_MIXED_CODE)"


def test_robustness_asks_test_bitacc_once_per_kind(monkeypatch):
    from nerf_signature_amd import quality
    asked = []
    monkeypatch.setattr(quality, "test_bitacc", lambda stage, n, seed, distortion="none", message_batch=None: (asked.append((n, seed, distortion)), (0.5, 0.0, 0))[1])
    out = quality.robustness({}, n_messages=7, seed=11)
    assert list(out) == ["none", "noise", "brightness", "blurring", "rotation", "scaling"] and set(out.values()) == {0.5}
    assert asked == [(7, 11, k) for k in out]
