"""The clean twin on the GPU: field_fwd_twin against the two single launches it replaces and against float64, render(clean_twin=True) against the render
without a message, the orbit sampler against its float64 mirror (tests/orbit_ref.py) and rg_get_rays, a training step that renders its own target against
the same step fed the stored target, and the README schedule with online targets against the stored-image run."""
import ctypes
import math

import numpy as np
import pytest
import torch

import closed_form as cf
import mlp_ref as mr
import orbit_ref as orb
from test_gpu_render import _data, _model

pytestmark = pytest.mark.gpu

KW = dict(dt_gamma=0, max_steps=1024)
RENDER = dict(staged=False, bg_color=1, perturb=False, force_all_rays=True, **KW)
COUNTS = (1, 31, 32, 33, 127, 128, 129, 1025)
# every arithmetic and plane layout field_fwd serves the training render in: (MLP arithmetic, NERFSIG_HALF_PLANES) -> fp16 + mixed, fp16 + fp32 planes, split bf16 + fp32 planes
SETTINGS = [("f16", "1"), ("f16", "0"), ("bf16x3", "1")]
RAY_COUNTS = (1, 63, 64, 65, 257)


@pytest.fixture(scope="module")
def fo():
    from nerf_signature_amd import fieldops
    return fieldops


@pytest.fixture(scope="module")
def field():
    """Tables, weights, the walking-count points and the float64 clean reference of every row: computed once, never modified."""
    from nerf_signature_amd import fieldops as fo
    base_d = [torch.from_numpy(cf.table(l)).cuda() for l in range(16)]
    cb_d = [torch.from_numpy(cf.table(100 + l, scale=0.05)).cuda() for l in range(64)]
    sp, cp = torch.from_numpy(cf.mlp_params(3072, 1337)).cuda(), torch.from_numpy(cf.mlp_params(7168, 1338)).cuda()
    n = mr.walking_count(torch.cuda.get_device_properties(0).multi_processor_count)
    pts, dirs, _, _ = (t.cuda() for t in mr.case(n))
    S = fo.codebook_presum(fo.select_tables(cb_d, fo.message_bits(torch.from_numpy(cf.messages(32)[2]))))
    assert float(S.abs().max()) > 0           # a non-zero S: the two results differ
    W = mr.split_params(sp, cp)
    ref = mr.forward(fo.encode((pts + 1) / 2, base_d, None).double().cpu(), dirs.cpu(), W)          # the clean field: the features without the codebook
    return {"base": base_d, "S": S, "sp": sp, "cp": cp, "n": n, "pts": pts, "dirs": dirs, "W": W, "ref": ref,
            "bound": {a: mr.forward_chain_bound(ref, W, mr.U_OP[a]) for a in ("f16", "bf16x3")}}


@pytest.mark.parametrize("pipelined", [2, 3], ids=["plain_loop", "pipelined"])
@pytest.mark.parametrize("arith,half", SETTINGS, ids=["f16_mixed", "f16_f32planes", "bf16x3_f32planes"])
def test_twin_equals_the_two_single_launches_and_the_clean_half_is_within_the_chain_bound(fo, field, arith, half, pipelined, monkeypatch):
    """field_fwd_twin at every row count where a tile, a workgroup or a wave's walk ends: sigma, rgb and the ReLU masks are field_fwd's with S bit for bit; the clean
    sigma and rgb are field_fwd's with S = NULL over a plane set encoded without S bit for bit -- and within mlp_ref's forward-chain bound (unchanged) of the float64
    field without a codebook."""
    from nerf_signature_amd import _native as nv
    monkeypatch.setenv("NERFSIG_HALF_PLANES", half)
    prec, pipe = nv.fn("mlp_get_precision")(), nv.fn("mlp_get_pipelined")()
    nv.set_mlp_precision(arith)
    nv.call("mlp_set_pipelined", pipelined)
    try:
        assert fo.mixed_planes() == (arith == "f16" and half == "1")
        packed = fo.pack_weights(field["sp"], field["cp"])
        worst = {}
        for M in COUNTS + (field["n"],):
            pts, dirs = field["pts"][:M].contiguous(), field["dirs"][:M].contiguous()
            args = (pts, dirs, 1.0, field["base"])
            s, c, _, masks, s_clean, c_clean = fo.field_forward(*args, field["S"], packed, want_masks=True, planes=True, twin=True)
            s1, c1, _, masks1 = fo.field_forward(*args, field["S"], packed, want_masks=True, planes=True)
            s0, c0, _, _ = fo.field_forward(*args, None, packed, planes=True)
            torch.cuda.synchronize()
            assert not any(torch.isnan(t).any() for t in (s, c, s_clean, c_clean)), M
            assert torch.equal(s, s1) and torch.equal(c, c1) and torch.equal(masks, masks1), (M, "the watermarked half is not field_fwd with S")
            assert torch.equal(s_clean, s0) and torch.equal(c_clean, c0), (M, "the clean half is not field_fwd without S")
            assert M < 32 or not torch.equal(s_clean, s), (M, "S changed nothing: the case proves nothing")
            b = field["bound"][arith]
            worst[M] = max(mr.ratio(s_clean, field["ref"]["sigma"][:M], b["sigma"][:M]), mr.ratio(c_clean, field["ref"]["rgb"][:M], b["rgb"][:M]))
        print(f"\n{arith} half_planes={half} pipelined={pipelined}: largest clean error / chain bound per M " + ", ".join(f"{k}: {v:.4f}" for k, v in worst.items()))
        assert max(worst.values()) <= 1.0, worst
    finally:
        nv.call("mlp_set_pipelined", pipe)
        nv.call("mlp_set_precision", prec)


def test_clean_image_of_a_render_is_the_render_without_a_message(mlp_prec):
    """render(o, d, message, clean_twin=True): "clean_image" is the "image" of render(o, d, None) on the training path bit for bit, "image" is the render's
    without the flag, and no gradient flows through the clean image.  Off the training path the flag is refused with the reason."""
    m, _, _ = _model()
    _, _, co, cd, _ = _data(n_content=max(RAY_COUNTS))
    msg = torch.from_numpy(cf.messages(32)[1])
    for N in RAY_COUNTS:
        o, d = co[:, :N].contiguous().cuda(), cd[:, :N].contiguous().cuda()
        out = m.render(o, d, msg, clean_twin=True, **RENDER)
        plain = m.render(o, d, msg, **RENDER)
        with torch.no_grad():
            clean = m.render(o, d, None, **RENDER)
        assert set(out) == set(plain) | {"clean_image"} and out["clean_image"].shape == (1, N, 3)
        assert torch.equal(out["clean_image"], clean["image"]), N
        assert torch.equal(out["image"], plain["image"]) and torch.equal(out["weights_sum"], plain["weights_sum"]), N
        assert torch.equal(out["depth"].nan_to_num(nan=-1.0), plain["depth"].nan_to_num(nan=-1.0)), N          # (a ray that misses the box has depth NaN, as in the reference)
        assert out["image"].requires_grad and not out["clean_image"].requires_grad
    assert not torch.equal(out["clean_image"], out["image"])
    with pytest.raises(NotImplementedError, match="staged"):
        m.render(o, d, msg, clean_twin=True, **dict(RENDER, staged=True))
    with pytest.raises(ValueError, match="needs a message"):
        m.render(o, d, None, clean_twin=True, **RENDER)
    m.eval()
    with pytest.raises(NotImplementedError, match="terminates rays per field"):
        m.render(o, d, msg, clean_twin=True, **RENDER)


# ---- the orbit sampler ----------------------------------------------------------------------------------------------------------------------------------

ORBIT = dict(radius=3.2248, theta_range=(0.9, 1.3), phi_range=(0.0, 2 * math.pi))        # (cf.orbit_rays' camera distance: the ball scene fills the view)
SEED = (5 << 32) + 77                                                                     # above 2^32: both halves of the seed enter the hash


def _intr():
    return tuple(float(v) for v in cf.orbit_rays(1)[1])


@pytest.mark.parametrize("step", [0, 7, 2 ** 31 - 1])
def test_orbit_sampler_pose_rays_and_indices(step):
    """rg_sample_rays_orbit: pose_out within orbit_ref.pose_bound (the documented ulp error of sinf / cosf, derived there) of the float64 mirror, the pixel
    indices the mirror's, rays_o / rays_d bit for bit rg_get_rays fed pose_out and inds_out; another offset is another pose."""
    from nerf_signature_amd import _native as nv, rays
    intr, H, W = _intr(), 400, 400
    counter = torch.tensor([step], dtype=torch.int32, device="cuda")
    poses = {}
    for N in RAY_COUNTS:
        for offset in (1, 2):
            s = rays.OrbitRaySampler(intr, H, W, N, stride=3, offset=offset, seed=SEED, **ORBIT)
            o, d = torch.full((N, 3), float("nan"), device="cuda"), torch.full((N, 3), float("nan"), device="cuda")
            inds = torch.full((N,), -1, dtype=torch.int64, device="cuda")
            s.sample_into(counter, o, d, inds_out=inds)
            pose = s.pose.clone()
            want = orb.pose(SEED, step, 3, offset, ORBIT["radius"], ORBIT["theta_range"], ORBIT["phi_range"])
            err = float(np.abs(pose.double().cpu().numpy() - want).max())
            assert err <= orb.pose_bound(ORBIT["radius"]), (N, offset, err, orb.pose_bound(ORBIT["radius"]))
            assert np.array_equal(inds.cpu().numpy(), orb.pixel_indices(SEED, step, N, H, W))
            ro, rd = torch.empty(1, N, 3, device="cuda"), torch.empty(1, N, 3, device="cuda")
            nv.call("rg_get_rays", nv.ptr(pose.view(1, 4, 4)), *intr, H, W, nv.ptr(inds.view(1, N)), 1, N, nv.ptr(ro), nv.ptr(rd), nv.stream())
            assert torch.equal(ro[0], o) and torch.equal(rd[0], d), (N, offset)
            poses.setdefault(offset, pose)
            assert torch.equal(poses[offset], pose)            # the pose does not depend on the ray count
    assert not torch.equal(poses[1], poses[2])
    # no counter: step 0
    s = rays.OrbitRaySampler(intr, H, W, 4, seed=SEED, **ORBIT)
    o, d = torch.empty(4, 3, device="cuda"), torch.empty(4, 3, device="cuda")
    s.sample_into(None, o, d)
    assert np.abs(s.pose.double().cpu().numpy() - orb.pose(SEED, 0, 1, 0, ORBIT["radius"], ORBIT["theta_range"], ORBIT["phi_range"])).max() <= orb.pose_bound(ORBIT["radius"])


# ---- a step that renders its own target ------------------------------------------------------------------------------------------------------------------

# 1000 content rays: their sample buffer is past fieldops.PLANES_MIN_POINTS, so the step on stored images reads a plane set too (as the bench-size step does, at 0.125 M
# points) and the node counts compare like with like -- below that size field_fwd gathers inside the MLP kernel, a route the twin does not have (it needs plane 16 apart)
N_CONTENT, STEPS = 1000, 20


def _messages(n):
    return [torch.from_numpy(np.random.RandomState(40 + s).randint(0, 2, 32).astype(np.float32)) for s in range(n)]


def _watermark():
    bo, bd, _, _, _ = _data(n_content=8)
    return {"rays_o_block": bo.cuda(), "rays_d_block": bd.cuda()}


def _sampler():
    from nerf_signature_amd import rays
    return rays.OrbitRaySampler(_intr(), 400, 400, N_CONTENT, seed=SEED, **ORBIT)


def _trained(m):
    return [e.weight.detach().clone() for e in m.msg_encoder.embeddings] + [p.detach().clone() for p in m.msg_decoder.parameters()]


def _stored_batches(sampler, first, n):
    """The batches the sampler draws at counters first .. first + n - 1 with the target the reference's pre-pass would have stored for them: the clean model's render
    of the same rays (a second, identical model: nothing the step trains enters a render without a message)."""
    clean, _, _ = _model()
    out, counter = [], torch.zeros(1, dtype=torch.int32, device="cuda")
    for k in range(first, first + n):
        counter.fill_(k)
        o, d = torch.empty(1, N_CONTENT, 3, device="cuda"), torch.empty(1, N_CONTENT, 3, device="cuda")
        sampler.sample_into(counter, o, d)
        with torch.no_grad():
            gt = clean.render(o, d, None, **RENDER)["image"]
        out.append({"rays_o": o, "rays_d": d, "images": gt.clone()})
    return out


def _hip_runtime():
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return ctypes.CDLL(line.split()[-1])
    raise RuntimeError("libamdhip64 is not mapped into this process")


def _graph_nodes(loop):
    """Nodes of one captured step: the loop's step captured once more into a graph that keeps its hipGraph_t (never replayed: a capture runs nothing)."""
    loop.optimizer.zero_grad(set_to_none=True)
    g = torch.cuda.CUDAGraph(keep_graph=True)
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=loop._capture_stream, capture_error_mode="thread_local"):
        loop._captured_step()
    loop._segment_ended()
    n = ctypes.c_size_t(0)
    hip = _hip_runtime()
    hip.hipGraphGetNodes.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_size_t)]
    assert hip.hipGraphGetNodes(ctypes.c_void_p(g.raw_cuda_graph()), None, ctypes.byref(n)) == 0
    nodes = (ctypes.c_void_p * n.value)()
    assert hip.hipGraphGetNodes(ctypes.c_void_p(g.raw_cuda_graph()), nodes, ctypes.byref(n)) == 0
    hip.hipGraphNodeGetType.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)]
    kinds = {}
    for node in nodes:
        t = ctypes.c_int(-1)
        assert hip.hipGraphNodeGetType(ctypes.c_void_p(node), ctypes.byref(t)) == 0
        kinds[t.value] = kinds.get(t.value, 0) + 1
    print(f"\nnode kinds (hipGraphNodeType: 0 kernel, 1 memcpy, 2 memset, 6 empty): {dict(sorted(kinds.items()))}")
    return int(n.value)


def _captured_run(online, batches=None, store=None):
    from nerf_signature_amd import trainer
    from nerf_signature_amd.optim import CodebookAdam
    torch.manual_seed(0)
    m, _, _ = _model()
    opt = CodebookAdam(m.get_params(1e-2), betas=(0.9, 0.99), eps=1e-15, capturable=True)
    msgs = _messages(STEPS + 1)
    content = {k: torch.zeros(1, N_CONTENT, 3, device="cuda") for k in (("rays_o", "rays_d") if online else ("rays_o", "rays_d", "images"))}
    sampler = store if store is not None else (_sampler() if online else None)
    if sampler is not None:
        sampler.sample_into(torch.ones(1, dtype=torch.int32, device="cuda"), content["rays_o"], content["rays_d"], content.get("images"))      # (sizes the capacity)
    else:
        for k, v in batches[0].items():
            content[k].copy_(v)
    # content_headroom: a new camera every step -- the sample total moves with the view; twice the first batch's keeps every replay inside the buffers
    loop = trainer.GraphedWatermarkLoop(m, opt, KW, {"watermark": _watermark(), "content": content}, content_sampler=sampler, content_headroom=1.0)
    return m, loop, msgs


def test_captured_step_with_orbit_sampler_equals_the_same_step_fed_the_stored_target(monkeypatch):
    """20 replays of GraphedWatermarkLoop(content_sampler=OrbitRaySampler), which draws its camera and renders its own target inside the graph, against the same loop
    fed, step by step, the rays the sampler draws at the same counters and as `images` render(o, d, None) of them made under no_grad outside the step -- the existing
    train_step on stored images.  One loop class on both sides: the captured and the eager loop differ in their optimiser launches and agree to 2e-3
    (test_graphed_loop_matches_eager_loop), which would hide what is compared here -- where the rays and the target come from; that must change NOTHING: every codebook table and
    decoder parameter torch.equal, the three losses of every step equal, no overflow.  The captured step has exactly one node more than the step with a
    DeviceRaySampler store: the compositing of the clean image.
    NERFSIG_DETERMINISTIC=1: at these sizes (fewer than 65 536 points per render) the default record scatter adds G with float atomics and two runs of ONE binary differ
    by an ulp (switches.py); through the fixed-point slice owners a run is bit-reproducible and torch.equal decides."""
    monkeypatch.setenv("NERFSIG_DETERMINISTIC", "1")
    m1, loop1, msgs = _captured_run(True)
    losses1 = []
    for k in range(STEPS):
        out = loop1.step(msgs[k], next_message=msgs[k + 1])
        losses1.append(torch.stack([out[3], out[4], out[5]]).detach().clone())
    assert not loop1.overflowed() and len(loop1.segments) == 1
    from nerf_signature_amd import fieldops
    assert loop1.content_capacity >= fieldops.PLANES_MIN_POINTS, loop1.content_capacity
    assert "images" not in loop1.data["content"]
    got = _trained(m1)
    batches = _stored_batches(_sampler(), 1, STEPS)          # (the opening kernel counts the replay before the sampler reads the counter: step k draws at k + 1)
    n_online = _graph_nodes(loop1)
    loop1.close()

    m2, loop2, _ = _captured_run(False, batches)
    losses2 = []
    for k in range(STEPS):
        out = loop2.step(msgs[k], data={"content": batches[k]}, next_message=msgs[k + 1])
        losses2.append(torch.stack([out[3], out[4], out[5]]).detach().clone())
    assert not loop2.overflowed()
    want = _trained(m2)
    loop2.close()
    assert torch.equal(torch.stack(losses1), torch.stack(losses2)), (torch.stack(losses1) - torch.stack(losses2)).abs().max(0)
    assert float(torch.stack(losses1)[:, 0].max()) > 0              # the image loss is not trivially zero: the message moves the image
    unequal = [i for i, (a, b) in enumerate(zip(got, want)) if not torch.equal(a, b)]
    assert len(got) > 64 and not unequal, unequal[:8]
    moved = sum(1 for a, l in zip(got[:64], range(64)) if not torch.equal(a.cpu(), torch.from_numpy(cf.table(100 + l, scale=0.05))))
    assert moved == 64                                               # 20 random messages select every table: all of them trained

    # node count: the step with a store sampler (ground truth gathered by the sampler's launch) + the clean image's compositing launch, nothing else
    from nerf_signature_amd import rays
    poses = torch.from_numpy(np.stack([cf.orbit_rays(1)[0]] * 2)).cuda()
    store = rays.DeviceRaySampler(poses, torch.rand(2, 400 * 400, 3, device="cuda"), _intr(), 400, 400, N_CONTENT, seed=SEED)
    _, loop3, _ = _captured_run(False, store=store)
    loop3.prepare(msgs[0])
    n_stored = _graph_nodes(loop3)
    loop3.close()
    print(f"\ngraph nodes of one captured step: store sampler {n_stored}, orbit sampler with online target {n_online}")
    assert n_online == n_stored + 1 and n_stored > 5


def test_captured_orbit_loop_tracks_the_eager_train_step_sequence(monkeypatch):
    """The comparison in the form the captured loop has always been held to the eager one (test_graphed_loop_matches_eager_loop): captured steps of
    GraphedWatermarkLoop(content_sampler=OrbitRaySampler) against an EAGER sequence -- the same rays drawn with the sampler, gt = render(o, d, None) under no_grad, the
    existing train_step on those images inside WatermarkLoop.  The two loops run different optimiser launches (opt_codebook_adam_sel with a tensor learning rate against
    opt_codebook_adam) and Adam with eps = 1e-15 turns last-bit differences of tiny gradients into +-lr steps, so they agree as that test states it, over the four steps
    its tolerances were set for: every loss within rtol 2e-3 / atol 2e-4, per-table Adam step counts equal, the codebook's movement within 5 % in aggregate, the decoder
    within 5 %.  (Bit equality is decided in the test above, where both sides are the captured loop.)"""
    monkeypatch.setenv("NERFSIG_DETERMINISTIC", "1")
    from nerf_signature_amd import trainer
    from nerf_signature_amd.optim import CodebookAdam
    steps = 4
    m1, loop1, msgs = _captured_run(True)
    held = []
    for k in range(steps):
        out = loop1.step(msgs[k], next_message=msgs[k + 1])
        held.append(torch.stack([out[3], out[4], out[5]]).detach().clone())
    assert not loop1.overflowed()
    losses1, got = torch.stack(held).cpu().numpy(), _trained(m1)
    counts1 = [float(loop1.optimizer.state[e.weight]["step"]) if len(loop1.optimizer.state[e.weight]) else 0.0 for e in m1.msg_encoder.embeddings]
    loop1.close()

    batches = _stored_batches(_sampler(), 1, steps)          # (captured step k draws at counter k + 1)
    torch.manual_seed(0)
    m2, _, _ = _model()
    opt = CodebookAdam(m2.get_params(1e-2), betas=(0.9, 0.99), eps=1e-15)
    loop2 = trainer.WatermarkLoop(m2, opt, KW)
    wm, held = _watermark(), []
    for k in range(steps):
        out = loop2.step({"watermark": wm, "content": batches[k]}, msgs[k])
        held.append(torch.stack([out[3], out[4], out[5]]).detach().clone())
    torch.cuda.synchronize()
    losses2, want = torch.stack(held).cpu().numpy(), _trained(m2)
    counts2 = [float(opt.state[e.weight]["step"]) if len(opt.state[e.weight]) else 0.0 for e in m2.msg_encoder.embeddings]
    print(f"\ncaptured orbit loop against the eager sequence, {steps} steps: largest |loss difference| per loss (image, watermark, total) {np.abs(losses1 - losses2).max(0)}")
    np.testing.assert_allclose(losses1, losses2, rtol=2e-3, atol=2e-4)
    assert counts1 == counts2 and sum(counts1) == steps * 32
    start = [torch.from_numpy(cf.table(100 + l, scale=0.05)).cuda() for l in range(64)]
    num = sum(float((a - b).pow(2).sum()) for a, b in zip(got[:64], want[:64])) ** 0.5
    den = sum(float((b - c).pow(2).sum()) for b, c in zip(want[:64], start)) ** 0.5
    d1, d2 = torch.cat([t.reshape(-1) for t in got[64:]]), torch.cat([t.reshape(-1) for t in want[64:]])
    print(f"codebook difference / movement {num / den:.4f}, decoder difference / norm {float((d1 - d2).norm() / d2.norm()):.4f}")
    assert den > 0 and num / den < 0.05
    assert float((d1 - d2).norm() / d2.norm()) < 0.05


def test_captured_loop_accepts_a_pose_list_sampler_without_images():
    """GraphedWatermarkLoop(content_sampler=DeviceRaySampler(poses, None, ...)) with a content part that has no image buffer: the pose-list variant of online
    targets.  Three replays; the step's gt_rgb is the clean render of the rays its sampler drew, bit for bit; no overflow; no "images" anywhere."""
    from nerf_signature_amd import rays
    poses = torch.from_numpy(np.stack([orb.pose(SEED, k, 1, 0, ORBIT["radius"], ORBIT["theta_range"], ORBIT["phi_range"]).astype(np.float32) for k in range(3)])).cuda()
    store = rays.DeviceRaySampler(poses, None, _intr(), 400, 400, N_CONTENT, seed=SEED)
    assert store.images is None
    m, loop, msgs = _captured_run(True, store=store)
    for k in range(3):
        out = loop.step(msgs[k], next_message=msgs[k + 1])
    assert not loop.overflowed() and "images" not in loop.data["content"]
    gt, pred = out[1].detach().clone(), out[2].detach().clone()
    o, d = loop.data["content"]["rays_o"].clone(), loop.data["content"]["rays_d"].clone()
    loop.close()
    clean, _, _ = _model()
    with torch.no_grad():
        want = clean.render(o, d, None, **RENDER)["image"]
    assert gt.shape == (1, N_CONTENT, 3) and torch.equal(gt, want) and not torch.equal(gt, pred)
    # the drawn rays are the store's third-replay pose (counter 3 mod 3 = pose 0)
    ro = torch.empty(1, N_CONTENT, 3, device="cuda")
    store.sample_into(torch.full((1,), 3, dtype=torch.int32, device="cuda"), ro, torch.empty(1, N_CONTENT, 3, device="cuda"))
    assert torch.equal(ro, o)


@pytest.mark.parametrize("overlap", [False, True], ids=["one_stream", "side_stream"])
def test_eager_loop_without_images_equals_the_same_loop_fed_the_stored_target(overlap, monkeypatch):
    """The same comparison for WatermarkLoop, with the content render on the main stream and on a side stream (NERFSIG_DETERMINISTIC=1, as above)."""
    monkeypatch.setenv("NERFSIG_DETERMINISTIC", "1")
    from nerf_signature_amd import trainer
    from nerf_signature_amd.optim import CodebookAdam
    msgs, sampler = _messages(STEPS), _sampler()
    batches = _stored_batches(sampler, 0, STEPS)
    runs = []
    for online in (True, False):
        torch.manual_seed(0)
        m, _, _ = _model()
        opt = CodebookAdam(m.get_params(1e-2), betas=(0.9, 0.99), eps=1e-15)
        loop = trainer.WatermarkLoop(m, opt, KW, side_stream=torch.cuda.Stream() if overlap else None)
        wm, losses = _watermark(), []
        for k in range(STEPS):
            content = {n: v for n, v in batches[k].items() if not (online and n == "images")}
            out = loop.step({"watermark": wm, "content": content}, msgs[k])
            losses.append(torch.stack([out[3], out[4], out[5]]).detach().clone())
            if online:
                assert torch.equal(out[1], batches[k]["images"]) and not out[1].requires_grad      # gt_rgb: the clean twin IS the stored target
        torch.cuda.synchronize()
        runs.append((torch.stack(losses), _trained(m)))
    assert torch.equal(runs[0][0], runs[1][0])
    unequal = [i for i, (a, b) in enumerate(zip(runs[0][1], runs[1][1])) if not torch.equal(a, b)]
    assert not unequal, unequal[:8]


def test_readme_schedule_with_online_targets_learns_like_the_stored_image_run():
    """quality.run over the README schedule (1000 steps, lambda_w 0.005, lr 1e-2 decayed), once with the stage's stored clean views and once with
    online_targets=True (no pre-pass, a new orbit camera every step, the target rendered inside the step): the bars tests/test_gpu_convergence.py puts on the
    captured mode -- bit accuracy >= 1 - 1/32 and within 1/32 of the stored-image run, PSNR of watermarked against clean held-out views within 2 dB of it."""
    from nerf_signature_amd import quality
    stored = quality.run("graphed")
    torch.cuda.empty_cache()
    online = quality.run("graphed", online_targets=True)
    stage = quality.LAST_STAGE
    assert stage["clean"] is None and stage["poses"] is None            # no pre-pass, no store
    print(f"\nstored images: bit acc {stored['bit_acc']:.5f}, PSNR {stored['psnr_db']:.3f} dB, {stored['train_ms_per_step']:.3f} ms/step; "
          f"online targets: bit acc {online['bit_acc']:.5f}, PSNR {online['psnr_db']:.3f} dB, {online['train_ms_per_step']:.3f} ms/step")
    for r in (stored, online):
        assert 0.35 < r["bit_acc_before_training"] < 0.65
        assert r["bit_acc"] >= 1.0 - 1.0 / 32, r["bit_acc"]
        assert not r["overflowed"] and r["recaptures"] == 0
    assert abs(online["bit_acc"] - stored["bit_acc"]) <= 1.0 / 32
    assert abs(online["psnr_db"] - stored["psnr_db"]) < 2.0, (online["psnr_db"], stored["psnr_db"])
