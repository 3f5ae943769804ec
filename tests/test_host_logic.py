"""CPU tests of the host-side mirror: synthetic inputs, message handling, module surface, meters, DP exchange."""
import os

import numpy as np
import pytest
import torch

import closed_form as cf
from oracle import field_ref as fr
from oracle import raymarch_ref as orm

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_synthetic_morton_and_scene_match_the_oracle():
    from nerf_signature_amd import synthetic
    c = np.random.RandomState(0).randint(0, 128, size=(4096, 3))
    np.testing.assert_array_equal(synthetic.morton3d_np(c), orm.morton3D(c.astype(np.int32)))
    grid = synthetic.density_grid(1.0)
    ref_grid, ref_bits, C = cf.ball_scene(1.0)
    np.testing.assert_array_equal(grid, ref_grid)
    bits, thresh = synthetic.pack_bits_np(grid, 10.0)
    np.testing.assert_array_equal(bits, ref_bits)
    g2 = synthetic.density_grid(2.0)
    assert g2.shape == (2, 128 ** 3) and g2[1].sum() > g2[0].sum() > 0


def test_get_rays_matches_reference_golden():
    from nerf_signature_amd import synthetic
    g = np.load(os.path.join(G, "g7_get_rays.npz"))
    o, d = synthetic.get_rays(torch.from_numpy(g["pose"])[None], g["intrinsics"], 400, 400, torch.from_numpy(g["inds"])[None])
    np.testing.assert_array_equal(o[0].numpy(), g["rays_o"])
    np.testing.assert_allclose(d[0].numpy(), g["rays_d"], rtol=0, atol=1e-7)


def test_block_and_content_rays_shapes():
    from nerf_signature_amd import synthetic
    bo, bd = synthetic.block_rays("hotdog")
    assert bo.shape == (32, 12, 12, 3) and bd.shape == (32, 12, 12, 3)
    o, d = synthetic.content_rays("hotdog", 4096, seed=3)
    assert o.shape == (1, 4096, 3) and torch.allclose(d.norm(dim=-1), torch.ones(1, 4096), atol=1e-5)
    o2, _ = synthetic.content_rays("hotdog", 4096, seed=4)
    assert not torch.equal(o, o2)          # ranks draw different cameras / pixels
    bo48, _ = synthetic.block_rays("fern")
    assert bo48.shape == (48, 11, 15, 3)   # LLFF/fern: 756x1008 image, 64x64 block grid


def test_message_bits_and_table_selection():
    from nerf_signature_amd import fieldops as fo
    msg = torch.tensor([1., 0., 0., 1.])
    assert fo.message_bits(msg) == (1, 0, 0, 1) and fo.message_bits(None) is None and fo.message_bits([0, 1]) == (0, 1)
    tables = list(range(8))
    assert fo.select_tables(tables, (1, 0, 0, 1)) == [1, 2, 4, 7]       # table 2i + bit_i
    with pytest.raises(ValueError):
        fo.select_tables(tables, (1, 0, 0))


def test_network_surface_and_state_dict_contract():
    from nerf_signature_amd.network import NeRFNetwork
    g = np.load(os.path.join(G, "g8_g9_glue.npz"))
    m = NeRFNetwork(bound=1.0, cuda_ray=True, density_scale=1, min_near=0.2, density_thresh=10, bg_radius=-1, message_dim=32, n_views=1)
    keys = sorted(m.state_dict().keys())
    assert keys == list(g["state_dict_keys"])
    assert [str(tuple(m.state_dict()[k].shape)) for k in keys] == list(g["state_dict_shapes"])
    groups = m.get_params(1e-2)
    assert len(groups) == 2 and len(list(groups[0]["params"])) == 64            # codebook, then decoder (network_wtmk_tcnn.py:185-188)
    assert sum(p.numel() for p in m.msg_decoder.parameters()) == 261893
    trainable = {n for n, p in m.named_parameters() if p.requires_grad and p.numel() > 0}   # encoder_dir.params is empty
    assert all(n.startswith(("msg_encoder.", "msg_decoder.")) for n in trainable)
    assert m.cascade == 1 and m.grid_size == 128 and m.density_bitfield.numel() == 128 ** 3 // 8
    m2 = NeRFNetwork(bound=2.0, cuda_ray=True, message_dim=48)
    assert m2.cascade == 2 and len(m2.msg_encoder.embeddings) == 96
    sd = m.state_dict()
    missing, unexpected = m.load_state_dict({k: v for k, v in sd.items() if not k.startswith("msg_")}, strict=False)  # a clean checkpoint
    assert all(k.startswith("msg_") for k in missing) and not unexpected
    with pytest.raises(ValueError):
        m._select(torch.zeros(16))
    with pytest.raises(NotImplementedError):
        NeRFNetwork(bound=1.0, hidden_dim=128)


def test_render_rejects_cpu_tensors_loudly():
    from nerf_signature_amd.network import NeRFNetwork
    m = NeRFNetwork(bound=1.0, cuda_ray=True, message_dim=32)
    with pytest.raises((ValueError, RuntimeError, AssertionError)):
        m.render(torch.zeros(1, 4, 3), torch.ones(1, 4, 3), None)


def test_meters_match_reference_golden():
    from nerf_signature_amd.trainer import BIT_ACC, PSNRMeter, loss_w_bce
    g = np.load(os.path.join(G, "g5_g6_decoder_meters.npz"))
    decoded, msg = torch.from_numpy(g["decoded"]), torch.from_numpy(g["msg"])
    acc = BIT_ACC()
    acc.update(decoded.permute(1, 0), msg[None])
    np.testing.assert_allclose(acc.measure(), float(g["bit_acc"]), atol=1e-7)
    pm = PSNRMeter()
    pm.update(torch.from_numpy(g["img"]), torch.from_numpy(g["img"]) * 0.9 + 0.02)
    np.testing.assert_allclose(pm.measure(), float(g["psnr"]), rtol=1e-5)
    np.testing.assert_allclose(float(loss_w_bce(decoded, msg.unsqueeze(-1))), float(g["lossw"]), rtol=1e-6)


def test_decoder_matches_reference_golden():
    from nerf_signature_amd.hidden_models import get_hidden_decoder_multi_views, normalize_img
    g = np.load(os.path.join(G, "g5_g6_decoder_meters.npz"))
    dec = get_hidden_decoder_multi_views(num_bits=1, redundancy=1, num_blocks=8, input_ch=3, channels=64)
    dec.load_state_dict({k[4:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("dec.")})
    img = torch.from_numpy(g["img"]).permute(0, 3, 1, 2).clone().requires_grad_(True)
    norm = normalize_img(img)
    np.testing.assert_allclose(norm.detach().numpy(), g["normalized"], atol=1e-6)
    out = dec(norm)
    np.testing.assert_allclose(out.detach().numpy(), g["decoded"], rtol=1e-4, atol=1e-5)


def _dp_worker(rank, world, port, q):
    import torch.distributed as dist
    from nerf_signature_amd import dp
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    r, w, _ = dp.init_from_env(backend="gloo")
    torch.manual_seed(0)
    dec = torch.nn.Sequential(torch.nn.Linear(4, 3), torch.nn.Linear(3, 1))
    for i, p in enumerate(dec.parameters()):
        p.grad = torch.full_like(p, float(rank + 1) * (i + 1))
    list(dec.parameters())[1].grad = None                     # a parameter without gradient on this rank
    G = torch.arange(16, dtype=torch.float32).view(8, 2) * (rank + 1)
    D = 3
    # route A: what autograd would give without the shared-gradient identity -- D dense gradients, each all-reduced
    dense = [G.clone() for _ in range(D)]
    for t in dense:
        dist.all_reduce(t)
        t /= w
    # route B: the product path -- all-reduce G alone, then fan out locally
    ex = dp.GradExchange(list(dec.parameters()))
    ex(G)
    fan = [G.clone() for _ in range(D)]
    ok = all(torch.equal(a, b) for a, b in zip(dense, fan))
    grads = [None if p.grad is None else p.grad.clone() for p in dec.parameters()]
    # stage-1 style: bucketed mean all-reduce of ordinary dense gradients
    ps = [torch.nn.Parameter(torch.zeros(5, 2)), torch.nn.Parameter(torch.zeros(7)), torch.nn.Parameter(torch.zeros(3))]
    ps[0].grad, ps[1].grad = torch.full((5, 2), float(rank)), torch.full((7,), 2.0 * rank + 1)
    nbytes = dp.allreduce_gradients(ps, bucket_bytes=48)
    assert nbytes == 68 and ps[2].grad is None
    assert torch.allclose(ps[0].grad, torch.full((5, 2), 0.5)) and torch.allclose(ps[1].grad, torch.full((7,), 2.0))
    # gradients that are views of one flat buffer (what the fused decoder hands out): all-reduced in place, as a sum
    dec2 = torch.nn.Sequential(torch.nn.Linear(4, 3), torch.nn.Linear(3, 1))
    ps2 = list(dec2.parameters())
    flat = torch.arange(sum(p.numel() for p in ps2), dtype=torch.float32) * (rank + 1)
    off = 0
    for p in ps2:
        p.grad = flat[off:off + p.numel()].view_as(p)
        off += p.numel()
    G2 = torch.ones(4, 2) * (rank + 1)
    ex2 = dp.GradExchange(ps2, average=False)
    ex2(G2)
    assert torch.equal(flat, torch.arange(flat.numel(), dtype=torch.float32) * 3) and torch.equal(G2, torch.full((4, 2), 3.0))
    assert ex2.bytes_per_step == (8 + flat.numel()) * 4 and ex2.collectives_per_step == 2
    # G and the decoder's gradient block in one allocation (GradSink(tail=...)): ONE collective covers both; unused tail
    # elements behind the block stay out of it
    n3 = sum(p.numel() for p in ps2)
    arena = torch.zeros(8 + n3 + 5)
    G3 = arena[:8].view(4, 2)
    G3 += rank + 1
    arena[8:8 + n3] = torch.arange(n3, dtype=torch.float32) * (rank + 1)
    arena[8 + n3:] = 7.0 + rank
    off = 8
    for p in ps2:
        p.grad = arena[off:off + p.numel()].view_as(p)
        off += p.numel()
    ex3 = dp.GradExchange(ps2, average=False)
    ex3(G3)
    assert ex3.collectives_per_step == 1 and ex3.bytes_per_step == (8 + n3) * 4
    assert torch.equal(G3, torch.full((4, 2), 3.0)) and torch.equal(arena[8:8 + n3], torch.arange(n3, dtype=torch.float32) * 3), arena
    assert torch.equal(arena[8 + n3:], torch.full((5,), 7.0 + rank))
    # numpy, not tensors: a tensor travels through the queue as a file descriptor that dies with this process
    q.put((rank, ok, G.numpy().copy(), [None if g is None else g.numpy().copy() for g in grads], ex.bytes_per_step))
    dist.barrier()
    dist.destroy_process_group()


def test_data_parallel_exchange_gloo_world2():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29511 + os.getpid() % 200
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=120) for _ in procs], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    base = torch.arange(16, dtype=torch.float32).view(8, 2)
    res = [(r, ok, torch.from_numpy(Gm), [None if g is None else torch.from_numpy(g) for g in grads], nb) for r, ok, Gm, grads, nb in res]
    for rank, ok, Gm, grads, nbytes in res:
        assert ok                                                  # shared-gradient exchange == D dense exchanges
        assert torch.allclose(Gm, base * 1.5)                      # mean over ranks of G*(rank+1)
        assert torch.allclose(grads[0], torch.full_like(grads[0], 1.5))
        assert torch.allclose(grads[1], torch.zeros_like(grads[1]))       # None on every rank -> zeros, stays consistent
        assert torch.allclose(grads[2], torch.full_like(grads[2], 4.5))
        assert nbytes == 16 * 4 + sum(g.numel() for g in grads) * 4
    assert torch.equal(res[0][2], res[1][2])


def _toy_problem():
    """A stand-in with the structure of the watermark step: a table theta [T,2] 'rendered' into D block images and N content pixels,
    a decoder with batch-statistics BatchNorm over the D blocks, BCE on its logits + MSE on the content pixels."""
    g = torch.Generator().manual_seed(11)
    T, D, P, N = 12, 4, 5, 6
    A_block = torch.randn(D, P, T * 2, generator=g)          # block d, pixel p: image = A_block[d,p] . theta
    A_content = [torch.randn(N, T * 2, generator=g) for _ in range(2)]   # per-rank content rays
    gt = [torch.randn(N, generator=g) for _ in range(2)]
    theta0 = torch.randn(T * 2, generator=g)
    msg = torch.tensor([1.0, 0.0, 0.0, 1.0])
    torch.manual_seed(3)
    dec = torch.nn.Sequential(torch.nn.Linear(P, 3), torch.nn.BatchNorm1d(3, track_running_stats=False), torch.nn.GELU(), torch.nn.Linear(3, 1))
    return A_block, A_content, gt, theta0, msg, dec


def _sharded_blocks_worker(rank, world, port, q):
    import torch.distributed as dist
    from nerf_signature_amd import dp
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dp.init_from_env(backend="gloo")
    A_block, A_content, gt, theta0, msg, dec = _toy_problem()
    D = A_block.shape[0]
    first, last = dp.block_shard(D)
    assert (first, last) == (rank * D // world, (rank + 1) * D // world) and dp.block_shard(D + 1) is None
    theta = theta0.clone().requires_grad_(True)
    local = A_block[first:last] @ theta                               # this rank's blocks only
    images = dp.gather_blocks(local, D, first)                         # [D,P] on every rank
    lossw = torch.nn.functional.binary_cross_entropy_with_logits(dec(images) * 10.0, msg[:, None])
    lossi = ((A_content[rank] @ theta - gt[rank]) ** 2).mean()
    (lossw + dp.content_grad_scale(True) * lossi).backward()           # what backward_from_loss_kernel(out, 1/world) seeds
    G = theta.grad.view(-1, 2).clone()
    ex = dp.GradExchange(list(dec.parameters()), shared_scale=1.0)
    ex(G)
    q.put((rank, images.detach().numpy().copy(), G.numpy().copy(), [p.grad.numpy().copy() for p in dec.parameters()], float(lossw.detach()), float(lossi.detach())))
    dist.barrier()
    dist.destroy_process_group()


def test_sharded_block_render_equals_single_process_gradient_gloo_world2():
    """Multi-GPU partitioning on two gloo ranks, GPU-free: each rank renders D/2 blocks, the blocks are
    all-gathered, the decoder (BatchNorm over all D blocks) runs replicated, each rank back-propagates its own blocks' image gradient
    plus its own content rays with the 1/world seed, ONE sum all-reduce of G follows -- and the result is the single-process gradient of
    lambda_w * BCE(D blocks) + lambda_i * MSE(all content rays of both ranks)."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29300 + os.getpid() % 200
    procs = [ctx.Process(target=_sharded_blocks_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=120) for _ in procs], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    A_block, A_content, gt, theta0, msg, dec = _toy_problem()
    theta = theta0.clone().requires_grad_(True)
    images = A_block @ theta
    lossw = torch.nn.functional.binary_cross_entropy_with_logits(dec(images) * 10.0, msg[:, None])
    lossi = ((torch.cat(A_content) @ theta - torch.cat(gt)) ** 2).mean()
    (lossw + lossi).backward()
    for rank, img, G, dgrads, lw, li in res:
        np.testing.assert_allclose(img, images.detach().numpy(), rtol=1e-6, atol=1e-6)
        np.testing.assert_allclose(G, theta.grad.view(-1, 2).numpy(), rtol=1e-5, atol=1e-6)
        for got, p in zip(dgrads, dec.parameters()):
            np.testing.assert_allclose(got, p.grad.numpy(), rtol=1e-5, atol=1e-6)
        assert abs(lw - float(lossw.detach())) < 1e-6
    assert abs(0.5 * (res[0][5] + res[1][5]) - float(lossi.detach())) < 1e-6 * float(lossi.detach())
    assert np.array_equal(res[0][2], res[1][2])


def _force_exchange_worker(q):
    import torch.distributed as dist
    from nerf_signature_amd import dp
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{29800 + os.getpid() % 150}", rank=0, world_size=1)
    lin = torch.nn.Linear(3, 2)
    for p in lin.parameters():
        p.grad = torch.ones_like(p)
    G = torch.full((4, 2), 2.0)
    ex = dp.GradExchange(list(lin.parameters()), average=False)
    inactive = not dp.exchange_active()
    ex(G)                                              # one rank, no switch: nothing runs
    idle_bytes = ex.bytes_per_step
    os.environ["NERFSIG_FORCE_EXCHANGE"] = "1"
    active = dp.exchange_active()
    ex(G)                                              # rehearsal: the collectives run over the one-rank group, values unchanged
    q.put((inactive, idle_bytes, active, ex.bytes_per_step, float(G.sum()), float(lin.weight.grad.sum())))
    dist.destroy_process_group()


def test_exchange_rehearsal_switch_on_one_rank():
    """NERFSIG_FORCE_EXCHANGE=1 makes a world-size-1 process group run the exchange (what the GPU rehearsal of the multi-rank
    execution relies on); without it a one-rank group exchanges nothing."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_force_exchange_worker, args=(q,))
    p.start()
    inactive, idle_bytes, active, nbytes, g_sum, w_sum = q.get(timeout=120)
    p.join(timeout=60)
    assert p.exitcode == 0
    assert inactive and idle_bytes == 0 and active
    assert nbytes == (8 + 6 + 2) * 4 and g_sum == 16.0 and w_sum == 6.0


def test_checkpoint_round_trip_and_clean_checkpoint(tmp_path):
    """N4: the reference's checkpoint dict format; strict=False loading of a clean (stage-1) checkpoint; fp16 tcnn params."""
    from nerf_signature_amd import checkpoint as ck
    from nerf_signature_amd.network import NeRFNetwork
    torch.manual_seed(0)
    a = NeRFNetwork(bound=1.0, cuda_ray=True, message_dim=32)
    a.mean_count, a.mean_density = 1234, 0.5
    with torch.no_grad():
        a.encoder.embeddings[3].weight.uniform_(-1, 1)
        a.msg_encoder.embeddings[7].weight.uniform_(-1, 1)
        a.density_bitfield.fill_(7)
    opt = torch.optim.Adam(a.get_params(1e-2), betas=(0.9, 0.99), eps=1e-15)
    path = ck.save_checkpoint(str(tmp_path / "checkpoints" / "ngp_ep0003.pth"), a, epoch=3, global_step=42, stats={"loss": [1.0]}, optimizer=opt, full=True)
    raw = torch.load(path, weights_only=False)
    assert set(raw) >= {"epoch", "global_step", "stats", "mean_count", "mean_density", "optimizer", "model"}
    b = NeRFNetwork(bound=1.0, cuda_ray=True, message_dim=32)
    missing, unexpected, meta = ck.load_checkpoint(path, b)
    assert not missing and not unexpected and meta["epoch"] == 3 and meta["global_step"] == 42 and b.mean_count == 1234
    for (k1, v1), (k2, v2) in zip(a.state_dict().items(), b.state_dict().items()):
        assert k1 == k2 and torch.equal(v1, v2)
    # a clean checkpoint as stage 1 would write it: no codebook / decoder keys, tcnn parameters in half precision
    clean = {k: (v.half() if k.endswith("_net.params") else v) for k, v in a.state_dict().items() if not k.startswith("msg_")}
    c = NeRFNetwork(bound=1.0, cuda_ray=True, message_dim=32)
    before = c.msg_encoder.embeddings[0].weight.clone()
    missing, unexpected, _ = ck.load_checkpoint({"model": clean, "epoch": 1, "global_step": 1, "stats": {}}, c, model_only=True)
    assert all(k.startswith("msg_") for k in missing) and not unexpected
    assert c.sigma_net.params.dtype == torch.float32 and torch.allclose(c.sigma_net.params, a.sigma_net.params, atol=1e-3)
    assert torch.equal(c.encoder.embeddings[3].weight, a.encoder.embeddings[3].weight) and torch.equal(c.msg_encoder.embeddings[0].weight, before)
    assert c._packed_cache is None
    missing, _, _ = ck.load_checkpoint(a.state_dict(), c)      # a bare state_dict is accepted too
    assert not missing


def test_checkpoint_loading_is_tolerant_and_keeps_optimizer_state_in_place(tmp_path, capsys):
    """utils_wtmk_disen.py:1497-1517: an optimizer / scheduler section that does not fit is reported and skipped, the rest of the resume
    goes on.  A section that does fit is loaded INTO the existing state tensors (a captured graph holds their addresses), and a learning
    rate that lives in a tensor keeps living there."""
    from nerf_signature_amd import checkpoint as ck
    from nerf_signature_amd.network import NeRFNetwork
    torch.manual_seed(0)
    a = NeRFNetwork(bound=1.0, cuda_ray=True, message_dim=4)
    opt = torch.optim.Adam(a.get_params(1e-2), betas=(0.9, 0.99), eps=1e-15)
    for p in a.msg_decoder.parameters():
        p.grad = torch.ones_like(p)
    opt.step()
    state = ck.checkpoint_state(a, epoch=1, global_step=1, optimizer=opt, full=True)
    b = NeRFNetwork(bound=1.0, cuda_ray=True, message_dim=4)
    opt_b = torch.optim.Adam(b.get_params(5e-3), betas=(0.9, 0.99), eps=1e-15)
    for p in b.msg_decoder.parameters():
        p.grad = torch.full_like(p, 2.0)
    opt_b.step()
    lr_dev = torch.tensor(5e-3)
    for g in opt_b.param_groups:
        g["lr"] = lr_dev
    p0 = next(iter(b.msg_decoder.parameters()))
    kept = opt_b.state[p0]["exp_avg"]
    _, _, meta = ck.load_checkpoint(state, b, optimizer=opt_b)
    assert "skipped" not in meta
    assert opt_b.state[p0]["exp_avg"] is kept and torch.equal(kept, opt.state[next(iter(a.msg_decoder.parameters()))]["exp_avg"])
    assert all(g["lr"] is lr_dev for g in opt_b.param_groups) and float(lr_dev) == pytest.approx(1e-2)
    # a checkpoint whose optimizer section belongs to another parameter grouping: warned about, skipped, model still loaded
    other = torch.optim.Adam([next(iter(a.msg_decoder.parameters()))], lr=1e-3)
    bad = dict(state, optimizer=other.state_dict(), lr_scheduler={"nonsense": 1})
    sched = torch.optim.lr_scheduler.LambdaLR(opt_b, lambda it: 1.0)
    _, _, meta = ck.load_checkpoint(bad, b, optimizer=opt_b, lr_scheduler=sched)
    assert meta["skipped"] == ["optimizer", "lr_scheduler"] and "Failed to load optimizer" in capsys.readouterr().out
    assert meta["epoch"] == 1


def test_block_selection_matches_reference_golden():
    """N2: process_image (JPEG compressibility ranking) and rand_poses vs the reference's own outputs (golden G10)."""
    pytest.importorskip("PIL")
    from nerf_signature_amd import blocks
    g = np.load(os.path.join(G, "g10_blocks.npz"))
    img = torch.from_numpy(g["image"])
    coords, bh, bw = blocks.process_image(img, 8, 10, 6)
    assert (bh, bw) == (int(g["bh"]), int(g["bw"])) == (12, 12)
    np.testing.assert_array_equal(coords.numpy(), g["coords"])
    o = torch.arange(96 * 120 * 3, dtype=torch.float32).view(1, 96, 120, 3)
    bo, bd = blocks.block_rays(o, -o, coords)
    assert bo.shape == (6, 12, 12, 3)
    r0, c0 = int(coords[2, 0]), int(coords[2, 1])
    assert torch.equal(bo[2], o[0, r0:r0 + 12, c0:c0 + 12]) and torch.equal(bd[2], -bo[2])
    torch.manual_seed(5)
    np.testing.assert_allclose(blocks.rand_poses(4, "cpu", radius=2.5).numpy(), g["rand_poses"], rtol=0, atol=1e-6)


def test_bench_starts_its_own_ranks_dry_launch():
    """`python bench.py --gpus 2` must start the two rank processes itself (the driver's scaling run has no external launcher):
    --dry-launch takes that path over gloo with the step's collectives (block all-gather, gradient all-reduce) on CPU tensors."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--dry-launch"], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout                      # exactly one JSON line, from rank 0
    line = json.loads(lines[0])
    assert line["dry_launch"] and line["n_gpus"] == 2 and line["world_size_seen"] == 2 and line["collectives_ok"]
    assert line["block_shard_rank0"] == [0, 16] and line["backend"] == "gloo"
    assert line["device_of_rank"] == ["0", "1"] and line["devices_distinct"]            # every rank binds a GPU of its own, decided before any GPU call
    # ... and a launch that would put two ranks on one GPU is refused by every rank before anything runs (no JSON line, exit code 5)
    clash = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--dry-launch", "--dry-device-count", "1"], env=env,
                           capture_output=True, text=True, timeout=300)
    assert clash.returncode != 0 and "would share device" in clash.stderr and not [l for l in clash.stdout.splitlines() if l.startswith("{")]


def test_bench_launcher_falls_back_when_the_first_attempt_fails():
    """NERFSIG_CAPTURE_COLLECTIVES=try: the launcher first starts the ranks with the collectives captured inside the step's graph; if those
    ranks fail (here: a test hook makes them exit with code 3) it starts them again with the collectives between captured segments, and
    only the successful attempt's JSON line reaches stdout."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "NERFSIG_CAPTURE_COLLECTIVES")}
    env["NERFSIG_TEST_FAIL_CAPTURED"] = "1"
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--dry-launch"], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1 and "starting the ranks again" in out.stderr
    line = json.loads(lines[0])
    assert line["collectives_ok"] and line["capture_collectives_env"] == "0"


def _sharded_checkpoint_worker(rank, world, port, q, tmp):
    """Two gloo ranks whose codebook optimiser is sharded (NERFSIG_SHARD_OPTIMIZER=1): each updates the tables and Adam moments of ITS bits
    only (what a captured step does), then both enter checkpoint_state -- which must gather first."""
    import types
    import torch.distributed as dist
    from nerf_signature_amd import checkpoint, dp, trainer
    from nerf_signature_amd.network import NeRFNetwork
    from nerf_signature_amd.optim import CodebookAdam, _prepare_device_state
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), NERFSIG_SHARD_OPTIMIZER="1")
    dp.init_from_env(backend="gloo")
    torch.manual_seed(0)
    D = 4
    model = NeRFNetwork(bound=1.0, cuda_ray=True, message_dim=D, n_views=1)
    opt = CodebookAdam(model.get_params(1e-2), betas=(0.9, 0.99), eps=1e-15)
    tables = model.msg_encoder.tables()
    loop = object.__new__(trainer.GraphedWatermarkLoop)          # (the captured loop itself needs a GPU; gather_codebook does not)
    loop.model, loop.optimizer, loop.tables, loop.opt_shard = model, opt, tables, dp.optimizer_shard(D)
    assert loop.opt_shard == (rank * D // world, (rank + 1) * D // world)
    model.codebook_shard, model._graphed_loops = loop.opt_shard, [loop]
    _prepare_device_state(opt, tables)
    b0, b1 = loop.opt_shard
    with torch.no_grad():
        for i in range(2 * b0, 2 * b1):                           # this rank's "steps": only the tables of its own bits move
            tables[i].add_(0.25 * (i + 1))
            opt.state[tables[i]]["exp_avg"].fill_(float(i + 1))
            opt.state[tables[i]]["exp_avg_sq"].fill_(float(i + 1) ** 2)
            opt.state[tables[i]]["step"].fill_(3.0 + i)
    model._codebook_stale = True                                  # what GraphedWatermarkLoop.step leaves behind with a sharded optimiser
    refused = False
    try:
        checkpoint.checkpoint_state(model, gather=False)
    except RuntimeError:
        refused = True
    select_refused = False
    try:
        model._select(torch.zeros(D))
    except RuntimeError:
        select_refused = True
    # save_checkpoint itself is the collective call -- both ranks make it, rank 0 alone writes, and the other rank returns
    # only once the file exists
    path = os.path.join(tmp, "sharded.pth")
    checkpoint.save_checkpoint(path, model, optimizer=opt, full=True)
    assert not model._codebook_stale and os.path.exists(path)
    writers = [f for f in os.listdir(tmp) if f.endswith(".pth")]
    assert writers == ["sharded.pth"]
    q.put((rank, refused, select_refused))
    dist.barrier()
    dist.destroy_process_group()


def test_checkpoint_of_a_sharded_codebook_optimizer_gathers_first_gloo_world2(tmp_path):
    """a rank-0 save in the middle of a sharded run wrote stale tables.  checkpoint_state now gathers (or refuses with
    gather=False), the host-side selection refuses stale tables, and the saved file equals what a single process would have written."""
    import torch.multiprocessing as mp
    from nerf_signature_amd import checkpoint
    from nerf_signature_amd.network import NeRFNetwork
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29650 + os.getpid() % 200
    procs = [ctx.Process(target=_sharded_checkpoint_worker, args=(r, 2, port, q, str(tmp_path))) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=300) for _ in procs])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert all(refused and select_refused for _, refused, select_refused in res)
    torch.manual_seed(0)
    D = 4
    single = NeRFNetwork(bound=1.0, cuda_ray=True, message_dim=D, n_views=1)
    with torch.no_grad():
        for i, t in enumerate(single.msg_encoder.tables()):
            t.add_(0.25 * (i + 1))
    ckpt = torch.load(os.path.join(str(tmp_path), "sharded.pth"), weights_only=False)
    want = single.state_dict()
    for k, v in ckpt["model"].items():
        assert torch.equal(v, want[k]), k
    st = ckpt["optimizer"]["state"]
    assert len(st) >= 2 * D
    for i in range(2 * D):
        assert float(st[i]["exp_avg"].mean()) == i + 1 and float(st[i]["exp_avg_sq"].mean()) == (i + 1) ** 2 and float(st[i]["step"]) == 3.0 + i
    fresh = NeRFNetwork(bound=1.0, cuda_ray=True, message_dim=D, n_views=1)
    checkpoint.load_checkpoint(ckpt, fresh)
    for a, b in zip(fresh.msg_encoder.tables(), single.msg_encoder.tables()):
        assert torch.equal(a, b)


def test_bench_launcher_walks_the_whole_chain_and_still_prints_a_line_when_every_attempt_fails():
    """the first real N > 1 run must not be able to die silently.  Every attempt fails here (test hook) -- four
    stderr blocks, one per attempt, then ONE JSON line with value null and the reasons, exit code non-zero; and a hung attempt is cut by
    the watchdog (ranks that sleep: killed after NERFSIG_LAUNCH_WATCHDOG_S, the chain still ends)."""
    import json
    import subprocess
    import sys
    import time
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "NERFSIG_CAPTURE_COLLECTIVES")}
    env["NERFSIG_TEST_FAIL_CAPTURED"] = "all"
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--dry-launch"], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode != 0
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    line = json.loads(lines[0])
    assert line["value"] is None and line["n_gpus"] == 2
    fails = line["config"]["launch_failures"]
    assert [f["attempt"] for f in fails] == [0, 1, 2, 3] and all(f["rc"] == 3 for f in fails), (fails, out.stderr[-3000:])
    # the stderr on record is the FAILING rank's (whichever exits first; the other is torn down, possibly before it printed anything)
    assert all(f["first_failed_rank"] in (0, 1) and "fails on purpose" in f["failed_rank_stderr_tail"] for f in fails), fails
    assert out.stderr.count("failed: rc 3") == 4 and "no attempt left" in out.stderr, out.stderr[-3000:]
    # hung ranks: every attempt is cut by the watchdog; the chain takes about attempts x (watchdog + kill)
    env["NERFSIG_TEST_FAIL_CAPTURED"] = "hang"
    env["NERFSIG_LAUNCH_WATCHDOG_S"] = "4"
    t0 = time.time()
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--dry-launch"], env=env, capture_output=True, text=True, timeout=600)
    took = time.time() - t0
    line = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][0])
    assert out.returncode != 0 and line["value"] is None
    assert [f["rc"] for f in line["config"]["launch_failures"]] == [124] * 4 and took < 120, (took, line["config"]["launch_failures"], out.stderr[-3000:])


def test_bench_under_an_external_launcher_supervises_its_own_worker_and_walks_the_chain():
    """The driver starts N > 1 as `python -m torch.distributed.run ... bench.py --gpus N`: RANK / WORLD_SIZE are set, bench.py's own launcher
    is not in play.  Every rank process then supervises a child worker through the same chain of modes (bench.supervise_rank): a failing
    first attempt is followed by the next mode on a fresh rendezvous; with every attempt failing rank 0 still prints the value-null line."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "NERFSIG_CAPTURE_COLLECTIVES")}
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port",
           str(29900 + os.getpid() % 90), os.path.join(root, "bench.py"), "--gpus", "2", "--dry-launch"]
    env["NERFSIG_TEST_FAIL_CAPTURED"] = "1"
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1 and json.loads(lines[0])["collectives_ok"] and json.loads(lines[0])["capture_collectives_env"] == "0"
    assert "rank 0: attempt 0" in out.stderr and "next attempt: default" in out.stderr
    env["NERFSIG_TEST_FAIL_CAPTURED"] = "all"
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode != 0
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    line = json.loads(lines[0])
    assert line["value"] is None and [f["attempt"] for f in line["config"]["launch_failures"]] == [0, 1, 2, 3]


def test_the_drivers_eight_rank_commands_start_eight_ranks_that_meet():
    """The two command lines an 8-GPU scaling run can use -- `python bench.py --gpus 8` (bench.py's own launcher) and the driver's `python -m torch.distributed.run
    --nproc-per-node 8 ... bench.py --gpus 8` (every rank supervising its own worker) -- rehearsed with --dry-launch: eight real processes over gloo, the step's
    collectives on CPU tensors, eight distinct devices, blocks sharded four per rank, one JSON line from rank 0."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE", "MASTER_PORT", "NERFSIG_CAPTURE_COLLECTIVES", "NERFSIG_TEST_FAIL_CAPTURED")}
    own = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "8", "--dry-launch"]
    external = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "8", "--master-addr", "127.0.0.1", "--master-port",
                str(29800 + os.getpid() % 90), os.path.join(root, "bench.py"), "--gpus", "8", "--dry-launch"]
    for cmd in (own, external):
        out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-3000:]
        lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, out.stdout
        line = json.loads(lines[0])
        assert line["n_gpus"] == 8 and line["world_size_seen"] == 8 and line["collectives_ok"] and line["devices_distinct"]
        assert line["device_of_rank"] == [str(r) for r in range(8)] and line["block_shard_rank0"] == [0, 4]


def test_tcnn_layout_checker_recovers_every_hypothesis_and_agrees_with_the_oracle_under_the_documented_one():
    """tools/check_tcnn_layout.py: the checker for the one unpinnable part of the path.  (a) its self-test: each
    of the 48 layout hypotheses is recovered from a dump generated under it, and a transposed / zero-padded checkpoint converts into the
    documented layout; (b) under the documented layout its own field evaluation (written independently, no oracle import) equals the
    oracle's NeRFNetwork.forward restatement, with and without a message -- so "matches the documented layout" means "matches what the
    kernels are tested against"."""
    import importlib.util
    from oracle import field_ref as fr
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("check_tcnn_layout", os.path.join(root, "tools", "check_tcnn_layout.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    assert tool.self_test() == 48
    src = open(os.path.join(root, "tools", "check_tcnn_layout.py")).read()
    assert "import oracle" not in src and "from oracle" not in src
    g = torch.Generator().manual_seed(3)
    base = [(torch.rand(1 << 19, 2, generator=g) - 0.5) for _ in range(16)]
    cb = [(torch.rand(1 << 19, 2, generator=g) - 0.5) * 0.1 for _ in range(8)]
    sp, cp = torch.randn(3072, generator=g) * 0.2, torch.randn(7168, generator=g) * 0.2
    x = (torch.rand(300, 3, generator=g) * 2 - 1) * 1.8
    d = torch.nn.functional.normalize(torch.randn(300, 3, generator=g), dim=-1)
    P = {"bound": 2.0, "base_tables": base, "cb_tables": cb, "sigma_params": sp, "color_params": cp}
    for msg in (None, torch.tensor([1.0, 0.0, 1.0, 1.0])):
        s0, c0 = fr.field_forward(x, d, msg, P)
        feat = tool.features(x, 2.0, base, cb, None if msg is None else msg.numpy())
        s1, c1 = tool.evaluate(feat, d, sp, cp, tool.ASSUMED)
        np.testing.assert_allclose(s1.numpy(), s0.numpy(), rtol=2e-5, atol=1e-6)
        np.testing.assert_allclose(c1.numpy(), c0.numpy(), rtol=0, atol=2e-6)


def test_distortion_layer_host_side_matches_the_oracle_restatement():
    """nerf_signature_amd.distortion's stock-operator forms (CPU) against the oracle's restatement of Trainer.distortion_layer
    (utils_wtmk_disen.py:551-577) with the same draws; the rotation's resampling on cases with a known answer; the reference's choice list."""
    import math
    import numpy as np
    import pytest
    from oracle import field_ref as fr
    from nerf_signature_amd import distortion as ds
    rng = np.random.RandomState(0)
    x = torch.from_numpy(rng.rand(4, 6, 5, 3).astype(np.float32))
    noise = torch.from_numpy(rng.randn(4, 6, 5, 3).astype(np.float32)) * math.sqrt(0.1)
    assert torch.equal(ds.reference_ops(x, "noise", None, noise), fr.distortion_layer(x, "noise", noise))
    for f in (0.5, 0.93, 1.5):
        assert torch.allclose(ds.reference_ops(x, "brightness", torch.tensor([f])), fr.distortion_layer(x, "brightness", f), atol=1e-7)
    for s in (0.01, 0.2, 0.5):
        assert torch.allclose(ds.reference_ops(x, "blurring", torch.tensor([s])), fr.distortion_layer(x, "blurring", s), atol=1e-7)
    img = torch.arange(3 * 5 * 5, dtype=torch.float32).reshape(3, 5, 5)
    assert torch.equal(ds.rotate_nearest(img, 1.0, 0.0), img)
    assert torch.equal(ds.rotate_nearest(img, 0.0, 1.0), torch.rot90(img, 1, (1, 2)))           # counter-clockwise, like torchvision's `angle`
    r30 = ds.rotate_nearest(torch.ones(3, 12, 12), math.cos(math.radians(30.0)), math.sin(math.radians(30.0)))
    assert float(r30[:, 5:7, 5:7].min()) == 1.0 and float(r30[:, 0, 0].max()) == 0.0              # centre kept, corners filled with zeros
    # rotation / scaling with the draws passed in, against the oracle's grid_sample / interpolate statement (non-square images, several angles per batch)
    degs = [-30.0, -7.3, 11.9, 29.5]
    cs = torch.tensor([[math.cos(math.radians(d)), math.sin(math.radians(d))] for d in degs], dtype=torch.float32).reshape(-1)
    assert torch.equal(ds.reference_ops(x, "rotation", cs), fr.distortion_layer(x, "rotation", degs))
    for sf in (0.75, 0.9, 1.0, 1.13, 1.2499):
        out = ds.reference_ops(x, "scaling", sf)
        assert out.shape == (4, 6, ds.scaled_width(5, sf), 3) and torch.equal(out, fr.distortion_layer(x, "scaling", sf))
    layer = ds.DistortionLayer("scaling", seed=1)
    layer.draw(tuple(x.shape), torch.device("cpu"))
    out = layer(x)
    assert 0.75 <= layer.factor <= 1.25 and out.shape == (4, 6, layer.out_width(5), 3)             # resized along W only (:564: a [3,H,W] image is a 1-d batch)
    layer = ds.DistortionLayer("rotation", seed=1)
    layer.draw(tuple(x.shape), torch.device("cpu"))
    c, s_ = layer.param.reshape(-1, 2).unbind(1)
    assert layer.param.shape == (8,) and torch.allclose(c * c + s_ * s_, torch.ones(4), atol=1e-6) and float(c.min()) >= math.cos(math.radians(30.0)) - 1e-6
    assert layer(x).shape == x.shape
    u = [ds.host_uniform(3, k, 0.75, 1.25) for k in range(2000)]                                   # the captured loop's host-side scaling factor
    assert 0.75 <= min(u) < 0.76 and 1.24 < max(u) < 1.25 and abs(sum(u) / len(u) - 1.0) < 0.01 and u[5] == ds.host_uniform(3, 5, 0.75, 1.25) != ds.host_uniform(4, 5, 0.75, 1.25)
    for name in ("none", "noise", "rotation", "scaling", "blurring", "brightness"):       # main_nerf_wtmk.py:75
        ds.DistortionLayer(name)
    with pytest.raises(ValueError):
        ds.DistortionLayer("jpeg")
    a, b = ds.DistortionLayer("brightness", seed=5), ds.DistortionLayer("brightness", seed=5)      # rank-consistent draws: same seed, same sequence
    a.draw((2, 2, 2, 3), torch.device("cpu")), b.draw((2, 2, 2, 3), torch.device("cpu"))
    assert float(a.param) == float(b.param) and 0.5 <= float(a.param) <= 1.5


def test_device_ordinal_follows_the_visibility_masks(monkeypatch):
    """dp.device_ordinal: LOCAL_RANK modulo the visible device count, mapped through HIP_VISIBLE_DEVICES / ROCR_VISIBLE_DEVICES when set; the clash check
    needs no process group and no GPU."""
    import pytest
    from nerf_signature_amd import dp
    for var in ("HIP_VISIBLE_DEVICES", "ROCR_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):
        monkeypatch.delenv(var, raising=False)
    assert dp.device_ordinal(3, device_count=8) == (3, "3")
    assert dp.device_ordinal(9, device_count=8) == (1, "1")
    monkeypatch.setenv("HIP_VISIBLE_DEVICES", "4,5,6,7")
    assert dp.device_ordinal(2) == (2, "6") and dp.device_ordinal(5) == (1, "5")
    monkeypatch.delenv("HIP_VISIBLE_DEVICES")
    monkeypatch.setenv("LOCAL_RANK", "3")
    monkeypatch.setenv("LOCAL_WORLD_SIZE", "4")
    assert dp.assert_distinct_devices(device_count=4) == (3, "3")
    with pytest.raises(RuntimeError, match="LOCAL_RANK 3 would share device 1 with LOCAL_RANK 1"):
        dp.assert_distinct_devices(device_count=2)
    # 3 ranks on 2 GPUs at LOCAL_RANK 1 used to name a negative partner; rank 1 shares with nobody by itself (ranks 0 and 2 collide)
    monkeypatch.setenv("LOCAL_RANK", "1")
    monkeypatch.setenv("LOCAL_WORLD_SIZE", "3")
    with pytest.raises(RuntimeError, match=r"would share device 1 \(other ranks of the node collide\)"):
        dp.assert_distinct_devices(device_count=2)
    monkeypatch.setenv("LOCAL_RANK", "2")
    with pytest.raises(RuntimeError, match="LOCAL_RANK 2 would share device 0 with LOCAL_RANK 0"):
        dp.assert_distinct_devices(device_count=2)


def test_bound_train_step_falls_back_to_the_reference_method_for_another_criterion():
    """trainer.reference_trainer_train_step hard-codes the MSE content loss; a Trainer whose criterion is not MSELoss(reduction='none') goes through the
    method of the class the bound one shadows (found over the MRO) instead of silently training on another loss."""
    from nerf_signature_amd import trainer

    class RefTrainer:
        def train_step(self, data, message):
            return ("the reference's own", data, message)

    class Bound(RefTrainer):
        train_step = trainer.reference_trainer_train_step

    t = Bound()
    t.criterion = torch.nn.L1Loss(reduction="none")
    assert t.train_step("d", "m") == ("the reference's own", "d", "m")
    t.criterion = torch.nn.MSELoss(reduction="mean")
    assert t.train_step("d", "m")[0] == "the reference's own"
    t.criterion = torch.nn.MSELoss(reduction="none")
    with pytest.raises((AttributeError, TypeError, KeyError)):      # the fused path is taken (and trips over the dummy arguments)
        t.train_step("d", "m")


def test_environment_switches_are_the_documented_ones(monkeypatch):
    """the package and bench.py read exactly the switches nerf_signature_amd/switches.py documents (at most 20); nothing else named
    NERFSIG_* occurs in product sources (rejected experiments leave no switch behind), and the few that no other test flips are flipped here."""
    import re
    import subprocess
    import sys
    from nerf_signature_amd import switches
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    found = set()
    files = [os.path.join(root, "bench.py"), os.path.join(root, "__graft_entry__.py")]
    for base, _, names in os.walk(os.path.join(root, "nerf_signature_amd")):
        files += [os.path.join(base, n) for n in names if n.endswith((".py", ".hip", ".h", ".md"))]
    for f in files:
        found |= set(re.findall(r"NERFSIG_[A-Z0-9_]+", open(f).read()))
    found -= {"NERFSIG_"}
    assert found == set(switches.DOCUMENTED), (sorted(found - set(switches.DOCUMENTED)), sorted(set(switches.DOCUMENTED) - found))
    assert len(switches.DOCUMENTED) <= 20 and all(name in switches.__doc__ for name in switches.DOCUMENTED)
    # NERFSIG_DROPIN_OFF: a list of known features; anything else is an error, not silently ignored
    monkeypatch.setenv("NERFSIG_DROPIN_OFF", "dense_adam, get_rays")
    assert switches.dropin_off("dense_adam") and switches.dropin_off("get_rays") and not switches.dropin_off("train_step")
    monkeypatch.setenv("NERFSIG_DROPIN_OFF", "premarch")
    with pytest.raises(ValueError, match="unknown feature"):
        switches.dropin_off("train_step")
    monkeypatch.delenv("NERFSIG_DROPIN_OFF")
    assert not any(switches.dropin_off(f) for f in switches.DROPIN_FEATURES)
    # NERFSIG_MLP: the arithmetic the library starts with (read once per process: fresh interpreters)
    for value, want in (("bf16x3", 0), ("f16", 1), (None, 1)):
        env = {k: v for k, v in os.environ.items() if k != "NERFSIG_MLP"}
        if value is not None:
            env["NERFSIG_MLP"] = value
        out = subprocess.run([sys.executable, "-c", "import sys; sys.path.insert(0, %r); from nerf_signature_amd import _native as nv; print(nv.fn('mlp_get_precision')())" % root],
                             env=env, capture_output=True, text=True, timeout=120)
        assert out.returncode == 0 and int(out.stdout.strip().splitlines()[-1]) == want, (value, out.stdout, out.stderr[-300:])
    # NERFSIG_REPLICATE_BLOCKS: no block shard even where an exchange runs (the launcher's last fallback)
    from nerf_signature_amd import dp
    monkeypatch.setattr(dp, "exchange_active", lambda: True)
    monkeypatch.setattr(dp.dist, "get_world_size", lambda: 2)
    monkeypatch.setattr(dp.dist, "get_rank", lambda: 1)
    assert dp.block_shard(32) == (16, 32)
    monkeypatch.setenv("NERFSIG_REPLICATE_BLOCKS", "1")
    assert dp.block_shard(32) is None


def _load_bench():
    import importlib.util
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_bench_line_stays_below_the_drivers_tail_whatever_the_record_holds(tmp_path, monkeypatch, capfd):
    """The driver keeps a 9 KB tail of stdout + stderr and parses the LAST line of stdout: round 5's 23.9 KB line came back `parsed: null`.  The emitter is run on
    a synthetic record stuffed with prose and nested secondaries; the stdout line must stay below 8 KB, parse from a 9000-byte tail, carry the contract's
    fields with `roofline` and `cpu_baseline`, and the complete record must land in bench_detail.json."""
    import json
    bench = _load_bench()
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    prose = "x" * 3000
    full = {"metric": "training rays/sec @4096 rays (hotdog, 32-bit msg)", "value": 4.4e6, "unit": "rays/s", "n_gpus": 1, "steps": 20, "warmup": 5, "ms_per_step": 0.92123456789,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32 + f16 MFMA", "data": "synthetic",
            "timing": {"ms_per_step_windows": [0.92, 0.91, 0.91], "ms_per_step_median": 0.91, "note": prose},
            "config": {"workload": prose, "content_rays": 4096, "block_rays_total": 4608, "points_per_step_per_rank": 1404940, "execution": "hipGraph replay, 1 captured segment(s)",
                       "hyper_parameters": prose, "fixed_blocks_variant": {"what": prose, "ms_per_step": 0.71}, "loss": 0.0025},
            "roofline": {"kernel": "k_encode_planes", "bound": "l2_l1_fill", "achieved": 21700.0, "peak": 34500.0, "unit": "GB/s", "frac": 0.63, "frac_l2": 0.63, "traffic": 4.7e8,
                         "frac_hbm_implemented_bytes": 0.76, "basis": prose, "observed_limiter": prose, "avg_launch_s": 2.3e-4, "points_per_launch": 1290137.0,
                         "algorithmic_bytes_per_point": 1088, "whole_step": {"frac": 0.37, "note": prose}},
            "roofline_mlp": {"kernel": "k_field_fwd", "bound": "mfma", "achieved": 600.0, "peak": 2500.0, "unit": "TFLOP/s", "frac": 0.24, "note": prose},
            "cpu_baseline": {"value": 3845.5, "unit": "rays/s", "cores": 16, "kind": "port", "sample": prose, "same_basis": {"value": 375.0, "unit": "content rays/s", "how": prose}},
            "quality": {"bit_acc": 1.0, "psnr_db": 61.3, "what": prose, "loss_log": [[i, 0.0, 0.1] for i in range(100)]},
            "secondary": {name: {"what": prose, "ms_per_step": 1.0, "windows": [{"note": prose}] * 5, "sparse_grid": {"ms_per_step": 0.3}, "noise": {"ms_per_step": 0.9, "what": prose},
                                 "rank_of_8": {"captured": {"ms_per_step": 0.48, "what": prose}}, "roofline_scatter": {"frac": 0.55, "kernel": prose}}
                          for name in ("quality_two_ranks_gloo", "counter", "fern", "rank_emulation", "eager_reference_trainer_shape", "eval_loop", "distortion_layer", "stage1",
                                       "one_more_child_added_later")}}
    assert len(json.dumps(full)) > 60000
    real_stdout = os.dup(1)
    try:
        bench.emit(full, real_stdout)
    finally:
        os.dup2(real_stdout, 1)
        os.close(real_stdout)
    out = capfd.readouterr().out
    tail = ("stderr noise\n" * 50 + out)[-9000:]
    last = [l for l in tail.splitlines() if l.strip()][-1]
    assert len(last) < 8192 and len(last) <= bench.LINE_LIMIT
    line = json.loads(last)
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert key in line, key
    assert set(("bound", "achieved", "peak", "unit", "frac", "traffic")) <= set(line["roofline"]) and line["roofline"]["frac"] == 0.63
    assert set(("value", "unit", "cores", "kind", "sample")) <= set(line["cpu_baseline"])
    assert "workload" in line["config"] and "model" not in line["config"]
    assert all(len(v) < 200 for v in _strings(line)), "prose leaked into the line"
    assert line["ms_per_step"] == pytest.approx(0.92123456789, rel=1e-5)
    assert json.load(open(tmp_path / bench.DETAIL_FILE)) == full                     # nothing is lost: the complete record is in the side file
    # the guard of last resort: a record whose numeric blocks alone exceed the limit loses optional blocks, never the contract's
    full["secondary"] = {f"child{i}": {"ms_per_step": float(i), "content_rays_per_s": 1e6, "points_per_step": i} for i in range(400)}
    short = bench.compact_line(full)
    assert len(json.dumps(short)) <= bench.LINE_LIMIT and "secondary" in short["dropped_for_length"] and "roofline" in short and "cpu_baseline" in short


def test_bench_plain_run_does_only_what_the_headline_needs(monkeypatch):
    """`bench.py --gpus 1 --steps K --warmup W` starts no secondary child and times one window; --full starts the secondaries and keeps three windows, and
    so does --dump-outputs (the dump has always been taken behind the third window); an explicit --windows wins."""
    import sys
    bench = _load_bench()
    calls = []
    monkeypatch.setattr(bench, "run_secondaries", lambda args: calls.append("secondaries") or {})
    monkeypatch.setattr(bench, "bench_training", lambda args, scene, real_stdout, secondary=None: calls.append((args.windows, args.full, secondary is not None)))
    for name in ("RANK", "WORLD_SIZE"):
        monkeypatch.delenv(name, raising=False)
    want = {(): [(1, False, False)], ("--full",): ["secondaries", (3, True, True)], ("--dump-outputs", "d"): [(3, False, False)],
            ("--full", "--no-secondary", "--windows", "2"): [(2, True, False)]}
    for extra, expected in want.items():
        del calls[:]
        monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5", *extra])
        saved = os.dup(1)
        try:
            bench.main()
        finally:
            os.dup2(saved, 1)
            os.close(saved)
        assert calls == expected, (extra, calls)


def _strings(o):
    if isinstance(o, str):
        yield o
    elif isinstance(o, dict):
        for v in o.values():
            yield from _strings(v)
    elif isinstance(o, list):
        for v in o:
            yield from _strings(v)


def test_bench_dump_outputs_writes_float32_arrays_at_fixed_sample_positions(tmp_path):
    """bench.py --dump-outputs: one float32 .npy per returned tensor and per parameter, never empty and never 0-d; a parameter above DUMP_WHOLE elements is written as DUMP_SAMPLE elements at
    positions that depend on its size alone (two builds compare file by file); a dump above DUMP_LIMIT is refused before anything is written."""
    bench = _load_bench()
    torch.manual_seed(0)
    model = torch.nn.Module()
    model.small = torch.nn.Parameter(torch.randn(3, 4, dtype=torch.float64))
    model.big = torch.nn.Parameter(torch.arange(bench.DUMP_WHOLE + 7, dtype=torch.float32))
    loss = torch.tensor(0.25)
    model.no_weights = torch.nn.Parameter(torch.zeros(0))          # (the SH encoder's parameter vector: no elements, no file)
    arrays = bench.dump_arrays(model, loss=loss, rgb=torch.ones(2, 3, dtype=torch.float16), missing=None, nothing=torch.zeros(0, 3))
    assert set(arrays) == {"loss", "rgb", "param.small", "param.big.sample"}
    bench.write_dump(str(tmp_path / "d"), arrays)
    got = {f[:-4]: np.load(tmp_path / "d" / f) for f in os.listdir(tmp_path / "d")}
    assert set(got) == set(arrays) and all(a.dtype == np.float32 and a.ndim >= 1 and a.size > 0 for a in got.values())
    assert got["loss"].shape == (1,) and got["loss"][0] == np.float32(0.25) and got["rgb"].shape == (2, 3)
    np.testing.assert_array_equal(got["param.small"], model.small.detach().reshape(-1).float().numpy())
    pos = got["param.big.sample"]                    # the parameter holds its own indices: the sample shows the positions
    assert pos.shape == (bench.DUMP_SAMPLE,) and np.all(np.diff(pos) > 0) and pos[-1] < bench.DUMP_WHOLE + 7
    np.testing.assert_array_equal(bench.dump_arrays(model)["param.big.sample"], pos)
    with pytest.raises(SystemExit):
        bench.write_dump(str(tmp_path / "too_big"), {"x": np.zeros(bench.DUMP_LIMIT // 4 + 1, np.float32)})
    assert not (tmp_path / "too_big").exists()


def test_static_live_rows_bound_every_row_a_level_can_touch():
    """stage1.live_rows (the packed data-parallel exchange of the coarse levels): the rows the oracle's encoder gathers from -- for points all over [0, 1]^3, corners and
    faces of the box included -- lie inside the static set; the set is the hash of the level's (res + 2)^3 grid corners (hash_encoding.py:11-22), sorted and unique;
    levels 0..4 are the ones worth packing."""
    from nerf_signature_amd import stage1
    rng = np.random.RandomState(0)
    pts = rng.rand(20000, 3).astype(np.float32)
    pts[:8] = np.array([[i & 1, (i >> 1) & 1, (i >> 2) & 1] for i in range(8)], np.float32)
    pts[8:2008, 0] = 1.0
    pts[2008:4008, 1] = 0.0
    x = torch.from_numpy(pts)
    assert stage1.SPARSE_EXCHANGE_LEVELS == (0, 1, 2, 3, 4)
    for level in (0, 2, 4, 5):
        live = stage1.live_rows(level)
        assert torch.equal(live, torch.unique(live)) and int(live.min()) >= 0 and int(live.max()) < (1 << 19)
        res = stage1.RESOLUTIONS[level]
        cell = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(res), dtype=torch.float32)
        idx = torch.floor(x.clamp(0, 1) / cell).to(torch.int64)                       # hash_encoding.py:33-39
        assert int(idx.max()) <= res
        rows = set()
        for dx in (0, 1):
            for dy in (0, 1):
                for dz in (0, 1):
                    c = idx + torch.tensor([dx, dy, dz])
                    h = (c[:, 0] ^ (c[:, 1] * 2654435761) ^ (c[:, 2] * 805459861)) & ((1 << 19) - 1)       # :11-22 (uint32 arithmetic: the low 19 bits agree)
                    rows.update(h.tolist())
        assert rows <= set(live.tolist()), level
        assert live.numel() <= (res + 2) ** 3
    assert sum(stage1.live_rows(l).numel() for l in stage1.SPARSE_EXCHANGE_LEVELS) == 305480


def test_gpu_suite_runs_sharpest_first():
    """tests/conftest.py orders the GPU suite so that a stop at the first failure (the driver's `-x`) cannot erase parity evidence: kernels against the reference's native
    module / goldens / oracle, then glue and gradients, then full-size workloads, and every multi-hundred-step training run last."""
    import conftest
    rank = conftest.gpu_suite_rank
    order = [("test_gpu_ref_native.py", "test_near_far_vs_reference"), ("test_gpu_raymarch.py", "test_near_far_bit_exact"), ("test_gpu_field.py", "test_hash_rows_bit_exact_vs_reference"),
             ("test_gpu_render.py", "test_fused_decoder_matches_stock_operators"), ("test_gpu_render.py", "test_render_matches_reference_glue_golden"),
             ("test_gpu_stage1.py", "test_all_parameter_gradients_vs_oracle"), ("test_gpu_amp_ckpt.py", "test_checkpoint_save_load_renders_bit_identically"),
             ("test_gpu_fullsize.py", "test_full_workload_march_is_bit_exact"), ("test_gpu_render.py", "test_training_trajectory_psnr_and_bit_accuracy_track_the_oracle"),
             ("test_gpu_stage1.py", "test_captured_loop_tracks_the_cpu_oracle_over_200_steps"), ("test_gpu_convergence.py", "test_two_hundred_steps_tracked_by_the_oracle_from_a_warm_state"),
             ("test_gpu_convergence.py", "test_bench_size_training_converges_the_same_in_every_execution_mode")]
    keys = [rank(*t) for t in order]
    assert keys == sorted(keys), keys
    assert rank("test_gpu_amp_ckpt.py", "test_dense_takeover_is_torch_adam_arithmetic")[0] < rank("test_gpu_convergence.py", "test_anything")[0] == 3


def test_adam_state_of_the_native_passes_is_torch_adams_own(monkeypatch):
    """The state the native Adam passes create on first use is torch.optim.Adam's own, in both of its formats, on a CPU parameter (the launch itself stubbed out):
    the host-count form (optim.fused_shared_step, the hooks) against what Adam creates on its first step(); the device-count form (optim._prepare_device_state, the
    captured loops) against Adam(capturable=True)'s; the move of an existing host count to the device form; and either one's state_dict() in a plain Adam."""
    import types
    from nerf_signature_amd import optim
    launched = []
    monkeypatch.setattr(optim, "nv", types.SimpleNamespace(ptr=lambda t: None if t is None else t.data_ptr(), stream=lambda: None,
                                                           ptr_array=lambda ts: [t.data_ptr() for t in ts], call=lambda name, *a: launched.append(name)))
    torch.manual_seed(0)
    kw = dict(lr=1e-2, betas=(0.9, 0.99), eps=1e-15)
    layout = lambda st: {k: (v.dtype, tuple(v.shape), v.device) for k, v in st.items()}

    # host counts: torch.optim.Adam after its first step()
    p, q = torch.nn.Parameter(torch.randn(7, 2)), torch.nn.Parameter(torch.randn(7, 2))
    q.grad = torch.ones_like(q)
    ref = torch.optim.Adam([q], **kw)
    ref.step()
    opt = torch.optim.Adam([p], **kw)
    optim.fused_shared_step(opt, opt.param_groups[0], [p], torch.zeros(7, 2))
    assert launched == ["opt_codebook_adam"]
    host = opt.state[p]
    assert list(host) == list(ref.state[q]) == ["step", "exp_avg", "exp_avg_sq"] and layout(host) == layout(ref.state[q])
    assert float(host["step"]) == float(ref.state[q]["step"]) == 1.0 and not host["exp_avg"].any() and not host["exp_avg_sq"].any()

    # device counts: what Adam(capturable=True) creates (its _init_group; its step() itself refuses a CPU parameter)
    cap = torch.optim.Adam([q], capturable=True, **kw)
    cap._init_group(cap.param_groups[0], [], [], [], [], [], [])
    p2 = torch.nn.Parameter(torch.randn(3, 5))
    opt2 = torch.optim.Adam([p2], **kw)
    optim._prepare_device_state(opt2, [p2])
    dev = opt2.state[p2]
    assert list(dev) == list(cap.state[q]) and {k: v[:1] + v[2:] for k, v in layout(dev).items()} == {k: v[:1] + v[2:] for k, v in layout(cap.state[q]).items()}
    assert dev["step"].dim() == 0 and dev["step"].dtype == torch.float32 and dev["step"].device == p2.device and float(dev["step"]) == 0.0
    assert dev["exp_avg"].shape == dev["exp_avg_sq"].shape == p2.shape and not dev["exp_avg"].any() and not dev["exp_avg_sq"].any()

    # an existing host-count state taken to the device form: only `step` is touched, its value kept
    m, v = host["exp_avg"], host["exp_avg_sq"]
    optim._prepare_device_state(opt, [p])
    moved = opt.state[p]
    assert moved is host and moved["exp_avg"] is m and moved["exp_avg_sq"] is v and list(moved) == ["step", "exp_avg", "exp_avg_sq"]
    assert moved["step"].dim() == 0 and moved["step"].dtype == torch.float32 and moved["step"].device == p.device and float(moved["step"]) == 1.0

    # either format's state_dict() is a plain torch.optim.Adam's
    for o, t in ((opt, p), (opt2, p2)):
        fresh_p = torch.nn.Parameter(t.detach().clone())
        fresh = torch.optim.Adam([fresh_p], **kw)
        fresh.load_state_dict(o.state_dict())
        count = float(o.state[t]["step"])      # (a host count travels through state_dict() as the tensor itself)
        assert layout(fresh.state[fresh_p]) == layout(o.state[t]) and float(fresh.state[fresh_p]["step"]) == float(o.state[t]["step"])
        fresh_p.grad = torch.ones_like(fresh_p)
        fresh.step()
        assert float(fresh.state[fresh_p]["step"]) == count + 1.0 and fresh.state[fresh_p]["exp_avg"].any()
