"""Training through ShardedHyperGNN with the HIP kernels: 2-3 ranks share one MI355X and exchange over gloo.

Every parameter gradient (and the feature gradient) of a sharded training step against float64 autograd through the oracle,
bitwise the same on every rank, and close to the single-GPU HyperGNN's; the range guard's collective fallback in training;
three optimizer steps that keep the replicas identical; and ghf_rows_accumulate (csrc/exchange.hip) on its own.
"""

import os
import socket

import numpy as np
import pytest
import torch

import cases
from graph_hypernetwork_forge_amd import _native, synth
from oracle import hypergnn_oracle as O
from test_hip_parity import DEV, _adversarial_graph, _grad_check, make_model

pytestmark = pytest.mark.gpu

LR, STEPS = 1e-3, 3


def _inputs(name):
    if name.startswith("adversarial"):
        cfg, params, feats, ei_np, texts = _adversarial_graph(int(name.split(":")[1]))
        return cfg, params, feats, ei_np, texts
    (case,) = cases.graph_cases(only=[name])
    cfg = cases.MODELS[case.model]
    return cfg, cfg.params(), case.node_features, case.edge_index, case.edge_texts


def _gout(n, d):
    return synth.normal(41, "gout", (n, d))


def _negatives(step, E):
    return torch.randperm(E, generator=torch.Generator().manual_seed(1000 + step)).to(DEV)


def _demo_loss(model, embs, ei, step):
    """The margin loss of the reference demo (demo.py:79-101) over every edge, negatives from a seeded generator."""
    src, dst = ei
    pos = model.score_edges(embs, src, dst)
    neg = model.score_edges(embs, src, dst[_negatives(step, dst.numel())])
    return torch.clamp(1.0 - pos + neg, min=0.0).mean()


def _rank_worker(rank, world, port, name, kw, job, ret):
    import torch.distributed as dist
    from graph_hypernetwork_forge_amd.dist import ShardedHyperGNN
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        cfg, params, feats, ei_np, texts = _inputs(name)
        model = make_model(cfg, params).train()
        runner = ShardedHyperGNN(model, chunks=3, **kw)
        x, ei = torch.from_numpy(feats).to(DEV), torch.from_numpy(ei_np).to(DEV)
        if job == "adam":
            opt = torch.optim.Adam(model.parameters(), lr=LR)
            for step in range(STEPS):
                opt.zero_grad()
                _demo_loss(model, runner(x, ei, texts), ei, step).backward()
                opt.step()
            torch.cuda.synchronize()
            ret[rank] = {k: p.detach().cpu().numpy() for k, p in model.named_parameters()}
            return
        x.requires_grad_(True)
        out = runner(x, ei, texts)
        assert out.grad_fn is not None
        (out * torch.from_numpy(_gout(*out.shape)).to(DEV)).sum().backward()
        torch.cuda.synchronize()
        grads = {k: p.grad.cpu().numpy() for k, p in model.named_parameters() if p.grad is not None}
        grads["node_features"] = x.grad.cpu().numpy()
        ret[rank] = (out.detach().cpu().numpy(), grads, runner.last_range_flags, runner.stats.get("bytes_recv_bwd", 0.0))
    finally:
        dist.destroy_process_group()


def _run(world, name, kw, job="grads"):
    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ret = mp.get_context("spawn").Manager().dict()
    mp.spawn(_rank_worker, args=(world, port, name, kw, job, ret), nprocs=world, join=True)
    assert sorted(ret.keys()) == list(range(world))
    return [ret[r] for r in range(world)]


def _oracle_grads(params, feats, ei_np, texts, gout):
    ref_p = {k: torch.from_numpy(np.ascontiguousarray(v)).double().requires_grad_(True) for k, v in params.items()}
    xr = torch.from_numpy(feats).double().requires_grad_(True)
    ref = O.forward(ref_p, xr, ei_np, texts, variant="factorised", dtype=torch.float64)
    (ref * torch.from_numpy(gout).double()).sum().backward()
    grads = {k: p.grad.numpy() for k, p in ref_p.items()}
    grads["node_features"] = xr.grad.numpy()
    return ref.detach().float().numpy(), grads


def _single_gpu_grads(cfg, params, feats, ei_np, texts, gout):
    model = make_model(cfg, params).train()
    x = torch.from_numpy(feats).to(DEV).requires_grad_(True)
    out = model(x, torch.from_numpy(ei_np).to(DEV), texts)
    (out * torch.from_numpy(gout).to(DEV)).sum().backward()
    grads = {k: p.grad.cpu().numpy() for k, p in model.named_parameters()}
    grads["node_features"] = x.grad.cpu().numpy()
    return grads


@pytest.mark.parametrize("name,world,kw", [
    ("g6_c3", 2, {}), ("g5_c2", 2, {}), ("g3_mid32", 3, {}),
    ("g6_c3", 3, dict(exchange="pairs")), ("g5_c2", 3, dict(exchange="pairs")),
    ("g6_c3", 2, dict(exchange="sparse")), ("g5_c2", 3, dict(exchange="sparse")), ("g3_mid32", 2, dict(exchange="sparse")),
    ("g6_c3_powerlaw", 2, dict(balance="edges")), ("g6_c3_powerlaw", 3, dict(balance="edges", exchange="sparse")),
])
def test_sharded_training_matches_the_oracle_and_one_gpu(name, world, kw):
    """d = 128 (the split-form kernel with its side output), d = 64, d = 32 (the generic kernel); every exchange and its adjoint;
    slots balanced by in-edges on a power-law graph."""
    cfg, params, feats, ei_np, texts = _inputs(name)
    res = _run(world, name, kw)
    gout = _gout(feats.shape[0], cfg.hidden_dim)
    ref_out, ref = _oracle_grads(params, feats, ei_np, texts, gout)
    single = _single_gpu_grads(cfg, params, feats, ei_np, texts, gout)
    for r in range(world):
        out, grads, flags, nbytes = res[r]
        assert flags == 0 and nbytes > 0
        np.testing.assert_allclose(out, ref_out, rtol=1e-4, atol=1e-5)
        for k in ref:
            if float(np.abs(ref[k]).max()) == 0.0:                       # (char embeddings no relation string uses)
                assert k not in grads or float(np.abs(grads[k]).max()) == 0.0
                continue
            _grad_check(f"{k} rank {r}", grads[k], ref[k])
            _grad_check(f"{k} rank {r} vs one GPU", grads[k], single[k], rtol=5e-4, l2=1e-4)
            assert np.array_equal(grads[k], res[0][1][k]), f"d{k} differs between rank {r} and rank 0"


def test_sharded_training_falls_back_collectively_when_the_range_guard_fires():
    """Rows the two-fp16-piece kernels cannot hold: the guard fires on some rank, every rank records the layers again on the
    exact shard plans, and the gradients are the oracle's."""
    cfg, params, feats, ei_np, texts = _adversarial_graph(128)
    res = _run(2, "adversarial:128", {})
    ref_out, ref = _oracle_grads(params, feats, ei_np, texts, _gout(feats.shape[0], 128))
    for r in range(2):
        out, grads, flags, _ = res[r]
        assert flags & _native.RANGE_ROWS, "the guard must have fired on some rank and be seen on every rank"
        np.testing.assert_allclose(out, ref_out, rtol=1e-4, atol=1e-5 * float(np.abs(ref_out).max()))
        for k in ref:
            if float(np.abs(ref[k]).max()) == 0.0:                       # (the adversarial model zeroes generator weights)
                assert k not in grads or float(np.abs(grads[k]).max()) == 0.0
                continue
            _grad_check(f"{k} rank {r}", grads[k], ref[k])
            assert np.array_equal(grads[k], res[0][1][k])


def test_adam_steps_keep_the_replicas_identical():
    """Three Adam steps of the demo loss (score_edges over the replicated output, the same negatives on every rank): the
    replicas stay bit-identical without any parameter broadcast, and follow the steps of one process."""
    name = "g6_c3"
    res = _run(2, name, {}, job="adam")
    cfg, params, feats, ei_np, texts = _inputs(name)
    model = make_model(cfg, params).train()
    opt = torch.optim.Adam(model.parameters(), lr=LR)
    x, ei = torch.from_numpy(feats).to(DEV), torch.from_numpy(ei_np).to(DEV)
    for step in range(STEPS):
        opt.zero_grad()
        _demo_loss(model, model(x, ei, texts), ei, step).backward()
        opt.step()
    one = {k: p.detach().cpu().numpy() for k, p in model.named_parameters()}
    moved = dsum = 0.0
    for k, p0 in params.items():
        for r in range(2):
            assert np.array_equal(res[r][k], res[0][k]), f"{k} differs between the ranks"
        d_one, d_sharded = one[k] - p0, res[0][k] - p0
        moved += float((d_one.astype(np.float64) ** 2).sum())
        dsum += float(((d_sharded - d_one).astype(np.float64) ** 2).sum())
    # (Adam moves a parameter by about LR whatever its gradient's size: where a gradient is at the rounding level, the two
    # runs may step opposite ways — a few such elements, not a different trajectory)
    assert moved > 0.0 and dsum ** 0.5 <= 3e-2 * moved ** 0.5, (dsum ** 0.5, moved ** 0.5)


def test_rows_accumulate_is_fp32_addition_in_call_order():
    g = torch.Generator().manual_seed(5)
    nrows, d, n = 1000, 132, 300
    rows = torch.randn(nrows, d, generator=g)
    idx = torch.randperm(nrows, generator=g)[:n]
    a, b = torch.randn(n, d, generator=g), torch.randn(n, d, generator=g)
    dev_rows = rows.to(DEV)
    _native.rows_accumulate(dev_rows, idx.to(DEV), a.to(DEV))
    _native.rows_accumulate(dev_rows, idx.to(DEV), b.to(DEV))         # two calls onto the same rows, in this order
    want = rows.numpy().copy()
    want[idx.numpy()] = (want[idx.numpy()] + a.numpy()) + b.numpy()
    torch.cuda.synchronize()
    assert np.array_equal(dev_rows.cpu().numpy(), want)
    # idx None: rows 0..n-1; out-of-range ids skipped; n = 0
    r2 = rows.to(DEV)
    _native.rows_accumulate(r2[:n], None, a.to(DEV))
    bad = torch.tensor([-1, nrows, 3, nrows + 7], dtype=torch.int64, device=DEV)
    _native.rows_accumulate(r2, bad, b[:4].to(DEV))
    _native.rows_accumulate(r2, torch.zeros(0, dtype=torch.int64, device=DEV), torch.zeros(0, d, device=DEV))
    want = rows.numpy().copy()
    want[:n] += a.numpy()
    want[3] += b.numpy()[2]
    assert np.array_equal(r2.cpu().numpy(), want)
    # a misaligned buffer is refused before any launch
    base = torch.zeros(nrows * d + 1, device=DEV)
    with pytest.raises(ValueError, match="misaligned"):
        _native.rows_accumulate(base[1:].view(nrows, d), None, a.to(DEV))
    with pytest.raises(ValueError):
        _native.rows_accumulate(r2, idx.to(DEV).to(torch.int32), a.to(DEV))
    with pytest.raises(ValueError):
        _native.rows_accumulate(r2, idx.to(DEV), a[:-1].to(DEV))
