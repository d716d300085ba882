"""Multi-label 1-vs-all BCE loss timing: HyperGNN.bce_loss forward alone and forward + backward, against softmax_loss at the
same B in the same process and against the formulation a user has without it — embs[q] @ embs.T in query chunks sized to 1 GB
of logits, dense labels, binary_cross_entropy_with_logits, autograd backward chunk by chunk — at the sizes of BASELINE
configs 3 and 2.  Prints one JSON line.

    python tools/bce_time.py [--configs c3,c2] [--batches 1024,16384] [--reps 5] [--no-torch] [--bias]

Per config and B in (1,024, 16,384), ten positives per query, smoothing 0.1, scale d^-1/2: medians of device-event windows
(ms, warm) of the forward (no autograd graph; also without lists), of the forward plus backward down to d embs, of
softmax_loss on the same queries and lists (a random target), and of the torch formulation; the ratios bce / softmax; the
peak memory each allocates beyond the embeddings; the achieved fraction of the fp32 matrix peak, counting one B x N x d
product forward and four backward.  The torch formulation reports "does not fit" where it raises an out-of-memory error.
--no-torch leaves it out (a counter collection of the kernels alone).

--bias adds bce_loss forward and forward + backward with a random candidate_bias= (a learned entity bias: N(0, 1), one entry
per node, requiring its gradient in the backward; `bias` holds the times), then times the two calls without the keyword
again (`fwd_again_ms`, `fwd_bwd_again_ms`: the same code twice in one command, i.e. the spread)."""

from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from graph_hypernetwork_forge_amd import HyperGNN  # noqa: E402

CONFIGS = {"c3": dict(N=1_000_000, d=128, seed=1003), "c2": dict(N=100_000, d=64, seed=1002)}
FP32_MATRIX_PEAK_TF = 157.3
SCORE_BYTES = 1 << 30
SMOOTHING = 0.1


def timed(fn, reps):
    """(median ms, peak bytes allocated above the starting level, last result) over `reps` device-event windows, after two
    warm-up calls."""
    for _ in range(2):
        out = fn()
    del out
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), int(torch.cuda.max_memory_allocated() - base), out


def torch_loss(embs, q, ptr, idx, scale, backward):
    """The loss per query (mean over the candidates), chunk by chunk; with `backward` the gradient of its mean as well,
    accumulated chunk by chunk so that only one chunk's logits and labels are alive at a time."""
    N, B = embs.size(0), q.numel()
    step = max(1, SCORE_BYTES // (4 * N))
    e = embs.detach().requires_grad_(backward)
    out = []
    for i in range(0, B, step):
        qi = q[i:i + step]
        s = scale * (e[qi] @ e.T)
        lens = ptr[i + 1:i + 1 + qi.numel()] - ptr[i:i + qi.numel()]
        rows = torch.repeat_interleave(torch.arange(qi.numel(), device=e.device), lens)
        cols = idx[int(ptr[i]):int(ptr[i + qi.numel()])]
        y = torch.full_like(s, SMOOTHING / N)
        y[rows, cols] = (1.0 - SMOOTHING) + SMOOTHING / N
        loss = F.binary_cross_entropy_with_logits(s, y, reduction="none").mean(1)
        if backward:
            (loss.sum() / B).backward()
        out.append(loss.detach())
    return torch.cat(out), e.grad


def run_config(name, reps, batches, with_torch, bias=False):
    cfg = CONFIGS[name]
    dev = torch.device("cuda:0")
    N, d = cfg["N"], cfg["d"]
    gen = torch.Generator(device=dev).manual_seed(cfg["seed"])
    embs = torch.nn.functional.layer_norm(torch.randn(N, d, device=dev, generator=gen), (d,),
                                          1.0 + 0.1 * torch.randn(d, device=dev, generator=gen),
                                          0.1 * torch.randn(d, device=dev, generator=gen))
    model = HyperGNN(text_dim=16, node_feat_dim=8, hidden_dim=16, num_layers=1).to(dev).eval()
    scale = d ** -0.5
    res = {}
    for B in batches:
        rng = np.random.default_rng(B)
        q = torch.from_numpy(rng.integers(0, N, B)).to(dev)
        t = torch.from_numpy(rng.integers(0, N, B)).to(dev)
        known = (q.repeat(10), torch.from_numpy(rng.integers(0, N, 10 * B)).to(dev))
        ptr, idx = model._filter_lists(embs, q, known, None, None)
        flops = 2.0 * B * N * d
        kw = dict(scale=scale, smoothing=SMOOTHING, pos_ptr=ptr, pos_idx=idx)
        r = {}
        r["softmax_fwd_ms"], _, _ = timed(lambda: model.softmax_loss(embs, q, t, scale=scale, filt_ptr=ptr, filt_idx=idx), reps)
        r["fwd_no_lists_ms"], _, _ = timed(lambda: model.bce_loss(embs, q, scale=scale, smoothing=SMOOTHING), reps)
        r["fwd_ms"], r["fwd_peak_bytes"], ours = timed(lambda: model.bce_loss(embs, q, **kw), reps)

        def softmax_step():
            e = embs.detach().requires_grad_(True)
            model.softmax_loss(e, q, t, scale=scale, filt_ptr=ptr, filt_idx=idx).mean().backward()
            return e.grad

        def step():
            e = embs.detach().requires_grad_(True)
            loss = model.bce_loss(e, q, **kw)
            loss.mean().backward()
            return loss.detach(), e.grad

        r["softmax_fwd_bwd_ms"], _, _ = timed(softmax_step, reps)
        r["fwd_bwd_ms"], r["fwd_bwd_peak_bytes"], (_, grad) = timed(step, reps)
        r["fwd_over_softmax"] = r["fwd_ms"] / r["softmax_fwd_ms"]
        r["fwd_bwd_over_softmax"] = r["fwd_bwd_ms"] / r["softmax_fwd_bwd_ms"]
        r["bwd_over_softmax"] = (r["fwd_bwd_ms"] - r["fwd_ms"]) / (r["softmax_fwd_bwd_ms"] - r["softmax_fwd_ms"])
        r["fwd_fraction_of_fp32_matrix_peak"] = flops / (r["fwd_ms"] * 1e-3) / (FP32_MATRIX_PEAK_TF * 1e12)
        r["bwd_fraction_of_fp32_matrix_peak"] = (4 * flops / ((r["fwd_bwd_ms"] - r["fwd_ms"]) * 1e-3) / (FP32_MATRIX_PEAK_TF * 1e12))
        if bias:
            b = torch.randn(N, device=dev, generator=torch.Generator(device=dev).manual_seed(cfg["seed"] + B))

            def bias_step():
                e, p = embs.detach().requires_grad_(True), b.detach().requires_grad_(True)
                loss = model.bce_loss(e, q, candidate_bias=p, **kw)
                loss.mean().backward()
                return loss.detach(), e.grad, p.grad

            s = {}
            s["fwd_ms"], _, _ = timed(lambda: model.bce_loss(embs, q, candidate_bias=b, **kw), reps)
            s["fwd_bwd_ms"], s["fwd_bwd_peak_bytes"], _ = timed(bias_step, reps)
            r["bias"] = s
            r["fwd_again_ms"], _, _ = timed(lambda: model.bce_loss(embs, q, **kw), reps)
            r["fwd_bwd_again_ms"], _, _ = timed(step, reps)
        if with_torch:
            for key, backward in (("torch_fwd", False), ("torch_fwd_bwd", True)):
                try:
                    r[key + "_ms"], r[key + "_peak_bytes"], ref = timed(lambda: torch_loss(embs, q, ptr, idx, scale, backward), reps)
                    r[key + "_loss_max_rel_diff"] = float(((ref[0] - ours).abs() / ref[0].abs()).max())
                    if backward:
                        r["torch_grad_rel_l2_diff"] = float((ref[1] - grad).norm() / ref[1].norm())
                        r["fwd_bwd_speedup"] = r["torch_fwd_bwd_ms"] / r["fwd_bwd_ms"]
                    else:
                        r["fwd_speedup"] = r["torch_fwd_ms"] / r["fwd_ms"]
                    del ref
                except torch.cuda.OutOfMemoryError:
                    r[key + "_ms"] = "does not fit"
                    torch.cuda.empty_cache()
        res[f"B{B}"] = r
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c3,c2")
    ap.add_argument("--batches", default="1024,16384")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--bias", action="store_true", help="also time the loss with a random candidate_bias=, then the plain calls again")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bce_time.py measures on an MI355X; no HIP device here")
    out = {"tool": "bce_time", "device": torch.cuda.get_device_name(0)}
    for name in args.configs.split(","):
        out[name] = run_config(name, args.reps, [int(b) for b in args.batches.split(",")], not args.no_torch, args.bias)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
