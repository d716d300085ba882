"""1-vs-all softmax loss timing: HyperGNN.softmax_loss forward alone and forward + backward, against the formulation a user
has without it — embs[q] @ embs.T in query chunks sized to 1 GB of scores, masked, logsumexp, autograd backward chunk by
chunk — at the sizes of BASELINE configs 3 and 2, with rank_candidates' time on the same box beside them.  Prints one JSON
line.

    python tools/softmax_time.py [--configs c3,c2] [--batches 1024,16384] [--reps 5] [--no-torch] [--candidates C[,C...]] [--bias]

Per config and B in (1,024, 16,384): medians of device-event windows (ms, warm) of the forward (no autograd graph), of the
forward plus backward down to d embs (both with a filter list per query built from `known` edges, 10 per query, and the
forward also without lists), and of the torch formulation; the peak memory each allocates beyond the embeddings
(torch.cuda.max_memory_allocated); the achieved fraction of the fp32 matrix peak, counting one B x N x d product forward
and four backward.  The torch formulation reports "does not fit" where it raises an out-of-memory error.  --no-torch leaves
it out (a counter collection of the kernels alone: tools/pmc.sh <prefix> softmax_bwd_kernel -- python tools/softmax_time.py
--configs c3 --batches 1024 --no-torch).

--candidates 16384,131072,N adds, per C, softmax_loss forward and forward + backward and bce_loss forward + backward (all
with lists) against a sorted random subset of C nodes (candidates=; "N" = every node, through the subset entry points; the
targets are drawn from the subset, so softmax_loss adds none): their times with C / N x the all-node time of the same call
beside them — bce_loss' all-node forward + backward is then timed as well — and, so that the two can be told apart from
noise, the all-node calls timed a second time after them (`*_again_ms`: the same code twice in one command).

--bias adds the same three calls (softmax_loss forward and forward + backward, bce_loss forward + backward, with lists) with a
random candidate_bias= (N(0, 1), one entry per node, requiring its gradient in the backward): `bias` holds their times, with
--candidates also against every subset; the calls without the keyword are then timed again (`*_again_ms`, as above)."""

from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from graph_hypernetwork_forge_amd import HyperGNN  # noqa: E402

CONFIGS = {"c3": dict(N=1_000_000, d=128, seed=1003), "c2": dict(N=100_000, d=64, seed=1002)}
FP32_MATRIX_PEAK_TF = 157.3
SCORE_BYTES = 1 << 30


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


def torch_loss(embs, q, t, ptr, idx, scale, backward):
    """The loss per query, chunk by chunk; with `backward` the gradient of its mean as well, accumulated chunk by chunk so
    that only one chunk's scores are alive at a time."""
    N, B = embs.size(0), q.numel()
    step = max(1, SCORE_BYTES // (4 * N))
    e = embs.detach().requires_grad_(backward)
    out = []
    for i in range(0, B, step):
        qi, ti = q[i:i + step], t[i:i + step]
        s = scale * (e[qi] @ e.T)
        tsc = s.gather(1, ti[:, None])[:, 0]
        lens = ptr[i + 1:i + 1 + qi.numel()] - ptr[i:i + qi.numel()]
        rows = torch.repeat_interleave(torch.arange(qi.numel(), device=e.device), lens)
        cols = idx[int(ptr[i]):int(ptr[i + qi.numel()])]
        keep = cols != ti[rows]                                             # the target always stays
        s = s.index_put((rows[keep], cols[keep]), torch.tensor(float("-inf"), device=e.device))
        loss = torch.logsumexp(s, 1) - tsc
        if backward:
            (loss.sum() / B).backward()
        out.append(loss.detach())
    return torch.cat(out), e.grad


def candidate_sets(spec, N, dev, seed):
    """{label: sorted int64 ids on the device} for a --candidates list ("N" = all nodes)"""
    sets = {}
    for item in [s for s in spec.split(",") if s]:
        C = N if item.upper() == "N" else int(item)
        gen = torch.Generator(device=dev).manual_seed(seed + C)
        sets[item.upper()] = torch.sort(torch.randperm(N, device=dev, generator=gen)[:C]).values if C < N else torch.arange(N, device=dev)
    return sets


def run_config(name, reps, batches, with_torch, candidates="", bias=False):
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
        r = {}
        r["rank_known_ms"], _, _ = timed(lambda: model.rank_candidates(embs, q, t, filt_ptr=ptr, filt_idx=idx), reps)
        r["fwd_ms"], _, _ = timed(lambda: model.softmax_loss(embs, q, t, scale=scale), reps)
        r["fwd_known_ms"], r["fwd_peak_bytes"], ours = timed(
            lambda: model.softmax_loss(embs, q, t, scale=scale, filt_ptr=ptr, filt_idx=idx), reps)

        def step():
            e = embs.detach().requires_grad_(True)
            loss = model.softmax_loss(e, q, t, scale=scale, filt_ptr=ptr, filt_idx=idx)
            loss.mean().backward()
            return loss.detach(), e.grad

        r["fwd_bwd_known_ms"], r["fwd_bwd_peak_bytes"], (_, grad) = timed(step, reps)
        r["fwd_fraction_of_fp32_matrix_peak"] = flops / (r["fwd_known_ms"] * 1e-3) / (FP32_MATRIX_PEAK_TF * 1e12)
        r["bwd_fraction_of_fp32_matrix_peak"] = (4 * flops / ((r["fwd_bwd_known_ms"] - r["fwd_known_ms"]) * 1e-3)
                                                 / (FP32_MATRIX_PEAK_TF * 1e12))
        def loss_step(kind, tt, cand, b=None):
            e = embs.detach().requires_grad_(True)
            b = None if b is None else b.detach().requires_grad_(True)
            if kind == "softmax":
                loss = model.softmax_loss(e, q, tt, scale=scale, filt_ptr=ptr, filt_idx=idx, candidates=cand, candidate_bias=b)
            else:
                loss = model.bce_loss(e, q, pos_ptr=ptr, pos_idx=idx, scale=scale, smoothing=0.1, candidates=cand, candidate_bias=b)
            loss.mean().backward()
            return loss.detach(), e.grad

        if candidates or bias:
            r["bce_fwd_bwd_known_ms"], _, _ = timed(lambda: loss_step("bce", t, None), reps)
        for label, cand in candidate_sets(candidates, N, dev, cfg["seed"]).items():
            C = cand.numel()
            tc = cand[torch.from_numpy(rng.integers(0, C, B)).to(dev)]      # targets among the candidates: none is added
            s = {"C": C}
            s["fwd_known_ms"], _, _ = timed(lambda: model.softmax_loss(embs, q, tc, scale=scale, filt_ptr=ptr, filt_idx=idx,
                                                                       candidates=cand), reps)
            s["fwd_bwd_known_ms"], s["fwd_bwd_peak_bytes"], _ = timed(lambda: loss_step("softmax", tc, cand), reps)
            s["bce_fwd_bwd_known_ms"], _, _ = timed(lambda: loss_step("bce", tc, cand), reps)
            for key in ("fwd_known_ms", "fwd_bwd_known_ms", "bce_fwd_bwd_known_ms"):
                s[key.replace("_ms", "_scaled_all_node_ms")] = r[key] * C / N
            r[f"candidates_{label}"] = s
        if bias:
            b = torch.randn(N, device=dev, generator=torch.Generator(device=dev).manual_seed(cfg["seed"] + B))
            s = {}
            s["fwd_known_ms"], _, _ = timed(lambda: model.softmax_loss(embs, q, t, scale=scale, filt_ptr=ptr, filt_idx=idx,
                                                                       candidate_bias=b), reps)
            s["fwd_bwd_known_ms"], s["fwd_bwd_peak_bytes"], _ = timed(lambda: loss_step("softmax", t, None, b), reps)
            s["bce_fwd_bwd_known_ms"], _, _ = timed(lambda: loss_step("bce", t, None, b), reps)
            for label, cand in candidate_sets(candidates, N, dev, cfg["seed"]).items():
                tc = cand[torch.from_numpy(np.random.default_rng(B + 1).integers(0, cand.numel(), B)).to(dev)]
                s[f"candidates_{label}"] = {
                    "fwd_known_ms": timed(lambda: model.softmax_loss(embs, q, tc, scale=scale, filt_ptr=ptr, filt_idx=idx, candidates=cand,
                                                                     candidate_bias=b), reps)[0],
                    "fwd_bwd_known_ms": timed(lambda: loss_step("softmax", tc, cand, b), reps)[0],
                    "bce_fwd_bwd_known_ms": timed(lambda: loss_step("bce", tc, cand, b), reps)[0]}
            r["bias"] = s
        if candidates or bias:
            r["fwd_known_again_ms"], _, _ = timed(lambda: model.softmax_loss(embs, q, t, scale=scale, filt_ptr=ptr, filt_idx=idx), reps)
            r["fwd_bwd_known_again_ms"], _, _ = timed(step, reps)
            r["bce_fwd_bwd_known_again_ms"], _, _ = timed(lambda: loss_step("bce", t, None), reps)
        if with_torch:
            for key, backward in (("torch_fwd", False), ("torch_fwd_bwd", True)):
                try:
                    r[key + "_ms"], r[key + "_peak_bytes"], ref = timed(lambda: torch_loss(embs, q, t, ptr, idx, scale, backward), reps)
                    r[key + "_loss_max_abs_diff"] = float((ref[0] - ours).abs().max())
                    if backward:
                        r["torch_grad_rel_l2_diff"] = float((ref[1] - grad).norm() / ref[1].norm())
                        r["fwd_bwd_speedup"] = r["torch_fwd_bwd_ms"] / r["fwd_bwd_known_ms"]
                    else:
                        r["fwd_speedup"] = r["torch_fwd_ms"] / r["fwd_known_ms"]
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
    ap.add_argument("--candidates", default="", help="C[,C...] or N: also time the losses against a sorted random subset")
    ap.add_argument("--bias", action="store_true", help="also time the losses with a random candidate_bias=, then the plain calls again")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("softmax_time.py measures on an MI355X; no HIP device here")
    out = {"tool": "softmax_time", "device": torch.cuda.get_device_name(0)}
    for name in args.configs.split(","):
        out[name] = run_config(name, args.reps, [int(b) for b in args.batches.split(",")], not args.no_torch, args.candidates, args.bias)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
