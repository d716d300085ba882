"""Link-prediction timing: HyperGNN.rank_candidates and topk_candidates(k = 10) against the formulation a user has without
them — embs[q] @ embs.T in query chunks sized to 1 GB of scores, then compare-and-count (resp. torch.topk) — at the sizes of
BASELINE configs 3 and 2.  Prints one JSON line.

    python tools/rank_time.py [--configs c3,c2] [--batches 1024,16384] [--reps 5] [--no-torch] [--candidates C[,C...]] [--bias]

Per config and B in (1,024, 16,384): medians of device-event windows (ms, warm) of the two calls without filter lists, of
the two calls with a filter list per query built from `known` edges (10 per query), and of the torch formulation; the ratio
torch / ours; the achieved fraction of the fp32 matrix peak, 2 B N d / time / 157.3 TF.  The embeddings are LayerNorm-shaped
random rows of the config's [N, d] (what the model's last layer emits): the time does not depend on their values beyond the
insertion rate of the top-k lists, which random rows set at its expected k ln(N / k).  --no-torch leaves the torch
formulation out (a counter collection of the kernels alone: tools/pmc.sh <prefix> rank_tile_kernel -- python tools/rank_time.py
--configs c3 --batches 1024 --no-torch).

--candidates 16384,131072,N adds, per C, the two calls with lists against a sorted random subset of C nodes (candidates=;
"N" = every node, through the subset entry points): their times, C / N x the all-node time of the same call beside them, and,
so that the two can be told apart from noise, the all-node calls timed a second time after them (`*_again_ms`: the same code
twice in one command).

--bias adds the two calls with lists and a random candidate_bias= (N(0, 1), one entry per node): `bias` holds their times,
after which the calls without the keyword are timed again (`*_again_ms`, as above: the same-code spread of this command);
with --candidates also the biased calls against every subset (`candidates_<C>` inside `bias`)."""

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
    """(median ms, last result) over `reps` device-event windows, after two warm-up calls."""
    for _ in range(2):
        out = fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), out


def torch_rank(embs, q, t):
    N = embs.size(0)
    step = max(1, SCORE_BYTES // (4 * N))
    greater, equal = [], []
    for i in range(0, q.numel(), step):
        s = embs[q[i:i + step]] @ embs.T
        ti = s.gather(1, t[i:i + step, None])
        greater.append((s > ti).sum(1))
        equal.append((s == ti).sum(1) - 1)
    return torch.cat(greater), torch.cat(equal)


def torch_topk(embs, q, k):
    N = embs.size(0)
    step = max(1, SCORE_BYTES // (4 * N))
    parts = [torch.topk(embs[q[i:i + step]] @ embs.T, k, dim=1) for i in range(0, q.numel(), step)]
    return torch.cat([p.values for p in parts]), torch.cat([p.indices for p in parts])


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
    res = {}
    for B in batches:
        rng = np.random.default_rng(B)
        q = torch.from_numpy(rng.integers(0, N, B)).to(dev)
        t = torch.from_numpy(rng.integers(0, N, B)).to(dev)
        known = (q.repeat(10), torch.from_numpy(rng.integers(0, N, 10 * B)).to(dev))
        flops = 2.0 * B * N * d
        r = {}
        r["rank_ms"], ours = timed(lambda: model.rank_candidates(embs, q, t), reps)
        r["rank_known_ms"], _ = timed(lambda: model.rank_candidates(embs, q, t, known=known), reps)
        if with_torch:
            r["torch_rank_ms"], ref = timed(lambda: torch_rank(embs, q, t), reps)
            r["rank_greater_max_diff_vs_torch"] = int((ours[0] - ref[0]).abs().max())     # rocBLAS sums in another order
            r["rank_speedup"] = r["torch_rank_ms"] / r["rank_ms"]
        r["topk_ms"], ours = timed(lambda: model.topk_candidates(embs, q, 10), reps)
        r["topk_known_ms"], _ = timed(lambda: model.topk_candidates(embs, q, 10, known=known), reps)
        if with_torch:
            r["torch_topk_ms"], ref = timed(lambda: torch_topk(embs, q, 10), reps)
            r["topk_ids_equal_fraction"] = float((ours[1] == ref[1]).float().mean())
            r["topk_speedup"] = r["torch_topk_ms"] / r["topk_ms"]
        r["rank_fraction_of_fp32_matrix_peak"] = flops / (r["rank_ms"] * 1e-3) / (FP32_MATRIX_PEAK_TF * 1e12)
        r["topk_fraction_of_fp32_matrix_peak"] = flops / (r["topk_ms"] * 1e-3) / (FP32_MATRIX_PEAK_TF * 1e12)
        for label, cand in candidate_sets(candidates, N, dev, cfg["seed"]).items():
            C = cand.numel()
            tc = cand[torch.from_numpy(rng.integers(0, C, B)).to(dev)]      # targets among the candidates
            s = {"C": C}
            s["rank_known_ms"], _ = timed(lambda: model.rank_candidates(embs, q, tc, known=known, candidates=cand), reps)
            s["topk_known_ms"], _ = timed(lambda: model.topk_candidates(embs, q, 10, known=known, candidates=cand), reps)
            s["rank_known_scaled_all_node_ms"] = r["rank_known_ms"] * C / N
            s["topk_known_scaled_all_node_ms"] = r["topk_known_ms"] * C / N
            r[f"candidates_{label}"] = s
        if bias:
            b = torch.randn(N, device=dev, generator=torch.Generator(device=dev).manual_seed(cfg["seed"] + B))
            s = {}
            s["rank_known_ms"], _ = timed(lambda: model.rank_candidates(embs, q, t, known=known, candidate_bias=b), reps)
            s["topk_known_ms"], _ = timed(lambda: model.topk_candidates(embs, q, 10, known=known, candidate_bias=b), reps)
            for label, cand in candidate_sets(candidates, N, dev, cfg["seed"]).items():
                tc = cand[torch.from_numpy(np.random.default_rng(B + 1).integers(0, cand.numel(), B)).to(dev)]
                s[f"candidates_{label}"] = {
                    "rank_known_ms": timed(lambda: model.rank_candidates(embs, q, tc, known=known, candidates=cand, candidate_bias=b), reps)[0],
                    "topk_known_ms": timed(lambda: model.topk_candidates(embs, q, 10, known=known, candidates=cand, candidate_bias=b), reps)[0]}
            r["bias"] = s
        if candidates or bias:
            r["rank_known_again_ms"], _ = timed(lambda: model.rank_candidates(embs, q, t, known=known), reps)
            r["topk_known_again_ms"], _ = timed(lambda: model.topk_candidates(embs, q, 10, known=known), reps)
        res[f"B{B}"] = r
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c3,c2")
    ap.add_argument("--batches", default="1024,16384")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--candidates", default="", help="C[,C...] or N: also time the calls against a sorted random subset")
    ap.add_argument("--bias", action="store_true", help="also time the calls with a random candidate_bias=, then the plain calls again")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rank_time.py measures on an MI355X; no HIP device here")
    out = {"tool": "rank_time", "device": torch.cuda.get_device_name(0)}
    for name in args.configs.split(","):
        out[name] = run_config(name, args.reps, [int(b) for b in args.batches.split(",")], not args.no_torch, args.candidates, args.bias)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
