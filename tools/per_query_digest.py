"""Bits of the per-query family (negatives=[B, K]) through the public HyperGNN methods, for comparing two builds on one MI355X:
one sha256 per output tensor, as one JSON line.  Equal lines from two checkouts on the same machine mean the same bits.

    python tools/per_query_digest.py [--timeout 120] > digest.json

For fixed seeds, over the shapes of tests/test_distance_gpu.py::SHAPES: rank_candidates (greater, equal), softmax_loss,
negative_sampling_loss and pairwise_loss in both kinds (the loss, for pairwise_loss the active counts, and the gradients of
embs, of query_rows and of the bias) under the dot product without and with candidate_bias and under each distance=, with
query_rows given and not given.  A tenth of the negatives is padding (-1)
and every query meets its own target among its negatives once.  Each score ("dot", "dot_bias", "l1", "l2", "complex") runs in
a child process under its own time limit; after a child that fails or runs out of time nothing more is started."""

from __future__ import annotations

import argparse
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (d, K, B, N), as tests/test_distance_gpu.py::SHAPES ("complex" doubles d <= 3: it needs an even d)
SHAPES = [(1, 1, 1, 300), (3, 7, 5, 300), (3, 257, 5, 5000), (20, 8, 5, 300), (20, 63, 129, 5000), (20, 1000, 5, 300),
          (64, 9, 129, 300), (64, 65, 5, 300), (64, 257, 5, 300), (128, 64, 5, 5000), (128, 256, 5, 300), (128, 257, 5, 300),
          (200, 65, 5, 300), (256, 9, 5, 300), (256, 1000, 1, 300)]
SCORES = ("dot", "dot_bias", "l1", "l2", "complex")


def sha(t) -> str:
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def worker(score: str) -> dict:
    import numpy as np
    import torch
    import torch.nn.functional as F
    from graph_hypernetwork_forge_amd import HyperGNN

    if not torch.cuda.is_available():
        raise SystemExit("per_query_digest.py runs on an MI355X; no HIP device here")
    dev = torch.device("cuda:0")
    model = HyperGNN(text_dim=16, node_feat_dim=8, hidden_dim=16, num_layers=1).to(dev).eval()
    metric = None if score.startswith("dot") else score
    out = {}
    for d, K, B, N in SHAPES:
        d = 2 * d if metric == "complex" and d <= 3 else d
        gen = torch.Generator(device=dev).manual_seed(d * 1000 + K)
        embs = F.layer_norm(torch.randn(N, d, device=dev, generator=gen), (d,))
        rows = torch.randn(B, d, device=dev, generator=gen)
        bias = 0.5 * torch.randn(N, device=dev, generator=gen) if score == "dot_bias" else None
        rng = np.random.default_rng(K * 7 + B)
        q, t = rng.integers(0, N, B), rng.integers(0, N, B)
        neg = rng.integers(0, N, (B, K))
        neg[rng.random((B, K)) < 0.1] = -1
        neg[np.arange(B), rng.integers(0, K, B)] = t
        q, t, neg = (torch.from_numpy(v).to(dev) for v in (q, t, neg))
        scale = d ** -0.5 if metric in (None, "l2") else 2.0 / d
        for with_rows in (False, True):
            key = f"d{d}-K{K}-B{B}-N{N}-" + ("rows" if with_rows else "ids")
            kw = dict(negatives=neg)
            if metric is not None:
                kw["distance"] = metric
            with torch.no_grad():
                pre = dict(kw, candidate_bias=bias) if bias is not None else kw
                g, e = model.rank_candidates(embs, q, t, query_rows=rows if with_rows else None, **pre)
            out[key + "-rank"] = [sha(g), sha(e)]
            for name in ("softmax", "negsamp", "hinge", "logistic"):
                leaf = [embs.clone().requires_grad_(True)]
                leaf.append(rows.clone().requires_grad_(True) if with_rows else None)
                leaf.append(bias.clone().requires_grad_(True) if bias is not None else None)
                args = dict(kw, scale=scale, query_rows=leaf[1])
                if leaf[2] is not None:
                    args["candidate_bias"] = leaf[2]
                extra = []
                if name == "softmax":
                    loss = model.softmax_loss(leaf[0], q, t, **args)
                elif name == "negsamp":
                    loss = model.negative_sampling_loss(leaf[0], q, t, margin=1.5, adversarial_temperature=0.5, **args)
                else:
                    loss, active = model.pairwise_loss(leaf[0], q, t, loss=name, margin=0.25, return_active=True, **args)
                    extra = [sha(active)]
                (loss * torch.linspace(0.5, 1.5, B, device=dev)).sum().backward()
                out[f"{key}-{name}"] = [sha(loss)] + extra + [sha(v.grad) for v in leaf if v is not None]
    torch.cuda.synchronize()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--timeout", type=int, default=120, help="seconds per child process")
    ap.add_argument("--worker", choices=SCORES, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        print(json.dumps(worker(args.worker)))
        return
    out = {"tool": "per_query_digest"}
    for score in SCORES:
        r = subprocess.run(["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--worker", score],
                           capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-2000:])
            raise SystemExit(f"per_query_digest: the {score} step ended with status {r.returncode}; nothing more was started")
        out[score] = json.loads(r.stdout.strip().splitlines()[-1])
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
