"""Bits of the shared-set distance family through the public HyperGNN methods, for comparing two builds on one MI355X: one
sha256 per output tensor, as one JSON line.  Equal lines from two checkouts on the same machine mean the same bits.

    python tools/sweep_digest.py [--timeout 120] > digest.json

For fixed seeds, over the shapes of tests/test_distance_loss_host.py::SHAPES: softmax_loss_by_distance,
negative_sampling_loss_by_distance (margin 1.5, temperature 0.5) and pairwise_loss_by_distance in both kinds with normalize on
and off (the loss, for the pairwise losses the active counts, and the gradients of embs and of query_rows), rank_by_distance
(greater, equal) and topk_by_distance (k = 10: scores, ids), each in two forms: "all", every node a candidate, the queries'
own rows and known=(src, dst); and "sub", a shuffled candidates= subset of twice as many nodes, query_rows given and the
lists as CSR.  Each metric ("l1", "l2", "complex") runs in a child process under its own time limit; the parent never opens
the device, and after a child that fails or runs out of time nothing more is started."""

from __future__ import annotations

import argparse
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (d, C, B), as tests/test_distance_loss_host.py::SHAPES ("complex" doubles d <= 3: it needs an even d)
SHAPES = [(1, 1, 1), (3, 2, 5), (4, 255, 64), (6, 256, 65), (20, 257, 129), (64, 1023, 5), (130, 1025, 64), (256, 2600, 5),
          (20, 2600, 129), (4, 513, 5), (6, 63, 65), (6, 64, 63), (6, 65, 64), (6, 70, 513)]
METRICS = ("l1", "l2", "complex")


def sha(t) -> str:
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def worker(metric: str) -> dict:
    import numpy as np
    import torch
    import torch.nn.functional as F
    from graph_hypernetwork_forge_amd import HyperGNN

    if not torch.cuda.is_available():
        raise SystemExit("sweep_digest.py runs on an MI355X; no HIP device here")
    dev = torch.device("cuda:0")
    model = HyperGNN(text_dim=16, node_feat_dim=8, hidden_dim=16, num_layers=1).to(dev).eval()
    out = {}
    for d, C, B in SHAPES:
        d = 2 * d if metric == "complex" and d <= 3 else d
        scale = d ** -0.5 if metric == "l2" else 2.0 / d
        for form in ("all", "sub"):
            N = C if form == "all" else 2 * C + 3
            gen = torch.Generator(device=dev).manual_seed(d * 1000 + C + (form == "sub"))
            embs = F.layer_norm(torch.randn(N, d, device=dev, generator=gen), (d,))
            rng = np.random.default_rng(C * 7 + B + (form == "sub"))
            if form == "all":
                q, t = rng.integers(0, N, B), rng.integers(0, N, B)
                src, dst = np.repeat(q, 3), rng.integers(0, N, 3 * B)      # three known partners a query, repeats allowed
                kw = dict(known=(torch.from_numpy(src).to(dev), torch.from_numpy(dst).to(dev)))
                rows = None
            else:
                cand = rng.permutation(N)[:C]
                q, t = rng.integers(0, N, B), cand[rng.integers(0, C, B)]  # the targets are candidates: the set stays C
                lists = [np.unique(rng.integers(0, N, rng.integers(0, 6))) for _ in range(B)]
                ptr = np.concatenate([[0], np.cumsum([len(v) for v in lists])]).astype(np.int64)
                idx = np.concatenate(lists + [np.zeros(0, np.int64)]).astype(np.int64)
                kw = dict(candidates=torch.from_numpy(cand).to(dev), filt_ptr=torch.from_numpy(ptr).to(dev),
                          filt_idx=torch.from_numpy(idx).to(dev))
                rows = torch.randn(B, d, device=dev, generator=gen)
            q, t = torch.from_numpy(q).to(dev), torch.from_numpy(t).to(dev)
            key = f"d{d}-C{C}-B{B}-{form}"
            with torch.no_grad():
                g, e = model.rank_by_distance(embs, q, t, metric, query_rows=rows, **kw)
                s, ids = model.topk_by_distance(embs, q, 10, metric, query_rows=rows, **kw)
            out[key + "-rank"] = [sha(g), sha(e)]
            out[key + "-topk"] = [sha(s), sha(ids)]
            for name in ("softmax", "negsamp", "hinge", "hinge-sum", "logistic", "logistic-sum"):
                leaf = [embs.clone().requires_grad_(True), None if rows is None else rows.clone().requires_grad_(True)]
                args = dict(kw, scale=scale, query_rows=leaf[1])
                extra = []
                if name == "softmax":
                    loss = model.softmax_loss_by_distance(leaf[0], q, t, metric, **args)
                elif name == "negsamp":
                    loss = model.negative_sampling_loss_by_distance(leaf[0], q, t, metric, margin=1.5, adversarial_temperature=0.5,
                                                                    **args)
                else:
                    loss, active = model.pairwise_loss_by_distance(leaf[0], q, t, metric, loss=name.split("-")[0], margin=0.25,
                                                                   normalize=not name.endswith("-sum"), return_active=True, **args)
                    extra = [sha(active)]
                (loss * torch.linspace(0.5, 1.5, B, device=dev)).sum().backward()
                out[f"{key}-{name}"] = [sha(loss)] + extra + [sha(v.grad) for v in leaf if v is not None]
    torch.cuda.synchronize()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--timeout", type=int, default=120, help="seconds per child process")
    ap.add_argument("--worker", choices=METRICS, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        print(json.dumps(worker(args.worker)))
        return
    out = {"tool": "sweep_digest"}
    for metric in METRICS:
        r = subprocess.run(["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--worker", metric],
                           capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-2000:])
            raise SystemExit(f"sweep_digest: the {metric} step ended with status {r.returncode}; nothing more was started")
        out[metric] = json.loads(r.stdout.strip().splitlines()[-1])
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
