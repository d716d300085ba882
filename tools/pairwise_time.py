"""Pairwise ranking losses on per-query negative sets: HyperGNN.pairwise_loss (hinge, logistic) under the dot product and
distance="l1" / "l2" / "complex", on one MI355X.  Prints one JSON line.

    python tools/pairwise_time.py [--shapes 16384x256x128,1024x1000x128,16384x256x64,16384x256x256] [--reps 5] [--no-torch]
                                  [--limit 300]

Every shape B x K x d runs as a child process of its own under a time limit of `--limit` seconds; after a shape that fails
(a non-zero exit, or the limit) nothing more is started, and the JSON says which shape it was.  Per shape (N = 1 M rows, K
uniformly random negatives per query, no padding, no filter lists, margin 1; scale 2 / d for "l1" and "complex", d^-1/2 for
"l2" and the dot product: scores of order 1), per score and per kind: medians of `reps` warm device-event windows (ms) of

  fwd          pairwise_loss                                               (no autograd graph)
  fwd_bwd      pairwise_loss, mean, backward down to d embs

beside, on the same inputs and in the same process:
  softmax      softmax_loss(negatives=)                 the same two windows
  negsamp      negative_sampling_loss(negatives=)       the same two windows (adversarial temperature 1)
  negsamp_again the negsamp windows timed once more at the very end: the spread of the same code within one process
  torch        the plain formulation — embs[neg] gathered as [B, K, d], the loss on it, autograd; a cell that does not fit
               in memory says so
`vs_negsamp` = pairwise / negsamp (the gathered bytes are the same; the expectation is a ratio within the box-to-box spread of
DESIGN.md §5 of 1), `vs_torch` = torch / pairwise.  The largest difference between the pairwise and the torch results is
reported beside the times."""

from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_ROWS = 1_000_000
MARGIN, ALPHA = 1.0, 1.0
SCORES = ("dot", "l1", "l2", "complex")
KINDS = ("hinge", "logistic")


def scale_for(score, d):
    return d ** -0.5 if score in ("l2", "dot") else 2.0 / d


def run_shape(B, K, d, reps, with_torch):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import torch.nn.functional as F

    from graph_hypernetwork_forge_amd import HyperGNN

    if not torch.cuda.is_available():
        raise SystemExit("pairwise_time.py measures on an MI355X; no HIP device here")

    def timed(fn):
        for _ in range(2):
            out = fn()
        del out
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

    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(1000 + d)
    embs = F.layer_norm(torch.randn(N_ROWS, d, device=dev, generator=gen), (d,), 1.0 + 0.1 * torch.randn(d, device=dev, generator=gen),
                        0.1 * torch.randn(d, device=dev, generator=gen))
    model = HyperGNN(text_dim=16, node_feat_dim=8, hidden_dim=16, num_layers=1).to(dev).eval()
    rng = np.random.default_rng(B + K)
    q, t = (torch.from_numpy(rng.integers(0, N_ROWS, B)).to(dev) for _ in range(2))
    neg = torch.from_numpy(rng.integers(0, N_ROWS, (B, K))).to(dev)

    def kw(score):
        return dict(negatives=neg, scale=scale_for(score, d), **({} if score == "dot" else dict(distance=score)))

    def pairwise(score, kind, e):
        return model.pairwise_loss(e, q, t, loss=kind, margin=MARGIN, **kw(score))

    def softmax(score, kind, e):
        return model.softmax_loss(e, q, t, **kw(score))

    def negsamp(score, kind, e):
        return model.negative_sampling_loss(e, q, t, margin=MARGIN, adversarial_temperature=ALPHA, **kw(score))

    def plain(score, kind, e):
        s = scale_for(score, d)
        eq, rows = e[q], e[neg]
        def S(x, y):
            if score == "dot":
                return (x * y).sum(-1)
            delta = x - y
            if score == "l1":
                return -delta.abs().sum(-1)
            if score == "l2":
                return -delta.norm(dim=-1)
            return -delta.reshape(*delta.shape[:-1], -1, 2).norm(dim=-1).sum(-1)
        u = s * S(eq.unsqueeze(1), rows) - s * S(eq, e[t]).unsqueeze(1) + MARGIN
        live = neg != t.unsqueeze(1)
        phi = torch.relu(u) if kind == "hinge" else F.softplus(u)
        return (phi * live).sum(1) / live.sum(1).clamp(min=1)

    def step(route, score, kind, bwd):
        if not bwd:
            with torch.no_grad():
                return route(score, kind, embs)
        e = embs.detach().requires_grad_(True)
        loss = route(score, kind, e)
        loss.mean().backward()
        return loss.detach(), e.grad

    res = {"bkd_tensor_gb": B * K * d * 4 / 1e9}
    for score in SCORES:
        res[score] = {}
        base = {}
        for name, route in (("softmax", softmax), ("negsamp", negsamp)):
            base[name] = {w: timed(lambda: step(route, score, None, bwd))[0] for w, bwd in (("fwd", False), ("fwd_bwd", True))}
        for kind in KINDS:
            r = {}
            for w, bwd in (("fwd", False), ("fwd_bwd", True)):
                c = {}
                c["ms"], ref = timed(lambda: step(pairwise, score, kind, bwd))
                ref = ref if isinstance(ref, tuple) else (ref,)
                c["softmax_ms"], c["negsamp_ms"] = base["softmax"][w], base["negsamp"][w]
                c["vs_negsamp"] = c["ms"] / c["negsamp_ms"]
                if with_torch:
                    try:
                        c["torch_ms"], out = timed(lambda: step(plain, score, kind, bwd))
                        out = out if isinstance(out, tuple) else (out,)
                        c["torch_loss_max_abs_diff"] = float((ref[0] - out[0]).abs().max())
                        if bwd:
                            c["torch_grad_rel_l2_diff"] = float((ref[1] - out[1]).norm() / out[1].norm())
                        c["vs_torch"] = c["torch_ms"] / c["ms"]
                        del out
                    except torch.cuda.OutOfMemoryError:
                        c["torch_ms"] = "does not fit"
                    torch.cuda.empty_cache()
                del ref
                r[w] = c
            res[score][kind] = r
        for w, bwd in (("fwd", False), ("fwd_bwd", True)):            # the negsamp call once more, at the end
            again = timed(lambda: step(negsamp, score, None, bwd))[0]
            for kind in KINDS:
                res[score][kind][w]["negsamp_again_ms"] = again
                res[score][kind][w]["spread"] = abs(again - base["negsamp"][w]) / min(again, base["negsamp"][w])
    return {"device": torch.cuda.get_device_name(0), "result": res}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="16384x256x128,1024x1000x128,16384x256x64,16384x256x256", help="BxKxd[,BxKxd...]")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--limit", type=int, default=300, help="seconds a shape's child process may take")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child is not None:                                        # one shape, in a process of its own
        B, K, d = (int(v) for v in args.child.lower().split("x"))
        print(json.dumps(run_shape(B, K, d, args.reps, not args.no_torch)))
        return 0
    out = {"tool": "pairwise_time", "N": N_ROWS, "reps": args.reps}
    for shape in args.shapes.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", shape, "--reps", str(args.reps)] + (["--no-torch"] if args.no_torch else [])
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
        except subprocess.TimeoutExpired:
            out["failed"] = {"shape": shape, "why": f"no result within {args.limit} s"}
            break                                                     # nothing is started after a shape that fails
        if r.returncode != 0:
            out["failed"] = {"shape": shape, "why": f"exit status {r.returncode}", "stderr": r.stderr[-2000:]}
            break
        child = json.loads(r.stdout.strip().splitlines()[-1])
        out["device"] = child["device"]
        out[shape] = child["result"]
    print(json.dumps(out))
    return 1 if "failed" in out else 0


if __name__ == "__main__":
    sys.exit(main())
