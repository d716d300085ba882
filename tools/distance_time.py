"""Distance scores for per-query negative sets: HyperGNN.rank_candidates / softmax_loss / negative_sampling_loss with
negatives=[B, K] and distance="l1" / "l2" / "complex", on one MI355X.  Prints one JSON line.

    python tools/distance_time.py [--shapes 16384x256x128,1024x1000x128,16384x256x64,16384x256x256] [--reps 5] [--no-torch]

Per shape B x K x d (N = 1 M rows, K uniformly random negatives per query, no padding, no filter lists, margin 1, adversarial
temperature 1; scale 2 / d for "l1" and "complex", d^-1/2 for "l2" and the dot product: logits of order 1) and per metric:
medians of `reps` warm device-event windows (ms) of

  rank                   rank_candidates                                           (no autograd graph)
  softmax forward        softmax_loss                                              (no autograd graph)
  softmax fwd + bwd      softmax_loss, mean, backward down to d embs
  negsamp fwd + bwd      negative_sampling_loss, mean, backward down to d embs

beside three comparisons:
  (a) `torch`     the plain formulation, which materialises (embs[query].unsqueeze(1) - embs[neg]) as [B, K, d]; a cell that
                  does not fit in memory says so
  (b) `dot`       the dot-product negatives= call on the same inputs, in the same command
  (c) `dot_again` (b) timed once more at the very end: the spread of the same code within one command, which a difference
                  has to exceed
`vs_torch` = torch / new and `vs_dot` = new / dot.  The largest difference between `new` and `torch` results is reported
beside the times."""

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

N_ROWS = 1_000_000
MARGIN, ALPHA = 1.0, 1.0
METRICS = ("l1", "l2", "complex")
OPS = (("rank", "rank", False), ("softmax_fwd", "softmax", False), ("softmax_fwd_bwd", "softmax", True),
       ("negsamp_fwd_bwd", "negsamp", True))


def timed(fn, reps):
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


def from_scores(op, z, zt, t, neg):
    """The result of `op` from the logits z [B, K] and the target's zt [B] (the target among its own negatives drops out)."""
    drop = neg == t.unsqueeze(1)
    if op == "rank":
        return ((z > zt.unsqueeze(1)) & ~drop).sum(1), ((z == zt.unsqueeze(1)) & ~drop).sum(1)
    zm = z.masked_fill(drop, float("-inf"))
    if op == "softmax":
        return torch.logsumexp(torch.cat([zt.unsqueeze(1), zm], 1), 1) - zt
    w = torch.softmax(ALPHA * zm, 1).detach()
    return F.softplus(-(zt + MARGIN)) + (w * F.softplus(z + MARGIN).masked_fill(drop, 0.0)).sum(1)


def torch_distance(metric, delta):
    if metric == "l1":
        return delta.abs().sum(-1)
    if metric == "l2":
        return delta.norm(dim=-1)
    return delta.reshape(*delta.shape[:-1], -1, 2).norm(dim=-1).sum(-1)


def scale_for(metric, d):
    return d ** -0.5 if metric in ("l2", None) else 2.0 / d


def run_shape(B, K, d, reps, with_torch):
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(1000 + d)
    embs = F.layer_norm(torch.randn(N_ROWS, d, device=dev, generator=gen), (d,), 1.0 + 0.1 * torch.randn(d, device=dev, generator=gen),
                        0.1 * torch.randn(d, device=dev, generator=gen))
    model = HyperGNN(text_dim=16, node_feat_dim=8, hidden_dim=16, num_layers=1).to(dev).eval()
    rng = np.random.default_rng(B + K)
    q, t = (torch.from_numpy(rng.integers(0, N_ROWS, B)).to(dev) for _ in range(2))
    neg = torch.from_numpy(rng.integers(0, N_ROWS, (B, K))).to(dev)

    def new(metric, op, e):                                   # metric None: the dot-product call
        kw = dict(negatives=neg) if metric is None else dict(negatives=neg, distance=metric)
        if op == "rank":
            return model.rank_candidates(e, q, t, **kw)
        if op == "softmax":
            return model.softmax_loss(e, q, t, scale=scale_for(metric, d), **kw)
        return model.negative_sampling_loss(e, q, t, scale=scale_for(metric, d), margin=MARGIN, adversarial_temperature=ALPHA, **kw)

    def plain(metric, op, e):
        s = 1.0 if op == "rank" else scale_for(metric, d)
        eq = e[q]
        return from_scores(op, -s * torch_distance(metric, eq.unsqueeze(1) - e[neg]), -s * torch_distance(metric, eq - e[t]), t, neg)

    def step(route, metric, op, bwd):
        if not bwd:
            with torch.no_grad():
                return route(metric, op, embs)
        e = embs.detach().requires_grad_(True)
        loss = route(metric, op, e)
        loss.mean().backward()
        return loss.detach(), e.grad

    res = {"bkd_tensor_gb": B * K * d * 4 / 1e9}
    dot = {key: timed(lambda: step(new, None, op, bwd), reps)[0] for key, op, bwd in OPS}
    for metric in METRICS:
        res[metric] = {}
        for key, op, bwd in OPS:
            r = {}
            r["new_ms"], ref = timed(lambda: step(new, metric, op, bwd), reps)
            ref = ref if isinstance(ref, tuple) else (ref,)
            if with_torch:
                try:
                    r["torch_ms"], out = timed(lambda: step(plain, metric, op, bwd), reps)
                    out = out if isinstance(out, tuple) else (out,)
                    if op == "rank":
                        r["torch_counts_differ"] = int(sum((a != b).sum() for a, b in zip(ref, out)))
                    else:
                        r["torch_loss_max_abs_diff"] = float((ref[0] - out[0]).abs().max())
                        if bwd:
                            r["torch_grad_rel_l2_diff"] = float((ref[1] - out[1]).norm() / out[1].norm())
                    r["vs_torch"] = r["torch_ms"] / r["new_ms"]
                    del out
                except torch.cuda.OutOfMemoryError:
                    r["torch_ms"] = "does not fit"
                torch.cuda.empty_cache()
            del ref
            r["dot_ms"] = dot[key]
            r["vs_dot"] = r["new_ms"] / dot[key]
            res[metric][key] = r
    for key, op, bwd in OPS:                                  # (c): the dot-product call once more, at the end
        again = timed(lambda: step(new, None, op, bwd), reps)[0]
        for metric in METRICS:
            res[metric][key]["dot_again_ms"] = again
            res[metric][key]["spread"] = abs(again - dot[key]) / min(again, dot[key])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="16384x256x128,1024x1000x128,16384x256x64,16384x256x256", help="BxKxd[,BxKxd...]")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("distance_time.py measures on an MI355X; no HIP device here")
    out = {"tool": "distance_time", "device": torch.cuda.get_device_name(0), "N": N_ROWS, "reps": args.reps}
    for shape in args.shapes.split(","):
        B, K, d = (int(v) for v in shape.lower().split("x"))
        out[shape] = run_shape(B, K, d, args.reps, not args.no_torch)
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
