"""Per-query negative sets: HyperGNN.rank_candidates / softmax_loss / negative_sampling_loss with negatives=[B, K] against the
two formulations a user has without the keyword, on one MI355X.  Prints one JSON line.

    python tools/negatives_time.py [--shapes 16384x256x128,1024x1000x128,16384x256x64,16384x256x256] [--reps 5] [--no-torch]

Per shape B x K x d (N = 1 M rows, K uniformly random negatives per query, no padding, no filter lists, scale d^-1/2, margin
1, adversarial temperature 1): medians of `reps` warm device-event windows (ms) of

  rank                   rank_candidates                                           (no autograd graph)
  softmax forward        softmax_loss                                              (no autograd graph)
  softmax fwd + bwd      softmax_loss, mean, backward down to d embs
  negsamp fwd + bwd      negative_sampling_loss, mean, backward down to d embs

for three routes: `new` (negatives=), `edges` — the same result through model.score_edges over the B K pairs (and the B target
pairs) plus torch on the [B, K] scores — and `torch`, the plain formulation (embs[neg], bmm).  The `edges` route is then
timed a SECOND time (`edges_again`): the spread of the same code within one command is what a difference between routes has
to exceed.  `new_kernel_ms` (rank and the softmax forward) is the raw C call alone, on checked ids with outputs and workspace
given, and `pairs_kernel_ms` the score_edges route's B K pairs alone: which part of a difference is the kernel and which
the keyword's host check.  `floor_ms` is B K d 4 bytes of gathered rows over the measured HBM rate (6.29 TB/s); `fraction_of_floor` = floor /
new.  The largest difference between the routes' results is reported beside the times."""

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
HBM_BYTES_PER_S = 6.29e12
MARGIN, ALPHA = 1.0, 1.0


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


def routes(model, embs, q, t, neg, scale):
    B, K = neg.shape
    qq, nn = q.repeat_interleave(K), neg.reshape(-1)

    def new(op, e):
        if op == "rank":
            return model.rank_candidates(e, q, t, negatives=neg)
        if op == "softmax":
            return model.softmax_loss(e, q, t, scale=scale, negatives=neg)
        return model.negative_sampling_loss(e, q, t, scale=scale, margin=MARGIN, adversarial_temperature=ALPHA, negatives=neg)

    def edges(op, e):
        s = 1.0 if op == "rank" else scale
        return from_scores(op, s * model.score_edges(e, qq, nn).view(B, K), s * model.score_edges(e, q, t), t, neg)

    def plain(op, e):
        s = 1.0 if op == "rank" else scale
        eq = e[q]
        return from_scores(op, s * torch.bmm(e[neg], eq.unsqueeze(2)).squeeze(2), s * (eq * e[t]).sum(1), t, neg)

    return {"new": new, "edges": edges, "torch": plain}


def run_shape(B, K, d, reps, with_torch):
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(1000 + d)
    embs = F.layer_norm(torch.randn(N_ROWS, d, device=dev, generator=gen), (d,), 1.0 + 0.1 * torch.randn(d, device=dev, generator=gen),
                        0.1 * torch.randn(d, device=dev, generator=gen))
    model = HyperGNN(text_dim=16, node_feat_dim=8, hidden_dim=16, num_layers=1).to(dev).eval()
    rng = np.random.default_rng(B + K)
    q, t = (torch.from_numpy(rng.integers(0, N_ROWS, B)).to(dev) for _ in range(2))
    neg = torch.from_numpy(rng.integers(0, N_ROWS, (B, K))).to(dev)
    fns = routes(model, embs, q, t, neg, d ** -0.5)
    floor = B * K * d * 4 / HBM_BYTES_PER_S * 1e3
    res = {"floor_ms": floor}

    def fwd(route, op):
        with torch.no_grad():
            return fns[route](op, embs)

    def fwd_bwd(route, op):
        e = embs.detach().requires_grad_(True)
        loss = fns[route](op, e)
        loss.mean().backward()
        return loss.detach(), e.grad

    # the kernels alone: the raw calls behind the two forward operations on checked ids, outputs and workspace given — what is
    # left of `new` beside them is the keyword's host check (one read of the ids' ranges) and the allocations
    from graph_hypernetwork_forge_amd import _native
    ws = torch.empty(_native.neg_workspace_bytes(B, K, d, 0), dtype=torch.uint8, device=dev)
    counts = (torch.empty(B, dtype=torch.int64, device=dev), torch.empty(B, dtype=torch.int64, device=dev))
    pair = (torch.empty(B, device=dev), torch.empty(B, device=dev))
    raw = {"rank": lambda: _native.score_neg_rank(embs, embs, t, neg, iq=q, workspace=ws, out=counts),
           "softmax_fwd": lambda: _native.score_neg_softmax_fwd(embs, embs, t, neg, iq=q, scale=d ** -0.5, workspace=ws, out=pair)}
    qq, nn = q.repeat_interleave(K), neg.reshape(-1)
    res["pairs_kernel_ms"], _ = timed(lambda: _native.score_pairs_fwd(embs, embs, qq, nn), reps)      # score_edges' B K pairs alone

    order = ["new", "edges"] + (["torch"] if with_torch else []) + ["edges_again"]
    for key, op, step in (("rank", "rank", fwd), ("softmax_fwd", "softmax", fwd), ("softmax_fwd_bwd", "softmax", fwd_bwd),
                          ("negsamp_fwd_bwd", "negsamp", fwd_bwd)):
        r, ref = {}, None
        for name in order:
            route = name.replace("_again", "")
            try:
                r[name + "_ms"], out = timed(lambda: step(route, op), reps)
            except torch.cuda.OutOfMemoryError:
                r[name + "_ms"] = "does not fit"
                torch.cuda.empty_cache()
                continue
            out = out if isinstance(out, tuple) else (out,)
            if name == "new":
                ref = out
            elif not name.endswith("_again"):
                if op == "rank":
                    r[name + "_counts_differ"] = int(sum((a != b).sum() for a, b in zip(ref, out)))
                else:
                    r[name + "_loss_max_abs_diff"] = float((ref[0] - out[0]).abs().max())
                    if len(out) > 1:
                        r[name + "_grad_rel_l2_diff"] = float((ref[1] - out[1]).norm() / out[1].norm())
            del out
        if key in raw:
            r["new_kernel_ms"], _ = timed(raw[key], reps)
            r["kernel_fraction_of_floor"] = floor / r["new_kernel_ms"]
        r["fraction_of_floor"] = floor / r["new_ms"]
        res[key] = r
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="16384x256x128,1024x1000x128,16384x256x64,16384x256x256", help="BxKxd[,BxKxd...]")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("negatives_time.py measures on an MI355X; no HIP device here")
    out = {"tool": "negatives_time", "device": torch.cuda.get_device_name(0), "N": N_ROWS, "reps": args.reps}
    for shape in args.shapes.split(","):
        B, K, d = (int(v) for v in shape.lower().split("x"))
        out[shape] = run_shape(B, K, d, args.reps, not args.no_torch)
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
