"""Negative-sampling loss timing: HyperGNN.negative_sampling_loss forward alone and forward + backward against C shared
candidates, beside bce_loss, softmax_loss and rank_candidates on the same queries, lists and candidates in the same process,
and beside the formulation a user has without it — scale * Q @ embs[cand].T as a [B, C] tensor, softmax(alpha z).detach(),
softplus, autograd — at the sizes where that fits.  Prints one JSON line.

    python tools/negsamp_time.py [--configs c3] [--batches 1024,16384] [--cands 16384,131072,0] [--reps 5] [--no-torch]
                                 [--torch-max-gb 10]

Per config, B and C (0 = every node): ten known partners per query, scale d^-1/2, margin 1, adversarial temperature 1.
Medians of device-event windows (ms, warm) of each loss's forward (no autograd graph) and forward plus backward down to
d embs; `rank_ms` is rank_candidates (the bare sweep with a compare in its epilogue).  `over_bce` = negsamp / bce;
`bce_over_rank` and `negsamp_over_bce_gap` = (negsamp - bce) / (bce - rank) place the new epilogue's cost beside the BCE
epilogue's.  The candidate set holds the batch's targets (the method adds them), so C grows by up to B.  The torch formulation
is tried where its [B, C] fp32 logits stay below --torch-max-gb; it reports its peak memory beyond the embeddings, and "does
not fit" where it raises an out-of-memory error."""

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

from bce_time import CONFIGS, timed  # noqa: E402
from graph_hypernetwork_forge_amd import HyperGNN  # noqa: E402

MARGIN, ALPHA, SMOOTHING = 1.0, 1.0, 0.1


def torch_loss(embs, q, t, cand, ptr, idx, scale, backward):
    """PyKEEN's NSSALoss per query on one shared negative set: the [B, C] logits, the listed candidates and the target masked
    out of the weights and of the sum."""
    e = embs.detach().requires_grad_(backward)
    c = e if cand is None else e[cand]
    ids = torch.arange(e.size(0), device=e.device) if cand is None else cand
    z = scale * (e[q] @ c.T)
    lens = ptr[1:] - ptr[:-1]
    rows = torch.repeat_interleave(torch.arange(q.numel(), device=e.device), lens)
    pos = torch.searchsorted(ids, idx).clamp_(max=ids.numel() - 1)
    hit = ids[pos] == idx
    out = torch.zeros_like(z, dtype=torch.bool)
    out[rows[hit], pos[hit]] = True
    out[torch.arange(q.numel(), device=e.device), torch.searchsorted(ids, t)] = True
    w = torch.softmax((ALPHA * z).masked_fill(out, float("-inf")), -1).detach()
    zt = scale * (e[q] * e[t]).sum(1)
    loss = F.softplus(-(zt + MARGIN)) + (w * F.softplus(z + MARGIN)).sum(1)
    if backward:
        loss.mean().backward()
    return loss.detach(), e.grad


def run_config(name, reps, batches, cands, with_torch, torch_max_bytes):
    cfg = CONFIGS[name]
    dev = torch.device("cuda:0")
    N, d = cfg["N"], cfg["d"]
    gen = torch.Generator(device=dev).manual_seed(cfg["seed"])
    embs = F.layer_norm(torch.randn(N, d, device=dev, generator=gen), (d,), 1.0 + 0.1 * torch.randn(d, device=dev, generator=gen),
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
        for C in cands:
            cand = None if C == 0 else torch.unique(torch.cat([torch.from_numpy(rng.choice(N, C, replace=False)).to(dev), t]))
            M = N if cand is None else cand.numel()
            lists = dict(filt_ptr=ptr, filt_idx=idx, candidates=cand)
            losses = {
                "negsamp": lambda e: model.negative_sampling_loss(e, q, t, scale=scale, margin=MARGIN, adversarial_temperature=ALPHA, **lists),
                "bce": lambda e: model.bce_loss(e, q, scale=scale, smoothing=SMOOTHING, pos_ptr=ptr, pos_idx=idx, candidates=cand),
                "softmax": lambda e: model.softmax_loss(e, q, t, scale=scale, **lists),
            }
            r = {"candidates": M}
            r["rank_ms"], _, _ = timed(lambda: model.rank_candidates(embs, q, t, **lists), reps)
            ours = grad = None
            for key, fn in losses.items():
                def step(fn=fn):
                    e = embs.detach().requires_grad_(True)
                    loss = fn(e)
                    loss.mean().backward()
                    return loss.detach(), e.grad

                r[key + "_fwd_ms"], r[key + "_fwd_peak_bytes"], out = timed(lambda fn=fn: fn(embs), reps)
                r[key + "_fwd_bwd_ms"], r[key + "_fwd_bwd_peak_bytes"], (_, g) = timed(step, reps)
                if key == "negsamp":
                    ours, grad = out, g
                del out, g
            r["fwd_over_bce"] = r["negsamp_fwd_ms"] / r["bce_fwd_ms"]
            r["fwd_bwd_over_bce"] = r["negsamp_fwd_bwd_ms"] / r["bce_fwd_bwd_ms"]
            r["fwd_over_softmax"] = r["negsamp_fwd_ms"] / r["softmax_fwd_ms"]
            r["fwd_bwd_over_softmax"] = r["negsamp_fwd_bwd_ms"] / r["softmax_fwd_bwd_ms"]
            r["bce_over_rank"] = r["bce_fwd_ms"] / r["rank_ms"]
            r["negsamp_over_bce_gap"] = (r["negsamp_fwd_ms"] - r["bce_fwd_ms"]) / max(r["bce_fwd_ms"] - r["rank_ms"], 1e-9)
            if with_torch:
                if 4 * B * M > torch_max_bytes:
                    r["torch_fwd_ms"] = r["torch_fwd_bwd_ms"] = "not tried: logits above --torch-max-gb"
                else:
                    for key, backward in (("torch_fwd", False), ("torch_fwd_bwd", True)):
                        try:
                            r[key + "_ms"], r[key + "_peak_bytes"], ref = timed(
                                lambda: torch_loss(embs, q, t, cand, ptr, idx, scale, backward), reps)
                            r[key + "_loss_max_rel_diff"] = float(((ref[0] - ours).abs() / ref[0].abs()).max())
                            if backward:
                                r["torch_grad_rel_l2_diff"] = float((ref[1] - grad).norm() / ref[1].norm())
                                r["fwd_bwd_speedup"] = r["torch_fwd_bwd_ms"] / r["negsamp_fwd_bwd_ms"]
                            else:
                                r["fwd_speedup"] = r["torch_fwd_ms"] / r["negsamp_fwd_ms"]
                            del ref
                        except torch.cuda.OutOfMemoryError:
                            r[key + "_ms"] = "does not fit"
                            torch.cuda.empty_cache()
            del ours, grad
            res[f"B{B}_C{C}"] = r
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c3")
    ap.add_argument("--batches", default="1024,16384")
    ap.add_argument("--cands", default="16384,131072,0", help="candidate counts; 0 = every node")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--torch-max-gb", type=float, default=10.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("negsamp_time.py measures on an MI355X; no HIP device here")
    out = {"tool": "negsamp_time", "device": torch.cuda.get_device_name(0), "margin": MARGIN, "adversarial_temperature": ALPHA}
    for name in args.configs.split(","):
        out[name] = run_config(name, args.reps, [int(b) for b in args.batches.split(",")], [int(c) for c in args.cands.split(",")],
                               not args.no_torch, int(args.torch_max_gb * (1 << 30)))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
