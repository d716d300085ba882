"""The pairwise ranking losses under a distance against every node or a shared candidate set:
HyperGNN.pairwise_loss_by_distance with distance="l1" / "l2" / "complex" and loss="hinge" / "logistic", forward and forward +
backward, on one MI355X, each beside negative_sampling_loss_by_distance — the same sweep with another epilogue — at the same
shape in the same process.  Prints one JSON line per shape and a last one with all of them.

    python tools/pairwise_sweep_time.py [--shapes 16384x16384x128,4096x1024x128,1024x1000000x128,1024x14541x256]
                                        [--reps 5] [--timeout 420]

Every shape B x C x d (C candidates out of N = C nodes) is measured in a child process of its own under `--timeout` seconds;
the parent never opens the device, and after a child that fails or runs out of time nothing more is started.  Rows are
LayerNorm-shaped, the query rows translated (query_rows = embs[q] + 0.5 v), no filter lists; margin 1 for the pairwise losses,
margin 6 and temperature 1 for the negative-sampling loss; scale 2 / d (d^-1/2 under "l2").  Per metric, medians of `reps` warm
device-event windows (ms) of

  ns_fwd / ns_step                 negative_sampling_loss_by_distance without grad / with .backward() into embs and query_rows
  hinge_fwd / hinge_step           pairwise_loss_by_distance(loss="hinge") likewise, and *_over_ns, its ratio to the line above
  logistic_fwd / logistic_step     pairwise_loss_by_distance(loss="logistic") likewise
and, per kind, the share of violated pairs (the hinge's backward skips a group of four rows whose pairs are all satisfied)."""

from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

METRICS = ("l1", "l2", "complex")
KINDS = ("hinge", "logistic")


def run_shape(B, C, d, reps):
    import numpy as np
    import torch
    import torch.nn.functional as F

    from graph_hypernetwork_forge_amd import HyperGNN

    def timed(fn, reps, warm=2):
        for _ in range(warm):
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
    N = C
    gen = torch.Generator(device=dev).manual_seed(1000 + d)
    embs = F.layer_norm(torch.randn(N, d, device=dev, generator=gen), (d,), 1.0 + 0.1 * torch.randn(d, device=dev, generator=gen),
                        0.1 * torch.randn(d, device=dev, generator=gen))
    model = HyperGNN(text_dim=16, node_feat_dim=8, hidden_dim=16, num_layers=1).to(dev).eval()
    rng = np.random.default_rng(B + N)
    q, t = (torch.from_numpy(rng.integers(0, N, B)).to(dev) for _ in range(2))
    rows = (embs[q] + 0.5 * torch.randn(B, d, device=dev, generator=gen)).contiguous()
    e_g, r_g = embs.clone().requires_grad_(), rows.clone().requires_grad_()

    def step(fn, e, r):
        e.grad = r.grad = None
        loss = fn(e, r)
        loss.sum().backward()
        return loss.detach()

    res = {"B": B, "C": C, "d": d, "bc_ids_gb": B * C * 8 / 1e9, "bc_coef_gb": B * C * 4 / 1e9}
    for metric in METRICS:
        if metric == "complex" and d % 2:
            continue
        scale = d ** -0.5 if metric == "l2" else 2.0 / d
        ns = lambda e, r: model.negative_sampling_loss_by_distance(e, q, t, metric, scale=scale, margin=6.0, adversarial_temperature=1.0,
                                                                   query_rows=r)
        r = {}
        with torch.no_grad():
            r["ns_fwd_ms"], a = timed(lambda: ns(embs, rows), reps)
        r["ns_step_ms"] = timed(lambda: step(ns, e_g, r_g), reps)[0]
        finite = bool(torch.isfinite(a).all())
        for kind in KINDS:
            pw = lambda e, rr: model.pairwise_loss_by_distance(e, q, t, metric, loss=kind, scale=scale, margin=1.0, query_rows=rr)
            with torch.no_grad():
                r[f"{kind}_fwd_ms"], _ = timed(lambda: pw(embs, rows), reps)
                loss, active = model.pairwise_loss_by_distance(embs, q, t, metric, loss=kind, scale=scale, margin=1.0, query_rows=rows,
                                                               return_active=True)
            r[f"{kind}_step_ms"] = timed(lambda: step(pw, e_g, r_g), reps)[0]
            r[f"{kind}_fwd_over_ns"] = r[f"{kind}_fwd_ms"] / r["ns_fwd_ms"]
            r[f"{kind}_step_over_ns"] = r[f"{kind}_step_ms"] / r["ns_step_ms"]
            r[f"{kind}_violated_share"] = float(active.double().sum()) / (B * max(C - 1, 1))
            finite = finite and bool(torch.isfinite(loss).all())
        r["losses_finite"] = finite
        print(f"{B}x{C}x{d} {metric}: negsamp fwd {r['ns_fwd_ms']:.2f} ms, step {r['ns_step_ms']:.2f} ms; hinge fwd "
              f"{r['hinge_fwd_ms']:.2f} ms, step {r['hinge_step_ms']:.2f} ms; logistic fwd {r['logistic_fwd_ms']:.2f} ms, step "
              f"{r['logistic_step_ms']:.2f} ms", file=sys.stderr, flush=True)
        res[metric] = r
    res["device"] = torch.cuda.get_device_name(0)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="16384x16384x128,4096x1024x128,1024x1000000x128,1024x14541x256", help="BxCxd[,BxCxd...]")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=420, help="seconds a shape's child process may take")
    ap.add_argument("--one", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.one is not None:                                  # the child: one shape, one JSON line
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("pairwise_sweep_time.py measures on an MI355X; no HIP device here")
        B, C, d = (int(v) for v in args.one.lower().split("x"))
        print(json.dumps(run_shape(B, C, d, args.reps)), flush=True)
        return
    out = {"tool": "pairwise_sweep_time", "reps": args.reps}
    for shape in args.shapes.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--one", shape, "--reps", str(args.reps)]
        try:                                                  # the child's progress lines go to this process's stderr
            r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=args.timeout)
        except subprocess.TimeoutExpired:
            out[shape] = f"ran past {args.timeout} s"
            print(json.dumps(out))
            raise SystemExit(f"{shape}: ran past {args.timeout} s; nothing more is started")
        if r.returncode != 0:
            out[shape] = f"exit status {r.returncode}"
            print(json.dumps(out))
            raise SystemExit(f"{shape}: exit status {r.returncode}; nothing more is started")
        out[shape] = json.loads(r.stdout.strip().splitlines()[-1])
        print(json.dumps({shape: out[shape]}), flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
