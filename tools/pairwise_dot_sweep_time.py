"""The pairwise ranking losses by dot product against every node or a shared candidate set: HyperGNN.pairwise_loss_by_dot with
loss="hinge" / "logistic", forward and forward + backward, on one MI355X, each beside negative_sampling_loss(candidates=) — the
same matrix-core sweep with a heavier epilogue — at the same shape in the same process, and beside
pairwise_loss(negatives=neg.expand(B, C)), the only route to the same loss before, where its [B, C] ids fit.  Prints one JSON
line per shape and a last one with all of them.

    python tools/pairwise_dot_sweep_time.py [--shapes 16384x16384x128,4096x1024x128,1024x1000000x128,1024x14541x256]
                                            [--windows 3] [--timeout 420]

Every shape B x C x d (a shared set of C candidates; N = C nodes, so candidates= names every node and the subset path with its
id map runs) is measured in a child process of its own under `--timeout` seconds; the parent never opens the device, and after
a child that fails or runs out of time nothing more is started.  Rows are LayerNorm-shaped, the query rows given (query_rows =
embs[q] + 0.5 v), no filter lists; scale d^-1/2; margin 1 for the pairwise losses, margin 1 and temperature 1 for the
negative-sampling loss.  The calls of one kind (forward, step) are measured in turn, window by window, so that drift of the
machine meets all of them alike; a window is `iters` calls between two device events (as many as fill ~ 50 ms), and the figure
is the median of `windows` warm windows per call (ms):

  ns_fwd / ns_step                 negative_sampling_loss without grad / with .backward() into embs and query_rows
  hinge_fwd / hinge_step           pairwise_loss_by_dot(loss="hinge") likewise, and *_over_ns, its ratio to the line above
  logistic_fwd / logistic_step     pairwise_loss_by_dot(loss="logistic") likewise
  expand_hinge_fwd / _step         pairwise_loss(negatives=neg.expand(B, C)) where B x C <= --expand-pairs"""

from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KINDS = ("hinge", "logistic")


def run_shape(B, C, d, windows, expand_pairs):
    import numpy as np
    import torch
    import torch.nn.functional as F

    from graph_hypernetwork_forge_amd import HyperGNN

    def window(fn, iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / iters

    def timed(fns):
        """{name: median ms per call} of the calls `fns`, measured in turn window by window after two warm calls each"""
        iters = {}
        for name, fn in fns.items():
            fn()
            torch.cuda.synchronize()
            iters[name] = max(1, min(200, int(50.0 / max(window(fn, 1), 1e-3))))
        ts = {name: [] for name in fns}
        for _ in range(windows):
            for name, fn in fns.items():
                ts[name].append(window(fn, iters[name]))
        return {name: float(np.median(v)) for name, v in ts.items()}

    dev = torch.device("cuda:0")
    N = C
    gen = torch.Generator(device=dev).manual_seed(1000 + d)
    embs = F.layer_norm(torch.randn(N, d, device=dev, generator=gen), (d,), 1.0 + 0.1 * torch.randn(d, device=dev, generator=gen),
                        0.1 * torch.randn(d, device=dev, generator=gen))
    model = HyperGNN(text_dim=16, node_feat_dim=8, hidden_dim=16, num_layers=1).to(dev).eval()
    rng = np.random.default_rng(B + N)
    q, t = (torch.from_numpy(rng.integers(0, N, B)).to(dev) for _ in range(2))
    cand = torch.arange(N, device=dev)
    rows = (embs[q] + 0.5 * torch.randn(B, d, device=dev, generator=gen)).contiguous()
    e_g, r_g = embs.clone().requires_grad_(), rows.clone().requires_grad_()
    scale = d ** -0.5

    def step(fn):
        e_g.grad = r_g.grad = None
        fn(e_g, r_g).sum().backward()

    calls = {"ns": lambda e, r: model.negative_sampling_loss(e, q, t, scale=scale, margin=1.0, adversarial_temperature=1.0, query_rows=r,
                                                             candidates=cand)}
    for kind in KINDS:
        calls[kind] = lambda e, r, kind=kind: model.pairwise_loss_by_dot(e, q, t, loss=kind, scale=scale, margin=1.0, query_rows=r,
                                                                         candidates=cand)
    if B * C <= expand_pairs:
        neg = cand.unsqueeze(0).expand(B, C).contiguous()
        calls["expand_hinge"] = lambda e, r: model.pairwise_loss(e, q, t, negatives=neg, loss="hinge", scale=scale, margin=1.0, query_rows=r)

    res = {"B": B, "C": C, "d": d, "bc_ids_gb": B * C * 8 / 1e9, "bc_coef_gb": B * C * 4 / 1e9}
    with torch.no_grad():
        fwd = timed({k: (lambda fn=fn: fn(embs, rows)) for k, fn in calls.items()})
        loss, active = model.pairwise_loss_by_dot(embs, q, t, loss="hinge", scale=scale, margin=1.0, query_rows=rows, candidates=cand,
                                                  return_active=True)
    stp = timed({k: (lambda fn=fn: step(fn)) for k, fn in calls.items()})
    for k in calls:
        res[f"{k}_fwd_ms"], res[f"{k}_step_ms"] = fwd[k], stp[k]
        if k != "ns":
            res[f"{k}_fwd_over_ns"], res[f"{k}_step_over_ns"] = fwd[k] / fwd["ns"], stp[k] / stp["ns"]
    res["violated_share"] = float(active.double().sum()) / (B * max(C - 1, 1))
    res["losses_finite"] = bool(torch.isfinite(loss).all())
    print(f"{B}x{C}x{d}: " + "; ".join(f"{k} fwd {fwd[k]:.3f} ms, step {stp[k]:.3f} ms" for k in calls), file=sys.stderr, flush=True)
    res["device"] = torch.cuda.get_device_name(0)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="16384x16384x128,4096x1024x128,1024x1000000x128,1024x14541x256", help="BxCxd[,BxCxd...]")
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=420, help="seconds a shape's child process may take")
    ap.add_argument("--expand-pairs", type=int, default=1 << 25, help="largest B x C at which the expanded per-query call is timed")
    ap.add_argument("--one", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.one is not None:                                  # the child: one shape, one JSON line
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("pairwise_dot_sweep_time.py measures on an MI355X; no HIP device here")
        B, C, d = (int(v) for v in args.one.lower().split("x"))
        print(json.dumps(run_shape(B, C, d, args.windows, args.expand_pairs)), flush=True)
        return
    out = {"tool": "pairwise_dot_sweep_time", "windows": args.windows}
    for shape in args.shapes.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--one", shape, "--windows", str(args.windows), "--expand-pairs",
               str(args.expand_pairs)]
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
