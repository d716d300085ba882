"""The two losses under a distance against every node or a shared candidate set: HyperGNN.softmax_loss_by_distance /
negative_sampling_loss_by_distance with distance="l1" / "l2" / "complex", forward and forward + backward, on one MI355X.  Prints
one JSON line per shape and a last one with all of them.

    python tools/distance_loss_time.py [--shapes 16384x16384x128,4096x1024x128,1024x1000000x128,1024x14541x256]
                                       [--reps 5] [--small-b 64] [--no-torch] [--timeout 420]

Every shape B x C x d (C candidates out of N = C nodes; "all nodes" is the same sweep without the id indirection) is measured
in a child process of its own under `--timeout` seconds; the parent never opens the device, and after a child that fails or
runs out of time nothing more is started.  Rows are LayerNorm-shaped, the query rows translated (query_rows = embs[q] + 0.5 v),
no filter lists; margin 6, temperature 1 for the negative-sampling loss; scale 2 / d (d^-1/2 under "l2").  Per metric, medians of
`reps` warm device-event windows (ms) of

  sm_fwd / sm_step     softmax_loss_by_distance without grad / with .backward() into embs and query_rows
  ns_fwd / ns_step     negative_sampling_loss_by_distance likewise
  rank                 rank_by_distance at the same shape: the sweep the forward's tile loop is
beside, in the same process:
  per_query_*          softmax_loss(negatives=all ids per row, distance=) at B = `--small-b` queries, where the [B, C] id tensor
                       fits, forward and step, beside new_small_*, the new call on the same queries
  torch_step           the [chunk, C, d] difference tensor and autograd, chunked over queries to about 1 GiB (softmax only)
and the VALU floor of the forward: distance_sweep_time.py's instructions per element x B C d / 39.3e12 lane-instructions per
second."""

from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

METRICS = ("l1", "l2", "complex")
VALU_PER_ELEMENT = {"l1": 2.0, "l2": 1.0, "complex": 2.75}
LANE_INSTR_PER_S = 39.3e12


def run_shape(B, C, d, reps, with_torch, small_b):
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

    def step(fn, e, r, n=None):
        e.grad = r.grad = None
        loss = fn(e, r)
        loss.sum().backward()
        return loss.detach()

    def torch_step(metric, scale):
        chunk = max(1, (1 << 28) // (C * d))
        e = embs.clone().requires_grad_()
        total = 0.0
        for lo in range(0, B, chunk):
            delta = rows[lo:lo + chunk].unsqueeze(1) - e.unsqueeze(0)
            if metric == "l1":
                D = delta.abs().sum(-1)
            elif metric == "l2":
                D = torch.sqrt((delta * delta).sum(-1) + 1e-30)
            else:
                D = torch.sqrt((delta * delta).reshape(delta.size(0), C, d // 2, 2).sum(-1) + 1e-30).sum(-1)
            loss = F.cross_entropy(-scale * D, t[lo:lo + chunk], reduction="sum")
            loss.backward()
            total += float(loss.detach())
        return total

    res = {"B": B, "C": C, "d": d, "bcd_tensor_gb": B * C * d * 4 / 1e9, "bc_ids_gb": B * C * 8 / 1e9}
    sb = min(small_b, B)
    all_ids = torch.arange(N, device=dev).unsqueeze(0).expand(sb, -1).contiguous()
    for metric in METRICS:
        if metric == "complex" and d % 2:
            continue
        scale = d ** -0.5 if metric == "l2" else 2.0 / d
        sm = lambda e, r: model.softmax_loss_by_distance(e, q, t, metric, scale=scale, query_rows=r)
        ns = lambda e, r: model.negative_sampling_loss_by_distance(e, q, t, metric, scale=scale, margin=6.0, adversarial_temperature=1.0,
                                                                   query_rows=r)
        r = {"fwd_floor_ms": VALU_PER_ELEMENT[metric] * B * C * d / LANE_INSTR_PER_S * 1e3}
        with torch.no_grad():
            r["rank_ms"] = timed(lambda: model.rank_by_distance(embs, q, t, metric, query_rows=rows), reps)[0]
            r["sm_fwd_ms"], a = timed(lambda: sm(embs, rows), reps)
            r["ns_fwd_ms"], b = timed(lambda: ns(embs, rows), reps)
        r["losses_finite"] = bool(torch.isfinite(a).all() and torch.isfinite(b).all())
        r["sm_step_ms"] = timed(lambda: step(sm, e_g, r_g), reps)[0]
        r["ns_step_ms"] = timed(lambda: step(ns, e_g, r_g), reps)[0]
        r["sm_fwd_of_floor"] = r["fwd_floor_ms"] / r["sm_fwd_ms"]
        r["sm_step_over_fwd"] = r["sm_step_ms"] / r["sm_fwd_ms"]
        print(f"{B}x{C}x{d} {metric}: softmax fwd {r['sm_fwd_ms']:.2f} ms, step {r['sm_step_ms']:.2f} ms; negsamp fwd "
              f"{r['ns_fwd_ms']:.2f} ms, step {r['ns_step_ms']:.2f} ms; rank {r['rank_ms']:.2f} ms", file=sys.stderr, flush=True)
        # the per-query workaround, where its id tensor fits
        qs, ts, rs = q[:sb].contiguous(), t[:sb].contiguous(), rows[:sb].clone().requires_grad_()
        new_s = lambda e, rr: model.softmax_loss_by_distance(e, qs, ts, metric, scale=scale, query_rows=rr)
        old_s = lambda e, rr: model.softmax_loss(e, qs, ts, scale=scale, query_rows=rr, negatives=all_ids, distance=metric)
        r["small_b"] = sb
        with torch.no_grad():
            r["new_small_fwd_ms"], x = timed(lambda: new_s(embs, rs.detach()), reps)
            r["per_query_fwd_ms"], y = timed(lambda: old_s(embs, rs.detach()), reps)
        r["per_query_max_abs_diff"] = float((x - y).abs().max())
        r["new_small_step_ms"] = timed(lambda: step(new_s, e_g, rs), reps)[0]
        r["per_query_step_ms"] = timed(lambda: step(old_s, e_g, rs), reps)[0]
        if with_torch:
            try:
                r["torch_step_ms"] = timed(lambda: torch_step(metric, scale), max(1, reps // 2), warm=1)[0]
                r["step_vs_torch"] = r["torch_step_ms"] / r["sm_step_ms"]
            except torch.cuda.OutOfMemoryError:
                r["torch_step_ms"] = "does not fit"
            torch.cuda.empty_cache()
        res[metric] = r
    res["device"] = torch.cuda.get_device_name(0)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="16384x16384x128,4096x1024x128,1024x1000000x128,1024x14541x256", help="BxCxd[,BxCxd...]")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--small-b", type=int, default=64, help="queries of the per-query comparison: its [B, C] id tensor has to fit")
    ap.add_argument("--timeout", type=int, default=420, help="seconds a shape's child process may take")
    ap.add_argument("--one", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.one is not None:                                  # the child: one shape, one JSON line
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("distance_loss_time.py measures on an MI355X; no HIP device here")
        B, C, d = (int(v) for v in args.one.lower().split("x"))
        print(json.dumps(run_shape(B, C, d, args.reps, not args.no_torch, args.small_b)), flush=True)
        return
    out = {"tool": "distance_loss_time", "reps": args.reps}
    for shape in args.shapes.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--one", shape, "--reps", str(args.reps), "--small-b", str(args.small_b)]
        if args.no_torch:
            cmd.append("--no-torch")
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
