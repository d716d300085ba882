"""Distance scores against every node: HyperGNN.rank_by_distance / topk_by_distance (k = 10) with distance="l1" / "l2" /
"complex", on one MI355X.  Prints one JSON line per shape and a last one with all of them.

    python tools/distance_sweep_time.py [--shapes 1024x1000000x128,1024x1000000x64,1024x1000000x256,20466x14541x128]
                                        [--reps 5] [--no-torch] [--timeout 420]

Every shape B x N x d is measured in a child process of its own under `--timeout` seconds; the parent never opens the device,
and after a child that fails or runs out of time nothing more is started.  Rows are LayerNorm-shaped, the query rows
translated (query_rows = embs[q] + 0.5 v), no filter lists.  Per metric, medians of `reps` warm device-event windows (ms) of

  new_rank / new_topk      rank_by_distance / topk_by_distance

beside, in the same process:
  torch_rank / torch_topk  the plain formulation, chunked over queries to about 1 GiB of temporaries: torch.cdist with p = 1 and
                           p = 2, an explicit pair modulus for "complex"; then the compare-and-count, or torch.topk
  per_query_rank           rank_candidates(negatives=all ids, distance=) at B = `--small-b` queries, where the [B, N] id tensor
                           fits, beside new_rank_small, the new call on the same queries
  dot_rank / dot_topk      the dot-product rank_candidates / topk_candidates at the same shape (the matrix-core sweep)
and the VALU roof of the new sweep: VALU instructions per element of its inner loop (from the listing: 2 for L1 — a packed
subtract, two ANDs and a packed add per two elements —, 1 for L2, 2.75 for the complex modulus) x B N d / 39.3e12 lane-instructions
per second (157.3 TFLOP/s over the 4 FLOP of a packed fma).  `vs_torch` = torch / new; `of_roof` = roof / new."""

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
K = 10


def run_shape(B, N, d, reps, with_torch, small_b, torch_reps):
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
    gen = torch.Generator(device=dev).manual_seed(1000 + d)
    embs = F.layer_norm(torch.randn(N, d, device=dev, generator=gen), (d,), 1.0 + 0.1 * torch.randn(d, device=dev, generator=gen),
                        0.1 * torch.randn(d, device=dev, generator=gen))
    model = HyperGNN(text_dim=16, node_feat_dim=8, hidden_dim=16, num_layers=1).to(dev).eval()
    rng = np.random.default_rng(B + N)
    q, t = (torch.from_numpy(rng.integers(0, N, B)).to(dev) for _ in range(2))
    rows = (embs[q] + 0.5 * torch.randn(B, d, device=dev, generator=gen)).contiguous()

    def torch_dist(metric, r):
        if metric == "l1":
            return torch.cdist(r, embs, p=1)
        if metric == "l2":
            return torch.cdist(r, embs, p=2)
        delta = (r.unsqueeze(1) - embs.unsqueeze(0)).reshape(r.size(0), N, d // 2, 2)
        return torch.sqrt((delta * delta).sum(-1)).sum(-1)

    def torch_call(metric, op):
        # temporaries of about 1 GiB: a [chunk, N] distance block, and for "complex" the [chunk, N, d] differences.  p = 1 is
        # one 256-thread block per pair in torch: chunk x N stays below 2^24 pairs, i.e. 2^32 threads, a launch's limit here
        chunk = max(1, (1 << 28) // (N * (d if metric == "complex" else 1)))
        if metric == "l1":
            chunk = max(1, ((1 << 24) - 1) // N)
        outs = []
        for lo in range(0, B, chunk):
            D = torch_dist(metric, rows[lo:lo + chunk])
            if op == "rank":
                Dt = D.gather(1, t[lo:lo + chunk].unsqueeze(1))
                outs.append(torch.stack([(D < Dt).sum(1), (D == Dt).sum(1) - 1]))
            else:
                outs.append(torch.topk(D, K, dim=1, largest=False).indices.T)
            del D
        return torch.cat(outs, 1)

    def float64_topk_ids(metric, n):
        """ids [n, K] of the first n queries from float64 differences, a query at a time: what both routes are held against"""
        e64, out = embs.double(), []
        for i in range(n):
            delta = rows[i].double().unsqueeze(0) - e64
            if metric == "l1":
                D = delta.abs().sum(-1)
            elif metric == "l2":
                D = (delta * delta).sum(-1)
            else:
                D = torch.sqrt((delta * delta).reshape(N, d // 2, 2).sum(-1)).sum(-1)
            out.append(torch.topk(D, K, largest=False).indices)
        return torch.stack(out)

    res = {"B": B, "N": N, "d": d, "bnd_tensor_gb": B * N * d * 4 / 1e9}
    with torch.no_grad():
        res["dot_rank_ms"] = timed(lambda: model.rank_candidates(embs, q, t, query_rows=rows), reps)[0]
        res["dot_topk_ms"] = timed(lambda: model.topk_candidates(embs, q, K, query_rows=rows), reps)[0]
        sb = min(small_b, B)
        all_ids = torch.arange(N, device=dev).unsqueeze(0).expand(sb, -1).contiguous()
        for metric in METRICS:
            if metric == "complex" and d % 2:
                continue
            r = {"roof_ms": VALU_PER_ELEMENT[metric] * B * N * d / LANE_INSTR_PER_S * 1e3}
            r["new_rank_ms"], got_r = timed(lambda: model.rank_by_distance(embs, q, t, metric, query_rows=rows), reps)
            r["new_topk_ms"], got_k = timed(lambda: model.topk_by_distance(embs, q, K, metric, query_rows=rows), reps)
            r["rank_of_roof"], r["topk_of_roof"] = r["roof_ms"] / r["new_rank_ms"], r["roof_ms"] / r["new_topk_ms"]
            r["new_rank_small_ms"], small = timed(lambda: model.rank_by_distance(embs, q[:sb], t[:sb], metric, query_rows=rows[:sb]), reps)
            r["per_query_rank_ms"], pq = timed(lambda: model.rank_candidates(embs, q[:sb], t[:sb], query_rows=rows[:sb], negatives=all_ids,
                                                                             distance=metric), reps)
            r["small_b"] = sb
            r["per_query_counts_differ"] = int((small[0] != pq[0]).sum() + (small[1] != pq[1]).sum())
            ids64 = float64_topk_ids(metric, 4)
            r["new_topk_ids_differ_float64_4q"] = int((got_k[1][:4] != ids64).sum())
            print(f"{B}x{N}x{d} {metric}: rank {r['new_rank_ms']:.2f} ms, top-{K} {r['new_topk_ms']:.2f} ms", file=sys.stderr, flush=True)
            if with_torch:
                try:
                    r["torch_rank_ms"], out = timed(lambda: torch_call(metric, "rank"), torch_reps, warm=1)
                    r["torch_counts_differ"] = int((out[0] != got_r[0]).sum() + (out[1] != got_r[1]).sum())
                    r["torch_topk_ms"], out = timed(lambda: torch_call(metric, "topk"), torch_reps, warm=1)
                    r["torch_topk_ids_differ"] = int((out.T != got_k[1]).sum())
                    r["torch_topk_ids_differ_float64_4q"] = int((out.T[:4] != ids64).sum())
                    r["rank_vs_torch"], r["topk_vs_torch"] = r["torch_rank_ms"] / r["new_rank_ms"], r["torch_topk_ms"] / r["new_topk_ms"]
                    del out
                    print(f"{B}x{N}x{d} {metric}: torch rank {r['torch_rank_ms']:.1f} ms, top-{K} {r['torch_topk_ms']:.1f} ms",
                          file=sys.stderr, flush=True)
                except torch.cuda.OutOfMemoryError:
                    r["torch_rank_ms"] = "does not fit"
                torch.cuda.empty_cache()
            r["rank_vs_dot"], r["topk_vs_dot"] = r["new_rank_ms"] / res["dot_rank_ms"], r["new_topk_ms"] / res["dot_topk_ms"]
            res[metric] = r
    res["device"] = torch.cuda.get_device_name(0)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1024x1000000x128,1024x1000000x64,1024x1000000x256,20466x14541x128", help="BxNxd[,BxNxd...]")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--torch-reps", type=int, default=0, help="windows of the torch cells (default: --reps)")
    ap.add_argument("--small-b", type=int, default=64, help="queries of the per-query comparison: its [B, N] id tensor has to fit")
    ap.add_argument("--timeout", type=int, default=420, help="seconds a shape's child process may take")
    ap.add_argument("--one", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.one is not None:                                  # the child: one shape, one JSON line
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("distance_sweep_time.py measures on an MI355X; no HIP device here")
        B, N, d = (int(v) for v in args.one.lower().split("x"))
        print(json.dumps(run_shape(B, N, d, args.reps, not args.no_torch, args.small_b, args.torch_reps or args.reps)), flush=True)
        return
    out = {"tool": "distance_sweep_time", "reps": args.reps, "k": K}
    for shape in args.shapes.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--one", shape, "--reps", str(args.reps), "--small-b", str(args.small_b),
               "--torch-reps", str(args.torch_reps)]
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
