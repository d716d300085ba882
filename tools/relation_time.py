"""Relation-typed scoring timing at BASELINE config 3's shapes (N = 1 M, d = 128, R = 64; B = 1,024 and 16,384).  Prints one
JSON line.

    python tools/relation_time.py [--batches 1024,16384] [--reps 5] [--no-torch] [--no-sweeps]

Medians of device-event windows (ms, warm), as tools/rank_time.py takes them:
  - the transform alone, Q = x[h] + x[h] @ A[rel] + b[rel]: ghf_relation_rows with the queries already grouped by relation
    ("rows_ms"; "rows_graph_ms": per call of ten calls replayed as one captured HIP graph, i.e. without the host's per-call
    cost, which exceeds the device time at these sizes), with the grouping (ghf_group_edges, what RelationDecoder runs per call: "rows_grouped_ms"), and the torch
    formulation in the same process, torch.bmm(x[h].unsqueeze(1), A[rel]) over one gathered d x d matrix per query
    ("torch_bmm_ms", "torch_bmm_graph_ms": B d^2 4 bytes written and read back), with the largest difference between the two results;
  - a typed rank_candidates (decoder rows + typed filter lists + the sweep) against the untyped call with lists of the same
    size, and a typed softmax_loss forward + backward (through the decoder, down to d embs and the generator's parameters)
    against the untyped recorded call.
The embeddings are LayerNorm-shaped random rows; the relation embeddings are random; ten known partners per query."""

from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from graph_hypernetwork_forge_amd import HyperGNN, RelationDecoder, _native  # noqa: E402

N, D, R, TEXT_DIM = 1_000_000, 128, 64, 64


def timed(fn, reps):
    """(median ms, last result) over `reps` device-event windows, after two warm-up calls."""
    for _ in range(2):
        out = fn()
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


def graphed(fn, reps, inner=10):
    """ms per call of `inner` back-to-back calls replayed as one captured HIP graph: the device time of a call, free of the
    host's per-call cost (the calls allocate nothing, so they can be captured)."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(inner):
            fn()
    return timed(g.replay, reps)[0] / inner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1024,16384")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--no-sweeps", action="store_true", help="the transform alone")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("relation_time.py measures on an MI355X; no HIP device here")
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(1003)
    embs = torch.nn.functional.layer_norm(torch.randn(N, D, device=dev, generator=gen), (D,),
                                          1.0 + 0.1 * torch.randn(D, device=dev, generator=gen),
                                          0.1 * torch.randn(D, device=dev, generator=gen))
    torch.manual_seed(0)
    model = HyperGNN(text_dim=16, node_feat_dim=8, hidden_dim=16, num_layers=1).to(dev).eval()
    dec = RelationDecoder(text_dim=TEXT_DIM, hidden_dim=D).to(dev).eval()
    rel_embs = torch.randn(R, TEXT_DIM, device=dev, generator=gen)
    with torch.no_grad():
        heads = dec.generator(rel_embs)
    A, b = heads["W_msg"], heads["bias"]
    scale = D ** -0.5
    out = {"tool": "relation_time", "device": torch.cuda.get_device_name(0), "N": N, "d": D, "R": R}
    for B in (int(v) for v in args.batches.split(",")):
        rng = np.random.default_rng(B)
        h = torch.from_numpy(rng.integers(0, N, B)).to(dev)
        t = torch.from_numpy(rng.integers(0, N, B)).to(dev)
        rel = torch.from_numpy(rng.integers(0, R, B)).to(dev)
        known = (h.repeat(10), torch.from_numpy(rng.integers(0, N, 10 * B)).to(dev), rel.repeat(10))
        r = {}
        group = _native.group_edges(rel, R)
        ws = torch.empty(_native.relation_rows_workspace_bytes(B, R), dtype=torch.uint8, device=dev)
        Q = torch.empty(B, D, dtype=torch.float32, device=dev)
        r["rows_ms"], ours = timed(lambda: _native.relation_rows(embs, rel, A, b, ix=h, group=group, workspace=ws, out=Q), args.reps)
        r["rows_graph_ms"] = graphed(lambda: _native.relation_rows(embs, rel, A, b, ix=h, group=group, workspace=ws, out=Q), args.reps)
        r["rows_grouped_ms"], _ = timed(lambda: _native.relation_rows(embs, rel, A, b, ix=h), args.reps)
        r["rows_fraction_of_fp32_matrix_peak"] = 2.0 * B * D * D / (r["rows_graph_ms"] * 1e-3) / 157.3e12
        if not args.no_torch:
            r["torch_bmm_ms"], ref = timed(lambda: embs[h] + torch.bmm(embs[h].unsqueeze(1), A[rel]).squeeze(1) + b[rel], args.reps)
            r["rows_max_abs_diff_vs_torch"] = float((ours - ref).abs().max())
            r["rows_speedup"] = r["torch_bmm_ms"] / r["rows_ms"]
            r["torch_bmm_graph_ms"] = graphed(lambda: embs[h] + torch.bmm(embs[h].unsqueeze(1), A[rel]).squeeze(1) + b[rel], args.reps)
            r["rows_graph_speedup"] = r["torch_bmm_graph_ms"] / r["rows_graph_ms"]
            del ref
        if not args.no_sweeps:
            kn2 = (known[0], known[1])
            with torch.no_grad():
                r["rank_untyped_ms"], _ = timed(lambda: model.rank_candidates(embs, h, t, known=kn2), args.reps)
                r["rank_typed_ms"], _ = timed(lambda: model.rank_candidates(
                    embs, h, t, query_rows=dec(embs, h, rel, rel_embs), known=known, query_rel=rel), args.reps)
            e = embs.clone().requires_grad_(True)

            def untyped():
                e.grad = None
                model.softmax_loss(e, h, t, scale=scale, known=kn2).sum().backward()
                return e.grad

            def typed():
                e.grad = None
                dec.zero_grad(set_to_none=True)
                loss = model.softmax_loss(e, h, t, scale=scale, query_rows=dec(e, h, rel, rel_embs), known=known, query_rel=rel)
                loss.sum().backward()
                return e.grad

            r["softmax_fwd_bwd_untyped_ms"], _ = timed(untyped, args.reps)
            r["softmax_fwd_bwd_typed_ms"], _ = timed(typed, args.reps)
            del e
        out[f"B{B}"] = r
    print(json.dumps(out))


if __name__ == "__main__":
    main()
