"""Relation-prediction timing, (head, ?, tail): every relation's score for every pair, at N = 1 M rows, d = 128,
B in {1,024, 16,384} pairs and U in {64, 237} relation texts.  Prints one JSON line.

    python tools/relation_predict_time.py [--batches 1024,16384] [--relations 64,237] [--reps 5] [--no-torch]

Medians of device-event windows (ms, warm), as tools/relation_time.py takes them, per (B, U):
  - "fwd_ms": RelationDecoder.score_relations without a graph (generator + ghf_relation_scores); "sweep_ms" /
    "sweep_graph_ms": the raw ghf_relation_scores call alone, eagerly and per call of ten calls replayed as one captured HIP
    graph, with its fraction of the fp32 matrix peak (2 B U d^2 flop against 157.3 Tflop/s);
  - "fwd_bwd_ms": score_relations recorded, (S * G).sum().backward() down to d embs and the generator's parameters;
  - the torch formulations in the same process: "einsum_*": einsum("bi,uij->buj", x[h], A) with its [B, U, d] intermediate
    (its size is reported; skipped above --max-intermediate-gb), and "per_relation_*": U calls of dec.score;
  - the largest difference between our table and einsum's."""

from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from graph_hypernetwork_forge_amd import RelationDecoder, _native  # noqa: E402

N, D, TEXT_DIM = 1_000_000, 128, 64


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
    """ms per call of `inner` back-to-back calls replayed as one captured HIP graph."""
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
    ap.add_argument("--relations", default="64,237")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--max-intermediate-gb", type=float, default=8.0, help="skip einsum when its [B, U, d] fp32 operand is larger")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("relation_predict_time.py measures on an MI355X; no HIP device here")
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(1003)
    embs = 0.5 * torch.nn.functional.layer_norm(torch.randn(N, D, device=dev, generator=gen), (D,))
    torch.manual_seed(0)
    dec = RelationDecoder(text_dim=TEXT_DIM, hidden_dim=D).to(dev).eval()
    out = {"tool": "relation_predict_time", "device": torch.cuda.get_device_name(0), "N": N, "d": D, "reps": args.reps}
    for U in (int(v) for v in args.relations.split(",")):
        rel_embs = torch.randn(U, TEXT_DIM, device=dev, generator=gen)
        with torch.no_grad():
            heads = dec.generator(rel_embs)
        A, b = heads["W_msg"], heads["bias"]
        for B in (int(v) for v in args.batches.split(",")):
            rng = np.random.default_rng(B + U)
            h = torch.from_numpy(rng.integers(0, N, B)).to(dev)
            t = torch.from_numpy(rng.integers(0, N, B)).to(dev)
            G = torch.randn(B, U, device=dev, generator=gen)
            r = {"intermediate_gb": B * U * D * 4 / 2 ** 30}
            S = torch.empty(B, U, device=dev)
            r["sweep_ms"], ours = timed(lambda: _native.relation_scores(embs, h, t, A, b, out=S), args.reps)
            ours = ours.clone()
            r["sweep_graph_ms"] = graphed(lambda: _native.relation_scores(embs, h, t, A, b, out=S), args.reps)
            r["sweep_fraction_of_fp32_matrix_peak"] = 2.0 * B * U * D * D / (r["sweep_graph_ms"] * 1e-3) / 157.3e12
            with torch.no_grad():
                r["fwd_ms"], _ = timed(lambda: dec.score_relations(embs, h, t, rel_embs), args.reps)
            e = embs.clone().requires_grad_(True)

            def ours_fb():
                e.grad = None
                dec.zero_grad(set_to_none=True)
                (dec.score_relations(e, h, t, rel_embs) * G).sum().backward()
                return e.grad

            r["fwd_bwd_ms"], _ = timed(ours_fb, args.reps)
            r["fwd_bwd_fraction_of_fp32_matrix_peak"] = 4 * 2.0 * B * U * D * D / (r["fwd_bwd_ms"] * 1e-3) / 157.3e12
            if not args.no_torch:
                def einsum_fwd(x, Ag, bg):
                    a = x[h]
                    return torch.einsum("buj,bj->bu", a.unsqueeze(1) + torch.einsum("bi,uij->buj", a, Ag) + bg.unsqueeze(0), x[t])

                def per_relation(x):
                    return torch.stack([dec.score(x, h, torch.full_like(h, u), t, rel_embs) for u in range(U)], dim=1)

                def per_relation_fb():
                    e.grad = None
                    dec.zero_grad(set_to_none=True)
                    (per_relation(e) * G).sum().backward()
                    return e.grad

                with torch.no_grad():
                    r["per_relation_fwd_ms"], _ = timed(lambda: per_relation(embs), args.reps)
                r["per_relation_fwd_bwd_ms"], _ = timed(per_relation_fb, args.reps)
                if r["intermediate_gb"] <= args.max_intermediate_gb:
                    with torch.no_grad():
                        r["einsum_fwd_ms"], ref = timed(lambda: einsum_fwd(embs, A, b), args.reps)
                    r["max_abs_diff_vs_einsum"] = float((ours - ref).abs().max())
                    del ref

                    def einsum_fb():
                        e.grad = None
                        dec.zero_grad(set_to_none=True)
                        hd = dec.generator(rel_embs)
                        (einsum_fwd(e, hd["W_msg"], hd["bias"]) * G).sum().backward()
                        return e.grad

                    r["einsum_fwd_bwd_ms"], _ = timed(einsum_fb, args.reps)
                    r["fwd_speedup_vs_einsum"] = r["einsum_fwd_ms"] / r["fwd_ms"]
                    r["fwd_bwd_speedup_vs_einsum"] = r["einsum_fwd_bwd_ms"] / r["fwd_bwd_ms"]
                r["fwd_speedup_vs_per_relation"] = r["per_relation_fwd_ms"] / r["fwd_ms"]
                r["fwd_bwd_speedup_vs_per_relation"] = r["per_relation_fwd_bwd_ms"] / r["fwd_bwd_ms"]
            del e
            out[f"B{B}_U{U}"] = r
            print(f"# B={B} U={U}: {json.dumps(r)}", file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
