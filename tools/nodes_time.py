"""Node-batch forward timing: HyperGNN.forward_nodes against the full forward, on BASELINE configs 3 and 2 (the bench's
synthetic graphs and seeds), with a breakdown of where a call's time goes.  Prints one JSON line.

    python tools/nodes_time.py [--configs c3,c2] [--reps 5]

Per config: the full inference forward; forward_nodes (eval) at 1,024 and 16,384 random seeds, split into the subgraph
extraction (ghf_subgraph_*, with its one host sync for the counts), the sub-plan build (build_plan: a device sort and
its host syncs), the input projection over all subgraph rows (with the feature gather) and the shrunk layers; one training
step (forward_nodes in train mode + backward) on 1,024 seeds against the same step through forward, with the per-call reversed-plan / grouping cost
(build_train_plan) on its own.  Times are medians of device-event windows (ms), warm (plans of the full graph cached)."""

from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from graph_hypernetwork_forge_amd import HyperGNN, _native, synth  # noqa: E402
from graph_hypernetwork_forge_amd.autograd import build_train_plan  # noqa: E402
from graph_hypernetwork_forge_amd.plan import build_plan  # noqa: E402

CONFIGS = {"c3": dict(N=1_000_000, E=10_000_000, R=64, d=128, L=3, T=64, seed=1003),
           "c2": dict(N=100_000, E=1_000_000, R=32, d=64, L=2, T=64, seed=1002)}


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


def run_config(name, reps):
    cfg = CONFIGS[name]
    dev = torch.device("cuda:0")
    N, E, R, d, L, T = (cfg[k] for k in ("N", "E", "R", "d", "L", "T"))
    ei_np, rel_np = synth.make_graph_arrays(N, E, R, cfg["seed"], "uniform")
    names = synth.relation_names(R)
    texts = [names[i] for i in rel_np.tolist()]
    ei = torch.from_numpy(ei_np).to(dev)
    x = torch.randn(N, d, generator=torch.Generator(device=dev).manual_seed(cfg["seed"]), device=dev)
    torch.manual_seed(0)
    model = HyperGNN(text_dim=T, node_feat_dim=d, hidden_dim=d, num_layers=L).to(dev).eval()
    res = {}
    with torch.no_grad():
        res["forward_ms"], full = timed(lambda: model(x, ei, texts), reps)
        plan = model.plan_for(ei, texts, N, dev)
        for S in (1024, 16384):
            seeds = torch.from_numpy(np.random.default_rng(S).choice(N, S, replace=False)).to(dev)
            t_all, out = timed(lambda: model.forward_nodes(x, ei, texts, seeds), reps)
            err = float((out - full[seeds]).abs().max())
            t_ex, sub = timed(lambda: _native.subgraph(plan, seeds, L), reps)
            m = sub["m"]
            t_plan, sp = timed(lambda: build_plan(sub["edge_index"], sub["rel"], plan.unique_texts, m[L], d, dev), reps)
            xs = x.index_select(0, sub["node_list"])
            split = sp.wlayout in _native.SPLIT_LAYOUTS
            hs = _native.alloc_split(m[L], d, sp.wlayout, dev) if split else None
            t_proj, _ = timed(lambda: _native.input_proj_fwd(x.index_select(0, sub["node_list"]), model.input_proj.weight,
                                                             model.input_proj.bias, h_split=hs,
                                                             split_layout=sp.wlayout if split else 0), reps)
            rows = [m[L - 1 - l] for l in range(L)]
            t_planned, _ = timed(lambda: model.forward_planned(xs, sp, rows_per_layer=rows), reps)
            res[f"nodes{S}"] = dict(ms=t_all, speedup=res["forward_ms"] / t_all, max_abs_diff_vs_forward=err, m=m,
                                    edges=sp.E, layer_rows=rows, block_nodes=sp.block_nodes, extract_ms=t_ex, subplan_ms=t_plan,
                                    input_proj_ms=t_proj, planned_ms=t_planned, layers_ms=t_planned - t_proj,
                                    rest_ms=t_all - t_ex - t_plan - t_planned)
    model.train()
    S = 1024
    seeds = torch.from_numpy(np.random.default_rng(S).choice(N, S, replace=False)).to(dev)
    g = torch.randn(S, d, device=dev, generator=torch.Generator(device=dev).manual_seed(5))

    def step():
        model.zero_grad(set_to_none=True)
        (model.forward_nodes(x, ei, texts, seeds) * g).sum().backward()

    def full_step():
        model.zero_grad(set_to_none=True)
        (model(x, ei, texts)[seeds] * g).sum().backward()

    t_step, _ = timed(step, reps)
    t_full, _ = timed(full_step, reps)
    sub = _native.subgraph(model.plan_for(ei, texts, N, dev, training=True), seeds, L)
    sp = build_plan(sub["edge_index"], sub["rel"], plan.unique_texts, sub["m"][L], d, dev)
    t_tp, _ = timed(lambda: build_train_plan(sub["edge_index"], sp.rel_ids, sp, d, dev), reps)
    res["train1024"] = dict(step_ms=t_step, full_step_ms=t_full, train_plan_ms=t_tp, m=sub["m"], edges=sp.E)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c3,c2")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("nodes_time.py measures on an MI355X; no HIP device here")
    out = {"tool": "nodes_time", "device": torch.cuda.get_device_name(0)}
    for name in args.configs.split(","):
        out[name] = run_config(name, args.reps)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
