"""Node-batch forward timing: HyperGNN.forward_nodes against the full forward, on BASELINE configs 3 and 2 (the bench's
synthetic graphs and seeds), with a breakdown of where a call's time goes.  Prints one JSON line.

    python tools/nodes_time.py [--configs c3,c2] [--reps 5] [--kind uniform|powerlaw] [--fanout 5,5,5[;10,10,10]]
                               [--exclude B[,B2]]

Per config: the full inference forward; forward_nodes (eval) at 1,024 and 16,384 random seeds, split into the subgraph
extraction (ghf_subgraph_*, with its one host sync for the counts), the sub-plan build (build_plan: a device sort and
its host syncs), the input projection over all subgraph rows (with the feature gather) and the shrunk layers; one training
step (forward_nodes in train mode + backward) on 1,024 seeds against the same step through forward, with the per-call reversed-plan / grouping cost
(build_train_plan) on its own.  Times are medians of device-event windows (ms), warm (plans of the full graph cached).

--fanout adds, per cap list (the first num_layers entries of each are used) and per seed count, the sampled call beside
the exact one: m, the sampled edges, the sampled extraction (ghf_subgraph_sample_*: its hop passes, sorts and host reads
together — split them with a kernel trace), the whole inference call and the training step, each with its exact
counterpart from the same process.

--exclude B draws B existing edges (the batch a link-prediction step scores), takes their heads and tails as the seeds
(2 B of them) and the batch in both directions, typed, as forward_nodes' exclusion list (2 B entries: --exclude 512,8192
gives 1,024 and 16,384 seeds with a list of the same size), and times — in one process, for the exact form and for
every --fanout list (default 5,5,5) — the extraction (ghf_subgraph_*_excl against ghf_subgraph_*, the sorted keys ready)
and the whole inference call (which also builds and sorts the keys) with and without the list."""

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


def setup(name, kind):
    """The config's synthetic graph (the bench's seeds), features and model on the device."""
    cfg = CONFIGS[name]
    dev = torch.device("cuda:0")
    N, E, R, d, L, T = (cfg[k] for k in ("N", "E", "R", "d", "L", "T"))
    ei_np, rel_np = synth.make_graph_arrays(N, E, R, cfg["seed"], kind)
    names = synth.relation_names(R)
    texts = [names[i] for i in rel_np.tolist()]
    ei = torch.from_numpy(ei_np).to(dev)
    x = torch.randn(N, d, generator=torch.Generator(device=dev).manual_seed(cfg["seed"]), device=dev)
    torch.manual_seed(0)
    model = HyperGNN(text_dim=T, node_feat_dim=d, hidden_dim=d, num_layers=L).to(dev).eval()
    return model, x, ei, texts, N, d, L, dev


def run_sampled(name, reps, kind, fanouts):
    """Per cap list and seed count: the sampled forward_nodes beside the exact one (inference call, extraction, training step)."""
    model, x, ei, texts, N, d, L, dev = setup(name, kind)
    res = {}
    for S in (1024, 16384):
        seeds = torch.from_numpy(np.random.default_rng(S).choice(N, S, replace=False)).to(dev)
        g = torch.randn(S, d, device=dev, generator=torch.Generator(device=dev).manual_seed(5))

        def measure(fan):
            kw = {} if fan is None else dict(fanout=fan, seed=12345)
            out = {}
            model.eval()
            with torch.no_grad():
                plan = model.plan_for(ei, texts, N, dev)
                out["ms"], _ = timed(lambda: model.forward_nodes(x, ei, texts, seeds, **kw), reps)
                if fan is None:
                    out["extract_ms"], sub = timed(lambda: _native.subgraph(plan, seeds, L), reps)
                else:
                    out["extract_ms"], sub = timed(lambda: _native.subgraph_sample(plan, seeds, fan, 12345), reps)
                    out["host_reads"] = sub["host_reads"]
                out["m"], out["edges"] = sub["m"], int(sub["edge_index"].size(1))
            model.train()

            def step():
                model.zero_grad(set_to_none=True)
                (model.forward_nodes(x, ei, texts, seeds, **kw) * g).sum().backward()

            out["step_ms"], _ = timed(step, reps)
            out["train_m"], out["train_edges"] = model.last_subgraph["m"], model.last_subgraph["edges"]
            model.eval()
            return out

        res[f"nodes{S}"] = {"exact": measure(None)}
        for fan in fanouts:
            res[f"nodes{S}"]["fanout " + ",".join(map(str, fan[:L]))] = measure(tuple(fan[:L]))
    return res


def run_exclude(name, reps, kind, fanouts, batches):
    """Per batch size B: B existing edges excluded in both directions, seeds = their heads and tails; extraction and
    inference call with and without the list, exact and per cap list."""
    model, x, ei, texts, N, d, L, dev = setup(name, kind)
    res = {}
    with torch.no_grad():
        plan = model.plan_for(ei, texts, N, dev)
        for B in batches:
            batch = torch.from_numpy(np.random.default_rng(B).choice(ei.size(1), B, replace=False)).to(dev)
            r = plan.rel_ids[batch].repeat(2)
            seeds = torch.cat([ei[0][batch], ei[1][batch]])
            h, t = seeds, torch.cat([ei[1][batch], ei[0][batch]])
            names = [plan.unique_texts[i] for i in r.tolist()]
            keys = torch.sort((h << 32) | (t * plan.R + r)).values
            row = {}
            for fan in [None] + [tuple(f[:L]) for f in fanouts]:
                kw = {} if fan is None else dict(fanout=fan, seed=12345)
                if fan is None:
                    extract = lambda ex: _native.subgraph(plan, seeds, L, exclude=ex)                    # noqa: E731
                else:
                    extract = lambda ex: _native.subgraph_sample(plan, seeds, fan, 12345, exclude=ex)    # noqa: E731
                out = {}
                out["extract_ms"], plain = timed(lambda: extract(None), reps)
                out["extract_excl_ms"], sub = timed(lambda: extract((keys, True)), reps)
                out["ms"], _ = timed(lambda: model.forward_nodes(x, ei, texts, seeds, **kw), reps)
                out["excl_ms"], _ = timed(lambda: model.forward_nodes(x, ei, texts, seeds, exclude=(h, t, names), **kw), reps)
                out["m"], out["edges"] = plain["m"], int(plain["edge_index"].size(1))
                out["excl_m"], out["excl_edges"] = sub["m"], int(sub["edge_index"].size(1))
                out["seeds"], out["entries"] = int(seeds.numel()), int(keys.numel())
                row["exact" if fan is None else "fanout " + ",".join(map(str, fan))] = out
            res[f"batch{B}"] = row
    return res


def run_config(name, reps, kind="uniform"):
    model, x, ei, texts, N, d, L, dev = setup(name, kind)
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
    ap.add_argument("--kind", default="uniform", choices=["uniform", "powerlaw"], help="the synthetic graph's degree law")
    ap.add_argument("--fanout", default="", help="per-hop caps, e.g. 5,5,5 (several lists: separate with ';'; -1 = no cap): "
                    "time the sampled forward_nodes beside the exact one instead of the exact call's breakdown")
    ap.add_argument("--exclude", default="", help="batch sizes B, e.g. 1024,16384: exclude B existing edges (seeds: their ends) "
                    "and time the extraction and the inference call with and without the list, exact and per --fanout list")
    args = ap.parse_args()
    fanouts = [[int(f) for f in part.split(",")] for part in args.fanout.split(";") if part.strip()]
    batches = [int(b) for b in args.exclude.split(",") if b.strip()]
    if batches and not fanouts:
        fanouts = [[5, 5, 5]]
    for name in args.configs.split(","):
        if any(len(f) < CONFIGS[name]["L"] for f in fanouts):
            raise SystemExit(f"--fanout needs {CONFIGS[name]['L']} caps per list for {name}")
    if not torch.cuda.is_available():
        raise SystemExit("nodes_time.py measures on an MI355X; no HIP device here")
    out = {"tool": "nodes_time", "device": torch.cuda.get_device_name(0), "kind": args.kind}
    for name in args.configs.split(","):
        if batches:
            out[name] = run_exclude(name, args.reps, args.kind, fanouts, batches)
        else:
            out[name] = run_sampled(name, args.reps, args.kind, fanouts) if fanouts else run_config(name, args.reps, args.kind)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
