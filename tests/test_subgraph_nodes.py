"""HyperGNN.forward_nodes on the MI355X: the k-hop subgraph extraction (include/ghf.h: ghf_subgraph_*) against a numpy
restatement, and the node-batch forward against forward(...)[nodes], the reference's golden outputs and the oracle."""

import os

import numpy as np
import pytest
import torch

import cases
from _util import assert_close
from graph_hypernetwork_forge_amd import HyperGNN, ToyKnowledgeGraph, _native, synth
from graph_hypernetwork_forge_amd.plan import build_plan, plan_config, relation_ids
from oracle import hypergnn_oracle as O

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def make_model(cfg: cases.ModelCfg, params=None) -> HyperGNN:
    m = HyperGNN(cfg.text_dim, cfg.node_feat_dim, cfg.hidden_dim, cfg.num_layers, char_emb_dim=cfg.char_emb_dim)
    m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in (params or cfg.params()).items()})
    return m.to(DEV).eval()


def _grad_check(name, got, want, rtol=2e-4, l2=5e-5):
    gw, gg = want.astype(np.float64), got.astype(np.float64)
    assert gg.shape == gw.shape, f"d{name}: shape {gg.shape} vs {gw.shape}"
    scale = float(np.abs(gw).max())
    assert np.allclose(gg, gw, rtol=rtol, atol=1e-4 * max(scale, 1e-30)), \
        f"d{name}: max abs err {np.abs(gg - gw).max():.3e} at scale {scale:.3e}"
    rel_l2 = np.linalg.norm(gg - gw) / max(np.linalg.norm(gw), 1e-30)
    assert rel_l2 < l2, f"d{name}: relative L2 {rel_l2:.3e}"


# ---- the numpy restatement ------------------------------------------------------------------------------------------

def np_subgraph(src, dst, rel, N, seeds, k):
    """dist, node_list, new_id, m, induced edges [2, E'] and their relations, in the order of the edges given."""
    dist = np.full(N, k + 1, dtype=np.int64)
    dist[np.asarray(seeds, dtype=np.int64) % N] = 0
    for j in range(k):
        s = src[dist[dst] == j]
        dist[s[dist[s] > k]] = j + 1
    inside = np.nonzero(dist <= k)[0]
    node_list = inside[np.lexsort((inside, dist[inside]))]
    new_id = np.full(N, -1, dtype=np.int64)
    new_id[node_list] = np.arange(node_list.size)
    m = [int((dist <= j).sum()) for j in range(k + 1)]
    keep = dist[dst] <= k - 1
    return dist, node_list, new_id, m, np.stack([new_id[src[keep]], new_id[dst[keep]]]), rel[keep]


def plan_order(ei, rel, N, R, bn):
    """The stable order of ghf_plan_build: key = (dst / BN) R BN + rel BN + dst % BN, or dst R + rel for CSR plans."""
    dst = ei[1]
    key = dst * R + rel if bn == 1 else (dst // bn) * (R * bn) + rel * bn + dst % bn
    return np.argsort(key, kind="stable")


def _graph_with_isolated(N, E, R, seed, kind, extra=40):
    """A synthetic graph whose last `extra` nodes have no edges at all."""
    ei, rel = synth.make_graph_arrays(N, E, R, seed, kind)
    return ei, rel, N + extra


@pytest.mark.parametrize("kind", ["uniform", "powerlaw"])
@pytest.mark.parametrize("d,R,generic", [(64, 7, False), (128, 7, False), (256, 200, True)])
def test_extraction_equals_the_numpy_restatement(kind, d, R, generic):
    ei, rel, N = _graph_with_isolated(3000, 20000, R, 71 + d, kind)
    plan = build_plan(torch.from_numpy(ei).to(DEV), torch.from_numpy(rel), synth.relation_names(R), N, d, DEV,
                      force_generic=generic)
    assert (plan.block_nodes == 1) == generic
    order = plan_order(ei, rel, N, R, plan.block_nodes)
    src, dst, rl = ei[0][order], ei[1][order], rel[order]
    hub = int(np.bincount(ei[1], minlength=N).argmax())
    rng = np.random.default_rng(d + R)
    picks = [rng.choice(3000, 17, replace=False).tolist() + [5, 5, 5],           # duplicates
             [N - 1, N - 3, N - 1],                                             # no in-edges (nor any edge)
             [hub, 11, N - 2, hub],                                             # a hub among the seeds
             list(range(N))]                                                    # every node
    for seeds in picks:
        for k in (1, 2, 3, 4):
            got = _native.subgraph(plan, torch.tensor(seeds, dtype=torch.int64, device=DEV), k)
            dist, nl, nid, m, e_sub, r_sub = np_subgraph(src, dst, rl, N, seeds, k)
            what = f"{kind} d={d} k={k} seeds={seeds[:4]}"
            assert np.array_equal(got["dist"].cpu().numpy(), dist), what
            assert got["m"] == m, what
            assert np.array_equal(got["node_list"].cpu().numpy(), nl), what
            assert np.array_equal(got["new_id"].cpu().numpy(), nid), what
            assert np.array_equal(got["edge_index"].cpu().numpy(), e_sub), what
            assert np.array_equal(got["rel"].cpu().numpy(), r_sub), what


# ---- the model: against the reference's outputs, forward(...)[nodes] and the oracle --------------------------------

def _subsets(N):
    rng = np.random.default_rng(N)
    out = [[0], [N - 1, 0, N - 1]]
    if N > 4:
        out.append(rng.choice(N, max(2, N // 5), replace=False).tolist())
        out.append((-rng.choice(N, 3, replace=False) - 1).tolist() + [1, 1])        # negative ids, duplicates
    return out


@pytest.mark.parametrize("name", [n for n in cases.GRAPH_CASE_NAMES if n != "g5_c2"])
def test_forward_nodes_matches_reference_golden(golden_dir, name):
    (case,) = cases.graph_cases(only=[name])
    g = np.load(os.path.join(golden_dir, f"{name}.npz"))
    model = make_model(cases.MODELS[case.model])
    x, ei = torch.from_numpy(case.node_features).to(DEV), torch.from_numpy(case.edge_index).to(DEV)
    for nodes in _subsets(x.size(0)):
        with torch.no_grad():
            out = model.forward_nodes(x, ei, case.edge_texts, torch.tensor(nodes))
        assert_close(out.cpu().numpy(), g["out"][nodes], f"{name} nodes {nodes[:4]}")


@pytest.mark.parametrize("name", ["g2_toy", "g3_mid32", "g_odd", "g6_c3", "g6_c3_powerlaw", "g7_c5"])
def test_forward_nodes_over_every_node_is_bit_equal_to_forward(name):
    """Every node a seed: the subgraph is the graph, its edges reach the sub-plan's stable sort in the full plan's order, so
    the sub-plan's arrays are the full plan's and every launch is the same."""
    (case,) = cases.graph_cases(only=[name])
    model = make_model(cases.MODELS[case.model])
    x, ei = torch.from_numpy(case.node_features).to(DEV), torch.from_numpy(case.edge_index).to(DEV)
    with torch.no_grad():
        full = model(x, ei, case.edge_texts)
        got = model.forward_nodes(x, ei, case.edge_texts, torch.arange(x.size(0), device=DEV))
    assert torch.equal(got, full), name


_BIG = {}


def _big(which):
    """BASELINE configs 3 and 2 at their own sizes (the bench's synthetic graphs and seeds)."""
    if which not in _BIG:
        N, E, R, name, seed = {"c3": (1_000_000, 10_000_000, 64, "c3", 1003), "c2": (100_000, 1_000_000, 32, "c2", 1002)}[which]
        cfg = cases.MODELS[name]
        kg = synth.make_kg(N, E, R, cfg.node_feat_dim, seed, "uniform")
        _BIG[which] = (cfg, cfg.params(), kg)
    return _BIG[which]


def test_c3_at_full_size_against_forward_and_the_oracle_on_the_3_hop_subgraph(monkeypatch):
    """Verdict item 3(a): the whole model at BASELINE config 3's size (1 M nodes, 10 M edges, 64 relations, d = 128, three
    layers) through the default plan, ~100 seeds, against forward(...)[seeds] and against the oracle run on the host over
    the seeds' 3-hop subgraph (which determines their rows exactly)."""
    monkeypatch.delenv("GHF_KERNEL", raising=False)
    cfg, params, kg = _big("c3")
    model = make_model(cfg, params)
    texts = kg.edge_texts()
    x, ei = torch.from_numpy(kg.node_features).to(DEV), torch.from_numpy(kg.edge_index).to(DEV)
    plan = model.plan_for(ei, texts, x.size(0), DEV)
    assert plan.block_nodes == 384 and plan.wlayout == _native.WLAYOUT_SPLIT2H
    seeds = np.random.default_rng(3).choice(kg.num_nodes, 100, replace=False)
    with torch.no_grad():
        got = model.forward_nodes(x, ei, texts, torch.from_numpy(seeds).to(DEV))
        assert model.last_range_flags == 0
        sub = model.last_subgraph
        assert sub["block_nodes"] == 384 and sub["wlayout"] == _native.WLAYOUT_SPLIT2H
        again = model.forward_nodes(x, ei, texts, torch.from_numpy(seeds).to(DEV))
        full = model(x, ei, texts)
    assert model.last_range_flags == 0
    assert torch.equal(got, again)
    assert_close(got.cpu().numpy(), full[torch.from_numpy(seeds).to(DEV)].cpu().numpy(), "C3: forward_nodes vs forward[seeds]")
    _, nl, nid, m, e_sub, r_sub = np_subgraph(kg.edge_index[0], kg.edge_index[1], kg.rel_ids, kg.num_nodes, seeds, 3)
    assert sub["m"] == m and sub["edges"] == e_sub.shape[1]
    names = kg.relation_texts
    ref = O.forward(params, kg.node_features[nl], e_sub, [names[r] for r in r_sub.tolist()], variant="factorised").numpy()
    assert_close(got.cpu().numpy(), ref[nid[seeds]], "C3: forward_nodes vs the oracle on the 3-hop subgraph")


def test_c2_at_full_size_1024_seeds(monkeypatch):
    monkeypatch.delenv("GHF_KERNEL", raising=False)
    cfg, params, kg = _big("c2")
    model = make_model(cfg, params)
    texts = kg.edge_texts()
    x, ei = torch.from_numpy(kg.node_features).to(DEV), torch.from_numpy(kg.edge_index).to(DEV)
    seeds = torch.from_numpy(np.random.default_rng(2).choice(kg.num_nodes, 1024, replace=False)).to(DEV)
    with torch.no_grad():
        got = model.forward_nodes(x, ei, texts, seeds)
        full = model(x, ei, texts)
    assert model.last_range_flags == 0
    assert_close(got.cpu().numpy(), full[seeds].cpu().numpy(), "C2: forward_nodes vs forward[seeds]")


def test_wide_rows_on_the_csr_plan():
    """d = 256 with many relations: the inference plan is a CSR plan (relation-stationary layer), over every subgraph row."""
    (case,) = cases.graph_cases(only=["g7_c5"])
    cfg = cases.MODELS["c5"]
    kg = synth.make_kg(5000, 40000, 96, cfg.node_feat_dim, 77, "powerlaw")
    for x_np, ei_np, texts in ((case.node_features, case.edge_index, case.edge_texts),
                               (kg.node_features, kg.edge_index, kg.edge_texts())):
        model = make_model(cfg)
        x, ei = torch.from_numpy(x_np).to(DEV), torch.from_numpy(ei_np).to(DEV)
        assert model.plan_for(ei, texts, x.size(0), DEV).block_nodes == 1
        with torch.no_grad():
            full = model(x, ei, texts)
            for nodes in _subsets(x.size(0)):
                got = model.forward_nodes(x, ei, texts, torch.tensor(nodes, dtype=torch.int32))
                assert model.last_subgraph["block_nodes"] == 1
                assert_close(got.cpu().numpy(), full[torch.tensor(nodes)].cpu().numpy(), f"wide rows, nodes {nodes[:4]}")


# ---- training -------------------------------------------------------------------------------------------------------

def _grads(model, fn, x_np, gout):
    model.zero_grad(set_to_none=True)
    x = torch.from_numpy(x_np).to(DEV).requires_grad_(True)
    out = fn(x)
    (out * gout).sum().backward()
    return out.detach(), {k: p.grad.detach().clone() if p.grad is not None else None for k, p in model.named_parameters()}, \
        x.grad.detach().clone()


def _compare_training(model, x_np, ei_np, texts, nodes, what, skip_zero=False):
    ei = torch.from_numpy(ei_np).to(DEV)
    idx = torch.tensor(nodes, device=DEV)
    gout = torch.from_numpy(synth.normal(41, "gout", (len(nodes), model.hidden_dim))).to(DEV)
    model.train()
    want_out, want, want_x = _grads(model, lambda x: model(x, ei, texts)[idx], x_np, gout)
    got_out, got, got_x = _grads(model, lambda x: model.forward_nodes(x, ei, texts, idx), x_np, gout)
    assert_close(got_out.cpu().numpy(), want_out.cpu().numpy(), f"{what}: training forward")
    for k in want:
        if want[k] is None or (skip_zero and float(want[k].abs().max()) == 0.0):
            assert got[k] is None or float(got[k].abs().max()) == 0.0, k
            continue
        assert got[k] is not None, f"{what}: no gradient on {k}"
        _grad_check(k, got[k].cpu().numpy(), want[k].cpu().numpy())
    _grad_check("node_features", got_x.cpu().numpy(), want_x.cpu().numpy())


def test_training_gradients_equal_those_of_forward_rows():
    cfg = cases.MODELS["small"]
    kg = ToyKnowledgeGraph(feat_dim=cfg.node_feat_dim)
    _compare_training(make_model(cfg), kg.node_features.numpy(), kg.edge_index.numpy(), kg.edge_texts, [3, 0, 3, 6], "toy")
    cfg = cases.MODELS["c3"]
    g = synth.make_kg(3000, 24000, 7, cfg.node_feat_dim, seed=55, kind="powerlaw")
    nodes = np.random.default_rng(5).choice(3000, 40, replace=False).tolist()
    _compare_training(make_model(cfg), g.node_features, g.edge_index, g.edge_texts(), nodes, "c3-shaped synthetic")


def test_training_at_c2_full_size():
    cfg, params, kg = _big("c2")
    nodes = np.random.default_rng(8).choice(kg.num_nodes, 1024, replace=False).tolist()
    _compare_training(make_model(cfg, params), kg.node_features, kg.edge_index, kg.edge_texts(), nodes, "C2 full size")


def test_training_range_guard_fallback_on_the_subgraph():
    """Feature rows 2^30 wide among the seeds' neighbours (every third row): the recorded forward on the sub-plan flags them
    and reruns on the exact kernels, as forward does."""
    d = 128
    cfg = cases.ModelCfg(text_dim=16, node_feat_dim=d, hidden_dim=d, num_layers=2, seed=909, log_scale=0.0, randomize_ln=True)
    p = cfg.params()
    p["input_proj.weight"] = np.eye(d, d, dtype=np.float32)
    p["input_proj.bias"] = np.zeros(d, np.float32)
    for head in ("W_msg", "W_self"):
        k = max(int(n.split(".")[4]) for n in p if n.startswith(f"weight_generators.0.generators.{head}."))
        p[f"weight_generators.0.generators.{head}.{k}.weight"][:d] = 0.0
        p[f"weight_generators.0.generators.{head}.{k}.bias"][:d] = 0.0
    kg = synth.make_kg(600, 5000, 5, d, seed=31)
    x = np.abs(kg.node_features).astype(np.float32) + 0.1
    x[::3, 0] *= 2.0 ** 30
    model = make_model(cfg, p)
    _compare_training(model, x, kg.edge_index, kg.edge_texts(), [1, 2, 4, 5, 100, 401], "range guard", skip_zero=True)
    assert model.last_range_flags & _native.RANGE_ROWS


# ---- edge cases -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["small", "c3"])
def test_duplicates_negative_ids_empty_subgraph_and_the_ids_form(name):
    cfg = cases.MODELS[name]
    ei_np, rel_np, N = _graph_with_isolated(500, 3000, 6, 91, "uniform", extra=30)
    x_np = synth.normal(92, "x", (N, cfg.node_feat_dim))
    texts_all = synth.relation_names(6)
    texts = [texts_all[r] for r in rel_np.tolist()]
    model = make_model(cfg)
    x, ei = torch.from_numpy(x_np).to(DEV), torch.from_numpy(ei_np).to(DEV)
    with torch.no_grad():
        full = model(x, ei, texts)
        for nodes in ([7, -1, 7, 3, -N], [N - 1, N - 5, N - 1], [-1]):       # the last two: seeds without in-edges
            idx = torch.tensor(nodes, device=DEV)
            got = model.forward_nodes(x, ei, texts, idx)
            assert_close(got.cpu().numpy(), full[idx].cpu().numpy(), f"{name} nodes {nodes}")
            if nodes[0] == N - 1:
                assert model.last_subgraph["edges"] == 0
            via_ids = model.forward_nodes_ids(x, ei, torch.from_numpy(rel_np).to(DEV), texts_all, idx.to(torch.int32))
            assert_close(via_ids.cpu().numpy(), got.cpu().numpy(), f"{name} forward_nodes_ids")
