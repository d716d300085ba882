"""forward_nodes(..., exclude=) on the MI355X: the extraction without given edges (include/ghf.h: ghf_subgraph_*_excl) bit
for bit against the numpy restatement (_exclude.py), the node-batch forward against forward_ids on the reduced edge arrays
(bit-equal over every node) and against the oracle on the reduced graph, and its gradients against those of forward's rows."""

import numpy as np
import pytest
import torch

import _exclude as X
import _sampling as S
import cases
from _util import assert_close
from graph_hypernetwork_forge_amd import HyperGNN, ToyKnowledgeGraph, _native, synth
from graph_hypernetwork_forge_amd.plan import build_plan
from oracle import hypergnn_oracle as O

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
KEYS = ("dist", "node_list", "new_id", "edge_index", "rel")
MATRIX = [(64, 7, False), (128, 7, False), (256, 200, True)]


def make_model(cfg: cases.ModelCfg, params=None) -> HyperGNN:
    m = HyperGNN(cfg.text_dim, cfg.node_feat_dim, cfg.hidden_dim, cfg.num_layers, char_emb_dim=cfg.char_emb_dim)
    m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in (params or cfg.params()).items()})
    return m.to(DEV).eval()


def _grad_check(name, got, want, rtol=2e-4, l2=5e-5):
    """The gradient tolerances of test_subgraph_nodes.py: rtol 2e-4, atol 1e-4 * scale, relative L2 5e-5."""
    gw, gg = want.astype(np.float64), got.astype(np.float64)
    assert gg.shape == gw.shape, f"d{name}: shape {gg.shape} vs {gw.shape}"
    scale = float(np.abs(gw).max())
    assert np.allclose(gg, gw, rtol=rtol, atol=1e-4 * max(scale, 1e-30)), \
        f"d{name}: max abs err {np.abs(gg - gw).max():.3e} at scale {scale:.3e}"
    rel_l2 = np.linalg.norm(gg - gw) / max(np.linalg.norm(gw), 1e-30)
    assert rel_l2 < l2, f"d{name}: relative L2 {rel_l2:.3e}"


def _seeds(v):
    return torch.tensor(v, dtype=torch.int64, device=DEV)


def _dev_keys(src, dst, rel=None, R=None):
    """(keys, typed) for _native.subgraph: the restatement's sorted uint64 keys as the int64 device tensor the binding takes."""
    return torch.from_numpy(X.keys(src, dst, rel, R).view(np.int64)).to(DEV), rel is not None


def _same(a, b, what):
    assert a["m"] == b["m"], what
    for key in KEYS:
        assert torch.equal(a[key], b[key]), f"{what}: {key}"


def _equals(got, want, what):
    dist, nl, nid, m, e_sub, r_sub = want
    assert np.array_equal(got["dist"].cpu().numpy(), dist), what
    assert got["m"] == m, what
    assert np.array_equal(got["node_list"].cpu().numpy(), nl), what
    assert np.array_equal(got["new_id"].cpu().numpy(), nid), what
    assert np.array_equal(got["edge_index"].cpu().numpy(), e_sub), what
    assert np.array_equal(got["rel"].cpu().numpy(), r_sub), what


# ---- the graphs of test_extraction_equals_the_numpy_restatement, with parallel edges and a crafted destination ------

_GRAPHS = {}


def _matrix_graph(kind, d, R, generic):
    """3,000 + 40 isolated nodes, 20,000 edges (test_subgraph_nodes.py's), plus hand-made edges: edge 0 again with the same
    relation and with two others, edge 1 again with another relation, and node N - 7 (isolated before) with four in-edges —
    one more than the cap 3 of the sampled test.  Returns the plan, the edges in the caller's and in the plan's order, the
    seed picks and the exclusion lists (name -> (src, dst, rel or None)); computed once per shape."""
    if (kind, d) in _GRAPHS:
        return _GRAPHS[kind, d]
    ei, rel = synth.make_graph_arrays(3000, 20000, R, 71 + d, kind)
    N = 3000 + 40
    crafted = N - 7
    s0, t0, r0, s1, t1, r1 = int(ei[0][0]), int(ei[1][0]), int(rel[0]), int(ei[0][1]), int(ei[1][1]), int(rel[1])
    extra = [(s0, t0, r0), (s0, t0, (r0 + 1) % R), (s0, t0, (r0 + 2) % R), (s1, t1, (r1 + 3) % R),
             (10, crafted, 0), (20, crafted, 1), (30, crafted, 0), (40, crafted, 2)]
    ei = np.concatenate([ei, np.array([[e[0] for e in extra], [e[1] for e in extra]], dtype=np.int64)], axis=1)
    rel = np.concatenate([rel, np.array([e[2] for e in extra], dtype=np.int64)])
    plan = build_plan(torch.from_numpy(ei).to(DEV), torch.from_numpy(rel), synth.relation_names(R), N, d, DEV,
                      force_generic=generic)
    assert (plan.block_nodes == 1) == generic
    order = S.plan_order(ei, rel, N, R, plan.block_nodes)
    src, dst, rl = ei[0][order], ei[1][order], rel[order]
    indeg = np.bincount(ei[1], minlength=N)
    hub = int(indeg.argmax())
    one = int(np.nonzero(indeg[:3000] >= 3)[0][0])                              # a seed with a few in-edges
    rng = np.random.default_rng(d + R)
    picks = [rng.choice(3000, 17, replace=False).tolist() + [5, one, 5, one],    # duplicates
             [N - 1, N - 3, N - 1],                                             # no in-edges (nor any edge)
             [hub, 11, N - 2, hub],                                             # a hub among the seeds
             [crafted, t0, t1, one],                                            # the hand-made edges' destinations
             list(range(N))]                                                    # every node
    E = ei.shape[1]
    pairs = set(zip(ei[0].tolist(), ei[1].tolist()))
    triples = set(zip(ei[0].tolist(), ei[1].tolist(), rel.tolist()))
    pick = np.unique(np.concatenate([[0, 1], rng.choice(E, 198, replace=False)]))         # edges 0 and 1: they have twins
    lists = {"200 edges, typed": (ei[0][pick], ei[1][pick], rel[pick]),
             "200 edges, untyped": (ei[0][pick], ei[1][pick], None)}
    # entries that match nothing: pairs that are no edge, and an edge's pair under a relation it does not carry
    ns, nt = rng.integers(0, N, 300), rng.integers(0, N, 300)
    no = [i for i in range(300) if (int(ns[i]), int(nt[i])) not in pairs]
    wrong = [(int(ei[0][e]), int(ei[1][e]), int((rel[e] + 1) % R)) for e in pick]
    wrong = [w for w in wrong if w not in triples]
    assert len(no) > 100 and len(wrong) > 100
    lists["non-edges, untyped"] = (ns[no], nt[no], None)
    lists["non-edges and wrong relations, typed"] = (np.r_[ns[no], [w[0] for w in wrong]], np.r_[nt[no], [w[1] for w in wrong]],
                                                     np.r_[rng.integers(0, R, len(no)), [w[2] for w in wrong]])
    lists["reverses only"] = (ei[1][pick], ei[0][pick], None)
    into_one = np.nonzero(ei[1] == one)[0]
    into_hub = np.nonzero(ei[1] == hub)[0]
    assert into_one.size >= 3 and into_hub.size > 10
    lists["every in-edge of one seed"] = (ei[0][into_one], ei[1][into_one], rel[into_one])
    lists["every in-edge of the hub"] = (ei[0][into_hub], ei[1][into_hub], None)
    twice = np.r_[pick[:50], pick[:50], pick[:7]]
    lists["duplicates"] = (ei[0][twice], ei[1][twice], rel[twice])
    lists["one in-edge of the crafted destination"] = (np.array([20]), np.array([crafted]), np.array([1]))
    masks = {name: X.excluded(src, dst, rl, R, *xl) for name, xl in lists.items()}
    # what the lists are meant to exercise, said of the masks
    twins0 = (src == s0) & (dst == t0)
    assert twins0.sum() >= 4 and masks["200 edges, untyped"][twins0].all()                  # every relation's twin goes
    assert masks["200 edges, typed"][twins0 & (rl == r0)].all() and masks["200 edges, typed"][twins0].sum() < twins0.sum()
    assert not masks["non-edges, untyped"].any() and not masks["non-edges and wrong relations, typed"].any()
    forward_only = np.array([(int(t), int(s)) not in pairs for s, t in zip(ei[0][pick], ei[1][pick])])
    assert forward_only.sum() > 150                                                       # their forward edges must stay:
    stay = set(zip(ei[0][pick][forward_only].tolist(), ei[1][pick][forward_only].tolist()))
    assert not any((s, t) in stay for s, t in zip(src[masks["reverses only"]].tolist(), dst[masks["reverses only"]].tolist()))
    assert np.array_equal(masks["duplicates"], X.excluded(src, dst, rl, R, ei[0][pick[:50]], ei[1][pick[:50]], rel[pick[:50]]))
    out = dict(plan=plan, ei=ei, rel=rel, edges=(src, dst, rl), N=N, R=R, picks=picks, lists=lists, masks=masks, hub=hub,
               crafted=crafted)
    _GRAPHS[kind, d] = out
    return out


@pytest.mark.parametrize("kind", ["uniform", "powerlaw"])
@pytest.mark.parametrize("d,R,generic", MATRIX)
def test_extraction_without_the_excluded_edges_equals_the_numpy_restatement(kind, d, R, generic):
    g = _matrix_graph(kind, d, R, generic)
    plan, (src, dst, rl), N = g["plan"], g["edges"], g["N"]
    for name, xl in g["lists"].items():
        keys, dead = _dev_keys(*xl, R=R), g["masks"][name]
        for seeds in g["picks"]:
            for k in (1, 2, 3):
                got = _native.subgraph(plan, _seeds(seeds), k, exclude=keys)
                what = f"{kind} d={d} k={k} list={name} seeds={seeds[:4]}"
                _equals(got, X.np_subgraph_excl(src, dst, rl, N, seeds, k, dead), what)
                if not dead.any():
                    _same(got, _native.subgraph(plan, _seeds(seeds), k), what)
    into_hub = g["masks"]["every in-edge of the hub"]
    got = _native.subgraph(plan, _seeds([g["hub"]]), 3, exclude=_dev_keys(*g["lists"]["every in-edge of the hub"], R=R))
    assert into_hub.sum() > 10 and got["m"] == [1, 1, 1, 1] and got["edge_index"].size(1) == 0


@pytest.mark.parametrize("kind", ["uniform", "powerlaw"])
@pytest.mark.parametrize("d,R,generic", MATRIX)
def test_sampled_extraction_without_the_excluded_edges_equals_the_numpy_restatement(kind, d, R, generic):
    g = _matrix_graph(kind, d, R, generic)
    plan, (src, dst, rl), N, crafted = g["plan"], g["edges"], g["N"], g["crafted"]
    for name, xl in g["lists"].items():
        keys, dead = _dev_keys(*xl, R=R), g["masks"][name]
        for seeds in g["picks"]:
            for fanout in ((3, 3, 3), (2, -1, 4), (-1, -1)):
                seed = 1000 * len(fanout) + fanout[0] + 2
                got = _native.subgraph_sample(plan, _seeds(seeds), fanout, seed, exclude=keys)
                what = f"{kind} d={d} fanout={fanout} list={name} seeds={seeds[:4]}"
                _equals(got, X.np_subgraph_sample_excl(src, dst, rl, N, seeds, fanout, seed, dead), what)
                assert got["host_reads"] <= sum(f != -1 for f in fanout), what
                if not dead.any():
                    _same(got, _native.subgraph_sample(plan, _seeds(seeds), fanout, seed), what)
    # cap 3, four in-edges of which one is excluded: all the rest stay, whatever the seed
    keys = _dev_keys(*g["lists"]["one in-edge of the crafted destination"], R=R)
    for seed in (1, 2, 3):
        got = _native.subgraph_sample(plan, _seeds([crafted]), (3, 3, 3), seed, exclude=keys)
        into = got["edge_index"][1] == got["new_id"][crafted]
        assert sorted(got["node_list"][got["edge_index"][0][into]].tolist()) == [10, 30, 40], seed
        plain = _native.subgraph_sample(plan, _seeds([crafted]), (3, 3, 3), seed)
        assert int((plain["edge_index"][1] == plain["new_id"][crafted]).sum()) == 3


@pytest.mark.parametrize("kind", ["uniform", "powerlaw"])
@pytest.mark.parametrize("d,R,generic", MATRIX)
def test_an_empty_list_is_the_call_without_exclude_bit_for_bit(kind, d, R, generic):
    g = _matrix_graph(kind, d, R, generic)
    plan = g["plan"]
    empty = torch.zeros(0, dtype=torch.int64, device=DEV)
    for typed in (False, True):
        for seeds in g["picks"]:
            for k in (1, 2, 3):
                _same(_native.subgraph(plan, _seeds(seeds), k, exclude=(empty, typed)), _native.subgraph(plan, _seeds(seeds), k),
                      f"exact k={k} typed={typed}")
            for fanout in ((3, 3, 3), (2, -1, 4), (-1, -1)):
                got = _native.subgraph_sample(plan, _seeds(seeds), fanout, 77, exclude=(empty, typed))
                _same(got, _native.subgraph_sample(plan, _seeds(seeds), fanout, 77), f"sampled {fanout} typed={typed}")


def test_an_unsorted_list_may_miss_matches_but_stays_in_bounds():
    """ghf.h's guarantee for a caller who forgot to sort: the search stays inside the list, so the call completes; each
    edge is then either excluded or not — the result lies between the two extractions."""
    g = _matrix_graph("powerlaw", 128, 7, False)
    plan, xl = g["plan"], g["lists"]["200 edges, typed"]
    keys, _ = _dev_keys(*xl, R=g["R"])
    shuffled = keys[torch.from_numpy(np.random.default_rng(1).permutation(keys.numel())).to(DEV)].contiguous()
    seeds = _seeds(list(range(g["N"])))
    got = _native.subgraph(plan, seeds, 2, exclude=(shuffled, True))["edge_index"].size(1)
    assert _native.subgraph(plan, seeds, 2, exclude=(keys, True))["edge_index"].size(1) <= got <= plan.E


# ---- the model: bit-equal to forward_ids on the reduced edge arrays, and against the oracle ------------------------

def _ids_case(name):
    (case,) = cases.graph_cases(only=[name])
    names = list(dict.fromkeys(case.edge_texts))
    at = {t: i for i, t in enumerate(names)}
    return case, names, np.array([at[t] for t in case.edge_texts], dtype=np.int64)


@pytest.mark.parametrize("name", ["g6_c3", "g6_c3_powerlaw", "g7_c5", "g2_toy"])
def test_over_every_node_the_result_is_bit_equal_to_forward_ids_on_the_reduced_edge_arrays(name):
    """Every node a seed, a typed tenth of the edges excluded: the compaction is stable, so the sub-plan's sort sees the
    reduced graph's edges in the reduced graph's order, and every launch is that of forward_ids on the reduced arrays."""
    case, names, rel = _ids_case(name)
    model = make_model(cases.MODELS[case.model])
    ei_np, N, E = case.edge_index, case.node_features.shape[0], case.edge_index.shape[1]
    pick = np.random.default_rng(E).choice(E, max(1, E // 10), replace=False)
    dead = X.excluded(ei_np[0], ei_np[1], rel, len(names), ei_np[0][pick], ei_np[1][pick], rel[pick])
    assert pick.size <= dead.sum() < E
    x, ei, rel_t = torch.from_numpy(case.node_features).to(DEV), torch.from_numpy(ei_np).to(DEV), torch.from_numpy(rel).to(DEV)
    ei2, rel2 = torch.from_numpy(ei_np[:, ~dead]).to(DEV), torch.from_numpy(rel[~dead]).to(DEV)
    excl = (torch.from_numpy(ei_np[0][pick]), torch.from_numpy(ei_np[1][pick]).to(DEV), torch.from_numpy(rel[pick]).to(torch.int32))
    with torch.no_grad():
        got = model.forward_nodes_ids(x, ei, rel_t, names, torch.arange(N, device=DEV), exclude=excl)
        sub = dict(model.last_subgraph)
        want = model.forward_ids(x, ei2, rel2, names)
        plain = model.forward_nodes_ids(x, ei, rel_t, names, torch.arange(N, device=DEV))
        none = model.forward_nodes_ids(x, ei, rel_t, names, torch.arange(N, device=DEV), exclude=(excl[0][:0], excl[1][:0]))
    assert sub["exclude"] == (pick.size, True) and sub["edges"] == int((~dead).sum()) and sub["m"][0] == N
    assert torch.equal(got, want), name
    assert model.last_subgraph["exclude"] == (0, False) and torch.equal(none, plain) and not torch.equal(got, plain)


def _oracle_rows(params, case, dead, nodes):
    texts = [t for t, gone in zip(case.edge_texts, dead.tolist()) if not gone]
    ref = O.forward(params, case.node_features, case.edge_index[:, ~dead], texts, variant="factorised").numpy()
    return ref[nodes]


@pytest.mark.parametrize("name", [n for n in cases.GRAPH_CASE_NAMES if n != "g5_c2"])
def test_partial_seeds_equal_the_oracle_on_the_reduced_graph(name):
    """The link-prediction recipe on the golden-case graphs: a batch of edges (every third one), seeds cat(heads, tails),
    exclude the batch — typed, the relations as strings (one entry more under a text that labels no edge), and untyped in
    both directions — against the oracle's forward on the graph without the excluded edges."""
    case, names, rel = _ids_case(name)
    cfg = cases.MODELS[case.model]
    params = cfg.params()
    model = make_model(cfg, params)
    ei_np, N, E = case.edge_index, case.node_features.shape[0], case.edge_index.shape[1]
    batch = np.arange(1, E, 3)[:64]                                      # (one edge: an empty batch, the plain call)
    h, t = ei_np[0][batch], ei_np[1][batch]
    nodes = np.r_[h, t, [0, N - 1]].astype(np.int64)
    x, ei = torch.from_numpy(case.node_features).to(DEV), torch.from_numpy(ei_np).to(DEV)
    typed = (torch.from_numpy(np.r_[h, [0]]), torch.from_numpy(np.r_[t, [N - 1]]),
             [case.edge_texts[e] for e in batch] + ["a text that labels no edge"])
    both = (torch.from_numpy(np.r_[h, t]).to(DEV), torch.from_numpy(np.r_[t, h] - N).to(DEV))   # (tails as negative ids)
    dead_typed = X.excluded(ei_np[0], ei_np[1], rel, len(names), h, t, rel[batch])
    dead_both = X.excluded(ei_np[0], ei_np[1], rel, len(names), np.r_[h, t], np.r_[t, h])
    assert dead_typed.sum() >= batch.size and dead_both.sum() >= dead_typed.sum()
    for excl, dead, is_typed in ((typed, dead_typed, True), (both, dead_both, False)):
        if dead.all():
            continue                                                     # (no edge left: the oracle cannot encode that graph)
        with torch.no_grad():
            got = model.forward_nodes(x, ei, case.edge_texts, torch.from_numpy(nodes), exclude=excl)
        assert model.last_subgraph["exclude"] == (excl[0].numel(), is_typed)
        assert_close(got.cpu().numpy(), _oracle_rows(params, case, dead, nodes), f"{name} typed={is_typed}: vs the oracle")
        with torch.no_grad():
            sampled = model.forward_nodes(x, ei, case.edge_texts, torch.from_numpy(nodes), fanout=-1, exclude=excl)
        assert torch.equal(sampled, got), f"{name} typed={is_typed}: fanout -1"


# ---- training -------------------------------------------------------------------------------------------------------

def _grads(model, fn, x_np, gout):
    model.zero_grad(set_to_none=True)
    x = torch.from_numpy(x_np).to(DEV).requires_grad_(True)
    out = fn(x)
    (out * gout).sum().backward()
    return out.detach(), {k: p.grad.detach().clone() if p.grad is not None else None for k, p in model.named_parameters()}, \
        x.grad.detach().clone()


def _check_grads(want, got, want_x, got_x, what):
    for k in want:
        if want[k] is None:
            assert got[k] is None or float(got[k].abs().max()) == 0.0, k
            continue
        assert got[k] is not None, f"{what}: no gradient on {k}"
        _grad_check(k, got[k].cpu().numpy(), want[k].cpu().numpy())
    _grad_check("node_features", got_x.cpu().numpy(), want_x.cpu().numpy())


def _training_case(which):
    if which == "toy":
        cfg = cases.MODELS["small"]
        kg = ToyKnowledgeGraph(feat_dim=cfg.node_feat_dim)
        return cfg, kg.node_features.numpy(), kg.edge_index.numpy(), list(kg.edge_texts), [3, 0, 3, 6]
    if which == "block":
        cfg = cases.MODELS["c3"]
        g = synth.make_kg(3000, 24000, 7, cfg.node_feat_dim, seed=55, kind="powerlaw")
        hub = int(np.bincount(g.edge_index[1], minlength=3000).argmax())
        return cfg, g.node_features, g.edge_index, g.edge_texts(), [hub] + np.random.default_rng(5).choice(3000, 40, replace=False).tolist()
    (case,) = cases.graph_cases(only=["g7_c5"])
    nodes = np.random.default_rng(6).choice(case.node_features.shape[0], 30, replace=False).tolist()
    return cases.MODELS["c5"], case.node_features, case.edge_index, case.edge_texts, nodes


def _rel_of(texts):
    at = {t: i for i, t in enumerate(dict.fromkeys(texts))}
    return np.array([at[t] for t in texts], dtype=np.int64), len(at)


@pytest.mark.parametrize("which", ["toy", "block", "wide"])
@pytest.mark.parametrize("every_in_edge", [False, True])
def test_training_gradients_equal_those_of_forward_rows_on_the_reduced_graph(which, every_in_edge):
    """train(): the gradients of a fixed linear functional of the rows, for every parameter and node_features, against
    forward(reduced graph)[nodes] recorded the same way (test_subgraph_nodes.py's reference and bounds).  every_in_edge: the
    exclusion names every in-edge of every seed — the subgraph has no edge, and the recorded forward runs on the reduced
    edge arrays (never on the full graph, which would put the excluded edges back)."""
    cfg, x_np, ei_np, texts, nodes = _training_case(which)
    rel, R = _rel_of(texts)
    model = make_model(cfg).train()
    if every_in_edge:
        batch = np.nonzero(np.isin(ei_np[1], nodes))[0]
        excl = (torch.from_numpy(ei_np[0][batch]), torch.from_numpy(ei_np[1][batch]))
        dead = X.excluded(ei_np[0], ei_np[1], rel, R, ei_np[0][batch], ei_np[1][batch])
    else:
        into = np.nonzero(np.isin(ei_np[1], nodes))[0]
        batch = np.unique(np.r_[into[::2], np.arange(0, ei_np.shape[1], 9)])   # half the seeds' in-edges, a ninth of all
        excl = (torch.from_numpy(ei_np[0][batch]).to(DEV), torch.from_numpy(ei_np[1][batch]).to(DEV), [texts[e] for e in batch])
        dead = X.excluded(ei_np[0], ei_np[1], rel, R, ei_np[0][batch], ei_np[1][batch], rel[batch])
    assert 0 < dead.sum() < dead.size
    ei, idx = torch.from_numpy(ei_np).to(DEV), torch.tensor(nodes, device=DEV)
    ei2, texts2 = torch.from_numpy(ei_np[:, ~dead]).to(DEV), [t for t, gone in zip(texts, dead.tolist()) if not gone]
    gout = torch.from_numpy(synth.normal(41, "gout", (len(nodes), model.hidden_dim))).to(DEV)
    want_out, want, want_x = _grads(model, lambda x: model(x, ei2, texts2)[idx], x_np, gout)
    got_out, got, got_x = _grads(model, lambda x: model.forward_nodes(x, ei, texts, idx, exclude=excl), x_np, gout)
    what = f"{which} every_in_edge={every_in_edge}"
    assert model.last_subgraph["exclude"] == (batch.size, not every_in_edge)
    assert (model.last_subgraph["edges"] == 0) == every_in_edge
    assert_close(got_out.cpu().numpy(), want_out.cpu().numpy(), f"{what}: training forward")
    _check_grads(want, got, want_x, got_x, what)
    # with fanout and no cap that bites, the sampled call is the same function
    got_out, got, got_x = _grads(model, lambda x: model.forward_nodes(x, ei, texts, idx, fanout=-1, exclude=excl), x_np, gout)
    assert (model.last_subgraph["edges"] == 0) == every_in_edge and model.last_subgraph["fanout"] == (-1,) * cfg.num_layers
    assert_close(got_out.cpu().numpy(), want_out.cpu().numpy(), f"{what}: training forward, fanout -1")
    _check_grads(want, got, want_x, got_x, f"{what}, fanout -1")


@pytest.mark.parametrize("which", ["block", "wide"])
def test_sampled_training_with_caps_equals_forward_on_the_sampled_subgraph_which_holds_no_excluded_edge(which):
    """fanout with caps that bite: the call is forward on the sampled subgraph's rows (the extraction is checked against
    the restatement above), which holds none of the excluded edges; gradients against forward recorded on that subgraph."""
    cfg, x_np, ei_np, texts, nodes = _training_case(which)
    rel, R = _rel_of(texts)
    model = make_model(cfg).train()
    k = cfg.num_layers
    into = np.nonzero(np.isin(ei_np[1], nodes))[0]
    batch = np.unique(np.r_[into[::2], np.arange(0, ei_np.shape[1], 9)])
    excl = (torch.from_numpy(ei_np[0][batch]), torch.from_numpy(ei_np[1][batch]), [texts[e] for e in batch])
    ei, idx = torch.from_numpy(ei_np).to(DEV), torch.tensor(nodes, device=DEV)
    fanout, seed = (3, 2, 4)[:k], 2025
    gout = torch.from_numpy(synth.normal(41, "gout", (len(nodes), model.hidden_dim))).to(DEV)
    got_out, got, got_x = _grads(model, lambda x: model.forward_nodes(x, ei, texts, idx, fanout=fanout, seed=seed, exclude=excl),
                                 x_np, gout)
    rec = dict(model.last_subgraph)
    plan = model.plan_for(ei, texts, x_np.shape[0], DEV, training=True)
    at = {t: i for i, t in enumerate(plan.unique_texts)}
    keys = _dev_keys(ei_np[0][batch], ei_np[1][batch], np.array([at[texts[e]] for e in batch]), plan.R)
    sub = _native.subgraph_sample(plan, _seeds(nodes), fanout, seed, exclude=keys)
    assert rec["m"] == sub["m"] and rec["edges"] == sub["edge_index"].size(1) and rec["exclude"] == (batch.size, True)
    assert sub["edge_index"].size(1) < _native.subgraph(plan, _seeds(nodes), k, exclude=keys)["edge_index"].size(1)
    nl = sub["node_list"]
    s_src, s_dst = nl[sub["edge_index"][0]].cpu().numpy(), nl[sub["edge_index"][1]].cpu().numpy()
    s_rel = sub["rel"].cpu().numpy()
    gone = set(zip(ei_np[0][batch].tolist(), ei_np[1][batch].tolist(), [texts[e] for e in batch]))
    assert not any((s, t, plan.unique_texts[r]) in gone for s, t, r in zip(s_src.tolist(), s_dst.tolist(), s_rel.tolist()))
    sub_texts = [plan.unique_texts[r] for r in s_rel.tolist()]
    rows = sub["new_id"][_seeds(nodes)]
    xs_np = x_np[nl.cpu().numpy()]
    want_out, want, want_xs = _grads(model, lambda xs: model(xs, sub["edge_index"], sub_texts)[rows], xs_np, gout)
    want_x = torch.zeros_like(got_x)
    want_x[nl] = want_xs
    assert_close(got_out.cpu().numpy(), want_out.cpu().numpy(), f"{which}: sampled training forward")
    _check_grads(want, got, want_x, got_x, f"{which}, fanout {fanout}")
