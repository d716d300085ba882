"""The crafted edge-case graphs of _edge_graphs.py through every tuned message kernel, forward and backward, against the
float64 reference; and the reference's own small graphs through the whole model at the hidden sizes of the tuned kernels.

Run one route at a time (`-k "bx128-"`, ...): some of these shapes are launched by no other test.

The relation-stationary layer runs at every width it declares itself correct for (ghf_message_rs_supported: 128 .. 1024 in
steps of 128).  The width is no passive loop bound there: d % 256 == 0 runs the LDS-DMA ring (256-column tiles, d / 16 steps
over three buffers: 256 and 1024 leave d / 16 % 3 == 1, 512 leaves 2, 768 leaves 0), the other widths the register-staged
kernel (128-column tiles: 384, 640, 896 divide the grid index by 3, 5, 7); passes 0 and 2 hold d / 64 columns per lane.  384,
512, 768 and 1024 run all four kinds (both pass-1 kernels, every ring residue, the largest column count) and train; 128, 640
and 896 run the two-piece kernel on per-edge rows."""

import functools

import numpy as np
import pytest
import torch

import _edge_graphs as G
import cases
from _util import assert_close
from graph_hypernetwork_forge_amd import HyperGNN, _native, synth
from graph_hypernetwork_forge_amd.autograd import MessageLayerFn, _layer_weights, build_train_plan
from graph_hypernetwork_forge_amd.plan import build_plan, build_rs
from oracle import hypergnn_oracle as O

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

# route -> (d, GHF_KERNEL or None, geometry of _edge_graphs.geometries(), kind, runs (rs only), has a training path)
ROUTES = {
    "bx128": (128, None, "bx128", "block", None, True),
    "bx64": (64, "bx", "bx64", "block", None, True),
    "pp128": (128, "pp", "pp128", "block", None, False),
    "pp64": (64, None, "pp64", "block", None, True),             # the default below D64_PIECES_MIN_EDGES
    "rs_edges": (256, None, "csr256", "rs", False, True),        # training at 256: the CSR backward
    "rs_runs": (256, None, "csr256", "rs", True, False),
    "rs32_edges": (256, "rs32", "csr256", "rs", False, False),
    "rs32_runs": (256, "rs32", "csr256", "rs", True, False),
    "generic": (20, None, "csr20", "generic", None, True),
}
for _d in (384, 512, 768, 1024):                                 # (a width's routes side by side: they share its references)
    ROUTES.update({f"rs_edges{_d}": (_d, None, f"csr{_d}", "rs", False, True), f"rs_runs{_d}": (_d, None, f"csr{_d}", "rs", True, False),
                   f"rs32_edges{_d}": (_d, "rs32", f"csr{_d}", "rs", False, False),
                   f"rs32_runs{_d}": (_d, "rs32", f"csr{_d}", "rs", True, False)})
for _d in (128, 640, 896):                                       # (128: the block kernel's width — the plan is forced onto CSR)
    ROUTES[f"rs_edges{_d}"] = (_d, None, f"csr{_d}", "rs", False, False)
assert {v[0] for v in ROUTES.values() if v[3] == "rs" and v[5]} == set(G.RS_TRAIN_WIDTHS)      # (the host file proves these)
GEO = {g[0]: g for g in G.geometries()}
CASES = {key: {c.name: c for c in G.edge_cases(*GEO[key][2:], GEO[key][1])} for key in GEO}
FWD = [(r, n) for r, v in ROUTES.items() for n in CASES[v[2]]]
BWD = [(r, n) for r, v in ROUTES.items() if v[5] for n in CASES[v[2]]]


def _rel_l2(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-30))


@functools.lru_cache(maxsize=None)
def _reference(key, name):
    """(aggregate, h') of the float64 reference, computed once per (geometry, case) and shared by its routes; read-only."""
    case, (h, *rest) = CASES[key][name], _inputs(key, name)
    ref = G.layer_ref64(h, case.edge_index, case.rel, *rest)
    for a in ref:
        a.flags.writeable = False
    return ref


@functools.lru_cache(maxsize=7)                                  # (one width's cases: the weights of a case are up to 50 MB)
def _inputs(key, name):
    return G.layer_inputs(CASES[key][name], GEO[key][1], G.seed_for(key, name))


def _setup(route, name, monkeypatch):
    d, env, key, kind, runs, _ = ROUTES[route]
    if env:
        monkeypatch.setenv("GHF_KERNEL", env)
    else:
        monkeypatch.delenv("GHF_KERNEL", raising=False)
    case = CASES[key][name]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)                       # noqa: E731
    plan = build_plan(t(case.edge_index), t(case.rel), [""] * case.R, case.N, d, DEV, force_generic=(kind == "rs" and d == 128))
    _, _, bn, cr, sc, npw = GEO[key]
    want = {"bx128": lambda: _native.message_config(128), "bx64": lambda: _native.message_config(64),
            "pp128": lambda: _native.message_config(128, "pp"), "pp64": lambda: _native.exact_config(64)}.get(key)
    if want is not None:
        cfg = want()
        assert (plan.block_nodes, plan.wlayout, plan.chunk_rows) == (cfg[0], cfg[1], cfg[2]) == (bn, cfg[1], cr), f"{route}: plan geometry"
        assert plan.wlayout == (_native.WLAYOUT_SPLIT2H if key.startswith("bx") else _native.WLAYOUT_FRAG16)
    else:
        assert (plan.block_nodes, plan.wlayout, plan.chunk_rows) == (1, _native.WLAYOUT_NATURAL, 0), f"{route}: a CSR plan"
        assert _native.rs_supported(d) == (kind == "rs")
    return case, plan, G.realised(case, bn, cr, sc, npw), G.seed_for(key, name), t


@pytest.mark.parametrize("route,name", FWD, ids=[f"{r}-{n}" for r, n in FWD])
def test_forward(route, name, monkeypatch):
    d, env, key, kind, runs, _ = ROUTES[route]
    flag = _native.range_flag(DEV)
    flag.zero_()
    case, plan, res, seed, t = _setup(route, name, monkeypatch)
    N, bn = case.N, plan.block_nodes
    if kind == "block":                      # the plan's cut is the one the case was built for
        assert np.array_equal(plan.blk_chunk_off.cpu().numpy(), res["blk_chunk_off"]), "blk_chunk_off"
        assert np.array_equal(np.asarray(plan.item_off_host), res["item_off"]), "item_off_host"
        assert plan.n_slots == int(res["items_per_block"][res["items_per_block"] > 1].sum())
    h, Wm, Ws, b, gamma, beta = _inputs(key, name)
    ref_agg, ref_out = _reference(key, name)
    h_d, b_d, g_d, bt_d = t(h), t(b), t(gamma), t(beta)
    sub = None                               # the row range launched on its own: (first row, rows)
    if kind == "rs":
        rs = build_rs(plan, runs=runs)
        assert (rs.run_start is not None) == bool(runs)
        Y = torch.full((max(rs.rows, 1), d), float("nan"), device=DEV)
        Wm_d, Ws_d = t(Wm), t(Ws)
        if N >= 4:
            sub = (N // 3, max(N // 4, 1))

        def launch(out, no_tail, row0=0, rows=None, flags=_native.GHF_FLAG_NO_TAIL):
            _native.edge_transform_fwd(h_d, rs, Wm_d, Ws_d, b_d, Y)
            if no_tail:
                _native.segment_tail_fwd(Y, rs, None, None, None, 0.0, out, row0=row0, rows=rows, flags=flags)
            else:
                _native.segment_tail_fwd(Y, rs, h_d, g_d, bt_d, 1e-5, out, row0=row0, rows=rows)
    else:
        W, W2 = _layer_weights(plan, t(Wm), t(Ws), transpose=False)
        if kind == "block" and N > bn:
            sub = (bn, min(2 * bn, N) - bn)

        def launch(out, no_tail, row0=0, rows=None):
            _native.message_layer_fwd(h_d, plan, W, W2, b_d, plan.wlayout, None if no_tail else g_d, None if no_tail else bt_d,
                                      1e-5, out, row0=row0, rows=rows, flags=_native.GHF_FLAG_NO_TAIL if no_tail else 0)
    for no_tail, ref in ((False, ref_out), (True, ref_agg)):
        out = torch.full_like(h_d, float("nan"))
        launch(out, no_tail)
        got = out.cpu().numpy()
        print(f"FIG fwd {route} {name} no_tail={int(no_tail)} E={case.rel.size} rel_l2={_rel_l2(got, ref):.3e} "
              f"max_abs={np.nanmax(np.abs(got - ref)):.3e}")
        assert_close(got, ref, f"{route} {name} no_tail={no_tail}")
        again = torch.full_like(h_d, float("nan"))
        launch(again, no_tail)
        assert torch.equal(out, again), "a second launch gives other bits"
        if sub is not None:
            lo, hi = sub[0], sub[0] + sub[1]
            part = torch.full_like(h_d, 7.0)
            launch(part, no_tail, row0=lo, rows=hi - lo)
            assert torch.equal(part[lo:hi], out[lo:hi]), f"the row range [{lo}, {hi}) differs from the full launch"
            assert bool((part[:lo] == 7.0).all()) and bool((part[hi:] == 7.0).all()), "rows outside the range were written"
    if kind == "rs":
        # GHF_FLAG_RAW_SUM (what the backward's passes run under): the sum the mean divides, left undivided.  Held to the
        # aggregate's bounds per unit of the divisor: raw / max(indeg, 1) against the reference aggregate (the division is
        # done here in float64; the kernel's own fp32 sum is the one both outputs start from).
        raw = torch.full_like(h_d, float("nan"))
        launch(raw, True, flags=_native.GHF_FLAG_NO_TAIL | _native.GHF_FLAG_RAW_SUM)
        div = np.maximum(res["indeg"], 1).astype(np.float64)[:, None]
        got = raw.cpu().numpy().astype(np.float64) / div
        print(f"FIG fwd {route} {name} raw_sum rel_l2={_rel_l2(got, ref_agg):.3e} max_abs={np.nanmax(np.abs(got - ref_agg)):.3e}")
        assert_close(got, ref_agg, f"{route} {name} raw sum / max(indeg, 1)")
    assert int(flag.item()) == 0, f"range guard word {int(flag.item())} on inputs of ordinary dynamic range"


@pytest.mark.parametrize("route,name", BWD, ids=[f"{r}-{n}" for r, n in BWD])
def test_backward(route, name, monkeypatch):
    d, env, key, kind, runs, _ = ROUTES[route]
    flag = _native.range_flag(DEV)
    flag.zero_()
    case, plan, res, seed, t = _setup(route, name, monkeypatch)
    tp = build_train_plan(t(case.edge_index), t(case.rel), plan, d, DEV)
    if name == "sources_hub_with_sc_plus_1_chunks_of_out_edges":
        assert tp.rev.n_slots > 0, "the hub source must be a split block of the reversed plan"
    ins = _inputs(key, name)
    gout = synth.normal(77, "gout", (case.N, d))
    th = torch.from_numpy
    ref_in = [th(a).double().requires_grad_(True) for a in ins]
    _, ref = G.layer_ref64_torch(ref_in[0], th(case.edge_index), th(case.rel), *ref_in[1:])
    ref.backward(th(gout).double())
    runs_ = []
    for _ in range(2):
        args = [t(a).requires_grad_(True) for a in ins]
        out = MessageLayerFn.apply(*args, 1e-5, tp)
        assert int(flag.item()) == 0 or len(runs_), f"range guard word {int(flag.item())} after the training forward"
        out.backward(t(gout))
        runs_.append((out.detach(), [a.grad for a in args]))
    assert_close(runs_[0][0].cpu().numpy(), ref.detach().numpy(), f"{route} {name} training forward")
    for n, got, again, want in zip(("h", "W_msg", "W_self", "bias", "gamma", "beta"), runs_[0][1], runs_[1][1], ref_in):
        gw, gg = want.grad.numpy(), got.cpu().numpy().astype(np.float64)
        scale = float(np.abs(gw).max())
        print(f"FIG bwd {route} {name} d{n} rel_l2={_rel_l2(gg, gw):.3e} max_abs={np.abs(gg - gw).max():.3e} scale={scale:.3e}")
        assert np.allclose(gg, gw, rtol=2e-4, atol=2e-5 * max(scale, 1.0)), \
            f"d{n}: max abs err {np.abs(gg - gw).max():.3e} at scale {scale:.3e}"
        assert _rel_l2(gg, gw) < 2e-5, f"d{n}: relative L2 {_rel_l2(gg, gw):.3e}"
        assert torch.equal(got, again), f"d{n}: a second backward gives other bits"
    # The rows the gradient passes cut are not the test's inputs: on the wide-row layer a graph with hubs sums rows of G that
    # lie 2^-12 apart (the hubs' are divided by their in-degree) and meets the guard's rule by itself at some widths.  The
    # word is held to what the rule gives on the float64 rows (_edge_graphs.cut_rows_margin; test_edge_graphs_host.py shows
    # that every case here can be called): 0 wherever they are of ordinary range, GHF_RANGE_ROWS where they are not.
    want_word = 0
    if kind == "rs":
        margin = G.cut_rows_margin(case, ins[0], _reference(key, name)[0], ins[4], gout)
        want_word = G.predicted_range_word(margin["backward"])
        print(f"FIG bwd {route} {name} guard margin fwd={margin['forward']:.3f} bwd={margin['backward']:.3f} word={int(flag.item())}")
    assert int(flag.item()) == want_word, f"range guard word {int(flag.item())}, the rows' own range gives {want_word}"


# ---- the reference's own small graphs through the whole model at hidden 64 / 128 / 256 ----------------------------------

SMALL_GRAPHS = ["g1_demo", "g2_chain", "g2_one_edge", "g2_all_unseen", "g2_empty_nonascii"]


def _small_graph(graph, cfg):
    (c,) = cases.graph_cases(toy_features=np.zeros((8, 1), dtype=np.float32), only=[graph])
    N = c.node_features.shape[0]
    return synth.normal(1300 + N, "x", (N, cfg.node_feat_dim)), c.edge_index, c.edge_texts


def _model(cfg, params, train=False):
    m = HyperGNN(cfg.text_dim, cfg.node_feat_dim, cfg.hidden_dim, cfg.num_layers, char_emb_dim=cfg.char_emb_dim)
    m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in params.items()})
    return m.to(DEV).train(train)


@pytest.mark.parametrize("model_name", ["c2", "c3", "c5"])
@pytest.mark.parametrize("graph", SMALL_GRAPHS)
def test_small_graphs_through_the_whole_model(graph, model_name):
    cfg = cases.MODELS[model_name]
    x, ei, texts = _small_graph(graph, cfg)
    params = cfg.params()
    model = _model(cfg, params)
    with torch.no_grad():
        out = model(torch.from_numpy(x).to(DEV), torch.from_numpy(ei).to(DEV), texts)
    ref = O.forward(params, x, ei, texts, variant="factorised").numpy()
    print(f"FIG model {model_name} {graph} rel_l2={_rel_l2(out.cpu().numpy(), ref):.3e}")
    assert_close(out.cpu().numpy(), ref, f"{model_name} on {graph}")
    assert model.last_range_flags == 0


@pytest.mark.parametrize("model_name", ["c2", "c3", "c5"])
def test_toy_graph_gradients_through_the_whole_model(model_name):
    cfg = cases.MODELS[model_name]
    x, ei, texts = _small_graph("g1_demo", cfg)
    params = cfg.params()
    gout = synth.normal(31, "gout", (x.shape[0], cfg.hidden_dim))
    model = _model(cfg, params, train=True)
    out = model(torch.from_numpy(x).to(DEV), torch.from_numpy(ei).to(DEV), texts)
    (out * torch.from_numpy(gout).to(DEV)).sum().backward()
    ref_p = {k: torch.from_numpy(np.ascontiguousarray(v)).double().requires_grad_(True) for k, v in params.items()}
    ref = O.forward(ref_p, torch.from_numpy(x).double(), ei, texts, variant="factorised", dtype=torch.float64)
    (ref * torch.from_numpy(gout).double()).sum().backward()
    assert_close(out.detach().cpu().numpy(), ref.detach().float().numpy(), "training forward")
    for k, p in model.named_parameters():
        assert p.grad is not None, f"no gradient on {k}"
        gw, gg = ref_p[k].grad.numpy(), p.grad.cpu().numpy().astype(np.float64)
        scale = float(np.abs(gw).max())
        print(f"FIG model_bwd {model_name} d{k} rel_l2={_rel_l2(gg, gw):.3e}")
        assert gg.shape == gw.shape
        assert np.allclose(gg, gw, rtol=2e-4, atol=1e-4 * max(scale, 1e-30)), f"d{k}: max abs err {np.abs(gg - gw).max():.3e} at scale {scale:.3e}"
        assert _rel_l2(gg, gw) < 5e-5, f"d{k}: relative L2 {_rel_l2(gg, gw):.3e}"
