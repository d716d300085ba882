"""The any-width route — every hidden size but 64, 128 and the multiples of 128 — at widths above the 16, 20 and 32 the rest of
the suite runs it at: message_generic_kernel and tail_kernel (csrc/message_generic.hip) with a second to fourth live wave,
column groups c >= 1 and a single live thread in the last group; the backward's tail_bwd_kernel, ghf_group_outer,
ghf_transpose_batched and ghf_colsum at da = d; input_proj_mfma_kernel at every NT and the vector-ALU projection; the whole
model at hidden 72, 96 and 200.  test_any_width_host.py proves every (width, case) admissible and the widths' arithmetic.

Bounds are the project's own: _util.assert_close forward, test_edge_graphs_gpu.py::test_backward's per-tensor check for the
gradients.  `FIG anyw` lines put every case's margin on record."""

import functools

import numpy as np
import pytest
import torch

import _edge_graphs as G
import cases
from _util import ATOL, REL_L2, RTOL, assert_close
from graph_hypernetwork_forge_amd import HyperGNN, _native, synth
from graph_hypernetwork_forge_amd.autograd import MessageLayerFn, _layer_weights, build_train_plan
from graph_hypernetwork_forge_amd.plan import CSR_CONFIG, build_plan, empty_plan
from oracle import hypergnn_oracle as O

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NAT, SPLIT2H = _native.WLAYOUT_NATURAL, _native.WLAYOUT_SPLIT2H
NO_TAIL, RAW_SUM = _native.GHF_FLAG_NO_TAIL, _native.GHF_FLAG_RAW_SUM

CASES = {c.name: c for c in G.any_width_cases()}
FWD = [(d, n) for d in G.ANY_FWD_WIDTHS for n in CASES]
BWD = [(d, n) for d in G.ANY_BWD_WIDTHS for n in CASES]


def _t(a) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _rel_l2(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-30))


def _fig(what, got, ref):
    """One `FIG anyw` line: relative L2, largest error and the share of assert_close's bounds the comparison uses."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    err = np.abs(got - ref)
    share = max(float((err / (ATOL + RTOL * np.abs(ref))).max()), _rel_l2(got, ref) / REL_L2)
    print(f"FIG anyw {what} rel_l2={_rel_l2(got, ref):.3e} max_abs={err.max():.3e} share={share:.3f}")


@functools.lru_cache(maxsize=8)                                  # (the weights of a case at d = 1023 are about 50 MB)
def _inputs(d, name):
    return G.layer_inputs(CASES[name], d, G.seed_for(f"any{d}", name))


@functools.lru_cache(maxsize=8)
def _reference(d, name):
    """(aggregate, h') of the float64 reference, once per (width, case); read-only."""
    case, (h, *rest) = CASES[name], _inputs(d, name)
    ref = G.layer_ref64(h, case.edge_index, case.rel, *rest)
    for a in ref:
        a.flags.writeable = False
    return ref


def _plan(d, name):
    case = CASES[name]
    plan = build_plan(_t(case.edge_index), _t(case.rel), [""] * case.R, case.N, d, DEV)
    assert (plan.block_nodes, plan.wlayout, plan.chunk_rows) == (1, NAT, 0), f"d={d}: a CSR plan on natural weights"
    assert not _native.rs_supported(d), f"d={d} has a relation-stationary kernel: not the any-width route"
    return case, plan


# ---- the layer, forward -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("d,name", FWD, ids=[f"any{d}-{n}" for d, n in FWD])
def test_forward(d, name):
    flag = _native.range_flag(DEV)
    flag.zero_()
    case, plan = _plan(d, name)
    N = case.N
    res = G.realised(case, 1, 0, 0, 0)
    h, Wm, Ws, b, gamma, beta = _inputs(d, name)
    ref_agg, ref_out = _reference(d, name)
    h_d, b_d, g_d, bt_d = _t(h), _t(b), _t(gamma), _t(beta)
    W, W2 = _layer_weights(plan, _t(Wm), _t(Ws), transpose=False)
    sub = (N // 3, max(N // 4, 1)) if N >= 4 else None

    def launch(out, flags, row0=0, rows=None):
        tail = not flags & NO_TAIL
        _native.message_layer_fwd(h_d, plan, W, W2, b_d, plan.wlayout, g_d if tail else None, bt_d if tail else None, 1e-5, out,
                                  row0=row0, rows=rows, flags=flags)

    full = {}
    for flags, ref, what in ((0, ref_out, "fused"), (NO_TAIL, ref_agg, "no_tail")):
        out = torch.full_like(h_d, float("nan"))
        launch(out, flags)
        full[flags] = out
        _fig(f"fwd d={d} {name} {what} E={case.rel.size}", out.cpu().numpy(), ref)
        assert_close(out.cpu().numpy(), ref, f"d={d} {name} {what}")
        again = torch.full_like(h_d, float("nan"))
        launch(again, flags)
        assert torch.equal(out, again), f"{what}: a second launch gives other bits"
        if sub is not None:
            lo, hi = sub[0], sub[0] + sub[1]
            part = torch.full_like(h_d, 7.0)
            launch(part, flags, row0=lo, rows=hi - lo)
            assert torch.equal(part[lo:hi], out[lo:hi]), f"{what}: the row range [{lo}, {hi}) differs from the full launch"
            assert bool((part[:lo] == 7.0).all()) and bool((part[hi:] == 7.0).all()), f"{what}: rows outside the range were written"
    # GHF_FLAG_RAW_SUM (what the backward's passes run under): raw / max(indeg, 1), divided here in float64
    raw = torch.full_like(h_d, float("nan"))
    launch(raw, NO_TAIL | RAW_SUM)
    got = raw.cpu().numpy().astype(np.float64) / np.maximum(res["indeg"], 1).astype(np.float64)[:, None]
    _fig(f"fwd d={d} {name} raw_sum", got, ref_agg)
    assert_close(got, ref_agg, f"d={d} {name} raw sum / max(indeg, 1)")
    # tail_kernel on the aggregate the NO_TAIL launch left: h' again, and h' under a dropout mask
    agg_d = full[NO_TAIL]
    out = _native.tail_fwd(agg_d, h_d, g_d, bt_d, 1e-5, torch.full_like(h_d, float("nan")))
    _fig(f"fwd d={d} {name} tail_fwd", out.cpu().numpy(), ref_out)
    assert_close(out.cpu().numpy(), ref_out, f"d={d} {name} tail_fwd on the NO_TAIL output")
    mask = G.dropout_mask(N, d)
    ref_drop = G.tail_ref64(ref_agg, h, gamma, beta, mask)
    out_drop = _native.tail_fwd(agg_d, h_d, g_d, bt_d, 1e-5, torch.full_like(h_d, float("nan")), drop=_t(mask))
    _fig(f"fwd d={d} {name} tail_fwd dropout", out_drop.cpu().numpy(), ref_drop)
    assert_close(out_drop.cpu().numpy(), ref_drop, f"d={d} {name} tail_fwd with a dropout mask")
    assert torch.equal(out_drop, _native.tail_fwd(agg_d, h_d, g_d, bt_d, 1e-5, torch.full_like(h_d, float("nan")), drop=_t(mask)))
    if d == 1:          # the only centred value is exactly 0: anything but beta means the mean or the last fma is wrong
        want = bt_d.expand(N, 1)
        assert torch.equal(full[0], want) and torch.equal(out, want) and torch.equal(out_drop, want), "d = 1: h' is not beta"
    assert int(flag.item()) == 0, f"range guard word {int(flag.item())}"


@pytest.mark.parametrize("d", [256, 1024])
def test_a_plan_without_edges_runs_the_generic_kernel_at_wide_rows(d):
    """E == 0: the rs-capable widths go to message_generic_kernel too (_message and the forward test plan.E > 0); 1024 is
    GEN_MAX_D — every column group of every thread is live."""
    N, R = 5, 2
    assert _native.rs_supported(d) and G.generic_geometry(d)["last_group_threads"] == 256
    plan = empty_plan(N, [""] * R, CSR_CONFIG, DEV)
    assert (plan.E, plan.block_nodes, plan.wlayout) == (0, 1, NAT)
    h = synth.normal(7100, "h", (N, d))
    Wm, Ws = (_t(synth.normal(7100, k, (R, d, d), std=0.15)) for k in ("Wm", "Ws"))
    b = _t(synth.normal(7100, "b", (R, d), std=0.3))
    gamma = (1.0 + 0.2 * synth.normal(7100, "g", (d,))).astype(np.float32)
    beta = (0.2 * synth.normal(7100, "bt", (d,))).astype(np.float32)
    h_d = _t(h)
    out = torch.full_like(h_d, float("nan"))
    _native.message_layer_fwd(h_d, plan, Wm, Ws, b, NAT, _t(gamma), _t(beta), 1e-5, out)
    ref = G.tail_ref64(np.zeros_like(h), h, gamma, beta)
    _fig(f"fwd d={d} no_edges", out.cpu().numpy(), ref)
    assert_close(out.cpu().numpy(), ref, f"d={d}, no edges: LayerNorm(ReLU(h))")
    for flags in (NO_TAIL, NO_TAIL | RAW_SUM):
        agg = torch.full_like(h_d, float("nan"))
        _native.message_layer_fwd(h_d, plan, Wm, Ws, b, NAT, None, None, 0.0, agg, flags=flags)
        assert torch.equal(agg, torch.zeros_like(agg)), "no edges: the aggregate is not exact zeros"


# ---- the layer, backward ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("d,name", BWD, ids=[f"any{d}-{n}" for d, n in BWD])
def test_backward(d, name):
    flag = _native.range_flag(DEV)
    flag.zero_()
    case, plan = _plan(d, name)
    tp = build_train_plan(_t(case.edge_index), _t(case.rel), plan, d, DEV)
    # ghf_group_outer, ghf_transpose_batched and ghf_add3: no edge_outer slices, natural weights in both directions
    assert tp.slice_tab is None and plan.wlayout == tp.rev.wlayout == NAT and tp.rev.block_nodes == 1
    ins = _inputs(d, name)
    gout = synth.normal(77, "gout", (case.N, d))
    th = torch.from_numpy
    ref_in = [th(a).double().requires_grad_(True) for a in ins]
    _, ref = G.layer_ref64_torch(ref_in[0], th(case.edge_index), th(case.rel), *ref_in[1:])
    ref.backward(th(gout).double())
    runs = []
    for _ in range(2):
        args = [_t(a).requires_grad_(True) for a in ins]
        out = MessageLayerFn.apply(*args, 1e-5, tp)
        out.backward(_t(gout))
        runs.append((out.detach(), [a.grad for a in args]))
    _fig(f"bwd d={d} {name} training forward", runs[0][0].cpu().numpy(), ref.detach().numpy())
    assert_close(runs[0][0].cpu().numpy(), ref.detach().numpy(), f"d={d} {name} training forward")
    assert torch.equal(runs[0][0], runs[1][0]), "a second training forward gives other bits"
    for n, got, again, want in zip(("h", "W_msg", "W_self", "bias", "gamma", "beta"), runs[0][1], runs[1][1], ref_in):
        gw, gg = want.grad.numpy(), got.cpu().numpy().astype(np.float64)
        scale = float(np.abs(gw).max())
        atol = 2e-5 * max(scale, 1.0)
        share = max(float((np.abs(gg - gw) / (atol + 2e-4 * np.abs(gw))).max()), _rel_l2(gg, gw) / 2e-5)
        print(f"FIG anyw bwd d={d} {name} d{n} rel_l2={_rel_l2(gg, gw):.3e} max_abs={np.abs(gg - gw).max():.3e} scale={scale:.3e} "
              f"share={share:.3f}")
        assert gg.shape == gw.shape and np.isfinite(gg).all()
        assert np.allclose(gg, gw, rtol=2e-4, atol=atol), f"d{n}: max abs err {np.abs(gg - gw).max():.3e} at scale {scale:.3e}"
        assert _rel_l2(gg, gw) < 2e-5, f"d{n}: relative L2 {_rel_l2(gg, gw):.3e}"
        assert torch.equal(got, again), f"d{n}: a second backward gives other bits"
    assert int(flag.item()) == 0, f"range guard word {int(flag.item())}"


# ---- the fp32 input projection ------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=4)
def _ip_inputs(N, F, d):
    """(x, W, b on the device, relu(x W^T + b) in float64); shared, not modified."""
    x = synth.normal(31, "x", (N, F))
    W = synth.normal(31, "W", (d, F), std=0.2)
    b = synth.normal(31, "b", (d,), std=0.5)
    ref = np.maximum(x.astype(np.float64) @ W.astype(np.float64).T + b.astype(np.float64), 0.0)
    return _t(x), _t(W), _t(b), ref


def _aligned(*ts):
    return all(t.data_ptr() % 16 == 0 for t in ts)


IP_MFMA = [(NT, F) for NT in G.IP_NT for F in G.IP_F]


@pytest.mark.parametrize("NT,F", IP_MFMA, ids=[f"NT{NT}-F{F}" for NT, F in IP_MFMA])
def test_input_projection_at_every_nt(NT, F):
    d = 16 * NT
    flag = _native.range_flag(DEV)
    flag.zero_()
    for N in G.IP_N:                         # 77: W_in's fragments from L2, the last tile partly filled; 8200: W_in in LDS where it fits
        x, W, b, ref = _ip_inputs(N, F, d)
        out = torch.full((N, d), float("nan"), device=DEV)
        assert _aligned(x, W, b, out) and G.ip_route(N, F, d) in ("mfma", "mfma_wlds")
        h0 = _native.input_proj_fwd(x, W, b, out=out)
        _fig(f"ip NT={NT} F={F} N={N} {G.ip_route(N, F, d)}", h0.cpu().numpy(), ref)
        assert_close(h0.cpu().numpy(), ref, f"input projection N={N} F={F} d={d}")
        assert torch.equal(h0, _native.input_proj_fwd(x, W, b)), "a second launch gives other bits"
    # the fused SPLIT epilogue, N = 77 (from N = 1024 the two-piece kernel may take over)
    N = G.IP_N[0]
    x, W, b, ref = _ip_inputs(N, F, d)
    plain = _native.input_proj_fwd(x, W, b)
    hs = _native.alloc_split(N, d, SPLIT2H, DEV)
    hs.fill_(0x7e7e)
    assert _aligned(hs)
    h0 = _native.input_proj_fwd(x, W, b, out=torch.full((N, d), float("nan"), device=DEV), h_split=hs, split_layout=SPLIT2H)
    assert torch.equal(h0, plain), "h0 with h_split is not the fp32 kernel's: another path ran"
    assert torch.equal(hs, _native.split_rows(plain, SPLIT2H)), "the rows' pieces and scales are not the cutting pass's"
    assert int(flag.item()) == 0, "benign inputs raised the range guard"


@pytest.mark.parametrize("F,d", G.IP_SIMPLE, ids=[f"F{F}-d{d}" for F, d in G.IP_SIMPLE])
def test_input_projection_on_the_vector_alu(F, d):
    N = G.IP_N[0]
    x, W, b, ref = _ip_inputs(N, F, d)
    assert G.ip_route(N, F, d) == "simple"
    h0 = _native.input_proj_fwd(x, W, b, out=torch.full((N, d), float("nan"), device=DEV))
    _fig(f"ip simple F={F} d={d} N={N}", h0.cpu().numpy(), ref)
    assert_close(h0.cpu().numpy(), ref, f"input projection (vector ALU) N={N} F={F} d={d}")
    assert torch.equal(h0, _native.input_proj_fwd(x, W, b)), "a second launch gives other bits"


# ---- the whole model at fallback widths ---------------------------------------------------------------------------------

MODEL_GRAPHS = ["g1_demo", "g2_one_edge", "g2_all_unseen"]


def _cfg(hidden):
    return cases.ModelCfg(text_dim=32, node_feat_dim=16, hidden_dim=hidden, num_layers=2, seed=900 + hidden, log_scale=0.0,
                          randomize_ln=True)


def _small_graph(graph, cfg):
    (c,) = cases.graph_cases(toy_features=np.zeros((8, 1), dtype=np.float32), only=[graph])
    N = c.node_features.shape[0]
    return synth.normal(1300 + N, "x", (N, cfg.node_feat_dim)), c.edge_index, c.edge_texts


def _model(cfg, params, train=False):
    m = HyperGNN(cfg.text_dim, cfg.node_feat_dim, cfg.hidden_dim, cfg.num_layers, char_emb_dim=cfg.char_emb_dim)
    m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in params.items()})
    return m.to(DEV).train(train)


@pytest.mark.parametrize("hidden", G.MODEL_WIDTHS)
@pytest.mark.parametrize("graph", MODEL_GRAPHS)
def test_small_graphs_through_the_whole_model(graph, hidden):
    cfg = _cfg(hidden)
    x, ei, texts = _small_graph(graph, cfg)
    params = cfg.params()
    model = _model(cfg, params)
    with torch.no_grad():
        out = model(torch.from_numpy(x).to(DEV), torch.from_numpy(ei).to(DEV), texts)
    ref = O.forward(params, x, ei, texts, variant="factorised").numpy()
    _fig(f"model hidden={hidden} {graph}", out.cpu().numpy(), ref)
    assert_close(out.cpu().numpy(), ref, f"hidden {hidden} on {graph}")
    assert model.last_range_flags == 0


@pytest.mark.parametrize("hidden", G.MODEL_WIDTHS)
def test_toy_graph_gradients_through_the_whole_model(hidden):
    cfg = _cfg(hidden)
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
        print(f"FIG anyw model_bwd hidden={hidden} d{k} rel_l2={_rel_l2(gg, gw):.3e} max_abs={np.abs(gg - gw).max():.3e} scale={scale:.3e}")
        assert gg.shape == gw.shape
        assert np.allclose(gg, gw, rtol=2e-4, atol=1e-4 * max(scale, 1e-30)), f"d{k}: max abs err {np.abs(gg - gw).max():.3e} at scale {scale:.3e}"
        assert _rel_l2(gg, gw) < 5e-5, f"d{k}: relative L2 {_rel_l2(gg, gw):.3e}"
