"""The plan builder (csrc/plan.hip) against its numpy restatement (_plan_ref.py), byte for byte: every table of
ghf_plan_build on the crafted inputs of _plan_cases.py — ordinary graphs, dropped edges, keys up to 2^32 - 3 and the last
round's work-item split, which depends on the card's compute-unit count — and the layer's values and gradients through blocks
that this split cuts.  Every case is built from the geometry it runs at and from the compute-unit count of the card."""

import functools

import numpy as np
import pytest
import torch

import _edge_graphs as G
import _plan_cases as P
from _plan_ref import plan_ref
from _util import assert_close
from graph_hypernetwork_forge_amd import _native, synth
from graph_hypernetwork_forge_amd.autograd import MessageLayerFn, _layer_weights, build_train_plan
from graph_hypernetwork_forge_amd.plan import build_plan

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

GEO = {g[0]: g for g in G.geometries() if g[0] != "csr20"}            # bx128, bx64, pp128, pp64 and the CSR plan (csr256)
BLOCK_GEO = [k for k, g in GEO.items() if g[2] > 1]
# the block routes of test_edge_graphs_gpu.py::ROUTES: route -> (d, GHF_KERNEL or None, geometry, has a training path)
ROUTES = {"bx128": (128, None, "bx128", True), "bx64": (64, "bx", "bx64", True), "pp128": (128, "pp", "pp128", False),
          "pp64": (64, None, "pp64", True)}
BLOCK_ROUTES = list(ROUTES)
TABLES = ("sorted_key", "sorted_src", "seg_off", "indeg", "chunk_tab", "blk_chunk_off", "item_tab", "blk_item_off", "status")
SEED = 9300


def _cus() -> int:
    return torch.cuda.get_device_properties(0).multi_processor_count


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _build(case, bn, cr, sc):
    return _native.plan_build(_t(case.edge_index), _t(case.rel), case.N, case.R, bn, cr, sc)


def _tables(pl, bn) -> dict:
    """The builder's arrays on the host, chunk_tab and item_tab cut to the entries the build defines."""
    out = {k: (None if pl[k] is None else pl[k].cpu().numpy()) for k in TABLES}
    out["sorted_key"] = out["sorted_key"].view(np.uint32)
    if bn > 1:
        chunks, items = int(out["blk_chunk_off"][-1]), int(out["status"][1])
        assert 0 <= 2 * chunks <= out["chunk_tab"].size and 0 <= 4 * items <= out["item_tab"].size, "the plan overflows its tables"
        assert not out["chunk_tab"][2 * chunks:].any() and not out["item_tab"][4 * items:].any(), "entries beyond the counted ones"
        out["chunk_tab"], out["item_tab"] = out["chunk_tab"][: 2 * chunks], out["item_tab"][: 4 * items]
    return out


def _assert_tables(case, geo, cus):
    """Builds `case` twice: the same bytes both times, and every table equal to plan_ref's.  Returns (tables, ref)."""
    _, _, bn, cr, sc, _ = geo
    ref = P.check(case, bn, cr, sc, cus)
    pl, again = _build(case, bn, cr, sc), _build(case, bn, cr, sc)
    for k in TABLES:
        assert (pl[k] is None and again[k] is None) or torch.equal(pl[k], again[k]), f"{case.name}: a second build gives another {k}"
    got = _tables(pl, bn)
    for k in ("status",) + TABLES[:-1]:                                # (the counts first: they say why a table has another length)
        if ref[k] is None:
            assert got[k] is None, f"{case.name}: {k}"
            continue
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape, f"{case.name}: {k} is {got[k].dtype}{got[k].shape}, want {ref[k].dtype}{ref[k].shape}"
        if not np.array_equal(got[k], ref[k]):
            i = int(np.nonzero(got[k] != ref[k])[0][0])
            raise AssertionError(f"{case.name}: {k} differs in {int((got[k] != ref[k]).sum())} of {ref[k].size} entries, first at {i}: "
                                 f"built {got[k][i]}, want {ref[k][i]}")
    return got, ref


@pytest.mark.parametrize("key", list(GEO))
def test_ordinary_graphs(key):
    geo = GEO[key]
    for case in P.ordinary_cases(geo[2], geo[3]):
        got, ref = _assert_tables(case, geo, _cus())
        assert got["status"][0] == 0


@pytest.mark.parametrize("key", list(GEO))
def test_dropped_edges(key):
    geo = GEO[key]
    for case in P.dropped_cases(geo[2], geo[3]):
        got, ref = _assert_tables(case, geo, _cus())
        (want,) = [e[1] for e in case.expects if e[0] == "status"]
        assert got["status"][0] == want, f"{case.name}: status word {got['status'][0]}"
        nv = ref["n_valid"]
        assert got["seg_off"][-1] == nv < case.rel.size
        assert (got["sorted_key"][nv:] == 0xFFFFFFFF).all() and not got["sorted_src"][nv:].any(), f"{case.name}: the dropped tail"
        if geo[2] > 1:
            tab = got["chunk_tab"].reshape(-1, 2)
            assert (tab[:, 0] + (tab[:, 1] & 127) <= nv).all(), f"{case.name}: a chunk reaches into the dropped edges"


@pytest.mark.parametrize("key", list(GEO))
def test_keys_up_to_the_end_of_32_bits(key):
    """Block plans: R = 2^23 - 1 on two blocks, or the largest R whose keys fit where 2 * block_nodes * (2^23 - 1) does not
    (block_nodes >= 256; keys above 2^31 occur either way: _plan_cases.check).  CSR: N * R = 2^32 - 2."""
    geo = GEO[key]
    for case in P.high_key_cases(geo[2]):
        got, ref = _assert_tables(case, geo, _cus())
        assert got["status"][0] == 0 and int(got["sorted_key"].max()) >= 1 << 31
    torch.cuda.empty_cache()


def test_refusals():
    ei, rel = torch.zeros(2, 1, dtype=torch.int64, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV)
    bn, _, cr, sc = _native.message_config(128)
    with pytest.raises(ValueError, match="does not fit 32-bit keys"):
        _native.plan_build(ei, rel, 3, 1431655765, 1)                  # N * R = 2^32 - 1 exactly
    with pytest.raises(ValueError, match=r"R < 2\^23"):
        _native.plan_build(ei, rel, bn, 1 << 23, bn, cr, sc)
    with pytest.raises(ValueError, match="run head"):
        _native.plan_build(ei, rel, (1 << 28) + 1, 1, bn, cr, sc)
    torch.cuda.empty_cache()


@pytest.mark.parametrize("key", BLOCK_GEO)
def test_last_round_split(key):
    geo, cus = GEO[key], _cus()
    _, _, bn, cr, sc, _ = geo
    for case in P.last_round_cases(bn, cr, sc, cus):
        got, ref = _assert_tables(case, geo, cus)
        per_block = np.diff(got["blk_item_off"])
        for e in case.expects:
            if e[0] == "block_items":
                assert per_block[e[1]] == e[2], f"{case.name}: block {e[1]} became {per_block[e[1]]} items, not {e[2]}"
        print(f"FIG plan_tail items {key} {case.name} cus={cus} tail0={ref['tail0']} cap={ref['tail_items']} "
              + " ".join(f"b{e[1]}:{per_block[e[1]]}" for e in case.expects if e[0] == "block_items"))


# ---- values and gradients through the split blocks of the last round -----------------------------------------------------

@functools.lru_cache(maxsize=8)
def _value_case(key, which):
    _, _, bn, cr, sc, _ = GEO[key]
    (case,) = [c for c in P.value_cases(bn, cr, sc, _cus()) if c.name == which]
    return case, P.check(case, bn, cr, sc, _cus())


@functools.lru_cache(maxsize=4)
def _rows_of_h(bn, d):
    """The rows of h for both value graphs of a route, made once (the shorter graph takes a prefix)."""
    return synth.normal(SEED, "h", ((_cus() + _cus() // 8) * bn, d))


def _inputs(case, bn, d):
    """(h, W_msg, W_self, bias, gamma, beta) at the scales of _edge_graphs.layer_inputs."""
    return (_rows_of_h(bn, d)[: case.N],) + G.layer_inputs(P.PCase("", 1, case.R, None, None, ()), d, SEED)[1:]


@pytest.fixture(scope="module", autouse=True)
def _drop_shared_inputs():
    yield
    _rows_of_h.cache_clear()
    _value_case.cache_clear()


def _rel_l2(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-30))


def _ref_rows(case, ins, rows):
    """G.layer_ref64 for the destination rows `rows`: the layer on these rows, their in-edges and the sources of those,
    renumbered (a row of the layer depends on nothing else)."""
    h, Wm, Ws, b, gamma, beta = ins
    keep = np.isin(case.edge_index[1], rows)
    nodes = np.unique(np.concatenate([rows, case.edge_index[0][keep]]))
    ei = np.searchsorted(nodes, case.edge_index[:, keep])
    agg, out = G.layer_ref64(h[nodes], ei, case.rel[keep], Wm, Ws, b, gamma, beta)
    at = np.searchsorted(nodes, rows)
    return agg[at], out[at]


def _setup(route, which, monkeypatch):
    d, env, key, _ = ROUTES[route]
    if env:
        monkeypatch.setenv("GHF_KERNEL", env)
    else:
        monkeypatch.delenv("GHF_KERNEL", raising=False)
    case, ref = _value_case(key, which)
    _, _, bn, cr, sc, _ = GEO[key]
    plan = build_plan(_t(case.edge_index), _t(case.rel), [""] * case.R, case.N, d, DEV)
    assert (plan.block_nodes, plan.chunk_rows) == (bn, cr), f"{route}: plan geometry"
    assert np.array_equal(plan.blk_chunk_off.cpu().numpy(), ref["blk_chunk_off"])
    assert np.array_equal(np.asarray(plan.item_off_host), ref["blk_item_off"]) and plan.n_slots == ref["status"][2] > 0
    assert np.array_equal(plan.item_tab.cpu().numpy()[: 4 * ref["status"][1]], ref["item_tab"])
    return case, ref, plan, d, bn


VALUES = [(r, w) for r in BLOCK_ROUTES for w in ("values_nb_c_plus_1", "values_remainder_c_over_8")]


@pytest.mark.parametrize("route,which", VALUES, ids=[f"{r}-{w}" for r, w in VALUES])
def test_values_through_split_last_round_blocks(route, which, monkeypatch):
    flag = _native.range_flag(DEV)
    flag.zero_()
    case, ref, plan, d, bn = _setup(route, which, monkeypatch)
    N, row0 = case.N, ref["tail0"] * bn
    assert 0 < row0 < N and (ref["items_per_block"][ref["tail0"]:] == 8).all()
    ins = _inputs(case, bn, d)
    rows = np.concatenate([np.arange(bn, 2 * bn), np.arange(row0, N)])          # an ordinary block and the whole last round
    ref_agg, ref_out = _ref_rows(case, ins, rows)
    h_d, Wm, Ws, b_d, g_d, bt_d = (_t(a) for a in ins)
    W, W2 = _layer_weights(plan, Wm, Ws, transpose=False)

    def launch(out, no_tail, row0=0, rows=None):
        _native.message_layer_fwd(h_d, plan, W, W2, b_d, plan.wlayout, None if no_tail else g_d, None if no_tail else bt_d,
                                  1e-5, out, row0=row0, rows=rows, flags=_native.GHF_FLAG_NO_TAIL if no_tail else 0)
    for no_tail, want in ((False, ref_out), (True, ref_agg)):
        out = torch.full_like(h_d, float("nan"))
        launch(out, no_tail)
        got = out[_t(rows)].cpu().numpy()
        print(f"FIG plan_tail fwd {route} {which} no_tail={int(no_tail)} cus={_cus()} N={N} E={case.rel.size} rows={rows.size} "
              f"rel_l2={_rel_l2(got, want):.3e} max_abs={np.nanmax(np.abs(got - want)):.3e}")
        assert_close(got, want, f"{route} {which} no_tail={no_tail}")
        assert bool(torch.isfinite(out).all()), "a full launch leaves rows unwritten"
        again = torch.full_like(h_d, float("nan"))
        launch(again, no_tail)
        assert torch.equal(out, again), "a second launch gives other bits"
        part = torch.full_like(h_d, 7.0)
        launch(part, no_tail, row0=row0, rows=N - row0)
        assert torch.equal(part[row0:], out[row0:]), "the last round's rows alone differ from the full launch"
        assert bool((part[:row0] == 7.0).all()), "rows outside the range were written"
    assert int(flag.item()) == 0, f"range guard word {int(flag.item())} on inputs of ordinary dynamic range"


def _ref_backward(case, ins, gout):
    """Float64 autograd of G.layer_ref64_torch over all N rows: the rows that touch an edge as one renumbered graph, the
    others (no in-edge, nobody's source: their row is LayerNorm(ReLU(h))) as a graph without edges.  Returns (h', leaves)."""
    th = torch.from_numpy
    leaves = [th(a).double().requires_grad_(True) for a in ins]
    N = case.N
    inv = np.unique(case.edge_index)
    rest = np.setdiff1d(np.arange(N), inv)
    ei = th(np.searchsorted(inv, case.edge_index))
    _, out_inv = G.layer_ref64_torch(leaves[0][th(inv)], ei, th(case.rel), *leaves[1:])
    none = torch.zeros(2, 0, dtype=torch.int64)
    _, out_rest = G.layer_ref64_torch(leaves[0][th(rest)], none, none[0], *leaves[1:])
    out = torch.zeros(N, leaves[0].shape[1], dtype=torch.float64).index_copy(0, th(inv), out_inv).index_copy(0, th(rest), out_rest)
    out.backward(th(gout).double())
    return out.detach().numpy(), leaves


TRAIN_ROUTES = [r for r in BLOCK_ROUTES if ROUTES[r][3]]


TRAIN = [(r, w) for r in TRAIN_ROUTES for w in ("values_nb_c_plus_1", "values_remainder_c_over_8")]


@pytest.mark.parametrize("route,which", TRAIN, ids=[f"{r}-{w}" for r, w in TRAIN])
def test_backward_through_split_last_round_blocks(route, which, monkeypatch):
    flag = _native.range_flag(DEV)
    flag.zero_()
    case, ref, plan, d, bn = _setup(route, which, monkeypatch)
    _, _, _, cr, sc, _ = GEO[ROUTES[route][2]]
    tp = build_train_plan(_t(case.edge_index), _t(case.rel), plan, d, DEV)
    rev = plan_ref(case.edge_index[::-1], case.rel, case.N, case.R, tp.rev.block_nodes, tp.rev.chunk_rows, sc, _cus())
    assert tp.rev.n_slots > 0 and tp.rev.n_slots == rev["status"][2], "the reversed plan must have a split last-round block"
    assert (tp.rev.block_nodes, tp.rev.chunk_rows) == (bn, cr) and (rev["items_per_block"][rev["tail0"]:] > 1).any()
    assert np.array_equal(np.asarray(tp.rev.item_off_host), rev["blk_item_off"])
    ins = _inputs(case, bn, d)
    gout = synth.normal(77, "gout", (case.N, d))
    want_out, leaves = _ref_backward(case, ins, gout)
    runs = []
    for _ in range(2):
        args = [_t(a).requires_grad_(True) for a in ins]
        out = MessageLayerFn.apply(*args, 1e-5, tp)
        out.backward(_t(gout))
        runs.append((out.detach(), [a.grad for a in args]))
    assert_close(runs[0][0].cpu().numpy(), want_out, f"{route} {which} training forward")
    for n, got, again, want in zip(("h", "W_msg", "W_self", "bias", "gamma", "beta"), runs[0][1], runs[1][1], leaves):
        gw, gg = want.grad.numpy(), got.cpu().numpy().astype(np.float64)
        scale = float(np.abs(gw).max())
        print(f"FIG plan_tail bwd {route} {which} d{n} rel_l2={_rel_l2(gg, gw):.3e} max_abs={np.abs(gg - gw).max():.3e} scale={scale:.3e}")
        assert np.allclose(gg, gw, rtol=2e-4, atol=2e-5 * max(scale, 1.0)), \
            f"d{n}: max abs err {np.abs(gg - gw).max():.3e} at scale {scale:.3e}"
        assert _rel_l2(gg, gw) < 2e-5, f"d{n}: relative L2 {_rel_l2(gg, gw):.3e}"
        assert torch.equal(got, again), f"d{n}: a second backward gives other bits"
    assert int(flag.item()) == 0, f"range guard word {int(flag.item())} on inputs of ordinary dynamic range"
