"""Fenced buffers on the device: every entry point of include/ghf.h stays inside its documented sizes, and its result does
not depend on bytes it never wrote.

Each row of CASES is (id, entry points, why it is in the table, build_inputs, call).  A case runs three times (tests/_fence.py:
run_three): plain; with every tensor the package allocates — outputs, workspaces, plan arrays, scratch — and every input placed
between two 64 KiB bands of 0xFF; and again with 0x5A.  After each fenced run every band must still hold its fill, and the
three results must be bit-equal.  The stand-in torch module makes each workspace exactly the size its query documents; an
`empty` buffer starts as poison, so scratch that must be written before it is read shows when it is not.

Calls that write part of an output by contract (row ranges, `accumulate`, rows_unpack, ids out of range that keep what the
message held) get that output from the case, placed with known content.  Shapes are the smallest that reach a launcher branch;
the reason stands in each row's `why` (listed in test_fenced_call's docstring).

What this cannot see: a stray read whose value reaches no result, and a write further than 64 KiB from the buffer it belongs
to.  Nothing here shrinks a buffer below its documented size or makes a kernel overrun on purpose; the one planted byte
(test_the_fence_reports_a_planted_byte_on_the_device) is written by torch into the raw buffer."""

import functools
import time
from typing import Callable, NamedTuple, Optional, Tuple

import numpy as np
import pytest
import torch

import _edge_graphs as G
import _edge_outer_cases as EO
import _exclude as X
import _fence as F
import _hyper_cases as H
import _plan_cases as P
import _reduce_cases as RC
import test_relation_bits_gpu as RB
import test_score_bits_gpu as SB
from _bits import hashed
from graph_hypernetwork_forge_amd import HyperGNN, _native, autograd, plan as plan_mod, synth
from graph_hypernetwork_forge_amd.autograd import _layer_weights
from graph_hypernetwork_forge_amd.models import hypergnn as hypergnn_mod
from graph_hypernetwork_forge_amd.plan import CSR_CONFIG, build_plan, build_rs, empty_plan

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NAT, FRAG16, SPLIT2H = _native.WLAYOUT_NATURAL, _native.WLAYOUT_FRAG16, _native.WLAYOUT_SPLIT2H
PATCHED = (_native, plan_mod, autograd, hypergnn_mod)
EINVAL = -1


class Case(NamedTuple):
    id: str
    symbols: Tuple[str, ...]          # entry points of include/ghf.h the call must reach (checked against what was called)
    why: str
    build: Callable
    call: Callable
    env: Optional[str] = None         # GHF_KERNEL for the case


CASES = []


def add(id, symbols, why, build, call, env=None):
    CASES.append(Case(id, tuple(s if s.startswith("ghf_") else "ghf_" + s for s in symbols.split()), why, build, call, env))


def _t(a) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _n(seed, name, shape, std=1.0) -> torch.Tensor:
    return _t(synth.normal(seed, name, tuple(shape), std=std))


def _empty(*shape, dtype=torch.float32) -> torch.Tensor:
    """An output the case hands to a call: through the package's torch, so that it is fenced (and poisoned) in the fenced runs."""
    return _native.torch.empty(*shape, dtype=dtype, device=DEV)


def _known(shape, value, dtype=torch.float32) -> torch.Tensor:
    """An output that a call writes in part: known content everywhere (placed with the inputs)."""
    return torch.full(tuple(shape), value, dtype=dtype, device=DEV)


# =====================================================================================================================
# front end
# =====================================================================================================================

def _ip(N, F_, d, split, why):
    def build():
        return dict(x=_n(31, "x", (N, F_)), W=_n(31, "W", (d, F_), 0.2), b=_n(31, "b", (d,), 0.5))

    def call(i):
        if not split:
            return (_native.input_proj_fwd(i["x"], i["W"], i["b"]),)
        hs = _native.alloc_split(N, d, SPLIT2H, DEV)
        return _native.input_proj_fwd(i["x"], i["W"], i["b"], h_split=hs, split_layout=SPLIT2H), hs
    add(f"input_proj/N{N}-F{F_}-d{d}/{'split' if split else 'plain'}", "input_proj_fwd", why, build, call)


for _N, _F, _d, _why in ((33, 16, 16, "fp32 MFMA kernel, one column tile, rows clamped past N = 33 in a 128-row block"),
                         (1, 32, 48, "one live row, three column tiles"),
                         (97, 64, 256, "W_in from L2 (no LDS staging), the widest MFMA instance"),
                         (8193, 32, 64, "65 blocks: W_in staged in LDS, a tile loop, one live row in the last tile")):
    _ip(_N, _F, _d, False, _why)
    _ip(_N, _F, _d, True, _why + "; the rows' pieces and the scales at h_split + N 4d (N >= 1024: the two-piece kernel)")
_ip(5, 20, 20, True, "vector-ALU projection, then the separate cutting pass")
_ip(1025, 32, 64, True, "two-piece kernel NT = 4, KS = 1: nine 128-row blocks, the last with one live row")
_ip(1025, 96, 128, True, "two-piece kernel NT = 8, KS = 3")


def _split_rows(N, d, sub):
    def build():
        i = dict(h=_n(32, f"h{N}.{d}", (N, d)))
        if sub:
            i["out"] = _known((N * (2 * d + 2),), 0x1111, torch.int16)
        return i

    def call(i):
        if sub:
            return (_native.split_rows(i["h"], SPLIT2H, out=i["out"], row0=3, rows=N - 5),)
        return (_native.split_rows(i["h"], SPLIT2H),)
    add(f"split_rows/N{N}-d{d}/{'rows3..N-2' if sub else 'full'}", "split_rows",
        "the cutting pass; scales behind the pieces" + ("; rows outside [3, N - 2) keep the caller's content" if sub else ""), build, call)


for _N in (5, 130):
    for _d in (64, 128, 256):
        _split_rows(_N, _d, False)
        _split_rows(_N, _d, True)


def _text(name, why):
    case = {c.name: c for c in H.TEXT_SHAPES}[name]

    def build():
        inp = H.text_inputs(case)
        return tuple(_t(a) for a in (inp.ids, inp.lens, inp.E, inp.W, inp.b, inp.dte))

    def call(i):
        ids, lens, E, W, b, dte = i
        te = _native.text_encode_fwd(ids, lens, E, W, b)
        return (te,) + tuple(_native.text_encode_bwd(ids, lens, E, W, te, dte))
    add(f"text_encode/{name}", "text_encode_fwd text_encode_bwd", why, build, call)


_text("empties", "every string empty (length 0 is read as one character)")
_text("long300", "the longest length: 300 characters, and a string of one")
_text("raw_lens", "lengths 0, -1 and Lmax + 4: clamped, not followed past the id matrix")
_text("raw_ids", "character ids below 0 and above V: clamped into the embedding table")
_text("c257", "a character embedding one wider than 256: the second column pass; backward scratch 2 U C + U T")
_text("u300", "300 strings: more than one workgroup's worth")

WG_T, WG_HH, WG_NH, WG_D = 64, 128, 2, 64


@functools.lru_cache(maxsize=None)
def _wg_case(R):
    return H._wg(f"fence_r{R}", (WG_T, WG_HH, WG_NH, WG_D, WG_D, R), 5300 + R)


def _wg_build(R, masks=False, L=1):
    def build():
        case = _wg_case(R)
        inp = H.wg_inputs(case)
        i = dict(x=_t(inp.x), g=[_t(inp.g[k]).view(R, -1) for k in H.HEADS], flats=[], lss=[])
        for g in range(L):
            _, flat, ls = H.wg_params(WG_T, WG_HH, WG_NH, WG_D, WG_D, case.seed + 7 * g)
            i["flats"].append([_t(p) for p in flat])
            i["lss"].append(_t(ls))
        if masks:
            m, log_keep = H.wg_masks(case, H.DROPOUT_P)
            i["masks"], i["log_keep"] = _t(m), torch.full((1,), log_keep, dtype=torch.float32, device=DEV)
        return i
    return build


def _wg_fwd(R, layout, acts, masks):
    def call(i):
        return _native.weightgen_fwd(i["x"], i["flats"][0], i["lss"][0], WG_T, WG_HH, WG_NH, WG_D, WG_D, layout,
                                     hidden_drop=i.get("masks"), want_acts=acts)
    tag = f"R{R}-{'split2h' if layout == SPLIT2H else 'natural'}{'-acts' if acts else ''}{'-drop' if masks else ''}"
    add(f"weightgen_fwd/{tag}", "weightgen_fwd", "hidden_ws = 3 2 R max(Hh, T) floats; merged output kernel"
        + (", packed with the scales behind" if layout == SPLIT2H else "") + (", activations saved" if acts else ""),
        _wg_build(R, masks), call)


for _R in (1, 33):
    for _layout in (NAT, SPLIT2H):
        _wg_fwd(_R, _layout, False, False)
        _wg_fwd(_R, _layout, True, True)
_wg_fwd(33, NAT, True, False)


def _wg_batched(R, layout):
    def call(i):
        outs = _native.weightgen_fwd_batched(i["x"], i["flats"], [[ls[k:k + 1] for k in range(3)] for ls in i["lss"]],
                                             WG_T, WG_HH, WG_NH, WG_D, WG_D, layout)
        return [t for o in outs for t in o]
    add(f"weightgen_fwd_batched/L3-R{R}-{'split2h' if layout == SPLIT2H else 'natural'}", "weightgen_fwd_batched",
        "three generators in one launch sequence: hidden_ws of L 3 2 R max(Hh, T) floats, four relations per workgroup",
        _wg_build(R, L=3), call)


for _R in (1, 33):
    for _layout in (NAT, SPLIT2H):
        _wg_batched(_R, _layout)


def _wg_bwd(R, masks, want_dx):
    def call(i):
        flat, ls = i["flats"][0], i["lss"][0]
        acts = _native.weightgen_acts(i["x"], flat, WG_T, WG_HH, WG_NH, hidden_drop=i.get("masks"))
        Wm, Ws, b = _native.weightgen_fwd(i["x"], flat, ls, WG_T, WG_HH, WG_NH, WG_D, WG_D, NAT, hidden_drop=i.get("masks"))
        dp, dls, dx = _native.weightgen_bwd(i["x"], flat, acts, [Wm.view(R, -1), Ws.view(R, -1), b], i["g"], ls, WG_T, WG_HH,
                                            WG_NH, WG_D, WG_D, log_keep=i.get("log_keep"), want_dx=want_dx)
        return [acts, dls, dx] + list(dp)
    add(f"weightgen_bwd/R{R}{'-drop' if masks else ''}{'' if want_dx else '-no_dx'}", "weightgen_acts weightgen_bwd weightgen_fwd",
        "the fused backward's scratch (ghf_weightgen_bwd_workspace_floats) and split partial sums", _wg_build(R, masks), call)


_wg_bwd(1, False, True)
_wg_bwd(33, False, True)
_wg_bwd(33, True, True)
_wg_bwd(33, False, False)


def _pack(layout, d, top, bottom, transpose):
    def build():
        Wm, Ws = H.pack_inputs(d)
        return dict(top=_t(Wm) if top else None, bottom=_t(Ws) if bottom else None)

    def call(i):
        return (_native.weights_pack(i["top"], i["bottom"], transpose, H.PACK_R, d, layout),)
    add(f"weights_pack/{'frag16' if layout == FRAG16 else 'split2h'}-d{d}-{int(top)}{int(bottom)}{'-T' if transpose else ''}",
        "weights_pack", "the packed layout's bytes (ghf_weights_bytes); a missing half is zeros", build, call)


for _layout, _d in H.PACK_SHAPES:
    _pack(_layout, _d, True, True, False)
_pack(SPLIT2H, 32, False, True, True)
_pack(FRAG16, 16, True, False, True)


def _pack_rs(R, d):
    def build():
        return dict(Wm=_n(33, f"rsm{d}", (R, d, d)), Ws=_n(33, f"rss{d}", (R, d, d)))

    def call(i):
        lib = _native.load()
        w2h = _empty(lib.ghf_weights_rs_bytes(R, d), dtype=torch.uint8)
        shift = _empty(R, dtype=torch.int32)
        _native._check(lib.ghf_weights_pack_rs(i["Wm"].data_ptr(), i["Ws"].data_ptr(), R, d, w2h.data_ptr(), shift.data_ptr(),
                                               _native._stream()), "ghf_weights_pack_rs")
        return w2h, shift
    add(f"weights_pack_rs/R{R}-d{d}", "weights_pack_rs", "ghf_weights_rs_bytes: the pieces of R relations, then R scales", build, call)


_pack_rs(3, 128)
_pack_rs(1, 384)


def _transpose(B, r, c):
    add(f"transpose_batched/{B}x{r}x{c}", "transpose_batched", "tiles past the matrix's edge in both directions",
        lambda: (_n(34, f"tr{r}.{c}", (B, r, c)),), lambda i: (_native.transpose_batched(i[0]),))


_transpose(3, 33, 65)
_transpose(1, 1, 1)
_transpose(2, 128, 20)


# =====================================================================================================================
# plans and subgraphs
# =====================================================================================================================

def _plan_geometry(kind):
    return _native.message_config(128) if kind == "block" else CSR_CONFIG


def _plan_build(kind, which):
    def build():
        bn, _, cr, sc = _plan_geometry(kind)
        if which == "last_round":
            cus = torch.cuda.get_device_properties(0).multi_processor_count
            case = P.last_round_cases(bn, cr, sc, cus)[0]
        else:
            case = {c.name: c for c in P.ordinary_cases(bn, cr)}[which]
        return dict(ei=_t(case.edge_index), rel=_t(case.rel), N=case.N, R=case.R)

    def call(i):
        bn, _, cr, sc = _plan_geometry(kind)
        return _native.plan_build(i["ei"], i["rel"], i["N"], i["R"], bn, cr, sc)
    add(f"plan_build/{kind}/{which}", "plan_build", "ghf_plan_workspace_bytes, _max_chunks, _max_items: a scan and a radix sort in one "
        "temp region" + ("; the last-round item split" if which == "last_round" else ""), build, call)


for _kind in ("block", "csr"):
    _plan_build(_kind, "powerlaw_repeated_pairs")
    _plan_build(_kind, "fewer_edges_than_groups")
_plan_build("block", "groups_around_chunk_rows")
_plan_build("block", "last_round")


def _group_edges(name):
    (keys, R), = [(k, r) for n, k, r in RC.group_edges_cases() if n == name]
    add(f"group_edges/{name.replace(' ', '_')}", "group_edges", "ghf_group_workspace_bytes: a stable counting sort",
        lambda: (_t(keys),), lambda i: _native.group_edges(i[0], R))


for _name in ("E=1 R=1", "R+1 > E", "E=300 R=257", "relations 0, 3, 6 absent", "E=70000 R=5"):
    _group_edges(_name)

SUB_N, SUB_LIVE, SUB_E, SUB_R = 340, 300, 2500, 5          # 40 isolated trailing nodes


@functools.lru_cache(maxsize=None)
def _sub_graph():
    ei, rel = synth.make_graph_arrays(SUB_LIVE, SUB_E, SUB_R, seed=9400, kind="powerlaw")
    ex = np.arange(0, SUB_E, 7)                                 # every seventh edge is excluded, and one pair that is no edge
    ex_src, ex_dst, ex_rel = np.append(ei[0][ex], SUB_N - 1), np.append(ei[1][ex], 0), np.append(rel[ex], 1)
    return ei, rel, X.keys(ex_src, ex_dst).view(np.int64), X.keys(ex_src, ex_dst, ex_rel, SUB_R).view(np.int64)


def _sub_build(kind, excl, E0=False):
    def build():
        ei, rel, untyped, typed = _sub_graph()
        d = 128 if kind == "block" else 20
        if E0:
            cfg = plan_mod.plan_config(d, 0, SUB_N) if kind == "block" else CSR_CONFIG
            pl = empty_plan(SUB_N, synth.relation_names(SUB_R), cfg, DEV)
        else:
            pl = build_plan(_t(ei), _t(rel), synth.relation_names(SUB_R), SUB_N, d, DEV, force_generic=(kind == "csr"))
        assert (pl.block_nodes > 1) == (kind == "block")
        keys = None if excl is None else (_t(typed if excl == "typed" else untyped), excl == "typed")
        return dict(plan=pl, seeds=_t(np.array([3, 0, 17, SUB_N - 2], dtype=np.int64)), keys=keys)
    return build


def _subgraph(kind, k, excl, E0=False):
    syms = "subgraph_hops subgraph_nodes subgraph_edges" if excl is None else "subgraph_hops_excl subgraph_nodes subgraph_edges_excl"
    add(f"subgraph/{kind}/k{k}/{excl or 'all'}{'/E0' if E0 else ''}", syms,
        "f[N] and pos[E] keep one extra entry; the workspace head is shared between the stages; outputs [2, max(E, 1)]",
        _sub_build(kind, excl, E0), lambda i: _native.subgraph(i["plan"], i["seeds"], k, exclude=i["keys"]))


def _subgraph_sample(kind, excl, E0=False):
    syms = "subgraph_sample_hops" + ("" if excl is None else "_excl") + " subgraph_nodes subgraph_sample_edges"
    add(f"subgraph_sample/{kind}/2.-1.1/{excl or 'all'}{'/E0' if E0 else ''}", syms,
        "fanout caps 2, none, 1: the selection's keep [max(E, 1)] and priorities in the shared workspace",
        _sub_build(kind, excl, E0), lambda i: _native.subgraph_sample(i["plan"], i["seeds"], [2, -1, 1], 77, exclude=i["keys"]))


for _kind in ("block", "csr"):
    for _excl in (None, "typed", "untyped"):
        for _k in (1, 2, 3):
            _subgraph(_kind, _k, _excl)
        _subgraph_sample(_kind, _excl)
    _subgraph(_kind, 2, None, E0=True)
    _subgraph_sample(_kind, None, E0=True)


# =====================================================================================================================
# layers
# =====================================================================================================================

# route -> (d, GHF_KERNEL, geometry of _edge_graphs.geometries() or None for a CSR plan at an odd width, kind)
ROUTES = {"bx128": (128, None, "bx128", "block"), "bx64": (64, "bx", "bx64", "block"), "pp128": (128, "pp", "pp128", "block"),
          "pp64": (64, None, "pp64", "block"), "generic20": (20, None, "csr20", "generic"), "generic65": (65, None, None, "generic")}


@functools.lru_cache(maxsize=4)
def _layer_np(route, name):
    d, _, key, kind = ROUTES[route]
    if key is None:
        case = {c.name: c for c in G.any_width_cases()}[name]
        return case, G.layer_inputs(case, d, G.seed_for(f"any{d}", name))
    geo = {g[0]: g for g in G.geometries()}[key]
    case = {c.name: c for c in G.edge_cases(*geo[2:], geo[1])}[name]
    return case, G.layer_inputs(case, d, G.seed_for(key, name))


def _layer(route, name, why):
    d, env, key, kind = ROUTES[route]

    def build():
        case, (h, Wm, Ws, b, gamma, beta) = _layer_np(route, name)
        pl = build_plan(_t(case.edge_index), _t(case.rel), [""] * case.R, case.N, d, DEV)
        assert (pl.block_nodes > 1) == (kind == "block")
        W, W2 = _layer_weights(pl, _t(Wm), _t(Ws), transpose=False)
        N, bn = case.N, max(pl.block_nodes, 2)
        lo = min(bn, N - 1) if kind == "block" else N // 3
        hi = min(2 * bn, N) if kind == "block" else max(N // 3 + N // 4, lo + 1)
        return dict(plan=pl, h=_t(h), W=W, W2=W2, b=_t(b), gamma=_t(gamma), beta=_t(beta), part=_known((N, d), 7.0), lo=lo, hi=min(hi, N),
                    part_split=_known((N * (2 * d + 2),), 0x1111, torch.int16) if pl.wlayout == SPLIT2H else None)

    def call(i):
        pl, h = i["plan"], i["h"]
        N = h.size(0)
        split = pl.wlayout == SPLIT2H
        out, agg_only = _empty(N, d), _empty(N, d)
        hs_out = _native.alloc_split(N, d, SPLIT2H, DEV) if split else None
        agg = _empty(N, d) if _native.side_output_supported(pl, d) else None
        args = (h, pl, i["W"], i["W2"], i["b"], pl.wlayout)
        _native.message_layer_fwd(*args, i["gamma"], i["beta"], 1e-5, out, h_split_out=hs_out, agg_out=agg)
        _native.message_layer_fwd(*args, None, None, 1e-5, agg_only, flags=_native.GHF_FLAG_NO_TAIL)
        _native.message_layer_fwd(*args, i["gamma"], i["beta"], 1e-5, i["part"], row0=i["lo"], rows=i["hi"] - i["lo"],
                                  h_split_out=i["part_split"])
        return out, agg_only, hs_out, agg, i["part"], i["part_split"]
    add(f"message_layer/{route}/{name}", "message_layer_fwd" + (" weights_pack split_rows" if route.startswith("bx") else
                                                                 " weights_pack" if kind == "block" else ""),
        why + "; with h_split_out / agg_out where the kernel has them, without tail, and on a row sub-range", build, call, env)


for _route in ("bx128", "bx64", "pp128", "pp64"):
    _layer(_route, "split_sc_plus_1_chunks", "a hub block split over work items: `partial` = n_slots BN d floats in use")
    _layer(_route, "size_only_last_node_has_in_edges", "N = 2 BN + 1: a last block of one row")
    _layer(_route, "relations_r64_one_edge_each", "64 relations, one edge each: chunks of one row")
for _route in ("generic20", "generic65"):
    _layer(_route, "csr_in_degrees", "the any-width kernel: in-degrees 0 .. many")
    _layer(_route, "csr_n1_self_loop", "N = 1")


@functools.lru_cache(maxsize=2)
def _rs_np(d, name):
    case = {c.name: c for c in G.edge_cases(1, 0, 0, 0, d)}[name]
    return case, G.layer_inputs(case, d, G.seed_for(f"csr{d}", name))


def _rs(d, name, runs, exact, why):
    def build():
        case, (h, Wm, Ws, b, gamma, beta) = _rs_np(d, name)
        pl = build_plan(_t(case.edge_index), _t(case.rel), [""] * case.R, case.N, d, DEV, force_generic=True)
        rs = build_rs(pl, runs=runs)
        N = case.N
        return dict(rs=rs, h=_t(h), Wm=_t(Wm), Ws=_t(Ws), b=_t(b), gamma=_t(gamma), beta=_t(beta), part=_known((N, d), 7.0),
                    part_split=_known((N * (2 * d + 2),), 0x1111, torch.int16))

    def call(i):
        rs, h = i["rs"], i["h"]
        N = h.size(0)
        assert (rs.run_start is not None) == bool(runs)
        Y = _empty(max(rs.rows, 1), d)
        out, raw, hs_out = _empty(N, d), _empty(N, d), _native.alloc_split(N, d, SPLIT2H, DEV)
        _native.edge_transform_fwd(h, rs, i["Wm"], i["Ws"], i["b"], Y, exact=exact)
        _native.segment_tail_fwd(Y, rs, h, i["gamma"], i["beta"], 1e-5, out, h_split_out=hs_out, exact=exact)
        _native.segment_tail_fwd(Y, rs, None, None, None, 0.0, raw, flags=_native.GHF_FLAG_NO_TAIL | _native.GHF_FLAG_RAW_SUM, exact=exact)
        lo, n = N // 3, max(N // 4, 1)
        _native.segment_tail_fwd(Y, rs, h, i["gamma"], i["beta"], 1e-5, i["part"], row0=lo, rows=n, h_split_out=i["part_split"], exact=exact)
        return out, raw, hs_out, i["part"], i["part_split"]
    syms = "edge_transform_fwd transpose_batched segment_tail_fwd" if exact else \
        "edge_transform_h_fwd weights_pack_rs split_rows segment_tail_fwd" + (" run_rows_fwd" if runs else "")
    if name == "csr_hubs_around_hub_rows":
        syms += " segment_partial_fwd"
    add(f"message_rs/d{d}/{name}/{'runs' if runs else 'edges'}{'-exact' if exact else ''}", syms, why, build, call)


for _d in (128, 1024):
    _rs(_d, "csr_hubs_around_hub_rows", False, False, "destinations above RS_HUB_ROWS rows: chunk sums (ghf_segment_partial_fwd) in the hub scratch")
    _rs(_d, "csr_runs_around_run_max", True, False, "rows that stand for runs of edges: ghf_run_rows_fwd into the run scratch (ghf_split_rows_bytes)")
    _rs(_d, "csr_relation_sizes_around_the_tile", False, False, "relation sizes around the 128-row tile")
_rs(128, "csr_hubs_around_hub_rows", False, True, "the fp32-MFMA pass 1 (transposed weights) on the hub graph")
_rs(256, "csr_runs_around_run_max", True, True, "the exact kernels on a run plan: the per-edge twin and its own scratch")
_rs(256, "csr_in_degrees", False, False, "d % 256 == 0: the LDS-DMA ring kernel")


def _tail(N, d, drop, sub):
    def build():
        i = dict(agg=_n(35, f"agg{N}.{d}", (N, d)), h=_n(35, f"h{N}.{d}", (N, d)), gamma=_n(35, f"g{d}", (d,)), beta=_n(35, f"b{d}", (d,)),
                 drop=_t(G.dropout_mask(N, d)) if drop else None)
        if sub:
            i["out"] = _known((N, d), 7.0)
        return i

    def call(i):
        if sub:
            return (_native.tail_fwd(i["agg"], i["h"], i["gamma"], i["beta"], 1e-5, i["out"], row0=1, rows=N - 3, drop=i["drop"]),)
        return (_native.tail_fwd(i["agg"], i["h"], i["gamma"], i["beta"], 1e-5, _empty(N, d), drop=i["drop"]),)
    add(f"tail_fwd/N{N}-d{d}{'-drop' if drop else ''}{'-rows1..N-2' if sub else ''}", "tail_fwd",
        "one row per workgroup, columns in groups of 256 threads" + ("; rows outside the range keep the caller's content" if sub else ""), build, call)


for _N, _d in ((5, 20), (130, 64), (5, 257), (130, 1023)):
    _tail(_N, _d, False, False)
    _tail(_N, _d, True, True)


def _tail_bwd(N, d, split, drop):
    def build():
        return dict(g=_n(36, f"g{N}.{d}", (N, d)), agg=_n(36, f"agg{N}.{d}", (N, d)), h=_n(36, f"h{N}.{d}", (N, d)),
                    gamma=_n(36, f"gm{d}", (d,)), indeg=_t((np.arange(N) % 5).astype(np.int32)),
                    drop=_t(G.dropout_mask(N, d)) if drop else None)

    def call(i):
        return _native.tail_bwd(i["g"], i["agg"], i["h"], i["gamma"], 1e-5, i["indeg"], drop=i["drop"], split_layout=SPLIT2H if split else None)
    add(f"tail_bwd/N{N}-d{d}{'-split' if split else ''}{'-drop' if drop else ''}", "tail_bwd",
        "ghf_tail_bwd_workspace_floats: per-block partial sums of dgamma / dbeta" + ("; G cut into pieces as well" if split else ""), build, call)


for _N in (5, 130):
    for _d in (20, 64, 128, 256):
        _tail_bwd(_N, _d, False, False)
        _tail_bwd(_N, _d, True, True)


def _colsum(N, d, masked, acc):
    def build():
        inp = RC.colsum_inputs(N, d, "normal")
        return dict(X=_t(inp["X"]), mask=_t(inp["mask"]) if masked else None, out=_t(inp["prior"]) if acc else None)
    add(f"colsum/N{N}-d{d}{'-mask' if masked else ''}{'-acc' if acc else ''}", "colsum",
        "ghf_colsum_workspace_floats: the tree's levels" + ("; accumulates onto the caller's out" if acc else ""),
        build, lambda i: (_native.colsum(i["X"], mask=i["mask"], out=i["out"]),))


for _N, _d in ((1, 3), (513, 4), (513, 1021), (511, 1028)):
    _colsum(_N, _d, True, False)
    _colsum(_N, _d, True, True)
_colsum(262145, 4, False, False)

for _n_ in (1, 4099, 300001):
    add(f"relu_mask/n{_n_}", "relu_mask", "grid-strided elementwise kernel",
        lambda n=_n_: (_n(37, f"rx{n}", (n,)), _n(37, f"rr{n}", (n,))), lambda i: (_native.relu_mask(i[0], i[1]),))
    add(f"scale_exp/n{_n_}", "scale_exp", "grid-strided elementwise kernel",
        lambda n=_n_: (_n(37, f"sx{n}", (n,)), _t(np.array([-0.5], dtype=np.float32))), lambda i: (_native.scale_exp(i[0], i[1]),))
    add(f"add3/n{_n_}", "add3", "grid-strided elementwise kernel, with and without the third operand",
        lambda n=_n_: (_n(37, f"a{n}", (n,)), _n(37, f"b{n}", (n,)), _n(37, f"c{n}", (n,))),
        lambda i: (_native.add3(i[0], i[1], i[2]), _native.add3(i[0], i[1])))
for _n_, _d in ((1, 1), (5, 20), (131, 257), (3000, 128)):
    add(f"rowscale/n{_n_}-d{_d}", "rowscale", "grid-strided elementwise kernel, one factor per row",
        lambda n=_n_, d=_d: (_n(37, f"rs{n}.{d}", (n, d)), _n(37, f"rg{n}", (n,))), lambda i: (_native.rowscale(i[0], i[1]),))


def _group_outer(da, db, mode, acc):
    def build():
        inp = RC.outer_inputs(da, db, mode, "normal")
        i = {k: (None if v is None else _t(v)) for k, v in inp.items()}
        i["goff"] = _t(RC.GOFF)
        i["out"] = _t(RC.outer_prior(da, db, "normal")) if acc else None
        return i
    add(f"group_outer/{da}x{db}-{mode}{'-acc' if acc else ''}", "group_outer",
        "partial row and column tiles; empty groups" + ("; accumulates onto the caller's out" if acc else ""),
        build, lambda i: (_native.group_outer(i["A"], i["ia"], i["B"], i["ib"], i["goff"], i["out"]),))


for _da, _db in ((0, 130), (17, 129), (20, 20), (16, 272)):
    _group_outer(_da, _db, "gather" if _da else "identity", False)
    _group_outer(_da, _db, "identity", True)


def _edge_outer(d, exact, scaled):
    def build():
        g = EO.graph("short")
        h, Gm = EO.inputs("normal", d, "short")
        i = dict(h=_t(h), G=_t(Gm), tabs=tuple(_t(g[k]) for k in ("src", "dst", "slice_tab", "slice_off")), R=g["R"])
        if scaled:
            i["hs"] = _native.split_row_scales(_native.split_rows(i["h"], SPLIT2H), EO.N, d).clone()
            i["gs"] = _native.split_row_scales(_native.split_rows(i["G"], SPLIT2H), EO.N, d).clone()
        return i

    def call(i):
        ns, D = i["tabs"][2].size(0), min(d, 128)
        ws = _empty(ns * (2 * D * D + D) + 64)
        dW, db = _native.edge_outer(i["h"], i["G"], *i["tabs"], i["R"], exact=exact, h_scales=i.get("hs"), G_scales=i.get("gs"), workspace=ws)
        return dW, db
    add(f"edge_outer/d{d}{'-exact' if exact else ''}{'-scaled' if scaled else ''}", "edge_outer_scaled" if scaled else "edge_outer",
        "the documented scratch nslices (2 D D + D) + 64 floats, exactly; slices of 1 .. 129 edges, an empty relation", build, call)


for _d in (64, 128, 384):
    _edge_outer(_d, True, False)
    _edge_outer(_d, False, False)
_edge_outer(128, False, True)
_edge_outer(384, False, True)


def _segment_axpy(d, nseg, clamp):
    def build():
        return {k: _t(v) for k, v in RC.seg_inputs(d, RC.seg_lengths(nseg), "normal", clamp=clamp).items()}
    add(f"segment_axpy/d{d}-nseg{nseg}{'-clamp' if clamp else ''}", "segment_axpy",
        "vector widths 1, 2, 4 with a second column pass; empty segments" + ("; row ids outside [0, nx) are clamped" if clamp else ""),
        build, lambda i: (_native.segment_axpy(i["w"], i["iw"], i["X"], i["ix"], i["off"]),))


for _d, _nseg, _clamp in ((7, 9, True), (130, 9, False), (260, 5, True), (1028, 4, False), (7, 4097, False)):
    _segment_axpy(_d, _nseg, _clamp)

for _n_ in (1, 8192, 8193):
    add(f"dot/n{_n_}", "dot", "the scratch of (n + 8191) / 8192 partial sums, exactly",
        lambda n=_n_: tuple(_t(a) for a in RC.dot_inputs(n, "normal")), lambda i: (_native.dot(i[0], i[1]),))
for _K, _M, _Nn in ((513, 17, 129), (2049, 3, 5)):
    add(f"matmul_tn/K{_K}-{_M}x{_Nn}", "group_outer colsum", "K above one slice: partial products, then their ordered sum",
        lambda K=_K, M=_M, N=_Nn: tuple(_t(a) for a in RC.matmul_inputs(K, M, N, "normal")), lambda i: (_native.matmul_tn(i[0], i[1]),))


# =====================================================================================================================
# scoring
# =====================================================================================================================

def _score_build(N, d, kind, mode, B=SB.B0, rows_q=SB.ROWS_Q):
    def build():
        q, c, target, iq, kw = SB.inputs(N, d, kind, B, rows_q)
        ic = np.arange(1, N, 3, dtype=np.int64) if mode in ("cand", "both") else None
        bias = hashed(N, 1, 21).reshape(N) if mode in ("bias", "both") else None
        return dict(q=q, c=c, target=target, iq=iq, ptr=kw.get("ptr"), idx=kw.get("idx"), ic=None if ic is None else _t(ic),
                    bias=None if bias is None else _t(bias), grad=SB.grad(B))
    return build


def _lists(i):
    return dict(iq=i["iq"], filt_ptr=i["ptr"], filt_idx=i["idx"], ic=i["ic"], bias=i["bias"])


def _pos(i):
    return dict(iq=i["iq"], pos_ptr=i["ptr"], pos_idx=i["idx"], ic=i["ic"], bias=i["bias"])


SUFFIX = {"all": "", "cand": "_sub", "bias": "_b", "both": "_b"}


def _score(op, N, d, kind, mode, **shape):
    sfx, scale = SUFFIX[mode], SB.scale_of(d)
    if op == "rank":
        syms, call = f"score_rank{sfx}", lambda i: _native.score_rank(i["q"], i["c"], i["target"], **_lists(i))
    elif op == "topk":
        syms, call = f"score_topk{sfx}", lambda i: _native.score_topk(i["q"], i["c"], 10, **{k: v for k, v in _lists(i).items()})
    elif op == "softmax":
        syms = f"score_softmax_fwd{sfx} score_softmax_bwd{sfx}"

        def call(i):
            loss, lse = _native.score_softmax_fwd(i["q"], i["c"], i["target"], scale=scale, **_lists(i))
            return (loss, lse) + tuple(_native.score_softmax_bwd(i["q"], i["c"], i["target"], lse, i["grad"], scale=scale, **_lists(i)))
    elif op == "bce":
        syms = f"score_bce_fwd{sfx} score_bce_bwd{sfx}"

        def call(i):
            loss = _native.score_bce_fwd(i["q"], i["c"], scale=scale, smoothing=0.1, **_pos(i))
            return (loss,) + tuple(_native.score_bce_bwd(i["q"], i["c"], loss, i["grad"], scale=scale, smoothing=0.1, **_pos(i)))
    else:
        syms = "score_negsamp_fwd score_negsamp_bwd"

        def call(i):
            kw = dict(scale=scale, margin=0.5, adversarial_temperature=1.0, **_lists(i))
            loss, lw = _native.score_negsamp_fwd(i["q"], i["c"], i["target"], **kw)
            return (loss, lw) + tuple(_native.score_negsamp_bwd(i["q"], i["c"], i["target"], lw, i["grad"], **kw))
    tag = "".join(f"_{k}{v}" for k, v in shape.items())
    add(f"score_{op}/N{N}{tag}-d{d}/{kind}/{mode}", syms,
        "slabs sized from B, N, C, k, nnz in the workspace query; " + {"all": "every node", "cand": "a candidate subset (every third node)",
                                                                        "bias": "a per-candidate bias", "both": "candidates and bias"}[mode],
        _score_build(N, d, kind, mode, **shape), call)


for _op in ("rank", "topk", "softmax", "bce", "negsamp"):
    for _mode in ("all", "cand", "bias", "both"):
        _score(_op, SB.N0, 20, "lists", _mode)                  # vectorised loads, a padded tail of k; some filter lists empty
    for _d in (18, 128):
        _score(_op, SB.N0, _d, "lists", "all")                  # 18: scalar loads; 128: the full 256-candidate tile
        _score(_op, SB.N0, _d, "plain", "both")                 # no lists at all
    if _op in ("softmax", "bce", "negsamp"):
        for _mode in ("all", "both"):
            _score(_op, SB.N0, 64, "hub4", _mode, B=SB.HUB_B, rows_q=SB.HUB_ROWS_Q)      # > SB_HCAP pairs in one owner tile
_score("topk", 5, 20, "plain", "all")                           # fewer candidates than k: the (-inf, -1) fill
_score("rank", SB.N0, 20, "bad_list", "all")                    # an id out of range: (-1, -1) for that query


def _score_pairs(d, indexed):
    def build():
        a, b = _n(38, f"pa{d}", (97, d)), _n(38, f"pb{d}", (97, d))
        ia = _t(synth.randint(38, "ia", 301, 97)) if indexed else None
        ib = _t(synth.randint(38, "ib", 301, 97)) if indexed else None
        return a, b, ia, ib
    add(f"score_pairs/d{d}{'-idx' if indexed else ''}", "score_pairs_fwd", "d % 4 != 0: scalar loads; 20: vectorised",
        build, lambda i: (_native.score_pairs_fwd(i[0], i[1], i[2], i[3]),))


for _d in (18, 20):
    _score_pairs(_d, False)
    _score_pairs(_d, True)


def _relation(d, transpose, bad=False):
    B, R = 150, 4

    def build():
        rel_sorted = np.repeat(np.arange(R, dtype=np.int64), (70, 5, 0, 75))
        rel = np.empty(B, dtype=np.int64)
        rel[(37 * np.arange(B)) % B] = rel_sorted
        ix = (np.arange(B, dtype=np.int64) * 7 + 3) % RB.ROWS_X
        if bad:
            ix[111] = RB.ROWS_X
        W, b = RB.weights(R, d)
        return dict(x=RB.rows(d), rel=_t(rel), ix=_t(ix), W=W, b=b, ia=RB.affine(B, 7, 3, RB.ROWS_X), ib=RB.affine(B, 11, 5, RB.ROWS_X),
                    G=RB.grads(B, R))

    def call(i):
        rows = _native.relation_rows(i["x"], i["rel"], i["W"], i["b"], ix=i["ix"], transpose=transpose)
        scores = _native.relation_scores(i["x"], i["ia"], i["ib"], i["W"], i["b"], transpose=transpose)
        drows = _native.relation_scores_bwd_rows(i["x"], i["ia"], i["G"], i["W"], i["b"], transpose=transpose)
        dW, db = _native.relation_scores_bwd_weights(i["x"], i["ia"], i["ib"], i["G"])
        return rows, scores, drows, dW, db
    add(f"relation/d{d}-{'T' if transpose else 'N'}{'-bad_id' if bad else ''}",
        "relation_rows group_edges relation_scores relation_scores_bwd_rows relation_scores_bwd_weights",
        "an empty relation, one of 5 and one of 75 queries; the split sums of the two backward sweeps" +
        ("; a row id out of range gives a NaN row" if bad else ""), build, call)


for _d in (18, 20, 64):
    _relation(_d, False)
_relation(20, True)
_relation(18, True, bad=True)


# =====================================================================================================================
# exchange
# =====================================================================================================================

def _rows_pack(rb, xb, n, bad):
    nrows = RC.rows_count(n)
    name = f"{rb}.{xb}.{n}"

    def build():
        rows, extra = RC.rows_tables(nrows, rb, xb, name)
        return dict(rows=_t(rows), extra=None if extra is None else _t(extra), idx=_t(RC.pack_indices(n, nrows, name, bad=bad)),
                    out=_known((n, rb + xb), RC.SENTINEL, torch.uint8))

    def call(i):
        tables = (i["rows"],) if i["extra"] is None else (i["rows"], i["extra"])
        _native._check(_native.load().ghf_rows_pack(i["rows"].data_ptr(), rb, _native._ptr(i["extra"]), xb, i["idx"].data_ptr(), n, nrows,
                                                    i["out"].data_ptr(), _native._stream()), "ghf_rows_pack")
        return (i["out"],) if bad else (i["out"], _native.rows_pack(tables, i["idx"]))
    add(f"rows_pack/{rb}+{xb}-n{n}{'-bad' if bad else ''}", "rows_pack",
        "message rows of row_bytes + extra_bytes" + ("; ids out of range keep what the message held" if bad else ""), build, call)


def _rows_unpack(rb, xb, n, bad):
    nrows = RC.rows_count(n)
    name = f"{rb}.{xb}.{n}"

    def build():
        rows, extra = RC.rows_tables(nrows, rb, xb, name)
        return dict(rows=_t(rows), extra=None if extra is None else _t(extra), idx=_t(RC.unpack_indices(n, nrows, name, bad=bad)),
                    msg=_t(RC.random_bytes(82, "msg." + name, (n, rb + xb))))

    def call(i):
        tables = (i["rows"],) if i["extra"] is None else (i["rows"], i["extra"])
        _native.rows_unpack(tables, i["idx"], i["msg"])
        return tables
    add(f"rows_unpack/{rb}+{xb}-n{n}{'-bad' if bad else ''}", "rows_unpack", "in place into the tables: every other row keeps its content", build, call)


for _rb, _xb, _n_, _bad in ((16, 0, 5, False), (16, 4, 5, True), (1040, 8, 3, True), (512, 4, 33000, False), (2048, 4, 1, False)):
    _rows_pack(_rb, _xb, _n_, _bad)
    _rows_unpack(_rb, _xb, _n_, _bad)


def _rows_accumulate(nrows, d, n, idx, any_width):
    def build():
        ids = None
        if idx:
            ids = np.argsort(synth.raw_u64(83, f"acc{nrows}", nrows), kind="stable")[:n].astype(np.int64)
            ids[0::5], ids[2::7] = -1, nrows
        return dict(rows=_n(83, f"r{nrows}.{d}", (nrows, d)), idx=None if ids is None else _t(ids), msg=_n(83, f"m{n}.{d}", (n, d)))
    add(f"rows_accumulate{'_any' if any_width else ''}/rows{nrows}-d{d}-n{n}{'-idx' if idx else ''}",
        "rows_accumulate_any" if any_width else "rows_accumulate",
        "in place; ids out of range are skipped" + ("; d % 4 != 0: the scalar instance" if d % 4 else ""),
        build, lambda i: (_native.rows_accumulate(i["rows"], i["idx"], i["msg"], any_width=any_width),))


_rows_accumulate(37, 64, 5, True, False)
_rows_accumulate(33007, 4, 33000, True, False)
_rows_accumulate(37, 128, 37, False, False)
_rows_accumulate(37, 18, 5, True, True)
_rows_accumulate(37, 1, 37, False, True)
_rows_accumulate(40, 260, 7, True, True)


# =====================================================================================================================
# end to end: _native, plan, autograd (and the model's own module) patched together
# =====================================================================================================================

E2E_N, E2E_E, E2E_R, E2E_F = 2000, 6000, 6, 32


def _e2e_build(train):
    def build():
        ei, rel = synth.make_graph_arrays(E2E_N, E2E_E, E2E_R, seed=9500, kind="powerlaw")
        torch.manual_seed(11)
        model = HyperGNN(text_dim=16, node_feat_dim=E2E_F, hidden_dim=64, num_layers=3).to(DEV).train(train)
        return dict(model=model, x=_n(39, "x", (E2E_N, E2E_F)), ei=_t(ei), rel=_t(rel), gout=_n(39, "gout", (E2E_N, 64)))
    return build


def _train_step(i):
    model = i["model"]
    out = model.forward_ids(i["x"], i["ei"], i["rel"], synth.relation_names(E2E_R))
    loss = (out * i["gout"]).sum()
    loss.backward()
    grads = [p.grad for _, p in sorted(model.named_parameters())]
    assert all(g is not None for g in grads)
    return [loss.detach().reshape(1), out.detach()] + grads


def _forward_nodes(i):
    nodes = torch.tensor([5, 0, 1999, 5, 123], dtype=torch.int64)
    with torch.no_grad():
        return (i["model"].forward_nodes_ids(i["x"], i["ei"], i["rel"], synth.relation_names(E2E_R), nodes, fanout=[2, -1, 1], seed=5,
                                             exclude=(i["ei"][0][:40], i["ei"][1][:40])),)


add("end_to_end/train_step", "message_layer_fwd tail_bwd edge_outer weightgen_bwd text_encode_bwd plan_build",
    "one training step of a 3-layer hidden-64 model on a 2000-node graph: the loss, the output and every parameter gradient",
    _e2e_build(True), _train_step)
add("end_to_end/forward_nodes", "subgraph_sample_hops_excl subgraph_nodes subgraph_sample_edges message_layer_fwd",
    "forward_nodes with fanout caps 2, none, 1 and an exclude list: the sampled subgraph's plan and rows", _e2e_build(False), _forward_nodes)


# =====================================================================================================================
# the tests
# =====================================================================================================================

class _Recorder:
    """The loaded library with every entry point's use noted; with `fence`, entry points that take workspace_bytes are first
    called with one byte less than they were given: they must refuse and write nothing, then the real call goes ahead."""

    def __init__(self, lib, fence=None) -> None:
        self._lib, self.called, self.sizes, self.rejected, self._fence = lib, set(), set(), set(), fence

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("ghf_"):
            return fn
        self.called.add(name)
        res, argtypes = _native.SIGNATURES[name]
        if name.endswith("_workspace_bytes"):
            def query(*args):
                n = fn(*args)
                self.sizes.add(int(n))
                return n
            return query
        if self._fence is None or res is not _native._i32 or _native._sz not in argtypes:
            return fn
        at = len(argtypes) - 1 - argtypes[::-1].index(_native._sz)      # (the last one: a 64-bit seed is the same ctypes class)

        def call(*args):
            need = int(args[at])
            if need == 0:                                   # (nothing to be short of)
                self.rejected.add(name)
                return fn(*args)
            if name == "ghf_subgraph_nodes":            # not told E: it requires the head of the shared workspace (include/ghf.h)
                need = int(self._lib.ghf_subgraph_workspace_bytes(args[1], 0, args[2]))
                assert 0 < need <= int(args[at])
            else:
                assert need in self.sizes, f"{name}: told {need} workspace bytes, which no *_workspace_bytes query returned"
            torch.cuda.synchronize()
            before = [a.raw.clone() for a in self._fence.allocs]
            rc = fn(*args[:at], need - 1, *args[at + 1:])
            torch.cuda.synchronize()
            assert rc == EINVAL, f"{name}: workspace_bytes = need - 1 = {need - 1} returned {rc}, not GHF_EINVAL"
            for a, b in zip(self._fence.allocs, before):
                assert torch.equal(a.raw, b), f"{name} refused a workspace of need - 1 bytes, yet wrote into {a.name()}"
            self.rejected.add(name)
            return fn(*args)
        return call


def _takes_workspace_bytes(name):
    res, argtypes = _native.SIGNATURES[name]
    return res is _native._i32 and _native._sz in argtypes


@pytest.fixture(scope="module")
def guard_word():
    """The registered range-guard word: one object for every run of every case (registered before anything is patched)."""
    _native.load()
    flag = _native.range_flag(DEV)
    flag.zero_()
    return flag


SLOWEST = {"id": None, "seconds": 0.0}


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_fenced_call(case, guard_word, monkeypatch):
    if case.env:
        monkeypatch.setenv("GHF_KERNEL", case.env)
    else:
        monkeypatch.delenv("GHF_KERNEL", raising=False)
    rec = _Recorder(_native.load())
    monkeypatch.setattr(_native, "_lib", rec)
    assert _native.range_flag(DEV) is guard_word
    before = int(guard_word.item())
    t0 = time.perf_counter()
    F.run_three(case.build, case.call, PATCHED, monkeypatch, what=case.id)
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    print(f"FENCE {case.id}: {seconds:.2f} s")
    if seconds > SLOWEST["seconds"]:
        SLOWEST.update(id=case.id, seconds=seconds)
    assert _native.range_flag(DEV) is guard_word and int(guard_word.item()) == before, "the range guard word changed"
    missing = set(case.symbols) - rec.called
    assert not missing, f"{case.id} claims {sorted(missing)} but never called them"


test_fenced_call.__doc__ = "Three runs of every row, bit-equal, every band intact.  The rows and what each is there for:\n\n" + \
    "\n".join(f"  {c.id}: {c.why}" for c in CASES)

REJECT = [c for c in CASES if any(_takes_workspace_bytes(s) for s in c.symbols) and not c.id.startswith("end_to_end")]


@pytest.mark.parametrize("case", REJECT, ids=[c.id for c in REJECT])
def test_a_workspace_one_byte_short_is_refused(case, guard_word, monkeypatch):
    """Every entry point that takes workspace_bytes returns GHF_EINVAL when told need - 1 — the buffer behind the pointer stays
    full-size and fenced, so an entry that forgot the check still writes only memory the test owns — and leaves every buffer
    of the call as it was."""
    if case.env:
        monkeypatch.setenv("GHF_KERNEL", case.env)
    else:
        monkeypatch.delenv("GHF_KERNEL", raising=False)
    fence = F.Fence(0xFF)
    rec = _Recorder(_native.load(), fence)
    monkeypatch.setattr(_native, "_lib", rec)
    with F.installed(fence, PATCHED, monkeypatch):
        case.call(fence.place_tree(case.build()))
    fence.check()
    want = {s for s in case.symbols if _takes_workspace_bytes(s)}
    assert want <= rec.rejected, f"not reached with need - 1: {sorted(want - rec.rejected)}"


def test_every_workspace_taking_entry_is_in_the_rejection_test():
    taking = {s for s in _native.SIGNATURES if _takes_workspace_bytes(s)}
    assert taking and taking <= {s for c in REJECT for s in c.symbols}


def test_the_fence_reports_a_planted_byte_on_the_device():
    """The only place where the fence is expected to find something."""
    fence = F.Fence(0x5A)
    t = fence.torch().empty(33, 7, dtype=torch.float32, device=DEV)
    assert t.is_cuda and t.data_ptr() % 256 == 0 and len(fence.allocs) == 1
    t.fill_(1.0)
    fence.check()
    a = fence.allocs[0]
    a.raw[a.off + a.nbytes + 4095] = 0                             # a torch indexing write on the raw buffer
    with pytest.raises(F.FenceError) as err:
        fence.check()
    at = a.nbytes + 4095
    assert f"after the interior, offsets {at}..{at} " in str(err.value) and "(33, 7) torch.float32" in str(err.value), str(err.value)
    a.raw[a.off - 1] = 0
    assert len(fence.damage()) == 2 and "offsets -1..-1 " in fence.damage()[0]


def test_report_the_slowest_case():
    print(f"FENCE slowest case: {SLOWEST['id']} {SLOWEST['seconds']:.2f} s")
    assert SLOWEST["seconds"] < 10.0, f"{SLOWEST['id']} took {SLOWEST['seconds']:.1f} s: shrink it to the next smaller shape that reaches its branch"
