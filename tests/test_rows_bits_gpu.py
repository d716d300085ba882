"""The bits of the kernels that cut a row into its two fp16 pieces (GHF_WLAYOUT_SPLIT2H) and count it for the range guard:
ghf_split_rows, ghf_input_proj_fwd, ghf_run_rows_fwd / ghf_segment_tail_fwd, the combine kernel of ghf_message_layer_fwd's
split blocks and ghf_tail_bwd produce, case by case, exactly the bytes recorded in tests/golden/rows_bits.json.

    python tests/test_rows_bits_gpu.py --record [--out PATH] [--commit ID]

records the fixture (tests/_bits.py).  Only public _native functions are called; inputs are integer hashes (tests/_bits.py)
and graphs from integer formulas or tests/_plan_cases.py.  Every case zeroes the range-guard word first and hashes its value
with the outputs; buffers a kernel writes into are zero- or 7-filled first, so that a store left out shows.

Every data matrix has one row whose largest magnitude stands in its LAST column alone (4.0 among values below 0.5; LayerNorm
outputs: beta[d - 1] = 32), so that a lane left out of the row's maximum changes the power of two, and one all-zero row.
Threshold rows (tests/_rows_cases.py, proven in test_rows_host.py) pin the guard's rule at every site: `fires` has
tiny * 8 == nonzero exactly, `holds` two entries fewer, standing at exactly 0.5 once scaled.  Sites that cut a LayerNorm output
get gamma = 0 and the row in beta (the output is beta exactly); the input projection gets the row as its bias under an all-zero
row of x; run_rows gets it as one source of a run whose other source is a zero row; tail_bwd gets it (signed, so that the
means of the LayerNorm backward vanish) as g_out over a constant row with eps = 0.25 and gamma = 1, where G = rstd * g_out.

Cases:
  split_rows   d = 64, 100, 128, 192; 9 rows; data / fires / holds / a sub-range (row0 = 2, 4 rows) into a 7-filled buffer.
  input_proj   d = 64, 128 x F = 32, 128.  N = 33 (a partial 32-row tile: the r >= N clamp is live) runs the fp32-MFMA kernel,
               without and with h_split; N = 1025 with h_split runs the two-piece kernel (launch_input_proj: it needs
               N >= 1024), which also cuts the rows of x: threshold rows in x and in the bias.  d = 64, F = 48, N = 8193: the
               fp32 kernel with W_in in LDS.
  wide rows    d = 128 (CPL 2, the four-wave pass 1), 256 (the eight-wave pass 1), 384 (not a power of two): a graph of 12
               nodes whose node 0 is a hub (hub_of >= 0: RS_HUB_ROWS lowered to 8), node 1 has one row, node 2 none, node 3 a
               run of several edges (RS_RUN_MAX lowered to 2, so that run_rows_kernel runs): tail, NO_TAIL, NO_TAIL | RAW_SUM, a
               row sub-range, and the threshold rows for pass 0 (run_rows) and pass 2 (segment_tail).  The guard tests at the
               end of this file (no fixture) run the same threshold rows at every width of the layer, 128 .. 1024.
  split blocks d = 64, 128, kernels bx and pp: a block of 5 rows (not a multiple of the rows per pass) with more than
               split_chunks chunks, and the last-round split of _plan_cases.value_cases: tail, NO_TAIL, NO_TAIL | RAW_SUM;
               bx also h_split_out + agg_out, NO_TAIL | ADD_H and the threshold rows (the split block's rows alone are launched,
               so the combine kernel is the only one that cuts).  The pp kernels take no h_split_out, agg_out or ADD_H
               (ghf_message_layer_fwd refuses them), so those variants cannot reach the combine kernel through pp.
  tail_bwd     d = 64, 128, 256; N = 5 and 130; without and with split_layout, without and with drop; row 2 has a zero g_out
               (a row the loss does not touch)."""

import contextlib
import functools
import os
import sys

import numpy as np
import pytest
import torch

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import _plan_cases as P  # noqa: E402
from _bits import dev, digest, hashed, load_fixture, record_main  # noqa: E402
from _rows_cases import KINDS, threshold_row  # noqa: E402
from graph_hypernetwork_forge_amd import _native  # noqa: E402
from graph_hypernetwork_forge_amd import plan as plan_mod  # noqa: E402
from graph_hypernetwork_forge_amd.autograd import _layer_weights  # noqa: E402

pytestmark = pytest.mark.gpu
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rows_bits.json")
DEV = "cuda:0"
S2H = _native.WLAYOUT_SPLIT2H
NO_TAIL, RAW_SUM, ADD_H = _native.GHF_FLAG_NO_TAIL, _native.GHF_FLAG_RAW_SUM, _native.GHF_FLAG_ADD_H
FLAGS = {"tail": 0, "no_tail": NO_TAIL, "raw_sum": NO_TAIL | RAW_SUM, "addh": NO_TAIL | ADD_H}


def zero_flag():
    flag = _native.range_flag(DEV)
    flag.zero_()
    return flag


def data(n, m, salt):
    """Hashed rows; row 1 has its largest magnitude in the last column alone, row n - 2 is zero."""
    a = hashed(n, m, salt).copy()
    a[1, m - 1] = 4.0
    a[n - 2] = 0.0
    return a


def zeros_split(N, d, fill=0):
    return torch.full_like(_native.alloc_split(N, d, S2H, DEV), fill)


def ln_params(d, kind):
    """(gamma, beta): data (beta[d - 1] = 32: every row's largest output stands in the last column) or a threshold row."""
    if kind in KINDS:
        return dev(np.zeros(d, dtype=np.float32)), dev(threshold_row(d, kind))
    gamma, beta = 1.0 + hashed(1, d, 41).reshape(d) * np.float32(0.25), hashed(1, d, 42).reshape(d).copy()
    beta[d - 1] = 32.0
    return dev(gamma), dev(beta)


# ---- ghf_split_rows ---------------------------------------------------------------------------------------------------

def case_split_rows(d, kind):
    h = data(9, d, 21)
    if kind in KINDS:
        h[3] = threshold_row(d, kind)
    flag = zero_flag()
    if kind == "sub":
        out = _native.split_rows(dev(h), S2H, out=zeros_split(9, d, 7), row0=2, rows=4)
    else:
        out = _native.split_rows(dev(h), S2H, out=zeros_split(9, d))
    return out, flag.clone()


# ---- ghf_input_proj_fwd -------------------------------------------------------------------------------------------------

def case_input_proj(d, F, N, split, kind):
    """kind: data, x_fires / x_holds (the threshold row as row 3 of x), b_fires / b_holds (as the bias: the zero row of x
    gives it back exactly)."""
    x, W, b = data(N, F, 31), hashed(d, F, 32), hashed(1, d, 33).reshape(d).copy()
    where, _, k = kind.partition("_")
    if where == "x":
        x[3] = threshold_row(F, k)
    if where == "b":
        b = threshold_row(d, k)
    flag = zero_flag()
    hs = zeros_split(N, d) if split else None
    h0 = _native.input_proj_fwd(dev(x), dev(W), dev(b), out=torch.zeros(N, d, device=DEV), h_split=hs, split_layout=S2H if split else 0)
    if where == "b":
        assert torch.equal(h0[N - 2], dev(b)), "the zero row of x must give the bias back exactly"
    return (h0, flag.clone()) + ((hs,) if split else ())


# ---- wide rows: ghf_run_rows_fwd, ghf_edge_transform_h_fwd, ghf_segment_tail_fwd ------------------------------------------

RS_N, RS_R = 12, 3


def rs_graph():
    i = np.arange(30)
    src = [(7 * i + 1) % RS_N, [5], [4, 6, 8]]
    dst = [np.zeros(30, dtype=np.int64), [1], [3, 3, 3]]
    rel = [i % 3, [1], [2, 2, 2]]
    v = np.arange(4, RS_N)
    src += [(3 * v + 2) % RS_N, (5 * v + 1) % RS_N]
    dst += [v, v]
    rel += [v % 3, (v + 1) % 3]
    cat = lambda parts: np.concatenate([np.asarray(p, dtype=np.int64) for p in parts])     # noqa: E731
    return np.stack([cat(src), cat(dst)]), cat(rel)


@functools.lru_cache(maxsize=None)
def rs_plan(d):
    ei, rel = rs_graph()
    plan = plan_mod.build_plan(dev(ei), dev(rel), [""] * RS_R, RS_N, d, torch.device(DEV), force_generic=True)
    old = plan_mod.RS_HUB_ROWS, plan_mod.RS_RUN_MAX
    plan_mod.RS_HUB_ROWS, plan_mod.RS_RUN_MAX = 8, 2
    try:
        rs = plan_mod.build_rs(plan, runs=True)
    finally:
        plan_mod.RS_HUB_ROWS, plan_mod.RS_RUN_MAX = old
    hub = rs.hub_of.cpu().numpy()
    off = rs.off.cpu().numpy()
    assert hub[0] >= 0 and (hub[1:] < 0).all() and off[2] - off[1] == 1 and off[3] == off[2] and rs.run_start.numel() > 1
    starts, runs = rs.run_start.cpu().numpy(), rs.run_src.cpu().numpy()
    assert any(sorted(runs[a:b]) == [4, 6] for a, b in zip(starts[:-1], starts[1:])), "node 3's run of sources 4 and 6"
    return rs


def case_rs(d, kind):
    """kind: tail / no_tail / raw_sum / sub (pass 2's variants), fires / holds (pass 2 cuts beta), run_fires / run_holds
    (pass 0 cuts h[4] + h[6] = the threshold row + 0)."""
    rs = rs_plan(d)
    h = hashed(RS_N, d, 51).copy()
    h[1, d - 1] = 4.0
    where, _, k = kind.partition("_")
    if where == "run":
        h[4], h[6] = threshold_row(d, k), 0.0
    Wm, Ws = (dev(hashed(RS_R * d, d, s).reshape(RS_R, d, d) * np.float32(0.25)) for s in (52, 53))
    b = dev(hashed(RS_R, d, 54))
    h_d = dev(h)
    hs = _native.split_rows(h_d, S2H)
    flag = zero_flag()                                   # (after the cut of h itself: the case is about the passes)
    Y = torch.zeros(rs.rows, d, device=DEV)
    _native.edge_transform_fwd(h_d, rs, Wm, Ws, b, Y, h_split=hs, exact=False)
    nx = rs.run_start.numel() - 1
    X = rs.run_scratch(nx, d)[: _native.load().ghf_split_rows_bytes(nx, d, S2H)].clone()
    flag1 = flag.clone()
    flag.zero_()
    gamma, beta = ln_params(d, kind)
    flags = FLAGS.get(kind, 0)
    sub = {"row0": 2, "rows": 7} if kind == "sub" else {}
    fill = 7 if kind == "sub" else 0
    out, split = torch.full((RS_N, d), float(fill), device=DEV), zeros_split(RS_N, d, fill)
    if flags & NO_TAIL:
        _native.segment_tail_fwd(Y, rs, None, None, None, 0.0, out, flags=flags, h_split_out=split, exact=False)
    else:
        _native.segment_tail_fwd(Y, rs, h_d, gamma, beta, 1e-5, out, h_split_out=split, exact=False, **sub)
    if kind in KINDS:
        assert torch.equal(out, beta.expand(RS_N, d)), "gamma = 0: every row must be beta exactly"
    return Y, X, flag1, out, split, flag.clone()


# ---- split blocks of ghf_message_layer_fwd: the combine kernel -------------------------------------------------------------

ROUTES = {"bx128": (128, None), "bx64": (64, "bx"), "pp128": (128, "pp"), "pp64": (64, None)}


@contextlib.contextmanager
def kernel_env(name):
    old = os.environ.get("GHF_KERNEL")
    try:
        if name is None:
            os.environ.pop("GHF_KERNEL", None)
        else:
            os.environ["GHF_KERNEL"] = name
        yield
    finally:
        if old is None:
            os.environ.pop("GHF_KERNEL", None)
        else:
            os.environ["GHF_KERNEL"] = old


def geometry(route):
    d, env = ROUTES[route]
    return _native.message_config(d, env) if route != "pp64" else _native.exact_config(d)


def hub_graph(bn, sc):
    """N = 2 bn + 5: the last block has 5 rows and sc + 2 chunks (one relation, two edges each); 30 edges elsewhere."""
    N, last0 = 2 * bn + 5, 2 * bn
    r, i = np.arange(sc + 2), np.arange(30)
    dst = np.concatenate([last0 + r % 5, last0 + (3 * r + 1) % 5, (13 * i + 2) % last0])
    src = np.concatenate([(11 * r + 3) % N, (7 * r + 5) % N, (5 * i + 1) % N])
    rel = np.concatenate([r, r, i % 2])
    return N, sc + 3, np.stack([src, dst]).astype(np.int64), rel.astype(np.int64), last0


@functools.lru_cache(maxsize=None)
def block_plan(route, graph):
    """(plan, first row of the split blocks) of the route's kernel for the hub graph or the last-round graph."""
    d, env = ROUTES[route]
    bn, wl, cr, sc = geometry(route)
    if graph == "hub":
        N, R, ei, rel, row0 = hub_graph(bn, sc)
    else:
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        case = P.value_cases(bn, cr, sc, cus)[0]
        N, R, ei, rel, row0 = case.N, case.R, case.edge_index, case.rel, cus * bn
    with kernel_env(env):
        plan = plan_mod.build_plan(dev(ei), dev(rel), [""] * R, N, d, torch.device(DEV))
    assert (plan.block_nodes, plan.wlayout) == (bn, wl) and plan.n_slots > 0, f"{route} {graph}: no split block"
    assert plan.item_off_host[-1] - plan.item_off_host[row0 // bn] > -(-(N - row0) // bn), "the rows from row0 on hold a split block"
    return plan, row0


def case_block(route, graph, kind):
    """kind: tail / no_tail / raw_sum; bx: split (h_split_out and agg_out), addh, fires / holds (the split blocks' rows alone)."""
    d, env = ROUTES[route]
    plan, row0 = block_plan(route, graph)
    N, R = plan.N, plan.R
    h_d = dev(data(N, d, 61))
    Wm, Ws = (dev(hashed(R * d, d, s).reshape(R, d, d) * np.float32(0.25)) for s in (62, 63))
    b = dev(hashed(R, d, 64))
    gamma, beta = ln_params(d, kind)
    W, W2 = _layer_weights(plan, Wm, Ws, transpose=False)
    hs = _native.split_rows(h_d, plan.wlayout) if plan.wlayout in _native.SPLIT_LAYOUTS else None
    flag = zero_flag()
    out = torch.zeros(N, d, device=DEV)
    flags = FLAGS.get(kind, 0)
    kw = {}
    if kind in KINDS + ("split",):
        kw["h_split_out"] = zeros_split(N, d)
    if kind == "split":
        kw["agg_out"] = torch.zeros(N, d, device=DEV)
    if kind in KINDS:
        kw.update(row0=row0, rows=N - row0)
    with kernel_env(env):
        if flags & NO_TAIL:
            _native.message_layer_fwd(h_d, plan, W, W2, b, plan.wlayout, None, None, 0.0, out, flags=flags, h_split=hs)
        else:
            _native.message_layer_fwd(h_d, plan, W, W2, b, plan.wlayout, gamma, beta, 1e-5, out, h_split=hs, **kw)
    if kind in KINDS:
        assert torch.equal(out[row0:], beta.expand(N - row0, d)), "gamma = 0: every row must be beta exactly"
    return (out, flag.clone()) + tuple(kw[k] for k in ("h_split_out", "agg_out") if k in kw)


# ---- ghf_tail_bwd ---------------------------------------------------------------------------------------------------------

def case_tail_bwd(d, N, split, drop, kind):
    g, agg, h = data(N, d, 71), hashed(N, d, 72).copy(), hashed(N, d, 73).copy()
    agg[1], h[1] = np.abs(agg[1]) + 0.25, np.abs(h[1])           # (row 1 passes the ReLU everywhere: its largest gradient stays last)
    g[1, : d - 2] = 0.0
    g[1, d - 2] = -4.0
    g[2] = 0.0                                                   # a row the loss does not touch
    gamma, eps = 1.0 + hashed(1, d, 74).reshape(d) * np.float32(0.25), 1e-5
    if kind in KINDS:                                            # row 3: pre = 1 throughout, rstd = 1 / sqrt(eps) = 2, G = 2 g_out
        g[3], agg[3], h[3] = threshold_row(d, kind, signed=True), 0.5, 0.5
        gamma, eps = np.ones(d, dtype=np.float32), 0.25
    indeg = dev(((np.arange(N) * 5 + 1) % 4).astype(np.int32))    # (rows 0, 3, ...: divisor max(indeg, 1) = 1)
    dm = dev((((np.arange(N)[:, None] * 3 + np.arange(d)[None, :]) % 5 != 0) * np.float32(1.25)).astype(np.float32)) if drop else None
    flag = zero_flag()
    dpre, G, Gs, dgamma, dbeta = _native.tail_bwd(dev(g), dev(agg), dev(h), dev(gamma), eps, indeg, drop=dm,
                                                  split_layout=S2H if split else None)
    if kind in KINDS:
        assert torch.equal(G[3], 2.0 * dev(g)[3]), "row 3 of G must be 2 g_out exactly"
    return (dpre, G, dgamma, dbeta, flag.clone()) + ((Gs,) if split else ())


# ---- the cases ----------------------------------------------------------------------------------------------------------

def build_cases():
    Pt = functools.partial
    cases = {}
    for d in (64, 100, 128, 192):
        for kind in ("data", "sub") + KINDS:
            cases[f"split_rows/d{d}/{kind}"] = Pt(case_split_rows, d, kind)
    for d in (64, 128):
        for F in (32, 128):
            cases[f"input_proj/fp32/d{d}/F{F}/N33/plain/data"] = Pt(case_input_proj, d, F, 33, False, "data")
            for kind in ("data", "b_fires", "b_holds"):
                cases[f"input_proj/fp32/d{d}/F{F}/N33/split/{kind}"] = Pt(case_input_proj, d, F, 33, True, kind)
            for kind in ("data", "x_fires", "x_holds", "b_fires", "b_holds"):
                cases[f"input_proj/pieces/d{d}/F{F}/N1025/split/{kind}"] = Pt(case_input_proj, d, F, 1025, True, kind)
    for split in (False, True):
        cases[f"input_proj/fp32_lds/d64/F48/N8193/{'split' if split else 'plain'}/data"] = Pt(case_input_proj, 64, 48, 8193, split, "data")
    for d in (128, 256, 384):
        for kind in ("tail", "no_tail", "raw_sum", "sub", "run_fires", "run_holds") + KINDS:
            cases[f"wide_rows/d{d}/{kind}"] = Pt(case_rs, d, kind)
    for route in ROUTES:
        bx = route.startswith("bx")
        for graph in ("hub", "last_round"):
            for kind in ("tail", "no_tail", "raw_sum") + (("split", "addh") if bx else ()):
                cases[f"split_blocks/{route}/{graph}/{kind}"] = Pt(case_block, route, graph, kind)
        if bx:
            for kind in KINDS:
                cases[f"split_blocks/{route}/hub/{kind}"] = Pt(case_block, route, "hub", kind)
    for d in (64, 128, 256):
        for N in (5, 130):
            for split in (False, True):
                for drop in (False, True):
                    cases[f"tail_bwd/d{d}/N{N}/{'split' if split else 'plain'}/{'drop' if drop else 'keep'}/data"] = \
                        Pt(case_tail_bwd, d, N, split, drop, "data")
        for kind in KINDS:
            cases[f"tail_bwd/d{d}/N5/split/keep/{kind}"] = Pt(case_tail_bwd, d, 5, True, False, kind)
    return cases


CASES = build_cases()


@functools.lru_cache(maxsize=None)
def recorded():
    return load_fixture(FIXTURE)


def test_the_fixture_names_exactly_these_cases():
    assert sorted(recorded()) == sorted(CASES)


@pytest.mark.parametrize("name", sorted(CASES))
def test_output_bytes_are_the_recorded_ones(name):
    got = digest(CASES[name]())
    print(f"{name}: {got}")
    assert got == recorded()[name]


# ---- the guard word, site by site, without the fixture ----------------------------------------------------------------------

def guard(kind):
    return _native.RANGE_ROWS if kind.endswith("fires") else 0


def scale_bits(split, N, d, row):
    return float(_native.split_row_scales(split, N, d)[row])


@pytest.mark.parametrize("d", (64, 100, 128, 192))
@pytest.mark.parametrize("kind", KINDS)
def test_guard_split_rows(d, kind):
    out, flag = case_split_rows(d, kind)
    assert int(flag) == guard(kind) and scale_bits(out, 9, d, 3) == 2.0 ** -13


@pytest.mark.parametrize("d,F", [(64, 32), (64, 128), (128, 32), (128, 128)])
@pytest.mark.parametrize("kind", KINDS)
def test_guard_input_proj_fp32_epilogue(d, F, kind):
    h0, flag, hs = case_input_proj(d, F, 33, True, "b_" + kind)
    assert int(flag) == guard(kind) and scale_bits(hs, 33, d, 31) == 2.0 ** -13


@pytest.mark.parametrize("d,F", [(64, 32), (64, 128), (128, 32), (128, 128)])
@pytest.mark.parametrize("kind", KINDS)
def test_guard_input_proj_pieces_epilogue(d, F, kind):
    h0, flag, hs = case_input_proj(d, F, 1025, True, "b_" + kind)
    assert int(flag) == guard(kind) and scale_bits(hs, 1025, d, 1023) == 2.0 ** -13


@pytest.mark.parametrize("d,F", [(64, 32), (64, 128), (128, 32), (128, 128)])
@pytest.mark.parametrize("kind", KINDS)
def test_guard_input_proj_pieces_rows_of_x(d, F, kind):
    h0, flag, hs = case_input_proj(d, F, 1025, True, "x_" + kind)
    assert int(flag) == guard(kind)


WIDE = (128, 256, 384, 512, 640, 768, 896, 1024)    # every width of the relation-stationary layer (the fixture records three)


@pytest.mark.parametrize("d", WIDE)
@pytest.mark.parametrize("kind", KINDS)
def test_guard_run_rows(d, kind):
    Y, X, flag1, out, split, flag2 = case_rs(d, "run_" + kind)
    assert int(flag1) == guard(kind) and int(flag2) == 0


@pytest.mark.parametrize("d", WIDE)
@pytest.mark.parametrize("kind", KINDS)
def test_guard_segment_tail(d, kind):
    Y, X, flag1, out, split, flag2 = case_rs(d, kind)
    assert int(flag1) == 0 and int(flag2) == guard(kind) and scale_bits(split, RS_N, d, 5) == 2.0 ** -13


@pytest.mark.parametrize("route", ("bx128", "bx64"))
@pytest.mark.parametrize("kind", KINDS)
def test_guard_combine_split(route, kind):
    out, flag, split = case_block(route, "hub", kind)
    N, d = out.shape
    assert int(flag) == guard(kind) and scale_bits(split, N, d, N - 1) == 2.0 ** -13


@pytest.mark.parametrize("d", (64, 128, 256))
@pytest.mark.parametrize("kind", KINDS)
def test_guard_tail_bwd(d, kind):
    dpre, G, dgamma, dbeta, flag, Gs = case_tail_bwd(d, 5, True, False, kind)
    assert int(flag) == guard(kind) and scale_bits(Gs, 5, d, 3) == 2.0 ** -12


if __name__ == "__main__":
    record_main(FIXTURE, CASES)
