"""The block epilogue of message_bx_kernel<128, *> (the helpers' register dump and the fused tail) at the smallest shapes at
which it can go wrong: a last block that ends inside the first half of a block's rows, on the half boundary and inside the
second half; blocks without chunks, isolated rows, a split hub block (partial sums + the combine kernel); every flag
combination the tail knows; a row sub-range; and the split rows a tail writes, gathered by the next layer.

Everything is compared with the float64 layer of _edge_graphs.py at the tolerance of
test_hip_parity.py::test_message_layer_matches_oracle (_util.assert_close), and every launch is repeated: same bits."""

import numpy as np
import pytest
import torch

import _edge_graphs as G
from _util import assert_close
from graph_hypernetwork_forge_amd import _native, synth
from graph_hypernetwork_forge_amd.autograd import MessageLayerFn, _layer_weights, build_train_plan
from graph_hypernetwork_forge_amd.plan import build_plan, empty_plan

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
D = 128
SIZES = [1, 191, 193, 384, 385, 581]
KINDS = ["no_in_edges", "isolated", "hub"]
F = _native


def _geometry():
    bn, wl, cr, sc = _native.message_config(D)
    assert (bn, wl) == (384, _native.WLAYOUT_SPLIT2H), "the sizes of this file are those of 384-row blocks"
    return bn, wl, cr, sc


def _graph(N, kind):
    """(edge_index [2, E], rel [E], R): the last block of the graph is the odd one."""
    bn, _, _, sc = _geometry()
    seed, tag = 9100 + N, f"bxepi/{kind}/{N}"
    last0 = ((N - 1) // bn) * bn                     # first row of the last block
    nl = N - last0
    if kind == "no_in_edges":                        # the last block has no chunk at all; an ordinary block before it, if there is one
        R = 3
        if last0 == 0:
            return np.zeros((2, 0), dtype=np.int64), np.zeros(0, dtype=np.int64), R
        dst = synth.randint(seed, tag + "/dst", 40, last0)
        src = synth.randint(seed, tag + "/src", 40, N)
        return np.stack([src, dst]), synth.randint(seed, tag + "/rel", 40, R - 1), R
    if kind == "isolated":                           # every third row has in-edges, the others none: h' = LN(ReLU(h)) there
        R = 4
        dst = np.repeat(np.arange(0, N, 3), 2)
        src = synth.randint(seed, tag + "/src", dst.size, N)
        return np.stack([src, dst]), synth.randint(seed, tag + "/rel", dst.size, R - 1), R
    # hub: sc + 2 chunks of two rows each in the last block (one chunk per relation) — more than split_chunks: two work items
    R = sc + 3
    rel = np.repeat(np.arange(sc + 2), 2)
    dst = last0 + synth.randint(seed, tag + "/dst", rel.size, nl)
    src = synth.randint(seed, tag + "/src", rel.size, N)
    if last0:
        dst = np.concatenate([dst, synth.randint(seed, tag + "/dst0", 30, last0)])
        src = np.concatenate([src, synth.randint(seed, tag + "/src0", 30, N)])
        rel = np.concatenate([rel, synth.randint(seed, tag + "/rel0", 30, 2)])
    return np.stack([src, dst]).astype(np.int64), rel.astype(np.int64), R


_CACHE: dict = {}


def _case(N, kind):
    """Graph, inputs, plan and the float64 references, made once per (N, kind) and never modified."""
    key = (N, kind)
    if key not in _CACHE:
        bn, wl, cr, sc = _geometry()
        ei, rel, R = _graph(N, kind)
        c = G.Case(f"{kind}_{N}", N, ei, rel, R, ())
        h, Wm, Ws, b, gamma, beta = G.layer_inputs(c, D, 7300 + N)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)                    # noqa: E731
        if rel.size:
            plan = build_plan(t(ei), t(rel), [""] * R, N, D, DEV)
        else:
            plan = empty_plan(N, [""] * R, (bn, wl, cr, sc), DEV)
        assert (plan.block_nodes, plan.wlayout) == (bn, wl)
        per_block = np.diff(plan.blk_chunk_off.cpu().numpy())
        if kind == "no_in_edges":
            assert per_block[-1] == 0, "the last block must have no chunk"
        if kind == "hub":
            assert per_block[-1] == sc + 2 and plan.n_slots == 2, "the last block must be split into two work items"
        else:
            assert plan.n_slots == 0
        ref_agg, ref_out = G.layer_ref64(h, ei, rel, Wm, Ws, b, gamma, beta)
        indeg = np.bincount(ei[1], minlength=N)
        if kind == "isolated":                       # what the case is for, stated on the reference
            lone = np.nonzero(indeg == 0)[0]
            assert lone.size or N == 1
            x = np.maximum(h[lone].astype(np.float64), 0.0)
            ln = (x - x.mean(1, keepdims=True)) / np.sqrt(x.var(1, keepdims=True) + G.LN_EPS) * gamma + beta
            assert np.allclose(ref_out[lone], ln, rtol=0, atol=1e-12)
        _CACHE[key] = dict(N=N, ei=ei, rel=rel, R=R, h=h, Wm=Wm, Ws=Ws, b=b, gamma=gamma, beta=beta, plan=plan, indeg=indeg,
                           ref_agg=ref_agg, ref_out=ref_out, dev={k: t(v) for k, v in
                                                                  dict(h=h, Wm=Wm, Ws=Ws, b=b, gamma=gamma, beta=beta).items()})
    return _CACHE[key]


def _twice(launch, like, what):
    """Run `launch(out)` twice into NaN-filled tensors: the same bits both times; returns the first."""
    a, b = torch.full_like(like, float("nan")), torch.full_like(like, float("nan"))
    launch(a)
    launch(b)
    assert torch.equal(a, b), f"{what}: a second launch gives other bits"
    return a


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("N", SIZES)
def test_tail_flag_combinations(N, kind):
    c = _case(N, kind)
    plan, dv = c["plan"], c["dev"]
    flag = _native.range_flag(DEV)
    flag.zero_()
    h_d = dv["h"]
    W, W2 = _layer_weights(plan, dv["Wm"], dv["Ws"], transpose=False)
    hs = _native.split_rows(h_d, plan.wlayout)
    what = f"N={N} {kind}"

    # the full tail, last-layer form (no split rows out)
    plain = _twice(lambda o: F.message_layer_fwd(h_d, plan, W, W2, dv["b"], plan.wlayout, dv["gamma"], dv["beta"], 1e-5, o, h_split=hs),
                   h_d, what + " tail")
    assert_close(plain.cpu().numpy(), c["ref_out"], what + " tail")

    # ... with the split rows for the next layer, and with the aggregate beside them
    split = torch.zeros_like(hs)
    out = _twice(lambda o: F.message_layer_fwd(h_d, plan, W, W2, dv["b"], plan.wlayout, dv["gamma"], dv["beta"], 1e-5, o, h_split=hs,
                                               h_split_out=split), h_d, what + " tail + split rows")
    assert torch.equal(out, plain), what + ": h' differs when the split rows are written too"
    assert torch.equal(split, _native.split_rows(plain, plan.wlayout)), what + ": h_split_out is not split_rows(h')"
    assert _native.side_output_supported(plan, D)
    split2, agg = torch.zeros_like(hs), torch.full_like(h_d, float("nan"))
    out = _twice(lambda o: F.message_layer_fwd(h_d, plan, W, W2, dv["b"], plan.wlayout, dv["gamma"], dv["beta"], 1e-5, o, h_split=hs,
                                               h_split_out=split2, agg_out=agg), h_d, what + " tail + agg_out")
    assert torch.equal(out, plain) and torch.equal(split2, split), what + ": h' or its split rows differ when agg_out is written too"
    assert_close(agg.cpu().numpy(), c["ref_agg"], what + " agg_out")

    # without the tail: the mean; the raw sum (destination half, <128, 1>); the mean plus a residual (source half, <128, 2>)
    mean = _twice(lambda o: F.message_layer_fwd(h_d, plan, W, W2, dv["b"], plan.wlayout, None, None, 0.0, o, h_split=hs,
                                                flags=F.GHF_FLAG_NO_TAIL), h_d, what + " NO_TAIL")
    assert_close(mean.cpu().numpy(), c["ref_agg"], what + " NO_TAIL")
    deg = np.maximum(c["indeg"], 1).astype(np.float64)[:, None]
    zero_b = torch.zeros_like(dv["b"])
    Wd, Wd2 = _layer_weights(plan, None, dv["Ws"], transpose=False)
    raw = _twice(lambda o: F.message_layer_fwd(h_d, plan, Wd, Wd2, zero_b, plan.wlayout, None, None, 0.0, o, h_split=hs,
                                               flags=F.GHF_FLAG_NO_TAIL | F.GHF_FLAG_RAW_SUM | F.GHF_FLAG_ZERO_SRC), h_d, what + " RAW_SUM")
    ref_self, _ = G.layer_ref64(c["h"], c["ei"], c["rel"], np.zeros_like(c["Wm"]), c["Ws"], np.zeros_like(c["b"]), c["gamma"], c["beta"])
    assert_close(raw.cpu().numpy(), ref_self * deg, what + " NO_TAIL | RAW_SUM | ZERO_SRC")
    res = synth.normal(7400 + N, "residual", (N, D))
    res_d = torch.from_numpy(res).to(DEV)
    Wu, Wu2 = _layer_weights(plan, dv["Wm"], None, transpose=False)
    addh = _twice(lambda o: F.message_layer_fwd(res_d, plan, Wu, Wu2, dv["b"], plan.wlayout, None, None, 0.0, o, h_split=hs,
                                                flags=F.GHF_FLAG_NO_TAIL | F.GHF_FLAG_ADD_H | F.GHF_FLAG_ZERO_DST), h_d, what + " ADD_H")
    ref_msg, _ = G.layer_ref64(c["h"], c["ei"], c["rel"], c["Wm"], np.zeros_like(c["Ws"]), c["b"], c["gamma"], c["beta"])
    assert_close(addh.cpu().numpy(), ref_msg + res, what + " NO_TAIL | ADD_H | ZERO_DST")

    # the next layer on the rows and the split rows this tail wrote (reference: the float64 layer on the same fp32 rows)
    nxt = _twice(lambda o: F.message_layer_fwd(plain, plan, W, W2, dv["b"], plan.wlayout, dv["gamma"], dv["beta"], 1e-5, o, h_split=split),
                 h_d, what + " next layer")
    _, ref2 = G.layer_ref64(plain.cpu().numpy(), c["ei"], c["rel"], c["Wm"], c["Ws"], c["b"], c["gamma"], c["beta"])
    assert_close(nxt.cpu().numpy(), ref2, what + " next layer")
    assert int(flag.item()) == 0, f"range guard word {int(flag.item())} on inputs of ordinary dynamic range"


@pytest.mark.parametrize("kind", ["isolated", "hub"])
def test_row_sub_range_leaves_the_other_rows_alone(kind):
    """Rows [bn, 2 bn) of a graph of 2 bn + 5 rows: the launch starts past row 0 and ends on a block boundary."""
    bn = _geometry()[0]
    c = _case(2 * bn + 5, kind)
    plan, dv = c["plan"], c["dev"]
    h_d = dv["h"]
    W, W2 = _layer_weights(plan, dv["Wm"], dv["Ws"], transpose=False)
    hs = _native.split_rows(h_d, plan.wlayout)
    for no_tail in (False, True):
        g, bt = (None, None) if no_tail else (dv["gamma"], dv["beta"])
        kw = dict(h_split=hs, flags=F.GHF_FLAG_NO_TAIL if no_tail else 0)
        full = torch.full_like(h_d, float("nan"))
        F.message_layer_fwd(h_d, plan, W, W2, dv["b"], plan.wlayout, g, bt, 1e-5, full, **kw)
        assert_close(full.cpu().numpy(), c["ref_agg"] if no_tail else c["ref_out"], f"{kind} full launch no_tail={no_tail}")
        part, split = torch.full_like(h_d, 7.0), torch.full_like(hs, 7)
        F.message_layer_fwd(h_d, plan, W, W2, dv["b"], plan.wlayout, g, bt, 1e-5, part, row0=bn, rows=bn,
                            h_split_out=None if no_tail else split, **kw)
        assert torch.equal(part[bn:2 * bn], full[bn:2 * bn]), "the rows of the range differ from the full launch"
        assert bool((part[:bn] == 7.0).all()) and bool((part[2 * bn:] == 7.0).all()), "rows outside the range were written"
        if not no_tail:
            N, per = c["N"], 2 * D
            rows = split.reshape(-1)[: N * per].reshape(N, per)
            want = _native.split_rows(full, plan.wlayout).reshape(-1)
            assert torch.equal(rows[bn:2 * bn], want[: N * per].reshape(N, per)[bn:2 * bn]), "split rows of the range"
            assert bool((rows[:bn] == 7).all()) and bool((rows[2 * bn:] == 7).all()), "split rows outside the range were written"
            scales, wsc = split.reshape(-1)[N * per:].view(torch.int32), want[N * per:].view(torch.int32)     # (the floats' bits)
            assert torch.equal(scales[bn:2 * bn], wsc[bn:2 * bn]), "row scales of the range"
            seven = torch.full((2,), 7, dtype=split.dtype, device=DEV).view(torch.int32)
            assert bool((scales[:bn] == seven).all()) and bool((scales[2 * bn:] == seven).all()), "row scales outside the range were written"


@pytest.mark.parametrize("N,kind", [(n, "isolated") for n in SIZES] + [(581, "hub"), (581, "no_in_edges")])
def test_h_gradient_through_the_backward_instances(N, kind):
    """dh of one layer: two RAW_SUM | ADD_H passes, on the plan (<128, 1>) and on the reversed plan (<128, 2>), against
    float64 autograd through the reference layer (the bounds of test_edge_graphs_gpu.py::test_backward)."""
    c = _case(N, kind)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)                        # noqa: E731
    tp = build_train_plan(t(c["ei"]), t(c["rel"]), c["plan"], D, DEV)
    ins = [c[k] for k in ("h", "Wm", "Ws", "b", "gamma", "beta")]
    gout = synth.normal(77, "gout", (N, D))
    th = torch.from_numpy
    ref_in = [th(a).double().requires_grad_(True) for a in ins]
    _, ref = G.layer_ref64_torch(ref_in[0], th(c["ei"]), th(c["rel"]), *ref_in[1:])
    ref.backward(th(gout).double())
    got = []
    for _ in range(2):
        args = [t(a).requires_grad_(True) for a in ins]
        out = MessageLayerFn.apply(*args, 1e-5, tp)
        out.backward(t(gout))
        got.append((out.detach(), args[0].grad))
    assert_close(got[0][0].cpu().numpy(), ref.detach().numpy(), f"N={N} {kind} training forward")
    gw, gg = ref_in[0].grad.numpy(), got[0][1].cpu().numpy().astype(np.float64)
    scale = float(np.abs(gw).max())
    l2 = float(np.linalg.norm(gg - gw) / max(np.linalg.norm(gw), 1e-30))
    print(f"FIG bx epilogue dh N={N} {kind} rel_l2={l2:.3e} max_abs={np.abs(gg - gw).max():.3e} scale={scale:.3e}")
    assert np.allclose(gg, gw, rtol=2e-4, atol=2e-5 * max(scale, 1.0)), f"dh: max abs err {np.abs(gg - gw).max():.3e} at scale {scale:.3e}"
    assert l2 < 2e-5, f"dh: relative L2 {l2:.3e}"
    assert torch.equal(got[0][1], got[1][1]), "dh: a second backward gives other bits"
