"""The helpers' split fold of message_bx_kernel: a helper wave folds the first eight of its staged rows of chunk k-1, waits for
"phase 0 of chunk k read", requests the destination rows of chunk k+1 and the descriptor pipeline's loads, and folds the rest
of its rows beside those round trips.  What can go wrong is a row folded twice or not at all around the split, a wave that
has nothing to fold and spins on the flag from the chunk's start, and the requests landing among the fold's LDS reads.

Cases, by a helper wave's rows per chunk (LENGTHS: only a first part; a first part exactly full; a second part of 1, 8, 9 rows;
the longest there is, a whole chunk):
  * one wave's rows: a block whose six relations have those lengths, every destination among ONE wave's nodes — the other three
    waves fold nothing;
  * alternating waves: a block of twelve chunks, chunk r in wave r mod 4, the lengths cycling — every wave meets an empty fold
    right behind a long one and the other way round;
  * every wave past the split: full chunks spread evenly over the four waves;
  * under load: one workgroup per CU (hidden 128) / two per CU (hidden 64) of a uniform graph, the only case in which late waves
    of other workgroups share a CU's LDS and memory path.  Run once, not looped.

The plan's cut is asserted on the host (chunks per block, chunk lengths, every helper wave's rows per chunk computed from the
destinations), so that a case cannot silently turn into another one.  Everything is compared with the float64 layer of
_edge_graphs.py at the tolerance of test_bx_epilogue_gpu.py (_util.assert_close), and every launch is repeated: same bits."""

import numpy as np
import pytest
import torch

import _edge_graphs as G
from _util import assert_close
from graph_hypernetwork_forge_amd import _native, synth
from graph_hypernetwork_forge_amd.autograd import _layer_weights
from graph_hypernetwork_forge_amd.plan import build_plan

DEV = torch.device("cuda:0")
F = _native
GEOMETRY = {128: (384, 76, 96), 64: (192, 64, 48)}      # d -> (block rows, chunk rows, nodes per helper wave)
SPLIT = 8                                               # rows a wave folds before its requests


def _lengths(cr):
    return [1, 8, 9, 16, 17, cr]


def _one_wave(d, hw):
    """One block, six relations of LENGTHS rows, every destination among helper wave hw's nodes.  -> (dst, rel, want)"""
    bn, cr, npw = GEOMETRY[d]
    dst, rel, want = [], [], []
    for r, n in enumerate(_lengths(cr)):
        dst.append(npw * hw + (7 * r + 5 * np.arange(n)) % npw)
        rel.append(np.full(n, r))
        want.append([n if w == hw else 0 for w in range(4)])
    return np.concatenate(dst), np.concatenate(rel), want


def _alternating(d):
    """One block of twelve chunks: chunk r's rows among the nodes of wave r mod 4, the lengths cycling."""
    bn, cr, npw = GEOMETRY[d]
    L = _lengths(cr)
    dst, rel, want = [], [], []
    for r in range(12):
        n, hw = L[r % len(L)], r % 4
        dst.append(npw * hw + (3 * r + 5 * np.arange(n)) % npw)
        rel.append(np.full(n, r))
        want.append([n if w == hw else 0 for w in range(4)])
    return np.concatenate(dst), np.concatenate(rel), want


def _every_wave(d):
    """One block of three full chunks, a quarter of each chunk's rows in every wave (more than SPLIT)."""
    bn, cr, npw = GEOMETRY[d]
    dst, rel, want = [], [], []
    for r in range(3):
        i = np.arange(cr)
        dst.append(npw * (i % 4) + (5 * (i // 4) + r) % npw)
        rel.append(np.full(cr, r))
        want.append([cr // 4] * 4)
    return np.concatenate(dst), np.concatenate(rel), want


CRAFTED = {"wave0": lambda d: _one_wave(d, 0), "wave1": lambda d: _one_wave(d, 1), "wave2": lambda d: _one_wave(d, 2),
           "wave3": lambda d: _one_wave(d, 3), "alternating": _alternating, "every_wave": _every_wave}


def _wave_rows(d, dst, rel):
    """From the destinations alone: per chunk in plan order (relations ascending, a relation's rows by destination, cut every
    chunk-rows rows) the rows of each helper wave.  One block."""
    bn, cr, npw = GEOMETRY[d]
    out = []
    for r in np.unique(rel):
        nodes = np.sort(dst[rel == r])
        for c0 in range(0, nodes.size, cr):
            out.append(np.bincount(nodes[c0:c0 + cr] // npw, minlength=4).tolist())
    return out


def test_the_cases_hold_the_row_counts_they_claim():
    """Host arithmetic only: every case's per-wave row counts are what its builder says, and over the cases a wave's fold has
    no row, 1 .. SPLIT rows (no second part), and a second part of 1, 8, 9 and the most rows, alone and beside others."""
    for d, (bn, cr, npw) in GEOMETRY.items():
        L = _lengths(cr)
        for hw in range(4):
            dst, rel, want = _one_wave(d, hw)
            got = _wave_rows(d, dst, rel)
            assert got == want and [g[hw] for g in got] == L
            assert all(g[w] == 0 for g in got for w in range(4) if w != hw)
            assert dst.min() >= npw * hw and dst.max() < npw * (hw + 1)
            assert [max(n - SPLIT, 0) for n in L] == [0, 0, 1, 8, 9, cr - SPLIT]
        dst, rel, want = _alternating(d)
        got = _wave_rows(d, dst, rel)
        assert got == want and len(got) == 12
        for w in range(4):
            mine = [g[w] for g in got]
            assert sum(n > 0 for n in mine) == 3
            # an empty fold right behind a long one (a second part) and a long one right behind an empty one
            assert any(a > SPLIT and b == 0 for a, b in zip(mine, mine[1:])), (d, w, mine)
            assert any(a == 0 and b > SPLIT for a, b in zip(mine, mine[1:])), (d, w, mine)
        assert {n for g in got for n in g} == set(L) | {0}
        dst, rel, want = _every_wave(d)
        got = _wave_rows(d, dst, rel)
        assert got == want and all(n > SPLIT for g in got for n in g) and cr % 4 == 0


_CACHE: dict = {}


def _reference(key, d, N, ei, rel, R, seed):
    c = G.Case(key, N, ei, rel, R, ())
    h, Wm, Ws, b, gamma, beta = G.layer_inputs(c, d, seed)
    ref_agg, ref_out = G.layer_ref64(h, ei, rel, Wm, Ws, b, gamma, beta)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)                    # noqa: E731
    return dict(N=N, ei=ei, rel=rel, R=R, h=h, Wm=Wm, Ws=Ws, b=b, gamma=gamma, beta=beta, ref_agg=ref_agg, ref_out=ref_out,
                indeg=np.bincount(ei[1], minlength=N), dev={n: t(v) for n, v in dict(h=h, Wm=Wm, Ws=Ws, b=b, gamma=gamma, beta=beta).items()})


def _check_geometry(d):
    bn, cr, npw = GEOMETRY[d]
    cfg = _native.message_config(d, "bx")
    assert (cfg[0], cfg[1], cfg[2]) == (bn, _native.WLAYOUT_SPLIT2H, cr) and bn == 4 * npw, "the cases of this file are made for this geometry"
    return cfg


def _crafted(d, name):
    """Graph, inputs, plan and the float64 references, made once per case and never modified (GHF_KERNEL is set by the test)."""
    key = (d, name)
    if key not in _CACHE:
        bn, cr, npw = GEOMETRY[d]
        cfg = _check_geometry(d)
        dst, rel, want = CRAFTED[name](d)
        N, R = bn, int(rel.max()) + 2
        seed, tag = 9500 + d, f"bxfold/{d}/{name}"
        src = synth.randint(seed, tag + "/src", dst.size, N)
        order = np.argsort(synth.raw_u64(seed, tag + "/order", dst.size), kind="stable")
        ei, rel = np.stack([src, dst]).astype(np.int64)[:, order], rel.astype(np.int64)[order]
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)                    # noqa: E731
        plan = build_plan(t(ei), t(rel), [""] * R, N, d, DEV)
        assert (plan.block_nodes, plan.wlayout, plan.chunk_rows) == (bn, cfg[1], cr) and plan.n_slots == 0
        # the plan's cut, on the host: one block, its chunks' lengths in order, and each helper wave's rows per chunk
        per_block = np.diff(plan.blk_chunk_off.cpu().numpy())
        assert per_block.tolist() == [len(want)], f"chunks per block {per_block.tolist()}"
        tab = plan.chunk_tab.cpu().numpy()[: 2 * len(want)].reshape(-1, 2)
        assert (tab[:, 1] & 127).tolist() == [sum(w) for w in want], "chunk lengths"
        assert _wave_rows(d, ei[1], rel) == want, "rows per helper wave and chunk"
        c = _reference(f"fold_{d}_{name}", d, N, ei, rel, R, 7700 + len(want))
        c["plan"] = plan
        _CACHE[key] = c
    return _CACHE[key]


def _twice(launch, like, what):
    """Run `launch(out)` twice into NaN-filled tensors: the same bits both times; returns the first."""
    a, b = torch.full_like(like, float("nan")), torch.full_like(like, float("nan"))
    launch(a)
    launch(b)
    assert torch.equal(a, b), f"{what}: a second launch gives other bits"
    return a


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CRAFTED))
@pytest.mark.parametrize("d", [128, 64])
def test_fold_split_row_counts(d, name, monkeypatch):
    monkeypatch.setenv("GHF_KERNEL", "bx")
    c = _crafted(d, name)
    plan, dv, N = c["plan"], c["dev"], c["N"]
    flag = _native.range_flag(DEV)
    flag.zero_()
    h_d = dv["h"]
    hs = _native.split_rows(h_d, plan.wlayout)
    what = f"d={d} {name}"

    # forward instance <d, 0>: the full tail with the split rows for a next layer, then that layer on them
    W, W2 = _layer_weights(plan, dv["Wm"], dv["Ws"], transpose=False)
    split = torch.zeros_like(hs)
    out = _twice(lambda o: F.message_layer_fwd(h_d, plan, W, W2, dv["b"], plan.wlayout, dv["gamma"], dv["beta"], 1e-5, o, h_split=hs,
                                               h_split_out=split), h_d, what + " forward")
    assert_close(out.cpu().numpy(), c["ref_out"], what + " forward")
    assert torch.equal(split, _native.split_rows(out, plan.wlayout)), what + ": h_split_out is not split_rows(h')"
    nxt = _twice(lambda o: F.message_layer_fwd(out, plan, W, W2, dv["b"], plan.wlayout, dv["gamma"], dv["beta"], 1e-5, o, h_split=split),
                 h_d, what + " second layer")
    _, ref2 = G.layer_ref64(out.cpu().numpy(), c["ei"], c["rel"], c["Wm"], c["Ws"], c["b"], c["gamma"], c["beta"])
    assert_close(nxt.cpu().numpy(), ref2, what + " second layer")

    # backward instances: the raw sum of the destination half (<d, 1>), the mean of the source half plus a residual (<d, 2>)
    deg = np.maximum(c["indeg"], 1).astype(np.float64)[:, None]
    zero_b = torch.zeros_like(dv["b"])
    Wd, Wd2 = _layer_weights(plan, None, dv["Ws"], transpose=False)
    raw = _twice(lambda o: F.message_layer_fwd(h_d, plan, Wd, Wd2, zero_b, plan.wlayout, None, None, 0.0, o, h_split=hs,
                                               flags=F.GHF_FLAG_NO_TAIL | F.GHF_FLAG_RAW_SUM | F.GHF_FLAG_ZERO_SRC), h_d, what + " RAW_SUM")
    ref_self, _ = G.layer_ref64(c["h"], c["ei"], c["rel"], np.zeros_like(c["Wm"]), c["Ws"], np.zeros_like(c["b"]), c["gamma"], c["beta"])
    assert_close(raw.cpu().numpy(), ref_self * deg, what + " NO_TAIL | RAW_SUM | ZERO_SRC")
    res = synth.normal(7800 + d, "residual", (N, d))
    res_d = torch.from_numpy(res).to(DEV)
    Wu, Wu2 = _layer_weights(plan, dv["Wm"], None, transpose=False)
    addh = _twice(lambda o: F.message_layer_fwd(res_d, plan, Wu, Wu2, dv["b"], plan.wlayout, None, None, 0.0, o, h_split=hs,
                                                flags=F.GHF_FLAG_NO_TAIL | F.GHF_FLAG_ADD_H | F.GHF_FLAG_ZERO_DST), h_d, what + " ADD_H")
    ref_msg, _ = G.layer_ref64(c["h"], c["ei"], c["rel"], c["Wm"], np.zeros_like(c["Ws"]), c["b"], c["gamma"], c["beta"])
    assert_close(addh.cpu().numpy(), ref_msg + res, what + " NO_TAIL | ADD_H | ZERO_DST")
    assert int(flag.item()) == 0, f"range guard word {int(flag.item())} on inputs of ordinary dynamic range"


LOAD_BLOCKS = {128: 256, 64: 512}                       # one workgroup per CU at hidden 128, two per CU at hidden 64 (256 CUs)


@pytest.mark.gpu
@pytest.mark.parametrize("d", [128, 64])
def test_fold_split_under_load(d, monkeypatch):
    """Every CU busy: the forward instance on a uniform graph, every row against the float64 layer, two launches with equal bits."""
    monkeypatch.setenv("GHF_KERNEL", "bx")
    bn, cr, npw = GEOMETRY[d]
    cfg = _check_geometry(d)
    N, R = LOAD_BLOCKS[d] * bn + 7, 17                  # 16 relations in use (a case's rel is never R - 1)
    E, seed, tag = 6 * N, 9600 + d, f"bxfold/load/{d}"
    ei = np.stack([synth.randint(seed, tag + "/src", E, N), synth.randint(seed, tag + "/dst", E, N)]).astype(np.int64)
    rel = synth.randint(seed, tag + "/rel", E, R - 1).astype(np.int64)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)                        # noqa: E731
    plan = build_plan(t(ei), t(rel), [""] * R, N, d, DEV)
    assert (plan.block_nodes, plan.wlayout, plan.chunk_rows) == (bn, cfg[1], cr)
    per_block = np.diff(plan.blk_chunk_off.cpu().numpy())
    assert per_block.size == LOAD_BLOCKS[d] + 1 and per_block[:-1].min() >= R - 1, "every full block has a chunk per relation"
    tab = plan.chunk_tab.cpu().numpy()[: 2 * int(per_block.sum())].reshape(-1, 2)
    assert int((tab[:, 1] & 127).sum()) == E and int((tab[:, 1] & 127).max()) == cr, "rows of all chunks; full chunks among them"
    c = _reference(f"fold_load_{d}", d, N, ei, rel, R, 7900 + d)
    dv = c["dev"]
    flag = _native.range_flag(DEV)
    flag.zero_()
    hs = _native.split_rows(dv["h"], plan.wlayout)
    W, W2 = _layer_weights(plan, dv["Wm"], dv["Ws"], transpose=False)
    out = _twice(lambda o: F.message_layer_fwd(dv["h"], plan, W, W2, dv["b"], plan.wlayout, dv["gamma"], dv["beta"], 1e-5, o, h_split=hs),
                 dv["h"], f"d={d} under load")
    assert_close(out.cpu().numpy(), c["ref_out"], f"d={d} under load")
    assert int(flag.item()) == 0, f"range guard word {int(flag.item())} on inputs of ordinary dynamic range"
