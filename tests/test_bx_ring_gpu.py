"""The chunk loop of message_bx_kernel (the ring of four A tiles: chunk j's source rows in tile j mod 4, its destination rows
and then its staged rows in tile (j - 1) mod 4) at the chunk counts at which the ring can go wrong: a last block of 1, 2, 3, 4,
5, 8 and 9 chunks — prologue and epilogue meet, the ring wraps once and twice — alone and behind an ordinary block; chunks of
1, 15, 16, 17, 64, 65 and 76 rows and a relation of 77 rows (two chunks of one relation back to back; hidden 64 cuts at 64
rows, so its 65-, 76- and 77-row relations are two chunks each); hidden 128 and 64; the forward instance and both backward
instances (ZERO_SRC | RAW_SUM and ZERO_DST | ADD_H); and a two-layer chain whose second layer gathers the split rows the
first one wrote.

What this file checks is the ring's indexing — which tile a role reads or writes at which chunk.  Its graphs are one or two
workgroups on an otherwise idle GPU: it says nothing about the flag hand-shakes between the waves (the order in which late
waves publish and read), which are argued in the kernel's header, not tested here.

The plan's chunk counts and chunk lengths are asserted on the host, so that a case cannot silently turn into another one.
Everything is compared with the float64 layer of _edge_graphs.py at the tolerance of test_bx_epilogue_gpu.py
(_util.assert_close), and every launch is repeated: same bits."""

import numpy as np
import pytest
import torch

import _edge_graphs as G
from _util import assert_close
from graph_hypernetwork_forge_amd import _native, synth
from graph_hypernetwork_forge_amd.autograd import _layer_weights
from graph_hypernetwork_forge_amd.plan import build_plan

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F = _native
GEOMETRY = {128: (384, 76), 64: (192, 64)}          # d -> (block rows, chunk rows) this file's cases are made for
LAST_CHUNKS = [1, 2, 3, 4, 5, 8, 9]
# rows of the last block's (block, relation) groups, per chunk rows of the geometry and chunk count of the block
GROUPS = {
    76: {1: [76], 2: [77], 3: [1, 77], 4: [15, 16, 17, 64], 5: [65, 77, 1, 15], 8: [1, 15, 16, 17, 64, 65, 76, 1],
         9: [1, 15, 16, 17, 64, 65, 76, 77]},
    64: {1: [64], 2: [77], 3: [1, 65], 4: [15, 16, 17, 64], 5: [76, 77, 1], 8: [1, 15, 16, 17, 64, 65, 1],
         9: [1, 15, 16, 17, 64, 65, 76]},
}
FIRST_BLOCK = [40, 3]                               # the ordinary block in front: two relations, one chunk each


def _cut(n, cr):
    """The chunk lengths a group of n rows is cut into."""
    return [cr] * (n // cr) + ([n % cr] if n % cr else [])


def _groups_for(k, cr):
    return GROUPS[cr][k]


def _graph(d, k, blocks):
    """(N, edge_index, rel, R, chunk lengths of every block in plan order)."""
    bn, cr = GEOMETRY[d]
    N = blocks * bn - (5 if blocks == 2 else 0)      # (the last of two blocks is a partial one)
    last0 = (blocks - 1) * bn
    nl = N - last0
    sizes = _groups_for(k, cr)
    seed, tag = 9300 + d + k, f"bxring/{d}/{k}/{blocks}"
    src, dst, rel, lens = [], [], [], [[] for _ in range(blocks)]
    if blocks == 2:
        for r, n in enumerate(FIRST_BLOCK):
            dst.append(synth.randint(seed, f"{tag}/dst0/{r}", n, bn))
            rel.append(np.full(n, r))
            lens[0] += _cut(n, cr)
    for r, n in enumerate(sizes):                    # distinct destinations, spread over the four helper waves' rows
        dst.append(last0 + (11 * r + 5 * np.arange(n)) % nl)
        rel.append(np.full(n, r))
        lens[-1] += _cut(n, cr)
    dst, rel = np.concatenate(dst).astype(np.int64), np.concatenate(rel).astype(np.int64)
    src = synth.randint(seed, tag + "/src", dst.size, N)
    order = np.argsort(synth.raw_u64(seed, tag + "/order", dst.size), kind="stable")
    return N, np.stack([src, dst])[:, order], rel[order], max(len(sizes), 2) + 1, lens


def test_the_cases_cover_what_they_claim():
    """Host arithmetic only: over LAST_CHUNKS the cases hold every chunk length and the back-to-back pair."""
    for d, (bn, cr) in GEOMETRY.items():
        seen, pairs = set(), set()
        for k in LAST_CHUNKS:
            sizes = _groups_for(k, cr)
            assert sum(len(_cut(n, cr)) for n in sizes) == k
            for n in sizes:
                seen.update(_cut(n, cr))
                if n > cr:
                    pairs.add(tuple(_cut(n, cr)))
        want = {1, 15, 16, 17, 64, 65, 76} if cr == 76 else {1, 15, 16, 17, 64, 12, 13}
        assert want <= seen, f"d={d}: chunk lengths {sorted(want - seen)} are in no case"
        assert (cr, 77 - cr) in pairs, f"d={d}: no relation of 77 rows"
        if cr == 64:
            assert {(64, 1), (64, 12), (64, 13)} <= pairs


_CACHE: dict = {}


def _case(d, k, blocks):
    """Graph, inputs, plan and the float64 references, made once per case and never modified (GHF_KERNEL is set by the test)."""
    key = (d, k, blocks)
    if key not in _CACHE:
        bn, cr = GEOMETRY[d]
        cfg = _native.message_config(d, "bx")
        assert (cfg[0], cfg[1], cfg[2]) == (bn, _native.WLAYOUT_SPLIT2H, cr), "the cases of this file are made for this geometry"
        N, ei, rel, R, lens = _graph(d, k, blocks)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)                    # noqa: E731
        plan = build_plan(t(ei), t(rel), [""] * R, N, d, DEV)
        assert (plan.block_nodes, plan.wlayout, plan.chunk_rows) == (bn, cfg[1], cr) and plan.n_slots == 0
        # the plan's cut, on the host: chunks per block, and every chunk's relation and rows in order
        per_block = np.diff(plan.blk_chunk_off.cpu().numpy())
        assert per_block.tolist() == [len(x) for x in lens] and per_block[-1] == k, f"chunks per block {per_block.tolist()}"
        tab = plan.chunk_tab.cpu().numpy()[: 2 * int(per_block.sum())].reshape(-1, 2)
        assert (tab[:, 1] & 127).tolist() == [n for x in lens for n in x], "chunk lengths"
        assert int((tab[:, 1] & 127).sum()) == rel.size, "rows of all chunks"
        rels = (tab[:, 1] >> 8)[-k:]
        twins = [i for i in range(1, k) if rels[i] == rels[i - 1]]
        assert len(twins) == sum(n > cr for n in _groups_for(k, cr)), "two chunks of one relation back to back"
        c = G.Case(f"ring_{d}_{k}_{blocks}", N, ei, rel, R, ())
        h, Wm, Ws, b, gamma, beta = G.layer_inputs(c, d, 7500 + k)
        ref_agg, ref_out = G.layer_ref64(h, ei, rel, Wm, Ws, b, gamma, beta)
        _CACHE[key] = dict(N=N, ei=ei, rel=rel, R=R, h=h, Wm=Wm, Ws=Ws, b=b, gamma=gamma, beta=beta, plan=plan,
                           indeg=np.bincount(ei[1], minlength=N), ref_agg=ref_agg, ref_out=ref_out,
                           dev={n: t(v) for n, v in dict(h=h, Wm=Wm, Ws=Ws, b=b, gamma=gamma, beta=beta).items()})
    return _CACHE[key]


def _twice(launch, like, what):
    """Run `launch(out)` twice into NaN-filled tensors: the same bits both times; returns the first."""
    a, b = torch.full_like(like, float("nan")), torch.full_like(like, float("nan"))
    launch(a)
    launch(b)
    assert torch.equal(a, b), f"{what}: a second launch gives other bits"
    return a


@pytest.mark.parametrize("blocks", [1, 2])
@pytest.mark.parametrize("k", LAST_CHUNKS)
@pytest.mark.parametrize("d", [128, 64])
def test_ring_chunk_counts(d, k, blocks, monkeypatch):
    monkeypatch.setenv("GHF_KERNEL", "bx")
    c = _case(d, k, blocks)
    plan, dv, N = c["plan"], c["dev"], c["N"]
    flag = _native.range_flag(DEV)
    flag.zero_()
    h_d = dv["h"]
    hs = _native.split_rows(h_d, plan.wlayout)
    what = f"d={d} chunks={k} blocks={blocks}"

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
    res = synth.normal(7600 + k, "residual", (N, d))
    res_d = torch.from_numpy(res).to(DEV)
    Wu, Wu2 = _layer_weights(plan, dv["Wm"], None, transpose=False)
    addh = _twice(lambda o: F.message_layer_fwd(res_d, plan, Wu, Wu2, dv["b"], plan.wlayout, None, None, 0.0, o, h_split=hs,
                                                flags=F.GHF_FLAG_NO_TAIL | F.GHF_FLAG_ADD_H | F.GHF_FLAG_ZERO_DST), h_d, what + " ADD_H")
    ref_msg, _ = G.layer_ref64(c["h"], c["ei"], c["rel"], c["Wm"], np.zeros_like(c["Ws"]), c["b"], c["gamma"], c["beta"])
    assert_close(addh.cpu().numpy(), ref_msg + res, what + " NO_TAIL | ADD_H | ZERO_DST")
    assert int(flag.item()) == 0, f"range guard word {int(flag.item())} on inputs of ordinary dynamic range"
