"""The row catalogue of _tail_rows.py through every implementation of the layer's tail, forward and backward: tail_kernel
(ghf_tail_fwd), segment_tail_kernel (ghf_segment_tail_fwd, Y handed in), the fused tails of message_generic_kernel, of
message_bx (both epilogues) and of message_pp (ghf_message_layer_fwd under all-zero weights: the aggregate is exactly 0
and pre = h; and one case with a bias row that cancels h), combine_split4_kernel (a split hub block), and ghf_tail_bwd's two
kernels — including launches long enough for a second and a third visit of the backward's grid-stride loop.

Bounds: _tail_rows.check_forward / check_backward (test_tail_rows_host.py shows a float32 two-pass tail inside them and a
one-pass variance outside).  Every launch is made twice: same bits.  A row's bits do not depend on its neighbours: the same
rows permuted, and each row alone, give the same bits; a NaN or inf row leaves every other row's bits alone."""

import numpy as np
import pytest
import torch

import _edge_graphs as G
import _tail_rows as T
from _util import assert_close
from graph_hypernetwork_forge_amd import _native, synth
from graph_hypernetwork_forge_amd.autograd import _layer_weights
from graph_hypernetwork_forge_amd.plan import RsPlan, build_plan, empty_plan

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SPLIT2H = _native.WLAYOUT_SPLIT2H
EPS = T.LN_EPS
TAIL_FWD_WIDTHS = (3, 20, 64, 65, 100, 128, 257, 1023, 1024)


def _t(a) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _np(t: torch.Tensor) -> np.ndarray:
    return t.cpu().numpy()


def _same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Bit equality of two float32 tensors (NaNs and the sign of zero included)."""
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _perm(K: int) -> np.ndarray:
    """A permutation that moves every row to another lane group, wave and workgroup: reversed, then rotated by 5."""
    return np.roll(np.arange(K)[::-1], 5)


def _flag():
    flag = _native.range_flag(DEV)
    flag.zero_()
    return flag


# ---- ghf_tail_fwd: tail_kernel -----------------------------------------------------------------------------------------

def _tail_fwd(cat: T.Catalogue, dropping: bool, what: str, row0: int = 0, rows=None, fill: float = float("nan")) -> torch.Tensor:
    agg, h, g, b = _t(cat.agg), _t(cat.h), _t(cat.gamma), _t(cat.beta)
    drop = _t(cat.drop) if dropping else None
    like = torch.full((cat.K, cat.d), fill, device=DEV)
    a, b2 = like.clone(), like.clone()
    for o in (a, b2):
        _native.tail_fwd(agg, h, g, b, EPS, o, row0=row0, rows=rows, drop=drop)
    assert _same_bits(a, b2), f"{what}: a second launch gives other bits"
    return a


@pytest.mark.parametrize("dropping", [False, True], ids=["keep", "drop"])
@pytest.mark.parametrize("d", TAIL_FWD_WIDTHS)
def test_tail_fwd(d, dropping):
    cat = T.catalogue(d)
    what = f"tail_fwd d={d} drop={int(dropping)}"
    out = _tail_fwd(cat, dropping, what)
    T.check_forward(_np(out), cat, dropping, what)
    # a row sub-range: the same bits inside, nothing written outside
    lo, n = cat.K // 3, cat.K // 4
    part = _tail_fwd(cat, dropping, what + " sub-range", row0=lo, rows=n, fill=7.0)
    assert _same_bits(part[lo:lo + n], out[lo:lo + n]), f"{what}: the row range differs from the full launch"
    assert bool((part[:lo] == 7.0).all()) and bool((part[lo + n:] == 7.0).all()), f"{what}: rows outside the range were written"
    # row isolation: permuted, and each row alone
    p = _perm(cat.K)
    outp = _tail_fwd(T.take(cat, p), dropping, what + " permuted")
    assert _same_bits(outp, out[_t(p)]), f"{what}: a row's bits depend on its position"
    for i in range(cat.K):
        alone = _tail_fwd(T.take(cat, [i]), dropping, what + f" row {i} alone")
        assert _same_bits(alone[0], out[i]), f"{what}: row {i} ({cat.names[i]}) alone gives other bits"


def _poisoned(cat: T.Catalogue):
    """(catalogue with one row's h NaN and one row's +inf, the two rows)."""
    bad = (cat.row("filler_1"), cat.row("filler_2"))
    h = cat.h.copy()
    h[bad[0]] = np.nan
    h[bad[1]] = np.inf
    return cat._replace(h=h), bad


def _others(K: int, bad) -> torch.Tensor:
    return _t(np.array([i for i in range(K) if i not in bad], dtype=np.int64))


@pytest.mark.parametrize("d", [20, 128, 1023])
def test_tail_fwd_keeps_a_nan_or_inf_row_to_itself(d):
    cat = T.catalogue(d)
    what = f"tail_fwd d={d}"
    clean = _tail_fwd(cat, True, what)
    pois, bad = _poisoned(cat)
    out = _tail_fwd(pois, True, what + " poisoned")
    keep = _others(cat.K, bad)
    assert _same_bits(out[keep], clean[keep]), f"{what}: a NaN / inf row changed another row's bits"
    beta = _t(cat.beta)
    for i in bad:                                    # fmaxf(NaN, 0) = 0: such a row may come out as beta
        ok = ~torch.isfinite(out[i]) | (out[i].view(torch.int32) == beta.view(torch.int32))
        assert bool(ok.all()), f"{what}: the poisoned row {i} is neither non-finite nor beta"


# ---- ghf_segment_tail_fwd: segment_tail_kernel, Y handed in ------------------------------------------------------------

def _segment_case(cat: T.Catalogue):
    """One row of Y per destination (agg is that row: the divisor is 1), and a destination without rows in third place —
    `kink_direct` once more, its aggregate the kernel's own +0.0.  Returns (catalogue of the N = K + 1 destinations, Y, off)."""
    k = cat.row("kink_direct")
    order = list(range(2)) + [k] + list(range(2, cat.K))
    dst = T.take(cat, order)
    agg = dst.agg.copy()
    agg[2] = 0.0
    dst = dst._replace(agg=agg)
    Y = np.delete(dst.agg, 2, axis=0)
    cnt = np.ones(dst.K, dtype=np.int64)
    cnt[2] = 0
    return dst, Y, np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)


def _rs(off: np.ndarray) -> RsPlan:
    z = torch.zeros(1, dtype=torch.int64, device=DEV)
    return RsPlan(src=z, dst=z, ypos=z, slice_tab=torch.zeros(0, 3, dtype=torch.int64, device=DEV), off=_t(off))


def _segment_tail(dst: T.Catalogue, Y: np.ndarray, off: np.ndarray, split: bool, what: str, beta=None, row0: int = 0, rows=None):
    """(h', its split form or None) of two identical launches; the guard word must read as before the call."""
    N, d = dst.K, dst.d
    rs, Y_d, h_d, g_d = _rs(off), _t(Y if Y.size else np.zeros((1, d), dtype=np.float32)), _t(dst.h), _t(dst.gamma)
    b_d = _t(dst.beta if beta is None else beta)
    flag = _flag()
    res = []
    for _ in range(2):
        out = torch.full((N, d), float("nan"), device=DEV)
        hs = _native.alloc_split(N, d, SPLIT2H, DEV).fill_(0x7e7e) if split else None
        _native.segment_tail_fwd(Y_d, rs, h_d, g_d, b_d, EPS, out, row0=row0, rows=rows, h_split_out=hs, exact=False)
        res.append((out, hs))
    assert int(flag.item()) == 0, f"{what}: range guard word {int(flag.item())} after the tail"
    assert _same_bits(res[0][0], res[1][0]), f"{what}: a second launch gives other bits"
    if split:
        assert torch.equal(res[0][1], res[1][1]), f"{what}: a second launch gives other split rows"
        assert torch.equal(res[0][1], _native.split_rows(res[0][0], SPLIT2H)), f"{what}: h_split_out is not split_rows(h')"
    return res[0]


@pytest.mark.parametrize("split", [False, True], ids=["plain", "split"])
@pytest.mark.parametrize("d", G.RS_WIDTHS)
def test_segment_tail_fwd(d, split):
    assert _native.rs_supported(d)
    cat = T.catalogue(d)
    dst, Y, off = _segment_case(cat)
    what = f"segment_tail_fwd d={d} split={int(split)}"
    out, _ = _segment_tail(dst, Y, off, split, what)
    T.check_forward(_np(out), dst, False, what)
    assert _same_bits(out[2], out[3 + cat.row("kink_direct") - 2]), f"{what}: the destination without rows differs from its twin"
    if split:                                        # beta = 0: `dead` is an all-zero row, cut like any other
        zero = np.zeros(d, dtype=np.float32)
        out0, hs0 = _segment_tail(dst, Y, off, True, what + " beta=0", beta=zero)
        assert bool((out0[dst.row("dead")] == 0).all()), f"{what}: dead under beta = 0 is not all zeros"
        T.check_forward(_np(out0), dst._replace(beta=zero), False, what + " beta=0")
    # row isolation: the destinations permuted (one row of Y each, the empty destination last), and each alone
    p = _perm(cat.K)
    per = T.take(cat, p)
    outp, _ = _segment_tail(per, per.agg, np.arange(cat.K + 1, dtype=np.int64), split, what + " permuted")
    want = torch.cat([out[:2], out[3:]])[_t(p)]
    assert _same_bits(outp, want), f"{what}: a row's bits depend on its position"
    for i in range(cat.K):
        one = T.take(cat, [i])
        alone, _ = _segment_tail(one, one.agg, np.array([0, 1], dtype=np.int64), split, what + f" row {i} alone")
        assert _same_bits(alone[0], torch.cat([out[:2], out[3:]])[i]), f"{what}: row {i} ({cat.names[i]}) alone gives other bits"


@pytest.mark.parametrize("d", [128, 640, 1024])
def test_segment_tail_fwd_keeps_a_nan_or_inf_row_to_itself(d):
    cat = T.catalogue(d)
    what = f"segment_tail_fwd d={d}"
    off = np.arange(cat.K + 1, dtype=np.int64)
    clean, _ = _segment_tail(cat, cat.agg, off, False, what)
    pois, bad = _poisoned(cat)
    out, _ = _segment_tail(pois, pois.agg, off, False, what + " poisoned")
    keep = _others(cat.K, bad)
    assert _same_bits(out[keep], clean[keep]), f"{what}: a NaN / inf row changed another row's bits"
    beta = _t(cat.beta)
    for i in bad:
        ok = ~torch.isfinite(out[i]) | (out[i].view(torch.int32) == beta.view(torch.int32))
        assert bool(ok.all()), f"{what}: the poisoned row {i} is neither non-finite nor beta"


# ---- the fused tails: ghf_message_layer_fwd under all-zero weights -------------------------------------------------------
# route -> (d, GHF_KERNEL or None, the geometry the plan must have)
FUSED = {
    "generic20": (20, None, lambda: (1, _native.WLAYOUT_NATURAL, 0, 0)),
    "generic100": (100, None, lambda: (1, _native.WLAYOUT_NATURAL, 0, 0)),
    "bx128": (128, None, lambda: _native.message_config(128)),
    "bx64": (64, "bx", lambda: _native.message_config(64)),
    "pp128": (128, "pp", lambda: _native.message_config(128, "pp")),
    "pp64": (64, None, lambda: _native.exact_config(64)),
}


def _route(route, monkeypatch):
    d, env, cfg = FUSED[route]
    if env:
        monkeypatch.setenv("GHF_KERNEL", env)
    else:
        monkeypatch.delenv("GHF_KERNEL", raising=False)
    cfg = cfg()
    if route.startswith("bx"):
        assert cfg[1] == SPLIT2H, f"{route}: the two-piece kernel"
    if route.startswith("pp"):
        assert cfg[1] == _native.WLAYOUT_FRAG16, f"{route}: the fp32-MFMA kernel"
    if route.startswith("generic"):
        assert not _native.rs_supported(d)
    return d, cfg


def _built(plan, cfg, what):
    assert (plan.block_nodes, plan.wlayout, plan.chunk_rows) == (cfg[0], cfg[1], cfg[2]), f"{what}: the plan is not the route's"
    return plan


def _placement(N: int, K: int, bn: int, cat: T.Catalogue, shift: int) -> np.ndarray:
    """[N] catalogue row of every graph row: the catalogue in turn from `shift`, and the hardest rows at the first and last
    row of a block, on both sides of the half-block boundary and at the end of the short last block."""
    idx = (np.arange(N) + shift) % K
    if bn > 1:
        spots = (0, bn // 2 - 1, bn // 2, bn - 1, bn, N - 1)
        hard = ("dead", "kink_direct", "offset", "const_3", f"one_live_{cat.d - 1}", "kink_cancel")
        for s, name in zip(spots, hard):
            idx[s] = cat.row(name)
    return idx


def _fused_launch(plan, h: np.ndarray, W, W2, bias, gamma, beta, what: str, split: bool):
    """(h', split rows or None): two identical launches; the guard word reads as it did before the call."""
    h_d = _t(h)
    flag = _flag()
    hs = _native.split_rows(h_d, plan.wlayout) if plan.wlayout == SPLIT2H else None     # (cutting `kink` rows may raise the word)
    before = int(flag.item())
    res = []
    for _ in range(2):
        out = torch.full_like(h_d, float("nan"))
        so = _native.alloc_split(h.shape[0], h.shape[1], SPLIT2H, DEV).fill_(0x7e7e) if split else None
        _native.message_layer_fwd(h_d, plan, W, W2, bias, plan.wlayout, gamma, beta, EPS, out, h_split=hs, h_split_out=so)
        res.append((out, so))
    assert int(flag.item()) == before, f"{what}: range guard word {before} -> {int(flag.item())} across the launch"
    assert _same_bits(res[0][0], res[1][0]), f"{what}: a second launch gives other bits"
    if split:
        assert torch.equal(res[0][1], res[1][1]), f"{what}: a second launch gives other split rows"
        assert torch.equal(res[0][1], _native.split_rows(res[0][0], SPLIT2H)), f"{what}: h_split_out is not split_rows(h')"
    return res[0]


def _isolated_graph(N: int, seed: int):
    """Every third row has two in-edges (relations 0 and 1 of R = 3), the others none."""
    dst = np.repeat(np.arange(0, N, 3), 2)
    src = synth.randint(seed, "tailrows/src", dst.size, N)
    return np.stack([src, dst]).astype(np.int64), synth.randint(seed, "tailrows/rel", dst.size, 2), 3


def _zero_weights(plan, R, d):
    z = torch.zeros(R, d, d, device=DEV)
    W, W2 = _layer_weights(plan, z, z, transpose=False)
    return W, W2, torch.zeros(R, d, device=DEV)


@pytest.mark.parametrize("route", list(FUSED))
def test_fused_tail_rows(route, monkeypatch):
    d, cfg = _route(route, monkeypatch)
    bn = cfg[0]
    base = T.catalogue(d)
    cat = T.as_h(base)
    K = cat.K
    N = bn + bn // 2 + 5 if bn > 1 else 2 * K + 3
    ei, rel, R = _isolated_graph(N, 9300 + d)
    plan = _built(build_plan(_t(ei), _t(rel), [""] * R, N, d, DEV), cfg, route)
    assert bn == 1 or plan.n_slots == 0
    W, W2, bias = _zero_weights(plan, R, d)
    g_d, b_d = _t(cat.gamma), _t(cat.beta)
    split = plan.wlayout == SPLIT2H
    outs = {}
    for shift in (0, 17):
        idx = _placement(N, K, bn, cat, shift)
        rows = T.take(cat, idx)
        what = f"fused {route} shift={shift}"
        out, _ = _fused_launch(plan, rows.h, W, W2, bias, g_d, b_d, what, split)
        T.check_forward(_np(out), rows, False, what)
        outs[shift] = (idx, out)
    if split:                                        # beta = 0: `dead` is an all-zero row, cut like any other
        idx = outs[0][0]
        zero = np.zeros(d, dtype=np.float32)
        out0, _ = _fused_launch(plan, T.take(cat, idx).h, W, W2, bias, g_d, _t(zero), f"fused {route} beta=0", True)
        assert bool((out0[_t(np.nonzero(idx == cat.row("dead"))[0])] == 0).all()), f"{route}: dead under beta = 0 is not all zeros"
        T.check_forward(_np(out0), T.take(cat, idx)._replace(beta=zero), False, f"fused {route} beta=0")
    # row isolation: every instance of a catalogue row, wherever it sits in either launch, has the bits of the row alone
    one = empty_plan(1, [""] * R, cfg, DEV)
    for k in range(K):
        alone, _ = _fused_launch(one, cat.h[k:k + 1], W, W2, bias, g_d, b_d, f"fused {route} row {k} alone", split)
        for shift, (idx, out) in outs.items():
            where = _t(np.nonzero(idx == k)[0])
            assert where.numel() >= 1
            assert _same_bits(out[where], alone.expand(where.numel(), d)), \
                f"fused {route} shift={shift}: {cat.names[k]} at rows {where.tolist()} differs from the row alone"


@pytest.mark.parametrize("route", list(FUSED))
def test_fused_tail_with_a_bias_that_cancels_h(route, monkeypatch):
    """One in-edge per chosen destination, from a relation of its own whose bias row is -h_v (or -h_v (1 + 2^-23)) on the
    kink columns: under zero weights the aggregate inside the fused kernel is that bias row, and agg + h lands on or beside 0."""
    d, cfg = _route(route, monkeypatch)
    N = 40
    dsts = np.array([0, 7, 13, 22, 31, 39])
    R = dsts.size + 1
    ei = np.stack([(dsts + 1) % N, dsts]).astype(np.int64)
    rel = np.arange(dsts.size, dtype=np.int64)
    plan = _built(build_plan(_t(ei), _t(rel), [""] * R, N, d, DEV), cfg, route)
    h = synth.normal(9400 + d, "h", (N, d))
    h = np.where(np.abs(h) < 0.05, np.float32(0.5), h).astype(np.float32)
    col = np.arange(d)
    bias = np.zeros((R, d), dtype=np.float32)
    for r, v in enumerate(dsts):
        beside = (-h[v] * np.float32(1.0 + 2.0 ** -23)).astype(np.float32)
        bias[r] = np.where(col % 3 == 0, synth.normal(9400 + d, f"bias{r}", (d,), std=0.5), np.where(col % 3 == 1, -h[v], beside))
    agg = np.zeros((N, d), dtype=np.float32)
    agg[dsts] = bias[:-1]
    pre = agg + h
    assert (pre[dsts][:, col % 3 == 1] == 0).all() and (pre[dsts][:, col % 3 == 2] != 0).all()
    base = T.catalogue(d)
    rows = T.Catalogue(d, [f"row{v}" for v in range(N)], agg, h, np.ones_like(h), base.gamma, base.beta, np.ones(N, dtype=np.int32))
    z = torch.zeros(R, d, d, device=DEV)
    W, W2 = _layer_weights(plan, z, z, transpose=False)
    what = f"fused {route} bias = -h"
    out, _ = _fused_launch(plan, h, W, W2, _t(bias), _t(base.gamma), _t(base.beta), what, plan.wlayout == SPLIT2H)
    T.check_forward(_np(out), rows, False, what)


# ---- combine_split4_kernel: the rows of a split hub block ---------------------------------------------------------------

@pytest.mark.parametrize("route", ["bx128", "bx64"])
def test_combine_split4_rows(route, monkeypatch):
    d, cfg = _route(route, monkeypatch)
    bn, _, _, sc = cfg
    N = bn + bn // 2 + 5
    last0, nl = bn, N - bn
    seed, R = 9500 + d, sc + 3
    rel = np.repeat(np.arange(sc + 2), 2)            # sc + 2 chunks of two rows in the last block: two work items
    dst = np.concatenate([last0 + synth.randint(seed, "hub/dst", rel.size, nl), synth.randint(seed, "hub/dst0", 30, last0)])
    src = synth.randint(seed, "hub/src", dst.size, N)
    rel = np.concatenate([rel, synth.randint(seed, "hub/rel0", 30, 2)])
    plan = _built(build_plan(_t(np.stack([src, dst]).astype(np.int64)), _t(rel.astype(np.int64)), [""] * R, N, d, DEV), cfg, route)
    per_block = np.diff(plan.blk_chunk_off.cpu().numpy())
    assert per_block[-1] == sc + 2 and plan.n_slots == 2, "the last block must be split into two work items"
    cat = T.as_h(T.catalogue(d))
    K = cat.K
    W, W2, bias = _zero_weights(plan, R, d)
    g_d, b_d = _t(cat.gamma), _t(cat.beta)
    first = {}
    for shift in (0, 17):
        idx = _placement(N, K, bn, cat, shift)
        rows = T.take(cat, idx)
        what = f"combine {route} shift={shift}"
        out, _ = _fused_launch(plan, rows.h, W, W2, bias, g_d, b_d, what, True)
        T.check_forward(_np(out), rows, False, what)
        for k in range(K):                           # every instance of a row inside the hub block: the same bits
            where = _t(last0 + np.nonzero(idx[last0:] == k)[0])
            assert where.numel() >= 1
            first.setdefault(k, out[where[0]].clone())
            assert _same_bits(out[where], first[k].expand(where.numel(), d)), \
                f"{what}: {cat.names[k]} at rows {where.tolist()} of the hub block: its bits depend on its position"
    zero = np.zeros(d, dtype=np.float32)
    idx = _placement(N, K, bn, cat, 0)
    out0, _ = _fused_launch(plan, T.take(cat, idx).h, W, W2, bias, g_d, _t(zero), f"combine {route} beta=0", True)
    assert bool((out0[_t(np.nonzero(idx == cat.row("dead"))[0])] == 0).all())


# ---- ghf_tail_bwd -------------------------------------------------------------------------------------------------------

def _splittable(d: int) -> bool:
    return d in (64, 128) or d % 128 == 0


def _off4(a: np.ndarray) -> torch.Tensor:
    """The array on the device, its base 4 bytes past a 16-byte boundary."""
    buf = torch.empty(a.size + 4, dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    v = buf[1:1 + a.size].view(a.shape)
    v.copy_(_t(a))
    assert v.data_ptr() % 16 == 4
    return v


def _tail_bwd(cat: T.Catalogue, go: np.ndarray, dropping: bool, split: bool, what: str, misaligned: bool = False):
    """(dpre, G, Gs, dgamma, dbeta) of two identical launches."""
    put = _off4 if misaligned else _t
    args = (put(go), put(cat.agg), put(cat.h), _t(cat.gamma), EPS, _t(cat.indeg))
    kw = dict(drop=put(cat.drop) if dropping else None, split_layout=SPLIT2H if split else None)
    a = _native.tail_bwd(*args, **kw)
    b = _native.tail_bwd(*args, **kw)
    for x, y, n in zip(a, b, ("dpre", "G", "G_split", "dgamma", "dbeta")):
        if x is not None:
            same = torch.equal(x, y) if x.dtype != torch.float32 else _same_bits(x, y)
            assert same, f"{what}: a second launch gives other bits of {n}"
    return a


def _check_G_split(G_: torch.Tensor, Gs: torch.Tensor, what: str):
    N, d = G_.shape
    ref = _native.split_rows(G_, SPLIT2H)                 # equal as numbers (a dropped entry's zero keeps its sign here)
    assert torch.equal(Gs[:2 * N * d].view(torch.float16), ref[:2 * N * d].view(torch.float16)), f"{what}: the pieces of G"
    assert torch.equal(Gs[2 * N * d:], ref[2 * N * d:]), f"{what}: the row scales of G"


BWD = [(d, dr, sp) for d in tuple(T.V4_LPR) + T.GENERIC_BWD_WIDTHS for dr in (False, True) for sp in (False, True) if not sp or _splittable(d)]


@pytest.mark.parametrize("d,dropping,split", BWD, ids=[f"d{d}-{'drop' if dr else 'keep'}-{'split' if sp else 'plain'}" for d, dr, sp in BWD])
def test_tail_bwd(d, dropping, split):
    """The catalogue through ghf_tail_bwd: the exact claims, G's pieces, row isolation, then dpre / G / dgamma / dbeta
    against the reference under _util.assert_close.

    d = 1024 is where this test found the v4 kernel short: dpre of `one_live_64` at its live column came out 0.0502420 against
    0.0502583, 1.635e-05 off where atol + rtol |ref| allows 1.503e-05.  That entry is dx_j = rstd (gg_j - s1 - xhat_j s2) of a
    row with one live column among 1024: it cancels to 1/500 of its terms and moves by 62 relative errors of rstd, and rstd
    was 4.5 ulps off — the lane that holds the live column added its fifteen mean^2 onto (2.5 - mean)^2 one by one, each
    addition a tie that rounds down.  The kernel now adds a lane's 8 or 16 squared deviations as a tree (row_pieces.h)."""
    full = T.catalogue(d)
    cat = T.take(full, T.backward_rows(full, dropping))
    K = cat.K
    go = T.gout_for(K, d)
    what = f"tail_bwd d={d} drop={int(dropping)} split={int(split)}"
    dpre, G_, Gs, dgamma, dbeta = _tail_bwd(cat, go, dropping, split, what)
    if split:
        _check_G_split(G_, Gs, what)
    # row isolation: permuted (another lane group, wave and workgroup), and each row alone
    p = _perm(K)
    dprep, Gp, *_ = _tail_bwd(T.take(cat, p), go[p], dropping, split, what + " permuted")
    assert _same_bits(dprep, dpre[_t(p)]) and _same_bits(Gp, G_[_t(p)]), f"{what}: a row's dpre / G bits depend on its position"
    for i in range(K):
        da, Ga, *_ = _tail_bwd(T.take(cat, [i]), go[i:i + 1], dropping, split, what + f" row {i} alone")
        assert _same_bits(da[0], dpre[i]) and _same_bits(Ga[0], G_[i]), f"{what}: row {i} ({cat.names[i]}) alone gives other bits"
    T.check_backward(_np(dpre), _np(G_), _np(dgamma), _np(dbeta), cat, go, dropping, what)


@pytest.mark.parametrize("dropping", [False, True], ids=["keep", "drop"])
def test_tail_bwd_generic_kernel_at_128_from_a_misaligned_base(dropping):
    """Operands 4 bytes past a 16-byte boundary send d = 128 to tail_bwd_kernel: the same bounds as the v4 run on the same data."""
    d = 128
    full = T.catalogue(d)
    cat = T.take(full, T.backward_rows(full, dropping))
    go = T.gout_for(cat.K, d)
    for mis in (False, True):
        what = f"tail_bwd d=128 drop={int(dropping)} {'generic kernel (misaligned)' if mis else 'v4 kernel'}"
        dpre, G_, _, dgamma, dbeta = _tail_bwd(cat, go, dropping, False, what, misaligned=mis)
        T.check_backward(_np(dpre), _np(G_), _np(dgamma), _np(dbeta), cat, go, dropping, what)


@pytest.mark.parametrize("d", [20, 32, 128, 1024])
def test_tail_bwd_keeps_a_nan_or_inf_row_to_itself(d):
    full = T.catalogue(d)
    cat = T.take(full, T.backward_rows(full, True))
    go = T.gout_for(cat.K, d)
    what = f"tail_bwd d={d}"
    dpre, G_, *_ = _tail_bwd(cat, go, True, False, what)
    pois, bad = _poisoned(cat)
    dp, Gp, *_ = _tail_bwd(pois, go, True, False, what + " poisoned")
    keep = _others(cat.K, bad)
    assert _same_bits(dp[keep], dpre[keep]) and _same_bits(Gp[keep], G_[keep]), f"{what}: a NaN / inf row changed another row's dpre / G"
    for i in bad:                                    # NaN > 0 is false: such a row may come out as zeros
        for x in (dp[i], Gp[i]):
            assert bool((~torch.isfinite(x) | (x == 0)).all()), f"{what}: the poisoned row {i} is neither non-finite nor zero"


# second and later visits of the grid-stride loop: (d, v4 kernel?) at the smallest N with a short third visit
VISITS = [(20, False), (32, True), (128, True), (1024, True)]
BASE_ROWS = 61                                           # distinct rows the long launches repeat (coprime to every rows-per-visit)


@pytest.mark.parametrize("only", ["visits_1_and_2", "last_partial_visit"])
@pytest.mark.parametrize("d,v4", VISITS, ids=[f"d{d}" for d, _ in VISITS])
def test_tail_bwd_later_visits(d, v4, only):
    """g_out holds small integers on the rows of later visits only: dbeta is then an exact integer per column — a dropped or
    doubled visit is a wrong integer — and dgamma the same sum weighted by xhat.  The rows repeat BASE_ROWS distinct ones,
    so the float64 reference is one small pass and a matrix product."""
    N = T.third_visit_N(d, v4)
    assert N == {20: 16389, 32: 131077, 128: 32773, 1024: 16389}[d]
    visit = T.visit_of(N, d, v4)
    assert visit.max() == 2 and (visit == 2).sum() == 5 and N % T.rows_per_visit(d, v4) != 0
    rows = visit >= 1 if only == "visits_1_and_2" else visit == 2
    seed = 9600 + d
    agg0, h0 = synth.normal(seed, "agg", (BASE_ROWS, d)), synth.normal(seed, "h", (BASE_ROWS, d))
    gamma = (0.5 + synth.uniform01(seed, "gamma", d)).astype(np.float32)
    which = np.arange(N) % BASE_ROWS
    go = np.zeros((N, d), dtype=np.float32)
    go[rows] = (synth.randint(seed, "go", int(rows.sum()) * d, 7) - 3).reshape(-1, d).astype(np.float32)
    indeg = (np.arange(N) % 5).astype(np.int32)
    what = f"tail_bwd d={d} N={N} g_out on {only}"
    args = (_t(go), _t(agg0[which]), _t(h0[which]), _t(gamma), EPS, _t(indeg))
    dpre, G_, _, dgamma, dbeta = _native.tail_bwd(*args)
    again = _native.tail_bwd(*args)
    for x, y in zip((dpre, G_, dgamma, dbeta), (again[0], again[1], again[3], again[4])):
        assert _same_bits(x, y), f"{what}: a second launch gives other bits"
    want_dbeta = go.astype(np.float64).sum(axis=0)
    assert np.abs(want_dbeta).max() < 2 ** 24
    assert np.array_equal(_np(dbeta).astype(np.float64), want_dbeta), f"{what}: dbeta is not the integer column sum"
    ref0 = T.tail_ref(agg0, h0, gamma, np.zeros(d, dtype=np.float32))
    S = np.stack([go[b::BASE_ROWS].sum(axis=0, dtype=np.float64) for b in range(BASE_ROWS)])   # per base row: exact integers
    want_dgamma = (S * ref0["xhat"]).sum(axis=0)
    scale = float(rows.sum()) ** 0.5                      # the column sums grow like sqrt(rows with a gradient)
    print(f"FIG tail {what} dgamma_max_err={np.abs(_np(dgamma) - want_dgamma).max():.3e} scale={scale:.1f}")
    assert_close(_np(dgamma) / scale, want_dgamma / scale, what + " dgamma")
    assert bool((dpre[_t(np.nonzero(~rows)[0])] == 0).all()), f"{what}: dpre is nonzero on a row without a gradient"
    # dpre / G of rows from every visit, the last partial one whole: the bits of the same rows in a short launch, which is
    # itself held to the reference
    pick = np.unique(np.concatenate([np.nonzero(visit == 2)[0], np.nonzero(rows)[0][:: max(int(rows.sum()) // 150, 1)][:150],
                                     np.arange(0, N, max(N // 40, 1))]))
    small = T.Catalogue(d, [f"row{v}" for v in pick], agg0[which[pick]], h0[which[pick]], np.ones((pick.size, d), dtype=np.float32), gamma,
                        np.zeros(d, dtype=np.float32), indeg[pick])
    dps, Gs_, _, dgs, dbs = _tail_bwd(small, go[pick], False, False, what + " picked rows")
    sel = _t(pick)
    assert _same_bits(dps, dpre[sel]) and _same_bits(Gs_, G_[sel]), f"{what}: rows of the long launch differ from the same rows in a short one"
    T.check_backward(_np(dps), _np(Gs_), _np(dgs), _np(dbs), small, go[pick], False, what + " picked rows")
