"""The numpy restatement of ghf_weights_pack_rs (tests/_rs_pack_ref.py) and its crafted matrices are what they claim, shown
without a GPU: the scaling is exact and lifts every relation's largest magnitude into [2^13, 2^14), the two pieces reproduce
the scaled value to the 22 bits include/ghf.h promises, the layout is the transposed one, and every guard matrix has exactly
the per-tile counts its name says — in one tile only."""

import numpy as np
import pytest
import torch

import _edge_graphs as G
import _rs_pack_ref as P
from _util import ATOL, REL_L2, RTOL
from oracle import hypergnn_oracle as O

WIDTHS = G.RS_WIDTHS
GUARD_WIDTHS = (128, 384, 1024)


@pytest.mark.parametrize("d", WIDTHS)
def test_the_scaling_is_exact_and_the_pieces_keep_22_bits(d):
    Wm, Ws = P.ordinary_weights(d)
    s = P.shifts(Wm, Ws)
    mx = [max(float(np.abs(Wm[r]).max()), float(np.abs(Ws[r]).max())) for r in range(3)]
    assert s.tolist() == [14 - np.frexp(m)[1] for m in mx] and s[1] == 12, s     # (frexp: m = f 2^e, 0.5 <= f < 1; relation 1: 3.0)
    assert float(np.abs(Wm[1]).max()) < 3.0 == mx[1] and not Wm[2].any()
    top = np.zeros(3)
    for W in (Wm, Ws):
        xs = P.scaled(W, s)
        assert np.array_equal(xs.astype(np.float64), W.astype(np.float64) * np.exp2(s.astype(np.float64))[:, None, None]), "x 2^s is not exact"
        top = np.maximum(top, np.abs(xs).reshape(3, -1).max(axis=1))
    assert ((top >= 2.0 ** 13) & (top < 2.0 ** 14)).all(), top
    for W in (Wm, Ws):
        xs = P.scaled(W, s)
        hi, lo = P.pieces(xs)
        err = np.abs(hi.astype(np.float64) + lo.astype(np.float64) - xs.astype(np.float64))
        near = np.abs(xs) >= (top * 2.0 ** -14)[:, None, None]                   # within 2^-14 of the relation's largest
        assert near.sum() > 0.99 * np.count_nonzero(W)                            # (the check below covers all but a few entries)
        assert (err[near] <= np.broadcast_to((top * 2.0 ** -22)[:, None, None], err.shape)[near]).all()
        assert (err[near] <= 2.0 ** -22 * np.abs(xs.astype(np.float64))[near]).all(), "common.h: |eps| <= 2^-22 |x 2^s|"
        assert np.isfinite(hi.astype(np.float32)).all() and np.isfinite(lo.astype(np.float32)).all()
    assert P.guard_word(Wm, Ws) == 0


def test_the_layout_is_transposed_pieces_per_half_then_the_scales():
    d = 128
    Wm, Ws = P.ordinary_weights(d)
    buf = P.pack_rs(Wm, Ws)
    assert buf.dtype == np.uint8 and buf.size == 3 * 8 * d * d + 3 * 4
    body = buf[: 3 * 8 * d * d].view(np.float16).reshape(3, 2, 2, d, d)
    inv = buf[3 * 8 * d * d:].view(np.float32)
    s = P.shifts(Wm, Ws)
    assert s[1] == 12 and inv.tolist() == [2.0 ** -int(v) for v in s]
    r, k, n = 1, d - 1, d - 3                                                     # relation 1's largest entry: W_self[1][k][n] = 3.0
    assert float(body[r, 1, 0, n, k]) == 3.0 * 2.0 ** 12 and float(body[r, 1, 1, n, k]) == 0.0
    assert float(body[r, 1, 0, k, n]) != 3.0 * 2.0 ** 12
    assert not body[2, 0].any() and body[2, 1, 0].any()                           # relation 2: W_msg is zero, W_self is not
    k, n = 5, 77
    x = np.float32(Wm[0, k, n]) * np.float32(2.0 ** int(s[0]))
    hi = np.float16(x)
    assert body[0, 0, 0, n, k] == hi and body[0, 0, 1, n, k] == np.float16(x - np.float32(hi))


def test_zero_and_extreme_relations_clamp_the_shift():
    d = 128
    Wm, Ws = np.zeros((3, d, d), np.float32), np.zeros((3, d, d), np.float32)
    Wm[1, 0, 0], Ws[2, 3, 4] = np.float32(2.0 ** -120), np.float32(2.0 ** 120)
    assert P.shifts(Wm, Ws).tolist() == [100, 100, -100]


@pytest.mark.parametrize("d", GUARD_WIDTHS)
@pytest.mark.parametrize("case", P.GUARD_CASES)
def test_guard_matrices_have_the_counts_they_claim(d, case):
    Wm, Ws, (half, r, k0, n0), word = P.guard_weights(d, case)
    fires = case.endswith("fires")
    assert word == (P.RANGE_WEIGHTS if fires else 0) and P.guard_word(Wm, Ws) == word
    nb = d // P.TILE
    if case.startswith("self_last"):
        assert (half, k0 // P.TILE, n0 // P.TILE) == (1, nb - 1, nb - 1)
    else:
        assert half == 0 and 0 < k0 // P.TILE < nb - 1 and 0 < n0 // P.TILE < nb - 1
    s = P.shifts(Wm, Ws)
    assert s[r] == 13
    hot = np.zeros((2, 3, nb, nb), dtype=bool)
    for h, W in enumerate((Wm, Ws)):
        tiny, nz = P.tile_counts(P.scaled(W, s))
        hot[h] = (tiny > 0) & (tiny * 8 >= nz)
        if h == half:
            t, n = int(tiny[r, k0 // P.TILE, n0 // P.TILE]), int(nz[r, k0 // P.TILE, n0 // P.TILE])
            assert n == 1008 and t == (126 if fires else 124)
            assert (t * 8 == n) if fires else (t * 8 == n - 16)
            assert not t * 8 > n                                                  # `>` for `>=`: a fires tile no longer fires
            assert not t * 8 >= P.TILE * P.TILE                                   # zeros counted as nonzero: neither
            xs = np.abs(P.scaled(W, s)[r, k0:k0 + P.TILE, n0:n0 + P.TILE])
            assert int((xs == 0.5).sum()) == (0 if fires else 2)                  # `<= 0.5` for `< 0.5`: the holds tile fires
            assert int(((xs != 0) & (xs <= 0.5)).sum()) == 126
    assert int(hot.sum()) == (1 if fires else 0) and bool(hot[half, r, k0 // P.TILE, n0 // P.TILE]) == fires


# ---- the two-layer chain of test_wide_rows_gpu.py is well conditioned -----------------------------------------------------

@pytest.mark.parametrize("name", ("csr_runs_around_run_max", "csr_in_degrees"))
@pytest.mark.parametrize("d", (384, 512))
def test_the_two_layer_chain_is_admissible(d, name):
    """The float32 oracle, two layers deep, lands within half of assert_close's bounds of the float64 reference."""
    key = f"csr{d}"
    geo = {g[0]: g for g in G.geometries()}[key]
    (case,) = [c for c in G.edge_cases(*geo[2:], d) if c.name == name]
    ins1, ins2 = G.two_layer_inputs(case, d, G.seed_for(key, name))
    ref = G.two_layer_ref64(case, ins1, ins2)
    th = torch.from_numpy
    ei, rel = th(case.edge_index), th(case.rel)
    h = th(ins1[0])
    for Wm, Ws, b, gamma, beta in (ins1[1:], ins2):
        agg = O.message_passing_factorised(h, ei, rel, th(Wm), th(Ws), th(b))
        h = O.layer_tail(agg, h, th(gamma), th(beta))
    got = h.numpy().astype(np.float64)
    rel_l2 = np.linalg.norm(got - ref) / np.linalg.norm(ref)
    assert (np.abs(got - ref) <= ATOL / 2 + RTOL / 2 * np.abs(ref)).all() and rel_l2 <= REL_L2 / 2, \
        f"{key} {name}: float32 oracle misses half the bound two layers deep (relative L2 {rel_l2:.3e})"
