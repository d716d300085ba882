"""What test_tail_rows_gpu.py relies on, shown without a GPU: the reference of _tail_rows.py agrees with float64 autograd
and with _edge_graphs.tail_ref64; the exactness the bit-for-bit comparisons assume holds in float32 for both forms of the
mean; a float32 two-pass tail stays inside the stated bounds on the whole catalogue at every width the GPU file runs,
and a one-pass variance does not; ghf_tail_bwd's walk over the rows is the one the large-N cases were sized for."""

import numpy as np
import pytest
import torch

import _edge_graphs as G
import _tail_rows as T
from _util import ATOL, RTOL, assert_close

FWD_WIDTHS = (3, 20, 64, 65, 100, 128, 257, 1023, 1024)                  # tail_fwd
BWD_WIDTHS = tuple(T.V4_LPR) + T.GENERIC_BWD_WIDTHS
WIDTHS = tuple(sorted(set(FWD_WIDTHS + G.RS_WIDTHS + BWD_WIDTHS)))
POW2 = tuple(d for d in WIDTHS if d & (d - 1) == 0)
ODD = (100, 257, 640, 896, 1023)


def test_reference_agrees_with_float64_autograd_and_tail_ref64():
    N, d = 37, 50
    g = torch.Generator().manual_seed(5)
    agg, h, go = (torch.randn(N, d, generator=g) for _ in range(3))
    gamma, beta = torch.rand(d, generator=g) + 0.5, torch.randn(d, generator=g)
    indeg = torch.randint(0, 6, (N,), generator=g, dtype=torch.int32)
    for drop in (None, (torch.rand(N, d, generator=g) < 0.75).float() / 0.75):
        ref = T.tail_ref(agg.numpy(), h.numpy(), gamma.numpy(), beta.numpy(), None if drop is None else drop.numpy(), go.numpy(),
                         indeg.numpy())
        pre = (agg + h).double().requires_grad_(True)                    # the float32 sum, as the reference forms it
        gam, bet = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
        x = torch.relu(pre) * (1.0 if drop is None else drop.double())
        out = torch.nn.functional.layer_norm(x, (d,), gam, bet, T.LN_EPS)
        out.backward(go.double())
        for key, want in (("out", out.detach()), ("dpre", pre.grad), ("dgamma", gam.grad), ("dbeta", bet.grad)):
            assert np.allclose(ref[key], want.numpy(), rtol=1e-11, atol=1e-12), key
        assert np.allclose(ref["G"], (pre.grad / indeg.clamp(min=1).double().unsqueeze(1)).numpy(), rtol=1e-11, atol=1e-12)
        assert np.array_equal(ref["G"], ref["dpre"] / np.maximum(indeg.numpy(), 1).astype(np.float64)[:, None])
        # tail_ref64 adds agg and h in float64: hand it the float32 sum
        want = G.tail_ref64(np.zeros((N, d)), ref["pre32"], gamma.numpy(), beta.numpy(), None if drop is None else drop.numpy())
        assert np.allclose(ref["out"], want, rtol=1e-13, atol=1e-14)


@pytest.mark.parametrize("d", WIDTHS)
def test_the_catalogue_is_what_its_names_say(d):
    cat = T.catalogue(d)
    pre = cat.pre32
    assert len(set(cat.names)) == cat.K and cat.K < 64
    assert (cat.gamma == 0).sum() == 1 and (cat.gamma < 0).sum() == 1 and (cat.beta != 0).all()
    others = cat.gamma[cat.gamma > 0]
    assert others.min() >= 0.5 and others.max() <= 1.5
    assert sorted(set(cat.indeg.tolist())) == sorted(T.INDEG) or cat.K < len(T.INDEG)
    dead = pre[cat.row("dead")]
    assert (dead <= 0).all() and np.signbit(dead[dead == 0]).any() and (~np.signbit(dead[dead == 0])).any()
    assert (dead <= -1).any()
    if d >= 7:
        assert ((dead < 0) & (np.abs(dead) < T.MIN_NORMAL)).any() and (dead == -T.MIN_NORMAL).any()
    for c in T.CONSTS:
        assert (pre[cat.row(f"const_{c:g}")] == np.float32(c)).all()
    off = pre[cat.row("offset")].astype(np.float64)
    assert ((off - 1024) * 8 == np.round((off - 1024) * 8)).all() and off.min() >= 1024 and off.max() < 1032
    assert T.sum_exact_in_any_order(pre[cat.row("offset")])
    want_cols = sorted({min(j, d - 1) for j in T.ONE_LIVE_COLUMNS + (d - 1,)})
    assert [int(n.split("_")[-1]) for n in cat.names if n.startswith("one_live_")] == want_cols
    for j in want_cols:
        r = pre[cat.row(f"one_live_{j}")]
        assert r[j] == 2.5 and (np.delete(r, j) == 0).all()
    k = pre[cat.row("kink_direct")]
    if d >= 20:
        for v in (T.SUBNORMAL, -T.SUBNORMAL, T.MIN_NORMAL, -T.MIN_NORMAL):
            assert (k == v).any()
        assert np.signbit(k[k == 0]).any() and (~np.signbit(k[k == 0])).any() and (np.abs(k) > 0.1).any()
    kc = pre[cat.row("kink_cancel")]
    col = np.arange(d)
    assert (kc[col % 3 == 1] == 0).all(), "agg = -h must land on zero"
    beside = kc[col % 3 == 2]
    hk = cat.h[cat.row("kink_cancel")][col % 3 == 2]
    assert (beside != 0).all() and (np.abs(beside) <= 2 * T.ulp32(hk)).all(), "agg = -h (1 + 2^-23) must land beside zero"
    assert (np.sign(beside) == -np.sign(hk)).all()
    for e in T.SCALES:
        r = pre[cat.row(f"scale_{e}")]
        assert 0.25 < (r > 0).mean() < 0.75 or d < 20
        assert np.array_equal(r, pre[cat.row("scale_20")] * np.float32(2.0 ** (e - 20)))
    xm = cat.x32(True)
    assert (pre[cat.row("masked_all")] > 0).any() and (xm[cat.row("masked_all")] == 0).all()
    assert (xm[cat.row("masked_one")] != 0).sum() == 1
    assert len(cat.rows("filler_")) == 4


@pytest.mark.parametrize("dropping", [False, True])
@pytest.mark.parametrize("d", WIDTHS)
def test_exactness_claims_hold_in_float32_for_both_mean_forms(d, dropping):
    cat = T.catalogue(d)
    exact = T.exact_mean_rows(cat, dropping)
    beta_rows = T.beta_rows(cat, dropping)
    assert cat.row("dead") in beta_rows and (not dropping or cat.row("masked_all") in beta_rows)
    consts = cat.rows("const_")
    if d in POW2:                                    # the helper's list holds every dyadic constant at every power of two
        assert set(consts) <= set(exact) and set(consts) <= set(beta_rows) and cat.row("offset") in exact
        assert T.mean_ulp_rows(cat, dropping) == []
    assert set(T.mean_ulp_rows(cat, dropping)) <= set(consts + [cat.row("offset")])
    assert set(T.backward_rows(cat, dropping)) >= set(range(cat.K)) - set(consts)
    for form in ("div", "rcp"):
        out = T.tail_f32(cat, dropping, form)
        for i in beta_rows:                          # zero variance and an exact mean: beta, bit for bit
            assert np.array_equal(T.bits(out[i]), T.bits(cat.beta)), f"{cat.names[i]} ({form}) is not beta bit for bit"
    # (sum / d of a dyadic constant is exact at every width: only the reciprocal form needs the helper's verdict)
    for i in consts:
        x = cat.x32(dropping)[i]
        assert np.float32(x.sum(dtype=np.float32) / np.float32(d)) == x[0]


@pytest.mark.parametrize("dropping", [False, True])
@pytest.mark.parametrize("d", WIDTHS)
def test_a_float32_two_pass_tail_stays_inside_the_bounds(d, dropping):
    """The reference alone within its cap: forward (both mean forms) on the whole catalogue, backward on the rows the GPU
    file runs."""
    cat = T.catalogue(d)
    go = T.gout_for(cat.K, d)
    ref = T.tail_ref(cat.agg, cat.h, cat.gamma, cat.beta, cat.drop if dropping else None, go, cat.indeg)
    bound = T.forward_bound(cat, ref, dropping)
    plain = [i for i in range(cat.K) if i not in T.mean_ulp_rows(cat, dropping)]
    rows = T.backward_rows(cat, dropping)
    for form in ("div", "rcp"):
        out = T.tail_f32(cat, dropping, form).astype(np.float64)
        err = np.abs(out - ref["out"])
        assert (err <= bound).all(), f"{form}: {cat.names[int(np.argmax((err - bound).max(axis=1)))]} leaves the bound"
        assert_close(out[plain], ref["out"][plain], f"d={d} {form}: the rows without the mean-ulp term")
        if d not in BWD_WIDTHS:
            continue
        bw = T.tail_bwd_f32(cat, go, dropping, form)
        assert_close(bw["dpre"][rows], ref["dpre"][rows], f"d={d} {form}: dpre")
        sub = T.tail_ref(cat.agg[rows], cat.h[rows], cat.gamma, cat.beta, cat.drop[rows] if dropping else None, go[rows])
        scale = np.sqrt(len(rows))
        sel = cat._replace(names=[cat.names[i] for i in rows], agg=cat.agg[rows], h=cat.h[rows], drop=cat.drop[rows], indeg=cat.indeg[rows])
        bw = T.tail_bwd_f32(sel, go[rows], dropping, form)
        assert_close(bw["dgamma"] / scale, sub["dgamma"] / scale, f"d={d} {form}: dgamma")
        assert_close(bw["dbeta"] / scale, sub["dbeta"] / scale, f"d={d} {form}: dbeta")


@pytest.mark.parametrize("d", WIDTHS)
def test_a_one_pass_variance_fails_on_offset(d):
    """E[x^2] - mean^2 in float32 on a row at 1024 with a spread of a few units: x^2 is 2^20, its ulp 2^-3, the variance a
    few units — off by percent.  The catalogue tells the two forms apart at every width."""
    cat = T.catalogue(d)
    ref = T.tail_ref(cat.agg, cat.h, cat.gamma, cat.beta)
    bound = T.forward_bound(cat, ref, False)
    i = cat.row("offset")
    for form in ("div", "rcp"):
        err = np.abs(T.tail_f32(cat, False, form, one_pass=True).astype(np.float64) - ref["out"])
        assert (err[i] > bound[i]).any(), f"d={d} {form}: a one-pass variance passes on `offset`"
        assert err[i].max() > 10 * (ATOL + RTOL), f"d={d} {form}: a one-pass variance is off by only {err[i].max():.2e}"


def test_offset_leaves_the_default_tolerance_only_where_the_mean_is_inexact():
    """The term of forward_bound is needed (some width leaves atol + rtol |ref| on a row of mean_ulp_rows) and is applied
    nowhere else (a power-of-two width has no such row)."""
    worst = 0.0
    for d in ODD:
        cat = T.catalogue(d)
        ref = T.tail_ref(cat.agg, cat.h, cat.gamma, cat.beta)
        rows = T.mean_ulp_rows(cat, False)
        assert cat.row("offset") in rows
        for form in ("div", "rcp"):
            err = np.abs(T.tail_f32(cat, False, form).astype(np.float64) - ref["out"])
            worst = max(worst, float((err[rows] - ATOL - RTOL * np.abs(ref["out"][rows])).max()))
    assert 0 < worst < 2e-4, worst


@pytest.mark.parametrize("d", [3, 20, 64, 100, 128, 640, 1023, 1024])
def test_the_comparisons_pass_a_float32_two_pass_tail(d):
    """check_forward / check_backward as the GPU file calls them — on the catalogue, on its rows handed over as h alone,
    repeated and permuted, under beta = 0 — fed with the float32 restatements."""
    base = T.catalogue(d)
    idx = np.roll(np.arange(3 * base.K) % base.K, 7)
    zero = np.zeros(d, dtype=np.float32)
    for cat in (base, T.take(T.as_h(base), idx), T.as_h(base)._replace(beta=zero)):
        for dropping in (False, True):
            for form in ("div", "rcp"):
                T.check_forward(T.tail_f32(cat, dropping, form), cat, dropping, f"f32 {form} d={d}")
    assert (T.tail_f32(T.as_h(base)._replace(beta=zero), False)[base.row("dead")] == 0).all()
    if d in BWD_WIDTHS:
        for dropping in (False, True):
            cat = T.take(base, T.backward_rows(base, dropping))
            go = T.gout_for(cat.K, d)
            bw = T.tail_bwd_f32(cat, go, dropping)
            inv = (np.float32(1.0) / np.maximum(cat.indeg, 1).astype(np.float32))[:, None]
            T.check_backward(bw["dpre"], (bw["dpre"] * inv).astype(np.float32), bw["dgamma"], bw["dbeta"], cat, go, dropping, f"f32 d={d}")
            wrong = T.tail_bwd_f32(cat, go, dropping)["dpre"].copy()
            wrong[cat.pre32 == 0] = 1.0                  # `pre >= 0` taken as live
            with pytest.raises(AssertionError):
                T.check_backward(wrong, wrong * inv, bw["dgamma"], bw["dbeta"], cat, go, dropping, "pre >= 0 as live")


def test_tail_bwd_geometry_matches_the_library():
    from graph_hypernetwork_forge_amd import _native
    lib = _native.load()
    for d in (3, 20, 32, 128, 1024):
        for N in (1, 4, 5, 8188, 8189, 8192, 8193, 16389, 131077, 10 ** 6):
            assert int(lib.ghf_tail_bwd_workspace_floats(N, d)) == T.tail_bwd_workspace_floats(N, d), (N, d)
        # the grid stops growing once cdiv(N, 4) reaches TB_BLOCKS, and not before
        assert T.tail_bwd_workspace_floats(4 * T.TB_BLOCKS - 4, d) < T.tail_bwd_workspace_floats(4 * T.TB_BLOCKS, d)
        assert T.tail_bwd_workspace_floats(4 * T.TB_BLOCKS, d) == T.tail_bwd_workspace_floats(10 ** 6, d)
    assert T.TB_BLOCKS == 2048
    assert {d: T.rows_per_visit(d) for d in T.V4_LPR} == {32: 65536, 64: 32768, 128: 16384, 256: 8192, 512: 8192, 1024: 8192}
    assert T.rows_per_visit(20) == T.rows_per_visit(128, v4=False) == 8192
    assert (T.third_visit_N(20), T.third_visit_N(32), T.third_visit_N(128), T.third_visit_N(1024)) == (16389, 131077, 32773, 16389)
    for d in (20, 32, 128, 1024):
        v = T.visit_of(T.third_visit_N(d), d)
        assert v.max() == 2 and (v == 2).sum() == 5 and (v == 1).sum() == T.rows_per_visit(d)
