"""The crafted edge-case graphs of _edge_graphs.py, checked on the host: every case has the structure its name promises in
every kernel's geometry, the float64 reference equals the oracle, and every case is well enough conditioned that the float32
oracle itself lands within half of the project's bounds of it (so a kernel failure on such a case is the kernel's)."""

import numpy as np
import pytest
import torch

import _edge_graphs as G
from _util import ATOL, REL_L2, RTOL
from oracle import hypergnn_oracle as O

GEOMETRIES = G.geometries()
PAIRS = [(geo, c.name) for geo in GEOMETRIES for c in G.edge_cases(*geo[2:], geo[1])]


def _case(geo, name):
    (case,) = [c for c in G.edge_cases(*geo[2:], geo[1]) if c.name == name]
    return case


@pytest.mark.parametrize("geo", GEOMETRIES, ids=[g[0] for g in GEOMETRIES])
def test_every_condition_is_realised(geo):
    key, d, bn, cr, sc, npw = geo
    cases = G.edge_cases(bn, cr, sc, npw, d)
    assert len({c.name for c in cases}) == len(cases)
    for c in cases:
        G.realised(c, bn, cr, sc, npw)
        assert c.rel.size <= 40_000 and c.edge_index.shape == (2, c.rel.size)
        assert c.edge_index.min() >= 0 and c.edge_index.max() < c.N and c.rel.min() >= 0 and c.rel.max() < c.R - 1
    names = {c.name for c in cases}
    if bn > 1:
        for stem in ("size_", "chunks_per_block_", "chunk_lengths", "runs", "split_", "sources_", "relations_"):
            assert any(n.startswith(stem) for n in names), stem
        assert ("helper_wave_boundaries" in names) == (npw > 0)
    else:
        assert len(names) == 7


def test_a_drifting_generator_is_caught():
    """A case that promises `split_chunks + 1` chunks fails `realised` when the plan's geometry is another one."""
    key, d, bn, cr, sc, npw = GEOMETRIES[0]
    (case,) = [c for c in G.edge_cases(bn, cr, sc, npw, d) if c.name == "split_sc_plus_1_chunks"]
    G.realised(case, bn, cr, sc, npw)
    for other in ((bn, cr - 4, sc, npw), (bn, cr, sc + 1, npw), (bn, cr + 4, sc, npw)):
        with pytest.raises(AssertionError, match="not realised"):
            G.realised(case, *other)


def _oracle(case, d, seed, dtype, grads=False):
    th = torch.from_numpy
    ins = [th(a).to(dtype).requires_grad_(grads) for a in G.layer_inputs(case, d, seed)]
    h, Wm, Ws, b, gamma, beta = ins
    agg = O.message_passing_factorised(h, th(case.edge_index), th(case.rel), Wm, Ws, b)
    out = O.layer_tail(agg, h, gamma, beta)
    if grads:
        out.backward(th(G.synth.normal(77, "gout", (case.N, d))).to(dtype))
    return agg.detach().numpy(), out.detach().numpy(), [t.grad.numpy() for t in ins] if grads else None


def _ref64(case, d, seed):
    th = torch.from_numpy
    ins = [th(a).double().requires_grad_(True) for a in G.layer_inputs(case, d, seed)]
    agg, out = G.layer_ref64_torch(ins[0], th(case.edge_index), th(case.rel), *ins[1:])
    out.backward(th(G.synth.normal(77, "gout", (case.N, d))).double())
    return agg.detach().numpy(), out.detach().numpy(), [t.grad.numpy() for t in ins]


def _within(got, ref, rtol, atol, l2):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    rel = np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-30)
    return bool((np.abs(got - ref) <= atol + rtol * np.abs(ref)).all()) and rel <= l2, rel


@pytest.mark.parametrize("geo,name", PAIRS, ids=[f"{g[0]}-{n}" for g, n in PAIRS])
def test_reference_equals_the_oracle_and_the_case_is_admissible(geo, name):
    key, d = geo[0], geo[1]
    case, seed = _case(geo, name), G.seed_for(geo[0], name)
    h, Wm, Ws, b, gamma, beta = G.layer_inputs(case, d, seed)
    agg_np, out_np = G.layer_ref64(h, case.edge_index, case.rel, Wm, Ws, b, gamma, beta)
    agg64, out64, g64 = _ref64(case, d, seed)
    o_agg, o_out, o_g = _oracle(case, d, seed, torch.float64, grads=True)
    for what, a, want in (("out", agg_np, o_agg), ("h'", out_np, o_out), ("out (torch)", agg64, o_agg), ("h' (torch)", out64, o_out)):
        assert np.allclose(a, want, rtol=1e-12, atol=1e-12), f"{what}: max abs diff {np.abs(a - want).max():.3e}"
    for n, a, want in zip(("h", "W_msg", "W_self", "bias", "gamma", "beta"), g64, o_g):
        assert np.allclose(a, want, rtol=1e-11, atol=1e-12 * max(np.abs(want).max(), 1.0)), f"d{n}: {np.abs(a - want).max():.3e}"
    # admissibility: the float32 oracle within HALF of the bounds the kernels are held to
    f_agg, f_out, f_g = _oracle(case, d, seed, torch.float32, grads=True)
    for what, a, want in (("out", f_agg, agg_np), ("h'", f_out, out_np)):
        ok, rel = _within(a, want, RTOL / 2, ATOL / 2, REL_L2 / 2)
        assert ok, f"{key} {name} seed {seed}: float32 oracle {what} misses half the bound (relative L2 {rel:.3e}): another seed"
    for n, a, want in zip(("h", "W_msg", "W_self", "bias", "gamma", "beta"), f_g, g64):
        scale = float(np.abs(want).max())
        ok, rel = _within(a, want, 1e-4, 1e-5 * max(scale, 1.0), 1e-5)
        assert ok, f"{key} {name} seed {seed}: float32 autograd d{n} misses half the bound (relative L2 {rel:.3e}): another seed"
    # the range word: the forward's rows must stay far from the guard's rule (the tests assert 0 there); the backward's may
    # meet it — graphs with hubs do, see _edge_graphs.cut_rows_margin — but never so narrowly that the word cannot be predicted
    if geo[2] == 1 and d % 128 == 0:
        margin = G.cut_rows_margin(case, h, agg_np, gamma, G.synth.normal(77, "gout", (case.N, d)))
        assert margin["forward"] <= 0.5, f"{key} {name} seed {seed}: rows of h reach {margin['forward']:.3f} of the range guard's rule"
        if d in G.RS_TRAIN_WIDTHS:
            word = G.predicted_range_word(margin["backward"])           # (asserts that it can be called)
            assert word == (G.RANGE_ROWS if margin["backward"] >= 1 else 0)
            assert name == "csr_hubs_around_hub_rows" or margin["backward"] <= 0.5, f"{key} {name}: {margin['backward']:.3f}"
