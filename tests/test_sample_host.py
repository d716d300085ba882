"""Host-side checks of neighbour sampling in HyperGNN.forward_nodes (fanout / seed) and its entry points
(include/ghf.h: ghf_subgraph_sample_*), and the numpy restatement's own properties: no GPU needed."""

import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _sampling as S
from graph_hypernetwork_forge_amd import HyperGNN, ToyKnowledgeGraph, _build, _native, synth

SAMPLE_CALLS = ("ghf_subgraph_sample_workspace_bytes", "ghf_subgraph_sample_hops", "ghf_subgraph_sample_edges")


def test_sample_entry_points_are_declared_bound_and_exported():
    with open(os.path.join(_build.INCLUDE, "ghf.h")) as f:
        text = f.read()
    assert re.search(r"#define GHF_ABI_VERSION 15\b", text)
    assert _native.ABI_VERSION == 15
    lib = _native.load()
    assert lib.ghf_abi_version() == 15
    for name in SAMPLE_CALLS:
        assert name in _native.header_symbols() and name in _native.SIGNATURES
        assert hasattr(lib, name), f"libghf_hip.so does not export {name}"
    assert "0x9E3779B97F4A7C15" in text and "0xBF58476D1CE4E5B9" in text and "0x94D049BB133111EB" in text


def _fan(*v):
    return (ctypes.c_int * len(v))(*v)


def test_sample_entry_points_reject_null_and_invalid_arguments_without_a_gpu():
    lib = _native.load()
    nb = lib.ghf_subgraph_sample_workspace_bytes(1000, 5000, 2)
    assert nb >= lib.ghf_subgraph_workspace_bytes(1000, 5000, 2) + 5000 * (2 * 8 + 2 * 4) and nb % 256 == 0
    assert lib.ghf_subgraph_sample_workspace_bytes(1000, 5000, 0) == 0
    assert lib.ghf_subgraph_sample_workspace_bytes(0, 5000, 2) == 0
    assert lib.ghf_subgraph_sample_workspace_bytes(1000, -1, 2) == 0
    fake = ctypes.c_void_p(4096)            # never dereferenced: every call below fails its checks on the host
    ws = ctypes.c_void_p(1 << 20)
    ok = _fan(5, -1)

    def hops(key=fake, src=fake, R=4, bn=1, seeds=fake, n_seeds=3, k=2, fan=ok, w=ws, w_bytes=nb, dist=fake, keep=fake):
        return lib.ghf_subgraph_sample_hops(key, src, 1000, 5000, R, bn, seeds, n_seeds, k, fan, 7, w, w_bytes, dist, keep, None, None)

    assert hops(key=None, src=None) == -1
    assert b"null" in lib.ghf_last_error()
    for name in ("seeds", "fan", "w", "dist", "keep"):
        assert hops(**{name: None}) == -1, name
        assert b"null" in lib.ghf_last_error(), name
    assert hops(k=0, fan=_fan(1)) == -1                                # k < 1
    assert hops(k=-3) == -1
    assert hops(fan=_fan(5, 0)) == -1                                  # fanout 0
    assert b"fanout" in lib.ghf_last_error()
    assert hops(fan=_fan(-2, 5)) == -1                                 # fanout < -1
    assert b"fanout" in lib.ghf_last_error()
    assert hops(R=0) == -1
    assert hops(n_seeds=-1) == -1
    assert hops(w_bytes=nb - 1) == -1                                  # small workspace
    assert b"workspace" in lib.ghf_last_error()
    assert hops(w_bytes=lib.ghf_subgraph_workspace_bytes(1000, 5000, 2)) == -1      # the exact call's workspace is too small
    assert hops(w=ctypes.c_void_p((1 << 20) + 4)) == -1               # misaligned
    assert b"aligned" in lib.ghf_last_error()

    def edges(key=fake, keep=fake, new_id=fake, w=ws, w_bytes=nb, out=fake, rel=fake, num=fake, bn=384):
        return lib.ghf_subgraph_sample_edges(key, fake, 1000, 5000, 4, bn, keep, new_id, w, w_bytes, out, rel, num, None)

    for name in ("key", "keep", "new_id", "w", "out", "rel", "num"):
        assert edges(**{name: None}) == -1, name
        assert b"null" in lib.ghf_last_error(), name
    assert edges(bn=0) == -1
    assert edges(w_bytes=lib.ghf_subgraph_sample_workspace_bytes(1000, 5000, 1) - 1) == -1
    assert b"workspace" in lib.ghf_last_error()
    assert edges(w=ctypes.c_void_p((1 << 20) + 8)) == -1


def test_restated_priority_is_the_documented_mix():
    pos = np.array([0, 1, 2, 12345, (1 << 31) - 2, (1 << 32) - 1])
    for seed in (0, 1, 0x0123456789ABCDEF, (1 << 63) - 1):
        assert S.priority(seed, pos).tolist() == [S.priority_scalar(seed, int(p)) for p in pos]
    assert S.priority_scalar(0, 0) == 0xE220A8397B1DCDAF >> 32        # splitmix64's first output from state 0


# ---- the Python interface: validation before any device work ----------------------------------------------------------

def _toy(layers=2):
    kg = ToyKnowledgeGraph(feat_dim=16)
    m = HyperGNN(text_dim=32, node_feat_dim=16, hidden_dim=16, num_layers=layers).eval()
    return kg, m, list(kg.relation_types), torch.tensor([kg.relation_types.index(t) for t in kg.edge_texts])


@pytest.mark.parametrize("ids", [True, False])
def test_fanout_and_seed_are_validated_before_any_device_work(ids):
    kg, m, rel_texts, rel = _toy()
    nodes = torch.tensor([0, 1])

    def call(**kw):
        with torch.no_grad():
            if ids:
                return m.forward_nodes_ids(kg.node_features, kg.edge_index, rel, rel_texts, nodes, **kw)
            return m.forward_nodes(kg.node_features, kg.edge_index, kg.edge_texts, nodes, **kw)

    for bad in ([5], [5, 5, 5], (), [5, 0], 0, [3, -2], -2):            # wrong length, a 0 entry, below -1
        with pytest.raises(ValueError):
            call(fanout=bad, seed=1)
    for bad in (2.5, [5, 2.0], "5", [5, None], True, torch.tensor([5, 5])):        # not integers
        with pytest.raises(TypeError):
            call(fanout=bad, seed=1)
    with pytest.raises(ValueError):                                     # a seed without fanout
        call(seed=3)
    for bad in (-1, 1 << 63):
        with pytest.raises(ValueError):
            call(fanout=5, seed=bad)
    with pytest.raises(TypeError):
        call(fanout=5, seed=1.5)
    for good in (dict(fanout=5, seed=0), dict(fanout=[5, -1], seed=(1 << 63) - 1), dict(fanout=(np.int64(2), 1)),
                 dict(fanout=-1), dict(fanout=None, seed=None)):
        with pytest.raises(RuntimeError, match="no CPU"):               # valid: the CPU features are what stops the call
            call(**good)
    with pytest.raises(ValueError):                                     # the checks of the exact call still run first
        with torch.no_grad():
            m.forward_nodes(kg.node_features[:, :8], kg.edge_index, kg.edge_texts, nodes, fanout=5)


def test_seed_none_draws_from_torchs_default_generator():
    _, m, _, _ = _toy(layers=3)
    torch.manual_seed(11)
    a = m._sample_args(4, None)
    b = m._sample_args(4, None)
    torch.manual_seed(11)
    c = m._sample_args(4, None)
    assert a[0] == (4, 4, 4) and 0 <= a[1] < 1 << 63
    assert a == c and a[1] != b[1]
    assert m._sample_args([3, -1, 2], 9) == ((3, -1, 2), 9)
    assert m._sample_args(None, None) is None


# ---- the restatement's own properties ---------------------------------------------------------------------------------

def _ordered(kind, bn, N=3000, E=20000, R=7, seed=5):
    ei, rel = synth.make_graph_arrays(N, E, R, seed, kind)
    order = S.plan_order(ei, rel, N, R, bn)
    return ei[0][order], ei[1][order], rel[order], N


@pytest.mark.parametrize("kind", ["uniform", "powerlaw"])
@pytest.mark.parametrize("bn", [1, 384])
def test_restatement_caps_keeps_all_below_the_cap_and_keeps_the_prefix_property(kind, bn):
    src, dst, rel, N = _ordered(kind, bn)
    indeg = np.bincount(dst, minlength=N)
    hub = int(indeg.argmax())
    for seeds in ([hub, 11, 17], list(range(0, N, 7))):
        for fanout in ((1, 1, 1), (3, 3), (2, -1, 5, 1), (4,)):
            k = len(fanout)
            dist, keep = S.np_sample_keep(src, dst, N, seeds, fanout, 77)
            kept_in = np.bincount(dst[keep], minlength=N)
            for j, f in enumerate(fanout):
                at = np.nonzero(dist == j)[0]
                want = indeg[at] if f == -1 else np.minimum(indeg[at], f)     # the cap, and keep-all at or below it
                assert np.array_equal(kept_in[at], want), (kind, bn, fanout, j)
            assert kept_in[dist >= k].sum() == 0                              # nodes at distance k are not expanded
            assert (dist[src[keep]] <= dist[dst[keep]] + 1).all()             # sources at most one hop further
            reached = np.unique(src[keep])
            assert set(np.nonzero((dist >= 1) & (dist <= k))[0]) <= set(reached)   # a distance means a kept edge led there
            _, nl, nid, m, e_sub, _ = S.np_subgraph_sample(src, dst, rel, N, seeds, fanout, 77)
            assert np.array_equal(dist[nl], np.sort(dist[nl])) and m[k] == nl.size
            for j in range(k + 1):                                            # rows within j hops are the first m[j]
                assert set(nl[:m[j]]) == set(np.nonzero(dist <= j)[0])
            for j in range(k):                                                # layer j's rows only read the next prefix
                into = e_sub[1] < m[j]
                assert (e_sub[0][into] < m[j + 1]).all()
            assert e_sub.shape[1] == int(keep.sum()) and e_sub.min(initial=0) >= 0


def test_restatement_is_deterministic_and_seeds_differ_on_a_hub():
    src, dst, rel, N = _ordered("powerlaw", 384)
    hub = int(np.bincount(dst, minlength=N).argmax())
    a = S.np_subgraph_sample(src, dst, rel, N, [hub], (5, 5), 1)
    b = S.np_subgraph_sample(src, dst, rel, N, [hub], (5, 5), 1)
    c = S.np_subgraph_sample(src, dst, rel, N, [hub], (5, 5), 2)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    assert not np.array_equal(a[1], c[1])


@pytest.mark.parametrize("kind", ["uniform", "powerlaw"])
@pytest.mark.parametrize("bn", [1, 384])
def test_restatement_without_caps_is_the_exact_subgraph(kind, bn):
    src, dst, rel, N = _ordered(kind, bn)
    big = int(np.bincount(dst, minlength=N).max())
    for seeds in ([5, 9, 5], list(range(N))):
        for k in (1, 2, 3):
            want = S.np_subgraph(src, dst, rel, N, seeds, k)
            for fanout in ((-1,) * k, (big,) * k, (big + 3, -1, big)[:k]):
                got = S.np_subgraph_sample(src, dst, rel, N, seeds, fanout, 123)
                for x, y in zip(got, want):
                    assert np.array_equal(x, y), (kind, bn, k, fanout)


def test_restatement_samples_uniformly():
    """4,096 destinations share the same 32 sources; every destination a seed, one hop, fanout 8: each source is chosen
    Binomial(4096, 1/4) times — 1024 +- 139 is five standard deviations (a uniform sampler misses with p ~ 2e-5)."""
    ei, rel, N = S.uniformity_graph()
    order = S.plan_order(ei, rel, N, 1, 1)
    src, dst = ei[0][order], ei[1][order]
    _, keep = S.np_sample_keep(src, dst, N, list(range(32, N)), (8,), S.UNIFORMITY_SEED)
    assert int(keep.sum()) == 4096 * 8
    assert (np.bincount(dst[keep], minlength=N)[32:] == 8).all()
    chosen = np.bincount(src[keep], minlength=32)[:32]
    print("times each source was chosen:", chosen.tolist())
    mean, dev = S.UNIFORMITY_BOUND
    assert (np.abs(chosen - mean) <= dev).all(), chosen.tolist()


def test_restatement_breaks_priority_ties_by_position():
    """One destination with 300,000 parallel in-edges: some pairs of them share a 32-bit priority (a birthday collision).
    With the cap set between the two edges of such a pair, the one at the lower plan position is kept."""
    src, dst, N, seed, pairs = S.tie_graph()
    assert len(pairs) > 0
    for lo, hi, fan in pairs[:3]:
        _, keep = S.np_sample_keep(src, dst, N, [N - 1], (fan,), seed)
        assert int(keep.sum()) == fan and keep[lo] and not keep[hi] and lo < hi
