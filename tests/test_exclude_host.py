"""Host-side checks of forward_nodes' `exclude` (include/ghf.h: ghf_subgraph_*_excl): the entry points, their argument checks,
the Python validation, and the numpy restatement's own properties.  No GPU needed."""

import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _exclude as X
import _sampling as S
from graph_hypernetwork_forge_amd import HyperGNN, ToyKnowledgeGraph, _build, _native, synth

EXCL_CALLS = ("ghf_subgraph_hops_excl", "ghf_subgraph_edges_excl", "ghf_subgraph_sample_hops_excl")


def test_excl_entry_points_are_declared_bound_and_exported_and_the_abi_is_still_15():
    with open(os.path.join(_build.INCLUDE, "ghf.h")) as f:
        text = f.read()
    assert re.search(r"#define GHF_ABI_VERSION 15\b", text)
    assert _native.ABI_VERSION == 15
    lib = _native.load()
    assert lib.ghf_abi_version() == 15
    for name in EXCL_CALLS:
        assert name in _native.header_symbols() and name in _native.SIGNATURES
        assert hasattr(lib, name), f"libghf_hip.so does not export {name}"
        twin = _native.SIGNATURES[name[:-len("_excl")]]
        assert _native.SIGNATURES[name] == (twin[0], twin[1] + [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int])
    assert "t * R + r" in text and "<< 32" in text                    # the key encoding is documented


def test_excl_entry_points_reject_bad_lists_and_null_arguments_without_a_gpu():
    lib = _native.load()
    nb = lib.ghf_subgraph_workspace_bytes(1000, 5000, 2)
    nbs = lib.ghf_subgraph_sample_workspace_bytes(1000, 5000, 2)
    fake = ctypes.c_void_p(4096)            # never dereferenced: every call below fails its checks on the host
    ws = ctypes.c_void_p(1 << 20)
    fan = (ctypes.c_int * 2)(5, -1)

    def hops(key=fake, seeds=fake, w=ws, w_bytes=nb, dist=fake, excl=fake, n=3, typed=0, k=2):
        return lib.ghf_subgraph_hops_excl(key, fake, 1000, 5000, 4, 1, seeds, 3, k, w, w_bytes, dist, None, excl, n, typed)

    def edges(key=fake, dist=fake, new_id=fake, w=ws, w_bytes=nb, out=fake, num=fake, excl=fake, n=3, typed=1, k=2):
        return lib.ghf_subgraph_edges_excl(key, fake, 1000, 5000, 4, 384, dist, new_id, k, w, w_bytes, out, fake, num, None,
                                           excl, n, typed)

    def shops(key=fake, seeds=fake, f=fan, w=ws, w_bytes=nbs, dist=fake, keep=fake, excl=fake, n=3, typed=0, k=2):
        return lib.ghf_subgraph_sample_hops_excl(key, fake, 1000, 5000, 4, 1, seeds, 3, k, f, 7, w, w_bytes, dist, keep, None,
                                                 None, excl, n, typed)

    for call in (hops, edges, shops):
        assert call(n=-1) == -1, call.__name__
        assert b"negative" in lib.ghf_last_error()
        assert call(excl=None, n=5) == -1, call.__name__
        assert b"null exclusion" in lib.ghf_last_error()
        for bad in (2, -1, 7):
            assert call(typed=bad) == -1, call.__name__
            assert b"typed" in lib.ghf_last_error()
        assert call(key=None) == -1 and b"null pointer" in lib.ghf_last_error()
        assert call(w=None) == -1 and b"null pointer" in lib.ghf_last_error()
        assert call(dist=None) == -1 and b"null pointer" in lib.ghf_last_error()
        assert call(k=0) == -1
        assert call(w_bytes=255) == -1                                   # the twins' checks: a small workspace,
        assert b"workspace" in lib.ghf_last_error()
        assert call(w=ctypes.c_void_p((1 << 20) + 4)) == -1               # a misaligned one
        assert b"aligned" in lib.ghf_last_error()
        assert call(excl=None, n=0, w_bytes=255) == -1                   # an empty list may be NULL: the next check speaks
        assert b"workspace" in lib.ghf_last_error()
    assert hops(seeds=None) == -1 and edges(new_id=None) == -1 and edges(out=None) == -1 and edges(num=None) == -1
    assert shops(keep=None) == -1 and shops(f=None) == -1
    assert shops(w_bytes=nb) == -1                                      # the sampled form needs the sampled workspace
    assert shops(f=(ctypes.c_int * 2)(5, 0)) == -1 and b"fanout" in lib.ghf_last_error()


# ---- the Python interface: validation before any device work ----------------------------------------------------------

def _toy(layers=2):
    kg = ToyKnowledgeGraph(feat_dim=16)
    m = HyperGNN(text_dim=32, node_feat_dim=16, hidden_dim=16, num_layers=layers).eval()
    return kg, m, list(kg.relation_types), torch.tensor([kg.relation_types.index(t) for t in kg.edge_texts])


@pytest.mark.parametrize("ids", [True, False])
def test_exclude_is_validated_before_any_device_work(ids):
    kg, m, rel_texts, rel = _toy()
    N, nodes = kg.node_features.size(0), torch.tensor([0, 1])
    a, b = torch.tensor([0, 1, 2]), torch.tensor([1, 2, 0])
    good_rel = torch.tensor([0, 1, 0]) if ids else [rel_texts[0], rel_texts[1], "a text that labels no edge"]

    def call(exclude, **kw):
        with torch.no_grad():
            if ids:
                return m.forward_nodes_ids(kg.node_features, kg.edge_index, rel, rel_texts, nodes, exclude=exclude, **kw)
            return m.forward_nodes(kg.node_features, kg.edge_index, kg.edge_texts, nodes, exclude=exclude, **kw)

    for bad in ((), (a,), (a, b, good_rel, a), a, "ab", 5):               # wrong arity, not a tuple of lists
        with pytest.raises(ValueError, match="exclude"):
            call(bad)
    with pytest.raises(ValueError, match="sources"):                     # unequal lengths
        call((a, b[:2]))
    with pytest.raises(ValueError):                                      # not 1-D
        call((a.view(1, 3), b.view(1, 3)))
    with pytest.raises(ValueError):                                      # not tensors
        call(([0, 1, 2], [1, 2, 0]))
    with pytest.raises(TypeError):                                       # float ids
        call((a.float(), b))
    with pytest.raises(TypeError):
        call((a, b.double()))
    for bad in (torch.tensor([0, N, 1]), torch.tensor([-N - 1, 0, 1])):   # node ids out of range (negative ones wrap)
        with pytest.raises(IndexError):
            call((bad, b))
        with pytest.raises(IndexError):
            call((a, bad))
    if ids:
        with pytest.raises(ValueError, match="negative"):                # relation ids do not wrap
            call((a, b, torch.tensor([0, -1, 0])))
        with pytest.raises(IndexError):
            call((a, b, torch.tensor([0, len(rel_texts), 0])))
        with pytest.raises(ValueError):                                  # one relation id per entry
            call((a, b, torch.tensor([0, 1])))
        with pytest.raises(TypeError):
            call((a, b, torch.tensor([0.0, 1.0, 0.0])))
        with pytest.raises(ValueError):                                  # texts belong to forward_nodes
            call((a, b, [rel_texts[0]] * 3))
    else:
        with pytest.raises(ValueError, match="relation texts"):          # rel strings of the wrong count
            call((a, b, [rel_texts[0]] * 2))
        with pytest.raises(TypeError):                                   # ids belong to forward_nodes_ids
            call((a, b, torch.tensor([0, 1, 0])))
        with pytest.raises(TypeError):
            call((a, b, [rel_texts[0], 1, rel_texts[0]]))
        with pytest.raises(TypeError):
            call((a, b, rel_texts[0]))
    with pytest.raises(ValueError):                                      # fanout's checks still run
        call((a, b), fanout=0)
    empty = torch.zeros(0, dtype=torch.int64)
    for good in ((a, b), (a.to(torch.int32), b), (torch.tensor([-1, -N, 0]), b), (a, b, good_rel), (empty, empty), None):
        with pytest.raises(RuntimeError, match="no CPU"):                # valid: the CPU features are what stops the call
            call(good)
        with pytest.raises(RuntimeError, match="no CPU"):
            call(good, fanout=3, seed=1)


def test_exclude_keys_follow_the_documented_encoding():
    """HyperGNN._exclude_keys against the restatement's keys (CPU tensors: nothing here launches anything)."""
    kg, m, rel_texts, rel = _toy()

    class Plan:
        R = len(rel_texts)
        unique_texts = rel_texts

    N = kg.node_features.size(0)
    a, b = torch.tensor([3, 0, -1, 3, 0]), torch.tensor([1, 2, 0, 1, -2])
    an, bn = np.array([3, 0, N - 1, 3, 0]), np.array([1, 2, 0, 1, N - 2])
    k, typed, entries = m._exclude_keys(m._exclude_args((a, b), kg.node_features, texts=True), Plan)
    assert (typed, entries) == (False, 5) and k.dtype == torch.int64
    assert np.array_equal(k.numpy().astype(np.uint64), X.keys(an, bn))
    r = torch.tensor([2, 0, 1, 2, 1])
    k, typed, entries = m._exclude_keys(m._exclude_args((a, b, r), kg.node_features, num_relations=Plan.R), Plan)
    assert (typed, entries) == (True, 5)
    assert np.array_equal(k.numpy().astype(np.uint64), X.keys(an, bn, r.numpy(), Plan.R))
    texts = [rel_texts[2], "no such relation", rel_texts[1], rel_texts[2], rel_texts[1]]
    k, typed, entries = m._exclude_keys(m._exclude_args((a, b, texts), kg.node_features, texts=True), Plan)
    assert (typed, entries) == (True, 5) and k.numel() == 4             # the unknown text matches nothing
    stay = np.array([0, 2, 3, 4])
    assert np.array_equal(k.numpy().astype(np.uint64), X.keys(an[stay], bn[stay], r.numpy()[stay], Plan.R))
    assert m._exclude_keys(None, Plan) is None


# ---- the restatement's own properties ---------------------------------------------------------------------------------

def _ordered(kind, bn, N=3000, E=20000, R=7, seed=5):
    ei, rel = synth.make_graph_arrays(N, E, R, seed, kind)
    order = S.plan_order(ei, rel, N, R, bn)
    return ei[0][order], ei[1][order], rel[order], N, R


def test_restated_keys_and_mask():
    assert X.keys([1, 0], [2, 3]).tolist() == [3, (1 << 32) | 2]
    assert X.keys([1], [2], [3], 7).tolist() == [(1 << 32) | 17]
    assert X.keys([(1 << 31) - 1], [5]).dtype == np.uint64
    src, dst, rel = np.array([0, 0, 1, 0, 2]), np.array([1, 1, 0, 1, 1]), np.array([0, 1, 0, 0, 0])
    assert X.excluded(src, dst, rel, 2, [0], [1]).tolist() == [True, True, False, True, False]          # every parallel edge
    assert X.excluded(src, dst, rel, 2, [0], [1], [0]).tolist() == [True, False, False, True, False]    # of that relation
    assert X.excluded(src, dst, rel, 2, [1, 1], [0, 0]).tolist() == [False, False, True, False, False]  # direction, duplicates
    assert not X.excluded(src, dst, rel, 2, [2, 0], [0, 1], [0, 5]).any()                               # matches nothing


@pytest.mark.parametrize("kind", ["uniform", "powerlaw"])
@pytest.mark.parametrize("bn", [1, 384])
def test_restatement_with_an_empty_list_is_the_plain_restatement(kind, bn):
    src, dst, rel, N, R = _ordered(kind, bn)
    none = X.excluded(src, dst, rel, R, [], [])
    assert not none.any()
    for seeds in ([5, 9, 5], list(range(0, N, 11))):
        for k in (1, 2, 3):
            for x, y in zip(X.np_subgraph_excl(src, dst, rel, N, seeds, k, none), S.np_subgraph(src, dst, rel, N, seeds, k)):
                assert np.array_equal(x, y), (kind, bn, k)
        for fanout in ((3, 3, 3), (2, -1, 4), (-1, -1)):
            got = X.np_subgraph_sample_excl(src, dst, rel, N, seeds, fanout, 31, none)
            for x, y in zip(got, S.np_subgraph_sample(src, dst, rel, N, seeds, fanout, 31)):
                assert np.array_equal(x, y), (kind, bn, fanout)


@pytest.mark.parametrize("kind", ["uniform", "powerlaw"])
@pytest.mark.parametrize("typed", [False, True])
def test_excluding_every_in_edge_of_every_seed_leaves_the_seeds_alone(kind, typed):
    src, dst, rel, N, R = _ordered(kind, 384)
    seeds = [int(np.bincount(dst, minlength=N).argmax()), 11, 17, 11]
    into = np.isin(dst, seeds)
    dead = X.excluded(src, dst, rel, R, src[into], dst[into], rel[into] if typed else None)
    assert np.array_equal(dead, into)
    n_seeds = len(set(seeds))
    for k in (1, 2, 3):
        dist, nl, nid, m, e_sub, r_sub = X.np_subgraph_excl(src, dst, rel, N, seeds, k, dead)
        assert m == [n_seeds] * (k + 1) and e_sub.shape == (2, 0) and r_sub.size == 0
        assert sorted(nl.tolist()) == sorted(set(seeds)) and (dist[nl] == 0).all()
        got = X.np_subgraph_sample_excl(src, dst, rel, N, seeds, (2, -1, 4)[:k], 9, dead)
        assert got[3] == [n_seeds] * (k + 1) and got[4].shape == (2, 0)


def test_restatement_equals_the_plain_one_on_the_reduced_graph_and_keeps_f_of_f_plus_one():
    """Exact form: the extraction with a mask is the plain extraction of the edges that are left.  Sampled form: the
    candidates are the edges that are left, the priorities those of the full arrays' positions."""
    src, dst, rel, N, R = _ordered("powerlaw", 384)
    rng = np.random.default_rng(3)
    pick = rng.choice(src.size, 400, replace=False)
    dead = X.excluded(src, dst, rel, R, src[pick], dst[pick], rel[pick])
    assert dead.sum() >= 400
    live = ~dead
    for seeds in ([5, 9, 5], list(range(0, N, 13))):
        for k in (1, 2, 3):
            got = X.np_subgraph_excl(src, dst, rel, N, seeds, k, dead)
            want = S.np_subgraph(src[live], dst[live], rel[live], N, seeds, k)
            for x, y in zip(got, want):
                assert np.array_equal(x, y), k
    indeg = np.bincount(dst, minlength=N)
    t = int(np.nonzero(indeg == 5)[0][0])
    into = np.nonzero(dst == t)[0]
    one = np.zeros(src.size, dtype=bool)
    one[into[2]] = True
    _, keep = X.np_sample_keep_excl(src, dst, N, [t], (4,), 77, one)
    assert np.array_equal(np.nonzero(keep)[0], np.delete(into, 2))      # cap 4, 5 in-edges, one excluded: the other 4 stay
    _, keep = X.np_sample_keep_excl(src, dst, N, [t], (3,), 77, one)
    prio = S.priority(77, into)
    rest = np.delete(into, 2)
    want = np.sort(rest[np.lexsort((rest, np.delete(prio, 2)))][:3])
    assert np.array_equal(np.nonzero(keep)[0], want)                    # below it: by the full positions' priorities
