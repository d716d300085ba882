"""Host-side checks of relation-typed link prediction (RelationDecoder, ghf_relation_rows, the typed filter lists and the
query_rows / query_rel arguments of HyperGNN.rank_candidates, topk_candidates and softmax_loss): no GPU needed."""

import ctypes
import os
import re

import pytest
import torch

import graph_hypernetwork_forge_amd as pkg
from graph_hypernetwork_forge_amd import HyperGNN, _build, _native

REL_CALLS = ("ghf_relation_rows_workspace_bytes", "ghf_relation_rows")


def test_relation_entry_points_are_declared_bound_and_exported():
    with open(os.path.join(_build.INCLUDE, "ghf.h")) as f:
        text = f.read()
    assert re.search(r"#define GHF_ABI_VERSION 15\b", text)
    assert "relation.hip" in _build.SOURCES
    lib = _native.load()
    assert lib.ghf_abi_version() == 15
    for name in REL_CALLS:
        assert name in _native.header_symbols() and name in _native.SIGNATURES
        assert hasattr(lib, name), f"libghf_hip.so does not export {name}"
    assert "RelationDecoder" in pkg.__all__ and callable(pkg.RelationDecoder)
    from graph_hypernetwork_forge_amd.models import RelationDecoder
    assert RelationDecoder is pkg.RelationDecoder


def test_hypergnn_is_unchanged_by_the_decoder():
    """The decoder is a module of its own: the model's parameters, their names and their count stay what they were."""
    torch.manual_seed(0)
    before = HyperGNN(text_dim=32, node_feat_dim=16, hidden_dim=16)
    keys, count = list(before.state_dict().keys()), before.num_parameters()
    dec = pkg.RelationDecoder(text_dim=32, hidden_dim=16)
    torch.manual_seed(0)
    after = HyperGNN(text_dim=32, node_feat_dim=16, hidden_dim=16)
    assert list(after.state_dict().keys()) == keys and after.num_parameters() == count
    assert not any("decoder" in k or "relation" in k for k in keys)
    for k, v in before.state_dict().items():                       # same draws: constructing a decoder in between changes nothing
        assert torch.equal(v, after.state_dict()[k]), k
    # the generator is sized as the model sizes its layers' generators
    g, g0 = dec.generator, after.weight_generators[0]
    assert (g.text_dim, g.d_in, g.d_out, g.hidden_dim, g.num_hidden) == (g0.text_dim, g0.d_in, g0.d_out, g0.hidden_dim, g0.num_hidden)
    assert list(g.state_dict().keys()) == list(g0.state_dict().keys())
    assert pkg.RelationDecoder(text_dim=8, hidden_dim=4, gen_hidden_dim=24).generator.hidden_dim == 24
    assert dec.num_parameters() == sum(p.numel() for p in g.parameters())


def test_workspace_query_without_a_gpu():
    lib = _native.load()
    small = lib.ghf_relation_rows_workspace_bytes(150, 7)
    assert small > 0 and small % 256 == 0
    big = lib.ghf_relation_rows_workspace_bytes(16384, 64)
    assert 8 * (16384 // 64 + 64) <= big <= 8 * (16384 // 64 + 64) + 256       # one (relation, tile) pair per work item
    for bad in ((0, 7), (-1, 7), (150, 0), (150, -2), (1 << 31, 7)):
        assert lib.ghf_relation_rows_workspace_bytes(*bad) == 0, bad


def test_relation_rows_rejects_invalid_arguments_without_a_gpu():
    lib = _native.load()
    fake = ctypes.c_void_p(4096)            # never dereferenced: every call below fails its checks on the host
    ws = ctypes.c_void_p(1 << 20)
    B, R, N, d = 150, 7, 5003, 64
    nb = lib.ghf_relation_rows_workspace_bytes(B, R)

    def rows(x=fake, ix=fake, rel=fake, W=fake, bias=fake, perm=fake, goff=fake, rows_x=N, B_=B, R_=R, d_=d, flags=1, w=ws, wb=nb,
             out=fake):
        return lib.ghf_relation_rows(x, ix, rel, W, bias, perm, goff, rows_x, B_, R_, d_, flags, w, wb, out, None)

    for kw in (dict(x=None), dict(rel=None), dict(W=None), dict(perm=None), dict(goff=None), dict(w=None), dict(out=None)):
        assert rows(**kw) == -1, kw
        assert b"null" in lib.ghf_last_error()
    assert rows(d_=0) == -1 and rows(d_=-4) == -1
    assert rows(d_=257) == -3 and rows(d_=512) == -3                         # GHF_EUNSUPPORTED: the rank calls' range
    assert rows(B_=0) == -1 and rows(R_=0) == -1 and rows(rows_x=0) == -1
    assert rows(flags=4) == -1 and b"flags" in lib.ghf_last_error()
    assert rows(ix=None, rows_x=B - 1) == -1                                  # no index list: B rows of x are needed
    assert rows(wb=nb - 1) == -1 and b"workspace" in lib.ghf_last_error()
    assert rows(wb=0) == -1
    assert rows(w=ctypes.c_void_p((1 << 20) + 8)) == -1 and b"aligned" in lib.ghf_last_error()
    assert rows(B_=B * 100) == -1                                              # a workspace sized for fewer queries


def test_cpu_tensors_raise_before_any_device_work():
    dec = pkg.RelationDecoder(text_dim=32, hidden_dim=16).eval()
    embs, rel_embs = torch.randn(8, 16), torch.randn(3, 32)
    nodes, rel, tail = torch.tensor([0, 1]), torch.tensor([2, 0]), torch.tensor([5, 6])
    with pytest.raises(RuntimeError, match="HIP device only"):
        dec(embs, nodes, rel, rel_embs)
    with pytest.raises(RuntimeError, match="HIP device only"):
        dec(embs, nodes, rel, rel_embs, direction="head")
    with pytest.raises(RuntimeError, match="HIP device only"):
        dec.score(embs, nodes, rel, tail, rel_embs)
    with pytest.raises(ValueError, match="direction"):
        dec(embs, nodes, rel, rel_embs, direction="both")
    with pytest.raises(RuntimeError, match="no CPU"):
        _native.relation_rows(embs, rel, torch.zeros(3, 16, 16), ix=nodes)
    m = HyperGNN(text_dim=32, node_feat_dim=16, hidden_dim=16).eval()
    Q = torch.randn(2, 16)
    with pytest.raises(RuntimeError, match="HIP device only"):
        m.rank_candidates(embs, nodes, tail, query_rows=Q)
    with pytest.raises(RuntimeError, match="HIP device only"):
        m.topk_candidates(embs, nodes, 3, query_rows=Q)
    with pytest.raises(RuntimeError, match="HIP device only"):
        m.softmax_loss(embs, nodes, tail, query_rows=Q)


def test_bad_typed_arguments_raise():
    embs = torch.zeros(12, 4)
    src, dst, rel = torch.tensor([0, 1, 2]), torch.tensor([3, 4, 5]), torch.tensor([0, 1, 2])
    query, qrel = torch.tensor([0, 1]), torch.tensor([0, 1])
    with pytest.raises(ValueError, match="query_rel"):                       # query_rel without a three-member known
        HyperGNN._filter_lists(embs, query, (src, dst), None, None, qrel)
    with pytest.raises(ValueError, match="query_rel"):
        HyperGNN._filter_lists(embs, query, None, None, None, qrel)
    with pytest.raises(ValueError, match="query_rel"):                       # and the reverse
        HyperGNN._filter_lists(embs, query, (src, dst, rel), None, None)
    with pytest.raises(ValueError):                                          # length mismatches
        HyperGNN._filter_lists(embs, query, (src, dst, rel), None, None, torch.tensor([0, 1, 2]))
    with pytest.raises(ValueError):
        HyperGNN._filter_lists(embs, query, (src, dst, rel[:2]), None, None, qrel)
    with pytest.raises(ValueError, match="negative"):                        # relation ids do not wrap
        HyperGNN._filter_lists(embs, query, (src, dst, torch.tensor([0, -1, 2])), None, None, qrel)
    with pytest.raises(ValueError, match="negative"):
        HyperGNN._filter_lists(embs, query, (src, dst, rel), None, None, torch.tensor([0, -1]))
    with pytest.raises(TypeError):
        HyperGNN._filter_lists(embs, query, (src, dst, rel), None, None, torch.tensor([0.0, 1.0]))
    with pytest.raises(ValueError, match="64-bit"):                          # (N R + R) N must fit the keys
        HyperGNN._filter_lists(torch.zeros(1, 1).expand(1 << 24, 1), query, (src, dst, torch.tensor([0, 1, 1 << 20])), None, None, qrel)
    with pytest.raises(ValueError):
        HyperGNN._filter_lists(embs, query, (src, dst, rel, rel), None, None, qrel)
    # query_rows: one fp32 row of width d per query, checked before anything needs the device
    m = HyperGNN(text_dim=32, node_feat_dim=16, hidden_dim=16).eval()
    embs16, tail = torch.randn(12, 16), torch.tensor([5, 6])
    for bad in (torch.randn(3, 16), torch.randn(2, 8), torch.randn(2 * 16), torch.randn(2, 16, 1)):
        with pytest.raises(ValueError, match="query_rows"):
            m.softmax_loss(embs16, query, tail, query_rows=bad)
        with pytest.raises(ValueError, match="query_rows"):
            HyperGNN._query_rows(embs16, query, bad, "rank_candidates")
    with pytest.raises(TypeError):
        m.softmax_loss(embs16, query, tail, query_rows=torch.randn(2, 16, dtype=torch.float64))


def test_typed_filter_lists_equal_a_brute_force_set_construction():
    """12 nodes, 3 relations, hand-written: parallel edges (same ends, other relation), a repeated triple, and a query with
    no edge of its relation."""
    embs = torch.zeros(12, 4)
    triples = [(3, 0, 5), (3, 1, 5),             # parallel edges 3 -> 5 under relations 0 and 1
               (3, 0, 4), (3, 0, 5),             # a repeated triple
               (3, 2, 11), (3, 0, 0),
               (1, 1, 2), (1, 1, 9), (1, 0, 9),
               (7, 2, 0), (7, 2, 7), (11, 0, 3), (0, 1, 0), (3, 1, 10)]
    src = torch.tensor([t[0] for t in triples])
    rel = torch.tensor([t[1] for t in triples])
    dst = torch.tensor([t[2] for t in triples])
    query = torch.tensor([3, 3, 3, 1, 1, 7, 7, 5, 0, 11, 3])
    qrel = torch.tensor([0, 1, 2, 1, 2, 2, 0, 0, 1, 0, 0])                 # (1, 2), (7, 0), (5, 0): no edge of that relation
    ptr, idx = HyperGNN._filter_lists(embs, query, (src, dst, rel), None, None, qrel)
    want = [sorted({d for s, r, d in triples if s == q and r == qr}) for q, qr in zip(query.tolist(), qrel.tolist())]
    assert want[0] == [0, 4, 5] and want[4] == [] and want[6] == [] and want[7] == []
    assert ptr.dtype == torch.int64 and idx.dtype == torch.int64
    assert ptr.tolist() == [0] + [sum(len(w) for w in want[:i + 1]) for i in range(len(want))]
    assert idx.tolist() == [v for w in want for v in w]
    # int32 ids and a larger relation id space give the same lists
    ptr32, idx32 = HyperGNN._filter_lists(embs, query.int(), (src.int(), dst.int(), rel.int()), None, None, qrel.int())
    assert torch.equal(ptr32, ptr) and torch.equal(idx32, idx)
    # no edge of any query's relation: no lists at all
    assert HyperGNN._filter_lists(embs, torch.tensor([5, 1]), (src, dst, rel), None, None, torch.tensor([0, 2])) == (None, None)
    # one relation throughout is the two-member form
    ptr2, idx2 = HyperGNN._filter_lists(embs, query, (src, dst), None, None)
    ptr1, idx1 = HyperGNN._filter_lists(embs, query, (src, dst, torch.full_like(rel, 2)), None, None, torch.full_like(qrel, 2))
    assert torch.equal(ptr1, ptr2) and torch.equal(idx1, idx2)
    # and the two-member form gives what it always gave
    want2 = [sorted({d for s, _, d in triples if s == q}) for q in query.tolist()]
    assert idx2.tolist() == [v for w in want2 for v in w]
    assert ptr2.tolist() == [0] + [sum(len(w) for w in want2[:i + 1]) for i in range(len(want2))]
    # negative node ids wrap, as everywhere
    ptrn, idxn = HyperGNN._filter_lists(embs, query, (src - 12, dst - 12, rel), None, None, qrel)
    assert torch.equal(ptrn, ptr) and torch.equal(idxn, idx)
