"""Host-side checks of relation prediction, (head, ?, tail): the ghf_relation_scores entry points, their argument checks,
RelationDecoder.score_relations / rank_relations / topk_relations / relation_loss and the helpers behind them
(_relation_filter_lists, _ranks_from_scores, _topk_from_scores, _loss_from_scores).  No GPU needed."""

import ctypes
import os
import re

import pytest
import torch
import torch.nn.functional as F

import graph_hypernetwork_forge_amd as pkg
from graph_hypernetwork_forge_amd import RelationDecoder, _build, _native, autograd

CALLS = ("ghf_relation_scores", "ghf_relation_scores_bwd_rows_workspace_bytes", "ghf_relation_scores_bwd_rows",
         "ghf_relation_scores_bwd_weights_workspace_bytes", "ghf_relation_scores_bwd_weights")
METHODS = ("score_relations", "rank_relations", "topk_relations", "relation_loss", "_relation_filter_lists",
           "_ranks_from_scores", "_topk_from_scores", "_loss_from_scores")


def test_entry_points_are_declared_bound_and_exported():
    with open(os.path.join(_build.INCLUDE, "ghf.h")) as f:
        text = f.read()
    assert re.search(r"#define GHF_ABI_VERSION 15\b", text)                     # entry points added, nothing changed
    assert "relation_predict.hip" in _build.SOURCES
    lib = _native.load()
    assert lib.ghf_abi_version() == 15
    for name in CALLS:
        assert name in _native.header_symbols() and name in _native.SIGNATURES
        assert hasattr(lib, name), f"libghf_hip.so does not export {name}"
    for name in ("relation_scores", "relation_scores_bwd_rows", "relation_scores_bwd_weights"):
        assert callable(getattr(_native, name))
    for name in METHODS:
        assert callable(getattr(RelationDecoder, name)), name
    assert issubclass(autograd.RelationScoresFn, torch.autograd.Function)


def test_workspace_queries_without_a_gpu():
    lib = _native.load()
    for q in (lib.ghf_relation_scores_bwd_rows_workspace_bytes, lib.ghf_relation_scores_bwd_weights_workspace_bytes):
        for B, U, d in ((150, 7, 20), (150, 37, 128), (1, 1, 1), (16384, 237, 128), (1 << 20, 64, 256)):
            n = q(B, U, d)
            assert n > 0 and n % 256 == 0, (B, U, d, n)
        for bad in ((0, 7, 64), (-1, 7, 64), (150, 0, 64), (150, -2, 64), (1 << 31, 7, 64), (150, 1 << 23, 64), (150, 7, 0),
                    (150, 7, -3), (150, 7, 257)):
            assert q(*bad) == 0, bad
    # nothing of size B x U x d: the partials stay below 600 tiles' worth of rows / 600 work items' worth of matrices
    B, U, d = 16384, 237, 128
    assert lib.ghf_relation_scores_bwd_rows_workspace_bytes(B, U, d) <= 2 * B * d * 4 + 256
    assert lib.ghf_relation_scores_bwd_rows_workspace_bytes(1 << 20, U, d) == 256           # tiles enough: no split, no partials
    assert lib.ghf_relation_scores_bwd_rows_workspace_bytes(1024, U, d) <= 600 * 64 * d * 4
    assert lib.ghf_relation_scores_bwd_weights_workspace_bytes(B, U, d) <= 2 * U * (d * d + d) * 4 + 256
    assert lib.ghf_relation_scores_bwd_weights_workspace_bytes(B, 7, d) <= 600 * 64 * (d + 1) * 4 + 256


def test_the_calls_reject_invalid_arguments_without_a_gpu():
    lib = _native.load()
    fake = ctypes.c_void_p(4096)            # never dereferenced: every call below fails its checks on the host
    ws = ctypes.c_void_p(1 << 20)
    B, U, N, d = 150, 7, 5003, 64

    def fwd(x=fake, ia=fake, ib=fake, W=fake, bias=fake, rows_x=N, B_=B, U_=U, d_=d, flags=1, out=fake):
        return lib.ghf_relation_scores(x, ia, ib, W, bias, rows_x, B_, U_, d_, flags, out, None)

    nr = lib.ghf_relation_scores_bwd_rows_workspace_bytes(B, U, d)

    def rows(x=fake, ia=fake, G=fake, W=fake, bias=fake, rows_x=N, B_=B, U_=U, d_=d, flags=1, w=ws, wb=nr, out=fake):
        return lib.ghf_relation_scores_bwd_rows(x, ia, G, W, bias, rows_x, B_, U_, d_, flags, w, wb, out, None)

    nw = lib.ghf_relation_scores_bwd_weights_workspace_bytes(B, U, d)

    def wts(x=fake, ia=fake, ib=fake, G=fake, rows_x=N, B_=B, U_=U, d_=d, flags=0, w=ws, wb=nw, dW=fake, db=fake):
        return lib.ghf_relation_scores_bwd_weights(x, ia, ib, G, rows_x, B_, U_, d_, flags, w, wb, dW, db, None)

    nulls = {fwd: ("x", "ia", "ib", "W", "out"), rows: ("x", "ia", "G", "W", "w", "out"), wts: ("x", "ia", "ib", "G", "w", "dW")}
    for call, names in nulls.items():
        for name in names:
            assert call(**{name: None}) == -1, (call.__name__, name)
            assert b"null" in lib.ghf_last_error()
        assert call(d_=0) == -1 and call(d_=-4) == -1
        assert call(d_=257) == -3 and call(d_=512) == -3                       # GHF_EUNSUPPORTED: the rank calls' range
        assert b"256" in lib.ghf_last_error()
        assert call(B_=0) == -1 and call(U_=0) == -1 and call(rows_x=0) == -1
        assert call(B_=1 << 31) == -1 and call(U_=1 << 23) == -1
        assert call(flags=4) == -1 and b"flags" in lib.ghf_last_error()
    assert wts(flags=1) == -1 and b"flags" in lib.ghf_last_error()             # the weight gradients define no flag
    assert nr > 256 and nw > 256                                                # B = 150: three tiles / slabs, so partials
    for call, nb in ((rows, nr), (wts, nw)):
        assert call(wb=nb - 1) == -1 and b"workspace" in lib.ghf_last_error()
        assert call(wb=0) == -1
        assert call(w=ctypes.c_void_p((1 << 20) + 8)) == -1 and b"aligned" in lib.ghf_last_error()


def _cpu_problem():
    dec = RelationDecoder(text_dim=32, hidden_dim=16).eval()
    embs, rel_embs = torch.randn(8, 16), torch.randn(3, 32)
    head, tail, rel = torch.tensor([0, 1]), torch.tensor([5, 6]), torch.tensor([2, 0])
    return dec, embs, rel_embs, head, tail, rel


def test_cpu_tensors_raise_before_any_device_work():
    dec, embs, rel_embs, head, tail, rel = _cpu_problem()
    known = (torch.tensor([0]), torch.tensor([5]), torch.tensor([1]))
    for direction in ("tail", "head"):
        with pytest.raises(RuntimeError, match="HIP device only"):
            dec.score_relations(embs, head, tail, rel_embs, direction=direction)
    with pytest.raises(RuntimeError, match="HIP device only"):
        dec.rank_relations(embs, head, tail, rel, rel_embs, known=known)
    with pytest.raises(RuntimeError, match="HIP device only"):
        dec.topk_relations(embs, head, tail, 2, rel_embs, known=known)
    with pytest.raises(RuntimeError, match="HIP device only"):
        dec.relation_loss(embs, head, tail, rel, rel_embs, scale=0.25, known=known)
    W = torch.zeros(3, 16, 16)
    with pytest.raises(RuntimeError, match="no CPU"):
        _native.relation_scores(embs, head, tail, W)
    with pytest.raises(RuntimeError, match="no CPU"):
        _native.relation_scores_bwd_rows(embs, head, torch.zeros(2, 3), W)
    with pytest.raises(RuntimeError, match="no CPU"):
        _native.relation_scores_bwd_weights(embs, head, tail, torch.zeros(2, 3))


def test_bad_arguments_raise():
    dec, embs, rel_embs, head, tail, rel = _cpu_problem()
    calls = {
        "score": lambda h=head, t=tail, r=rel, e=embs, re_=rel_embs, **kw: dec.score_relations(e, h, t, re_, **kw),
        "rank": lambda h=head, t=tail, r=rel, e=embs, re_=rel_embs, **kw: dec.rank_relations(e, h, t, r, re_, **kw),
        "topk": lambda h=head, t=tail, r=rel, e=embs, re_=rel_embs, **kw: dec.topk_relations(e, h, t, 2, re_, **kw),
        "loss": lambda h=head, t=tail, r=rel, e=embs, re_=rel_embs, **kw: dec.relation_loss(e, h, t, r, re_, **kw),
    }
    for name, call in calls.items():
        with pytest.raises(ValueError, match="direction"):
            call(direction="both")
        with pytest.raises(ValueError):                                       # mismatched lengths
            call(t=torch.tensor([5, 6, 7]))
        with pytest.raises(ValueError):
            call(h=torch.tensor([], dtype=torch.int64), t=torch.tensor([], dtype=torch.int64), r=torch.tensor([], dtype=torch.int64))
        with pytest.raises(TypeError):                                        # float ids
            call(h=torch.tensor([0.0, 1.0]))
        with pytest.raises(IndexError):                                       # node ids are checked as indexing checks them
            call(t=torch.tensor([5, 8]))
        with pytest.raises(ValueError, match="embs"):
            call(e=torch.randn(8, 12))
        with pytest.raises(ValueError, match="rel_embs"):
            call(re_=torch.randn(3, 16))
    for name in ("rank", "loss"):
        with pytest.raises(ValueError, match="negative"):                    # relation ids do not wrap
            calls[name](r=torch.tensor([2, -1]))
        with pytest.raises(ValueError):
            calls[name](r=torch.tensor([2, 0, 1]))
        with pytest.raises(TypeError):
            calls[name](r=torch.tensor([2.0, 0.0]))
        with pytest.raises(IndexError):
            calls[name](r=torch.tensor([2, 3]))                               # three texts: ids 0..2
    for name in ("rank", "topk", "loss"):
        with pytest.raises(ValueError, match="known"):
            calls[name](known=(head, tail))
    for k in (0, -1, 129):
        with pytest.raises(ValueError, match="1..128"):
            dec.topk_relations(embs, head, tail, k, rel_embs)
    for scale in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="scale"):
            dec.relation_loss(embs, head, tail, rel, rel_embs, scale=scale)
    with pytest.raises(ValueError, match="negative"):
        RelationDecoder._relation_filter_lists(embs, head, tail, rel, (head, tail, torch.tensor([0, -2])))
    with pytest.raises(ValueError, match="negative"):
        RelationDecoder._relation_filter_lists(embs, head, tail, torch.tensor([0, -2]), (head, tail, rel))
    with pytest.raises(TypeError):
        RelationDecoder._relation_filter_lists(embs, head, tail, rel, (head, tail, torch.tensor([0.0, 1.0])))
    with pytest.raises(ValueError):
        RelationDecoder._relation_filter_lists(embs, head, tail, rel, (head, tail, rel, rel))
    with pytest.raises(ValueError, match="64-bit"):
        RelationDecoder._relation_filter_lists(torch.zeros(1, 1).expand(1 << 28, 1), head, tail, rel,
                                               (head, tail, torch.tensor([0, 1 << 10])))


# ---- the filter lists -------------------------------------------------------------------------------------------------------
N_NODES, N_REL = 12, 4
TRIPLES = [(3, 0, 5), (3, 1, 5), (3, 3, 5),      # the same pair under three relations
           (3, 1, 5),                            # a repeated triple
           (5, 2, 3),                            # 5 -> 3 only: says nothing about 3 -> 5 ...
           (9, 2, 4),                            # ... and (4, ?, 9) has the reverse edge only
           (1, 1, 2), (1, 0, 2), (7, 2, 7), (0, 3, 11), (11, 3, 0), (6, 0, 8)]
PAIRS = [(3, 5, 0), (3, 5, 1), (3, 5, 2), (5, 3, 2), (4, 9, 2), (10, 10, 0), (1, 2, 1), (7, 7, 2), (0, 11, 3), (6, 8, 0), (2, 1, 1)]


def brute_lists(pairs, triples, with_target):
    return [sorted({r for s, r, t in triples if s == h and t == ta and (with_target or r != q)}) for h, ta, q in pairs]


def test_relation_filter_lists_equal_a_brute_force_set_construction():
    embs = torch.zeros(N_NODES, 4)
    src = torch.tensor([t[0] for t in TRIPLES])
    rel = torch.tensor([t[1] for t in TRIPLES])
    dst = torch.tensor([t[2] for t in TRIPLES])
    head = torch.tensor([p[0] for p in PAIRS])
    tail = torch.tensor([p[1] for p in PAIRS])
    qrel = torch.tensor([p[2] for p in PAIRS])
    want = brute_lists(PAIRS, TRIPLES, False)
    assert want[0] == [1, 3] and want[1] == [0, 3] and want[2] == [0, 1, 3]      # three relations; the target itself is not listed
    assert want[3] == [] and want[4] == [] and want[5] == []                      # own target only; the reverse edge only; nothing known
    ptr, idx = RelationDecoder._relation_filter_lists(embs, head, tail, qrel, (src, dst, rel))
    assert ptr.dtype == torch.int64 and idx.dtype == torch.int64
    assert ptr.tolist() == [0] + [sum(len(w) for w in want[:i + 1]) for i in range(len(want))]
    assert idx.tolist() == [v for w in want for v in w]
    # without targets (top-k): every known relation of the pair
    want_all = brute_lists(PAIRS, TRIPLES, True)
    assert want_all[0] == [0, 1, 3] and want_all[3] == [2]
    ptr_a, idx_a = RelationDecoder._relation_filter_lists(embs, head, tail, None, (src, dst, rel))
    assert ptr_a.tolist() == [0] + [sum(len(w) for w in want_all[:i + 1]) for i in range(len(want_all))]
    assert idx_a.tolist() == [v for w in want_all for v in w]
    # int32 ids give the same lists; negative node ids wrap, as everywhere
    p32, i32 = RelationDecoder._relation_filter_lists(embs, head.int(), tail.int(), qrel.int(), (src.int(), dst.int(), rel.int()))
    assert torch.equal(p32, ptr) and torch.equal(i32, idx)
    pn, i_n = RelationDecoder._relation_filter_lists(embs, head - N_NODES, tail, qrel, (src, dst - N_NODES, rel))
    assert torch.equal(pn, ptr) and torch.equal(i_n, idx)
    # candidate texts fewer than the known relation ids: ids past them are dropped
    pc, ic = RelationDecoder._relation_filter_lists(embs, head, tail, qrel, (src, dst, rel), num_relations=3)
    want3 = [[r for r in w if r < 3] for w in want]
    assert ic.tolist() == [v for w in want3 for v in w] and pc[-1].item() == ic.numel()
    # nothing known about any pair: no lists
    assert RelationDecoder._relation_filter_lists(embs, torch.tensor([10, 2]), torch.tensor([10, 1]), torch.tensor([0, 1]),
                                                  (src, dst, rel)) == (None, None)
    assert RelationDecoder._relation_filter_lists(embs, head, tail, qrel, None) == (None, None)
    # only the pairs' own targets are known: nothing to leave out
    assert RelationDecoder._relation_filter_lists(embs, torch.tensor([5]), torch.tensor([3]), torch.tensor([2]),
                                                  (src, dst, rel)) == (None, None)


# ---- ranks, top-k and the loss from a score table ---------------------------------------------------------------------------
S_HAND = torch.tensor([[0.5, 2.0, 2.0, -1.0, 0.5],       # ties: 1 = 2 and 0 = 4
                       [3.0, 1.0, 0.0, 1.0, -2.0],       # the maximum (0) is listed
                       [1.0, 1.0, 1.0, 1.0, 1.0],        # everything ties
                       [0.0, 4.0, -3.0, 2.0, 1.0],       # all but the target and one more are listed: fewer than k survivors
                       [-1.0, -2.0, 0.25, 7.0, 7.0]])    # no list
REL_HAND = torch.tensor([0, 1, 3, 2, 4])
LISTS_HAND = [[3], [0, 4], [], [0, 1, 4], []]


def _csr(lists):
    ptr = torch.tensor([0] + [sum(len(w) for w in lists[:i + 1]) for i in range(len(lists))], dtype=torch.int64)
    return ptr, torch.tensor([v for w in lists for v in w], dtype=torch.int64)


def test_ranks_from_scores_equal_a_python_loop():
    ptr, idx = _csr(LISTS_HAND)
    g, e = RelationDecoder._ranks_from_scores(S_HAND, REL_HAND, ptr, idx)
    assert g.dtype == torch.int64 and e.dtype == torch.int64
    for i, row in enumerate(S_HAND.tolist()):
        t = REL_HAND[i].item()
        others = [u for u in range(len(row)) if u != t and u not in LISTS_HAND[i]]
        assert g[i].item() == sum(row[u] > row[t] for u in others), i
        assert e[i].item() == sum(row[u] == row[t] for u in others), i
    assert g.tolist() == [2, 0, 0, 1, 0] and e.tolist() == [1, 1, 4, 0, 1]
    g0, e0 = RelationDecoder._ranks_from_scores(S_HAND, REL_HAND)                  # unfiltered
    assert g0.tolist() == [2, 1, 0, 4, 0] and e0.tolist() == [1, 1, 4, 0, 1]
    g1, e1 = RelationDecoder._ranks_from_scores(torch.tensor([[3.0]]), torch.tensor([0]))       # U = 1: nothing to compare with
    assert g1.tolist() == [0] and e1.tolist() == [0]
    assert pkg.link_prediction_metrics(g, e)["mrr"] > 0


def test_topk_from_scores_is_score_descending_id_ascending():
    ptr, idx = _csr(LISTS_HAND)
    k = 3
    s, ids = RelationDecoder._topk_from_scores(S_HAND, k, ptr, idx)
    assert s.shape == (5, k) and ids.shape == (5, k) and ids.dtype == torch.int64
    for i, row in enumerate(S_HAND.tolist()):
        left = sorted((u for u in range(len(row)) if u not in LISTS_HAND[i]), key=lambda u: (-row[u], u))[:k]
        pad = k - len(left)
        assert ids[i].tolist() == left + [-1] * pad, i
        assert s[i].tolist() == [row[u] for u in left] + [float("-inf")] * pad, i
    assert ids[0].tolist() == [1, 2, 0] and ids[1].tolist() == [1, 3, 2] and ids[2].tolist() == [0, 1, 2]
    assert ids[3].tolist() == [3, 2, -1]                                            # two survivors, then padding
    # k beyond U pads; U = 1; a listed only candidate leaves nothing
    s8, i8 = RelationDecoder._topk_from_scores(S_HAND, 8)
    assert i8[4].tolist() == [3, 4, 2, 0, 1, -1, -1, -1] and bool(torch.isinf(s8[:, 5:]).all())
    s1, i1 = RelationDecoder._topk_from_scores(torch.tensor([[3.0]]), 2)
    assert i1.tolist() == [[0, -1]] and s1.tolist() == [[3.0, float("-inf")]]
    s1, i1 = RelationDecoder._topk_from_scores(torch.tensor([[3.0]]), 1, *_csr([[0]]))
    assert i1.tolist() == [[-1]] and s1.tolist() == [[float("-inf")]]
    # a score of -inf that is NOT listed is a candidate, after every finite one and before the padding
    s2, i2 = RelationDecoder._topk_from_scores(torch.tensor([[float("-inf"), 1.0, 5.0]]), 3, *_csr([[2]]))
    assert i2.tolist() == [[1, 0, -1]]


def test_loss_from_scores_equals_masked_cross_entropy_in_float64():
    S = S_HAND.double()
    lists = [l + ([REL_HAND[i].item()] if i == 2 else []) for i, l in enumerate(LISTS_HAND)]     # the target listed: it stays in
    ptr, idx = _csr(lists)
    for scale in (1.0, 0.25):
        got = RelationDecoder._loss_from_scores(S, REL_HAND, ptr, idx, scale)
        logits = scale * S.clone()
        for i, l in enumerate(LISTS_HAND):
            logits[i, l] = float("-inf")
        want = F.cross_entropy(logits, REL_HAND, reduction="none")
        assert got.dtype == torch.float64 and torch.allclose(got, want, rtol=1e-13, atol=1e-13), (got, want)
    got1 = RelationDecoder._loss_from_scores(torch.tensor([[3.0]], dtype=torch.float64), torch.tensor([0]))
    assert got1.tolist() == [0.0]                                                    # U = 1: the target is the whole sum
    # differentiable in S: the gradient is softmax - onehot over the surviving relations, zero on the listed ones
    Sg = S.clone().requires_grad_(True)
    RelationDecoder._loss_from_scores(Sg, REL_HAND, ptr, idx).sum().backward()
    assert Sg.grad[1, 0].item() == 0 and Sg.grad[1, 4].item() == 0 and abs(Sg.grad.sum(1)).max().item() < 1e-12
