"""Host-side checks of the rank / top-k link prediction (HyperGNN.rank_candidates, topk_candidates, ghf_score_rank,
ghf_score_topk): no GPU needed."""

import ctypes
import os
import re

import pytest
import torch

import graph_hypernetwork_forge_amd as pkg
from graph_hypernetwork_forge_amd import HyperGNN, _build, _native

RANK_CALLS = ("ghf_score_rank_workspace_bytes", "ghf_score_rank", "ghf_score_topk_workspace_bytes", "ghf_score_topk")


def test_rank_entry_points_are_declared_bound_and_exported():
    with open(os.path.join(_build.INCLUDE, "ghf.h")) as f:
        text = f.read()
    assert re.search(r"#define GHF_ABI_VERSION 15\b", text)
    assert "rank.hip" in _build.SOURCES
    lib = _native.load()
    assert lib.ghf_abi_version() == 15
    for name in RANK_CALLS:
        assert name in _native.header_symbols() and name in _native.SIGNATURES
        assert hasattr(lib, name), f"libghf_hip.so does not export {name}"
    assert "link_prediction_metrics" in pkg.__all__ and callable(pkg.link_prediction_metrics)
    assert callable(HyperGNN.rank_candidates) and callable(HyperGNN.topk_candidates)


def test_workspace_queries_without_a_gpu():
    lib = _native.load()
    B, N = 1024, 1_000_000
    rank = lib.ghf_score_rank_workspace_bytes(B, N, 128)
    assert 2 * 4 * B <= rank <= 64 * B                         # O(B): the target scores and a flag per query
    assert lib.ghf_score_rank_workspace_bytes(1, 1, 16) > 0
    for bad in ((0, N, 128), (B, 0, 128), (B, N, 0), (B, N, -4), (B, N, 257), (-1, N, 128), (B, 1 << 31, 128)):
        assert lib.ghf_score_rank_workspace_bytes(*bad) == 0, bad
    topk = lib.ghf_score_topk_workspace_bytes(B, N, 128, 10)
    assert topk >= B * 10 * 8                                  # at least one list of k (score, id) entries per query
    assert topk < B * N * 4 // 16                              # and far from a score matrix
    assert lib.ghf_score_topk_workspace_bytes(16384, N, 128, 10) < 16384 * N * 4 // 16
    assert lib.ghf_score_topk_workspace_bytes(B, N, 128, 128) > topk
    for bad in ((B, N, 128, 0), (B, N, 128, 129), (B, N, 128, -1), (0, N, 128, 10), (B, 0, 128, 10), (B, N, 0, 10),
                (B, N, 300, 10)):
        assert lib.ghf_score_topk_workspace_bytes(*bad) == 0, bad


def test_rank_entry_points_reject_invalid_arguments_without_a_gpu():
    lib = _native.load()
    fake = ctypes.c_void_p(4096)            # never dereferenced: every call below fails its checks on the host
    ws = ctypes.c_void_p(1 << 20)
    B, N, d = 100, 5000, 64
    nb = lib.ghf_score_rank_workspace_bytes(B, N, d)

    def rank(q=fake, c=fake, iq=fake, target=fake, fp=None, fi=None, nnz=0, rows_q=N, N_=N, B_=B, d_=d, w=ws, wb=nb, g=fake,
             e=fake):
        return lib.ghf_score_rank(q, c, iq, target, fp, fi, nnz, rows_q, N_, B_, d_, w, wb, g, e, None)

    for kw in (dict(q=None), dict(c=None), dict(target=None), dict(w=None), dict(g=None), dict(e=None)):
        assert rank(**kw) == -1, kw
        assert b"null" in lib.ghf_last_error()
    assert rank(nnz=5) == -1 and b"filter" in lib.ghf_last_error()            # nnz > 0 without lists
    assert rank(fp=fake, nnz=5) == -1
    assert rank(d_=0) == -1 and rank(d_=-8) == -1
    assert rank(B_=0) == -1 and rank(N_=0) == -1 and rank(rows_q=0) == -1 and rank(nnz=-1) == -1
    assert rank(iq=None, rows_q=B - 1) == -1                                  # no index list: B rows of q are needed
    assert rank(wb=nb - 1) == -1 and b"workspace" in lib.ghf_last_error()
    assert rank(w=ctypes.c_void_p((1 << 20) + 4)) == -1 and b"aligned" in lib.ghf_last_error()
    assert rank(d_=512, wb=1 << 30) == -3                                     # GHF_EUNSUPPORTED: wider than any model here

    k = 10
    tb = lib.ghf_score_topk_workspace_bytes(B, N, d, k)

    def topk(q=fake, c=fake, iq=fake, fp=None, fi=None, nnz=0, rows_q=N, N_=N, B_=B, d_=d, k_=k, w=ws, wb=tb, s=fake, i=fake):
        return lib.ghf_score_topk(q, c, iq, fp, fi, nnz, rows_q, N_, B_, d_, k_, w, wb, s, i, None)

    for kw in (dict(q=None), dict(c=None), dict(w=None), dict(s=None), dict(i=None)):
        assert topk(**kw) == -1, kw
        assert b"null" in lib.ghf_last_error()
    assert topk(nnz=3) == -1 and topk(fi=fake, nnz=3) == -1
    for bad_k in (0, -1, 129, 1 << 20):
        assert topk(k_=bad_k, wb=1 << 30) == -1 and b"k =" in lib.ghf_last_error()
    assert topk(d_=0) == -1 and topk(B_=0) == -1 and topk(N_=0) == -1
    assert topk(wb=tb - 1) == -1 and b"workspace" in lib.ghf_last_error()
    assert topk(wb=lib.ghf_score_topk_workspace_bytes(B, N, d, 1), k_=64) == -1   # sized for a smaller k
    assert topk(w=ctypes.c_void_p((1 << 20) + 8)) == -1


def test_link_prediction_metrics_against_hand_computed_values():
    greater = torch.tensor([0, 0, 2, 9, 0])
    equal = torch.tensor([0, 1, 0, 2, 4])
    # ranks 1 + g + e/2 = 1, 1.5, 3, 11, 3
    m = pkg.link_prediction_metrics(greater, equal)
    assert set(m) == {"mrr", "mean_rank", "hits@1", "hits@3", "hits@10"}
    assert m["mrr"] == pytest.approx((1 + 1 / 1.5 + 1 / 3 + 1 / 11 + 1 / 3) / 5, abs=1e-12)
    assert m["mean_rank"] == pytest.approx((1 + 1.5 + 3 + 11 + 3) / 5, abs=1e-12)
    assert m["hits@1"] == pytest.approx(1 / 5) and m["hits@3"] == pytest.approx(4 / 5) and m["hits@10"] == pytest.approx(4 / 5)
    m = pkg.link_prediction_metrics(greater, equal, ks=(2, 11))
    assert set(m) == {"mrr", "mean_rank", "hits@2", "hits@11"} and m["hits@2"] == pytest.approx(2 / 5) and m["hits@11"] == 1.0
    with pytest.raises(ValueError):
        pkg.link_prediction_metrics(torch.tensor([0, -1]), torch.tensor([0, -1]))
    with pytest.raises(ValueError):
        pkg.link_prediction_metrics(torch.tensor([0, 1]), torch.tensor([0]))


def test_cpu_tensors_raise_and_arguments_are_checked_before_any_device_work():
    m = HyperGNN(text_dim=32, node_feat_dim=16, hidden_dim=16).eval()
    embs = torch.randn(8, 16)
    q, t = torch.tensor([0, 1]), torch.tensor([2, 3])
    with pytest.raises(RuntimeError, match="HIP device only"):
        m.rank_candidates(embs, q, t)
    with pytest.raises(RuntimeError, match="HIP device only"):
        m.topk_candidates(embs, q, 3)
    with pytest.raises(RuntimeError, match="no CPU"):                   # the typed wrappers refuse host tensors too
        _native.score_rank(embs, embs, t, iq=q)
    with pytest.raises(RuntimeError, match="no CPU"):
        _native.score_topk(embs, embs, 3, iq=q)


def test_out_of_range_ids_raise_index_error():
    """As indexing raises; the check runs on the ids before anything needs the device."""
    embs = torch.randn(8, 16)
    for bad in ([0, 8], [-9], [100]):
        with pytest.raises(IndexError):
            HyperGNN._rank_ids(torch.tensor(bad), 8, embs, "query")
    got = HyperGNN._rank_ids(torch.tensor([3, -1, -8], dtype=torch.int32), 8, embs, "query")
    assert got.dtype == torch.int64 and got.tolist() == [3, 7, 0]
    with pytest.raises(ValueError):
        HyperGNN._rank_ids(torch.tensor([[0, 1]]), 8, embs, "query")
    with pytest.raises(TypeError):
        HyperGNN._rank_ids(torch.tensor([0.0]), 8, embs, "query")


def test_filter_lists_from_known_edges_and_from_csr_agree():
    """The host-side list building (plain torch, device-agnostic): partners of each query, sorted, repeats removed."""
    embs = torch.zeros(10, 4)
    src = torch.tensor([3, 1, 3, 3, 7, 1, 3])
    dst = torch.tensor([5, 2, 4, 5, 0, 9, 9])
    query = torch.tensor([3, 0, 1, 3])
    ptr, idx = HyperGNN._filter_lists(embs, query, (src, dst), None, None)
    assert ptr.tolist() == [0, 3, 3, 5, 8] and idx.tolist() == [4, 5, 9, 2, 9, 4, 5, 9]
    ptr2, idx2 = HyperGNN._filter_lists(embs, query, None, torch.tensor([0, 4, 4, 6, 9]), torch.tensor([9, 5, 4, 5, 9, 2, 5, 9, 4]))
    assert ptr2.tolist() == [0, 4, 4, 6, 9] and idx2.tolist() == [4, 5, 5, 9, 2, 9, 4, 5, 9]      # sorted inside each list
    assert HyperGNN._filter_lists(embs, query, None, None, None) == (None, None)
    assert HyperGNN._filter_lists(embs, query, (torch.tensor([8]), torch.tensor([8])), None, None) == (None, None)
    with pytest.raises(IndexError):
        HyperGNN._filter_lists(embs, query, (torch.tensor([10]), torch.tensor([0])), None, None)
    with pytest.raises(IndexError):
        HyperGNN._filter_lists(embs, query, None, torch.tensor([0, 1, 1, 1, 1]), torch.tensor([10]))
    with pytest.raises(ValueError):
        HyperGNN._filter_lists(embs, query, None, torch.tensor([0, 1, 1, 1, 2]), torch.tensor([1]))
    with pytest.raises(ValueError):
        HyperGNN._filter_lists(embs, query, (src, dst), torch.tensor([0, 0, 0, 0, 0]), torch.tensor([], dtype=torch.int64))
