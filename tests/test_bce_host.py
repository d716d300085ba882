"""Host-side checks of the multi-label 1-vs-all BCE loss (HyperGNN.bce_loss, ghf_score_bce_fwd / _bwd): no GPU needed."""

import ctypes
import inspect
import os
import re

import pytest
import torch

from graph_hypernetwork_forge_amd import HyperGNN, _build, _native, autograd

BCE_CALLS = ("ghf_score_bce_workspace_bytes", "ghf_score_bce_fwd", "ghf_score_bce_bwd_workspace_bytes", "ghf_score_bce_bwd")


def test_bce_entry_points_are_declared_bound_and_exported():
    with open(os.path.join(_build.INCLUDE, "ghf.h")) as f:
        text = f.read()
    assert re.search(r"#define GHF_ABI_VERSION 15\b", text)            # entry points were added only
    assert "bce.hip" in _build.SOURCES
    lib = _native.load()
    assert lib.ghf_abi_version() == 15 and _native.ABI_VERSION == 15
    for name in BCE_CALLS:
        assert name in _native.header_symbols() and name in _native.SIGNATURES
        assert hasattr(lib, name), f"libghf_hip.so does not export {name}"
    assert callable(HyperGNN.bce_loss)
    assert issubclass(autograd.BceLossFn, torch.autograd.Function)     # one Function: query ids, or the query rows given
    assert {"rows", "query"} <= set(inspect.signature(autograd.BceLossFn.forward).parameters)
    assert callable(_native.score_bce_fwd) and callable(_native.score_bce_bwd)


def test_workspace_queries_without_a_gpu():
    lib = _native.load()
    B, N = 1024, 1_000_000
    fwd = lib.ghf_score_bce_workspace_bytes(B, N, 128)
    # a flag per query plus one triple of floats per (query, candidate slab), at most 128 slabs: far from a score matrix
    assert 4 * B + 12 * B <= fwd <= 4 * B + 12 * 128 * B + 512
    assert fwd < B * N * 4 // 256
    assert lib.ghf_score_bce_workspace_bytes(1, 1, 16) > 0
    assert lib.ghf_score_bce_workspace_bytes(2 * B, N, 128) > fwd                      # grows with B
    assert lib.ghf_score_bce_workspace_bytes(B, 100, 128) < fwd                        # fewer slabs when N is small
    # the slabs depend on N and d alone: the bytes per query do not change with B
    per_q = (lib.ghf_score_bce_workspace_bytes(4096, N, 128) - lib.ghf_score_bce_workspace_bytes(2048, N, 128)) // 2048
    assert per_q == (lib.ghf_score_bce_workspace_bytes(8192, N, 128) - lib.ghf_score_bce_workspace_bytes(4096, N, 128)) // 4096
    bwd = lib.ghf_score_bce_bwd_workspace_bytes(B, N, 128)
    assert bwd >= B * 128 * 4                                                          # at least one [B, d] partial of dq
    assert bwd == lib.ghf_score_softmax_bwd_workspace_bytes(B, N, 128)                 # the same sweep, the same partials
    assert bwd <= B * N * 4 // 32
    for bad in ((0, N, 128), (B, 0, 128), (B, N, 0), (B, N, -4), (B, N, 257), (-1, N, 128), (B, 1 << 31, 128), (1 << 31, N, 128)):
        assert lib.ghf_score_bce_workspace_bytes(*bad) == 0, bad
        assert lib.ghf_score_bce_bwd_workspace_bytes(*bad) == 0, bad


def test_bce_entry_points_reject_invalid_arguments_without_a_gpu():
    lib = _native.load()
    fake = ctypes.c_void_p(4096)            # never dereferenced: every call below fails its checks on the host
    ws = ctypes.c_void_p(1 << 20)
    B, N, d = 100, 5000, 64
    nf, nb = lib.ghf_score_bce_workspace_bytes(B, N, d), lib.ghf_score_bce_bwd_workspace_bytes(B, N, d)

    def fwd(q=fake, c=fake, iq=fake, pp=None, pi=None, nnz=0, rows_q=N, N_=N, B_=B, d_=d, scale=1.0, sm=0.1, w=ws, wb=nf, loss=fake):
        return lib.ghf_score_bce_fwd(q, c, iq, pp, pi, nnz, rows_q, N_, B_, d_, scale, sm, w, wb, loss, None)

    def bwd(q=fake, c=fake, iq=fake, pp=None, pi=None, nnz=0, rows_q=N, N_=N, B_=B, d_=d, scale=1.0, sm=0.1, loss=fake, g=fake,
            w=ws, wb=nb, dq=fake, dc=fake):
        return lib.ghf_score_bce_bwd(q, c, iq, pp, pi, nnz, rows_q, N_, B_, d_, scale, sm, loss, g, w, wb, dq, dc, None)

    for call, nulls in ((fwd, ("q", "c", "w", "loss")), (bwd, ("q", "c", "loss", "g", "w", "dq", "dc"))):
        for name in nulls:
            assert call(**{name: None}) == -1, name
            assert b"null" in lib.ghf_last_error()
        assert call(nnz=5) == -1 and b"positive list" in lib.ghf_last_error()       # nnz > 0 without lists
        assert call(pp=fake, nnz=5) == -1 and call(pi=fake, nnz=5) == -1
        for bad_scale in (0.0, -1.0, float("inf"), float("nan")):
            assert call(scale=bad_scale) == -1 and b"scale" in lib.ghf_last_error(), bad_scale
        for bad_sm in (1.0, 1.5, -0.01, float("nan"), float("inf")):
            assert call(sm=bad_sm) == -1 and b"smoothing" in lib.ghf_last_error(), bad_sm
        assert call(d_=0) == -1 and call(d_=-8) == -1
        assert call(B_=0) == -1 and call(N_=0) == -1 and call(rows_q=0) == -1 and call(nnz=-1) == -1
        assert call(iq=None, rows_q=B - 1) == -1                                       # no index list: B rows of q are needed
        assert call(w=ctypes.c_void_p((1 << 20) + 4)) == -1 and b"aligned" in lib.ghf_last_error()
        assert call(d_=512, wb=1 << 30) == -3                                          # GHF_EUNSUPPORTED
    assert fwd(wb=nf - 1) == -1 and b"workspace" in lib.ghf_last_error()
    assert bwd(wb=nb - 1) == -1 and b"workspace" in lib.ghf_last_error()


def test_python_arguments_are_checked_in_order_before_any_device_work():
    m = HyperGNN(text_dim=32, node_feat_dim=16, hidden_dim=16).eval()
    embs = torch.randn(12, 16)
    q = torch.tensor([0, 1])
    src, dst, rel = torch.tensor([0, 1, 2]), torch.tensor([3, 4, 5]), torch.tensor([0, 1, 2])
    with pytest.raises(ValueError, match=r"\[N, d\]"):
        m.bce_loss(embs[0], q)
    for bad in (torch.randn(3, 16), torch.randn(2, 8), torch.randn(2 * 16)):                # query_rows: before scale
        with pytest.raises(ValueError, match="query_rows"):
            m.bce_loss(embs, q, query_rows=bad, scale=-1.0)
    with pytest.raises(TypeError):
        m.bce_loss(embs, q, query_rows=torch.randn(2, 16, dtype=torch.float64))
    for bad_scale in (0.0, -2.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="scale"):                                      # scale: before smoothing and the ids
            m.bce_loss(embs, torch.tensor([99]), scale=bad_scale, smoothing=1.0)
    for bad_sm in (1.0, 1.25, -0.1, float("nan")):
        with pytest.raises(ValueError, match="smoothing"):                                  # smoothing: before the ids
            m.bce_loss(embs, torch.tensor([99]), smoothing=bad_sm)
    with pytest.raises(IndexError):                                                         # the ids: before the lists' form
        m.bce_loss(embs, torch.tensor([12]), known=(src, dst, rel))
    with pytest.raises(TypeError):
        m.bce_loss(embs, torch.tensor([0.5]))
    with pytest.raises(ValueError, match="query_rel"):                                      # typed known without query_rel
        m.bce_loss(embs, q, known=(src, dst, rel))
    with pytest.raises(ValueError, match="query_rel"):                                      # and the reverse
        m.bce_loss(embs, q, known=(src, dst), query_rel=torch.tensor([0, 1]))
    with pytest.raises(ValueError, match="not both"):
        m.bce_loss(embs, q, known=(src, dst), pos_ptr=torch.tensor([0, 0, 0]), pos_idx=torch.tensor([], dtype=torch.int64))
    with pytest.raises(RuntimeError, match="HIP device only"):                              # everything in order, on the host
        m.bce_loss(embs, q, known=(src, dst), smoothing=0.1)
    with pytest.raises(RuntimeError, match="HIP device only"):
        m.bce_loss(embs, q, query_rows=torch.randn(2, 16))
    with pytest.raises(RuntimeError, match="no CPU"):                                       # the typed wrappers refuse host tensors
        _native.score_bce_fwd(embs, embs, iq=q)
    with pytest.raises(RuntimeError, match="no CPU"):
        _native.score_bce_bwd(embs, embs, torch.zeros(2), torch.ones(2), iq=q)
    # the shared form check is the one the filter lists always made: same messages through _filter_lists
    with pytest.raises(ValueError, match="query_rel"):
        HyperGNN._filter_lists(embs, q, (src, dst, rel), None, None)
