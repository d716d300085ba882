"""Host-side checks of the 1-vs-all softmax link-prediction loss (HyperGNN.softmax_loss, ghf_score_softmax_fwd,
ghf_score_softmax_bwd): no GPU needed."""

import ctypes
import os
import re

import pytest
import torch

from graph_hypernetwork_forge_amd import HyperGNN, _build, _native, autograd

SOFTMAX_CALLS = ("ghf_score_softmax_workspace_bytes", "ghf_score_softmax_fwd", "ghf_score_softmax_bwd_workspace_bytes",
                 "ghf_score_softmax_bwd")


def test_softmax_entry_points_are_declared_bound_and_exported():
    with open(os.path.join(_build.INCLUDE, "ghf.h")) as f:
        text = f.read()
    assert re.search(r"#define GHF_ABI_VERSION 15\b", text)          # entry points were added, nothing changed
    assert "softmax.hip" in _build.SOURCES and "rank.hip" in _build.SOURCES
    lib = _native.load()
    assert lib.ghf_abi_version() == 15
    for name in SOFTMAX_CALLS:
        assert name in _native.header_symbols() and name in _native.SIGNATURES
        assert hasattr(lib, name), f"libghf_hip.so does not export {name}"
    assert callable(HyperGNN.softmax_loss) and issubclass(autograd.SoftmaxLossFn, torch.autograd.Function)
    assert callable(_native.score_softmax_fwd) and callable(_native.score_softmax_bwd)


def forward_slabs(N, d):
    """The forward's candidate slabs (csrc/softmax.hip: softmax_geom), restated: at most 128, whatever B is."""
    ctiles = -(-N // (256 if d <= 128 else 128))
    slab_tiles = -(-ctiles // 128)
    return -(-ctiles // slab_tiles)


def test_workspace_queries_without_a_gpu():
    lib = _native.load()
    fwd, bwd = lib.ghf_score_softmax_workspace_bytes, lib.ghf_score_softmax_bwd_workspace_bytes
    assert fwd(1, 1, 16) > 0 and bwd(1, 1, 16) > 0
    B, N = 1024, 1_000_000
    for bad in ((0, N, 128), (B, 0, 128), (B, N, 0), (B, N, -4), (B, N, 257), (-1, N, 128), (B, 1 << 31, 128)):
        assert fwd(*bad) == 0 and bwd(*bad) == 0, bad
    for B in (1024, 16384):
        cap = B * N * 4 // 16                                        # "far from a score matrix" (test_rank_host.py)
        assert 0 < fwd(B, N, 128) < cap and 0 < bwd(B, N, 128) < cap
        assert fwd(B, N, 128) < 64 * B * forward_slabs(N, 128)       # a (max, sum) per (query, slab) and O(B) beside it
        assert fwd(B, N, 128) >= 8 * B * forward_slabs(N, 128)
        assert bwd(B, N, 128) >= B * 128 * 4                         # at least one [B, d] partial of dq
    assert bwd(1024, N, 256) < 1024 * N * 4 // 16
    assert forward_slabs(N, 128) == forward_slabs(N, 64) <= 128      # the slabs do not depend on the batch


def test_softmax_entry_points_reject_invalid_arguments_without_a_gpu():
    lib = _native.load()
    fake = ctypes.c_void_p(4096)            # never dereferenced: every call below fails its checks on the host
    ws = ctypes.c_void_p(1 << 20)
    B, N, d = 100, 5000, 64
    fb = lib.ghf_score_softmax_workspace_bytes(B, N, d)
    bb = lib.ghf_score_softmax_bwd_workspace_bytes(B, N, d)

    def fwd(q=fake, c=fake, iq=fake, target=fake, fp=None, fi=None, nnz=0, rows_q=N, N_=N, B_=B, d_=d, scale=0.5, w=ws, wb=fb,
            loss=fake, lse=fake):
        return lib.ghf_score_softmax_fwd(q, c, iq, target, fp, fi, nnz, rows_q, N_, B_, d_, scale, w, wb, loss, lse, None)

    def bwd(q=fake, c=fake, iq=fake, target=fake, fp=None, fi=None, nnz=0, rows_q=N, N_=N, B_=B, d_=d, scale=0.5, lse=fake,
            g=fake, w=ws, wb=bb, dq=fake, dc=fake):
        return lib.ghf_score_softmax_bwd(q, c, iq, target, fp, fi, nnz, rows_q, N_, B_, d_, scale, lse, g, w, wb, dq, dc, None)

    for kw in (dict(q=None), dict(c=None), dict(target=None), dict(w=None), dict(loss=None), dict(lse=None)):
        assert fwd(**kw) == -1, kw
        assert b"null" in lib.ghf_last_error()
    for kw in (dict(q=None), dict(c=None), dict(target=None), dict(w=None), dict(lse=None), dict(g=None), dict(dq=None), dict(dc=None)):
        assert bwd(**kw) == -1, kw
        assert b"null" in lib.ghf_last_error()
    for call, nb in ((fwd, fb), (bwd, bb)):
        assert call(nnz=5) == -1 and b"filter" in lib.ghf_last_error()            # nnz > 0 without lists
        assert call(fp=fake, nnz=5) == -1 and call(fi=fake, nnz=5) == -1
        for bad in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
            assert call(scale=bad) == -1 and b"scale" in lib.ghf_last_error(), bad
        assert call(d_=0) == -1 and call(d_=-8) == -1
        assert call(B_=0) == -1 and call(N_=0) == -1 and call(rows_q=0) == -1 and call(nnz=-1) == -1
        assert call(iq=None, rows_q=B - 1) == -1                                  # no index list: B rows of q are needed
        assert call(wb=nb - 1) == -1 and b"workspace" in lib.ghf_last_error()
        assert call(w=ctypes.c_void_p((1 << 20) + 4)) == -1 and b"aligned" in lib.ghf_last_error()
        assert call(d_=512, wb=1 << 30) == -3                                     # GHF_EUNSUPPORTED, as the rank calls


def test_cpu_tensors_bad_ids_and_bad_scale_raise_before_any_device_work():
    m = HyperGNN(text_dim=32, node_feat_dim=16, hidden_dim=16).eval()
    embs = torch.randn(8, 16)
    q, t = torch.tensor([0, 1]), torch.tensor([2, 3])
    with pytest.raises(RuntimeError, match="HIP device only"):
        m.softmax_loss(embs, q, t)
    with pytest.raises(RuntimeError, match="HIP device only"):
        m.softmax_loss(embs.requires_grad_(True), q, t, scale=0.25, known=(q, t))
    embs = embs.detach()
    with pytest.raises(RuntimeError, match="no CPU"):                   # the typed wrappers refuse host tensors too
        _native.score_softmax_fwd(embs, embs, t, iq=q)
    with pytest.raises(RuntimeError, match="no CPU"):
        _native.score_softmax_bwd(embs, embs, t, torch.zeros(2), torch.ones(2), iq=q)
    for bad in (0.0, -0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="scale"):
            m.softmax_loss(embs, q, t, scale=bad)
    for bad in ([0, 8], [-9, 0]):
        with pytest.raises(IndexError):
            m.softmax_loss(embs, torch.tensor(bad), t)
        with pytest.raises(IndexError):
            m.softmax_loss(embs, q, torch.tensor(bad))
    with pytest.raises(TypeError):
        m.softmax_loss(embs, torch.tensor([0.0, 1.0]), t)
    with pytest.raises(ValueError):
        m.softmax_loss(embs, torch.tensor([[0, 1]]), t)
    with pytest.raises(ValueError):
        m.softmax_loss(embs, q, torch.tensor([1, 2, 3]))
    with pytest.raises(ValueError):
        m.softmax_loss(embs[0], q, t)
