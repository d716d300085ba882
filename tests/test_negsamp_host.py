"""Host-side checks of the negative-sampling loss with self-adversarial weighting (HyperGNN.negative_sampling_loss,
ghf_score_negsamp_fwd / _bwd): the float64 restatement the GPU tests compare with (tests/_negsamp_ref.py) against an
independently written PyKEEN-style formulation, and the argument checks of the four entry points.  No GPU needed."""

import ctypes
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _negsamp_ref import negsamp_reference
from graph_hypernetwork_forge_amd import HyperGNN, _build, _native, autograd

CALLS = ("ghf_score_negsamp_workspace_bytes", "ghf_score_negsamp_fwd", "ghf_score_negsamp_bwd_workspace_bytes",
         "ghf_score_negsamp_bwd")


# ---- the restatement ---------------------------------------------------------------------------------------------------
def pykeen_style(qrows, c, target, lists, scale, margin, alpha, grad, ic=None, bias=None):
    """NSSALoss as PyKEEN writes it, per query and without its / 2 and mean: -logsigmoid(margin + pos) - sum_j w_j
    logsigmoid(-(margin + neg_j)), w = softmax(alpha * neg, -1).detach(); one row of negatives per query, gathered."""
    q = qrows.double().requires_grad_(True)
    cc = c.double().requires_grad_(True)
    b = None if bias is None else bias.double().requires_grad_(True)
    P = list(range(c.size(0))) if ic is None else [int(v) for v in ic]
    losses, lws = [], []
    for i in range(q.size(0)):
        listed = set() if lists is None else {int(v) for v in lists[i]}
        t = int(target[i])
        J = torch.tensor([j for j in P if j not in listed and j != t], dtype=torch.long)
        pos = scale * (q[i] * cc[t]).sum() + (0 if b is None else b[t])
        neg = scale * (cc[J] @ q[i]) + (0 if b is None else b[J])
        w = torch.softmax(alpha * neg, -1).detach()
        losses.append(-F.logsigmoid(margin + pos) - (w * F.logsigmoid(-(margin + neg))).sum())
        lws.append(torch.logsumexp(alpha * neg.detach(), -1) if len(J) else torch.tensor(-math.inf, dtype=torch.float64))
    loss = torch.stack(losses)
    (loss * grad.double()).sum().backward()
    db = None if b is None else b.grad
    return loss.detach(), torch.stack(lws), q.grad, cc.grad, db


def rows(N, B, d, seed):
    g = torch.Generator().manual_seed(seed)
    c = F.layer_norm(torch.randn(N, d, generator=g), (d,))
    iq = torch.randint(0, N, (B,), generator=g)
    target = torch.randint(0, N, (B,), generator=g)
    rng = np.random.default_rng(seed)
    lists = [np.unique(rng.integers(0, N, 4)) if i % 5 else np.zeros(0, dtype=np.int64) for i in range(B)]
    if B > 2:
        lists[1] = np.unique(np.append(lists[1], int(target[1])))          # a listed target: still the positive, never a negative
    return c, iq, target, lists, torch.rand(B, generator=g) + 0.5


def close(a, b, tol=1e-10):
    a, b = a.double(), b.double()
    return bool(torch.equal(torch.isinf(a), torch.isinf(b))) and bool(torch.allclose(
        torch.nan_to_num(a, posinf=0, neginf=0), torch.nan_to_num(b, posinf=0, neginf=0), rtol=tol, atol=tol))


@pytest.mark.parametrize("N,B,d", [(257, 65, 20), (70, 9, 64), (1, 3, 8)])
def test_the_restatement_agrees_with_a_pykeen_style_autograd_formulation(N, B, d):
    c, iq, target, lists, g = rows(N, B, d, seed=N + d)
    if N == 1:
        target = torch.zeros(B, dtype=torch.long)
    for alpha in (0.0, 0.5, 1.0):
        for margin in (0.0, 2.0, -1.0):
            scale = d ** -0.5 if margin else 1.0
            got = negsamp_reference(c[iq], c, target, lists, scale, margin, alpha, grad=g)
            want = pykeen_style(c[iq], c, target, lists, scale, margin, alpha, g)
            for name, a, b in zip(("loss", "lw", "dq", "dc"), got, want):
                assert close(a, b), f"{name} at alpha={alpha} margin={margin}"
            assert torch.isfinite(got[0]).all()


def test_the_restatement_with_a_subset_and_a_bias():
    N, B, d = 120, 17, 20
    c, iq, _, lists, g = rows(N, B, d, seed=5)
    ic = torch.unique(torch.randint(0, N, (40,), generator=torch.Generator().manual_seed(1)))
    target = ic[torch.randint(0, ic.numel(), (B,), generator=torch.Generator().manual_seed(2))]
    bias = torch.randn(N, generator=torch.Generator().manual_seed(3))
    got = negsamp_reference(c[iq], c, target, lists, 0.3, 1.0, 0.5, grad=g, ic=ic, bias=bias)
    want = pykeen_style(c[iq], c, target, lists, 0.3, 1.0, 0.5, g, ic=ic, bias=bias)
    assert close(got[0], want[0]) and close(got[1], want[1]) and close(got[2], want[2])
    assert close(got[3], want[3][ic]) and close(got[4], want[4][ic])        # per candidate: [C, d] and [C]
    outside = torch.ones(N, dtype=torch.bool)
    outside[ic] = False
    assert not want[3][outside].any() and not want[4][outside].any()
    # a target outside the candidates: NaN, and the query takes no part
    bad = target.clone()
    bad[3] = int(torch.nonzero(outside)[0])
    l2, w2, dq2, dc2, db2 = negsamp_reference(c[iq], c, bad, lists, 0.3, 1.0, 0.5, grad=g, ic=ic, bias=bias)
    assert torch.isnan(l2[3]) and torch.isnan(w2[3]) and not dq2[3].any() and torch.isfinite(l2[torch.arange(B) != 3]).all()


def test_temperature_zero_is_the_uniform_mean_and_lw_is_log_count():
    N, B, d = 257, 33, 20
    c, iq, target, lists, g = rows(N, B, d, seed=9)
    loss, lw, dq, dc, _ = negsamp_reference(c[iq], c, target, lists, 0.5, 1.5, 0.0, grad=g)
    z = 0.5 * (c[iq].double() @ c.double().T)
    for i in range(B):
        J = [j for j in range(N) if j != int(target[i]) and j not in set(lists[i].tolist())]
        mean = F.softplus(z[i, J] + 1.5, threshold=1e9).mean() + F.softplus(-(z[i, target[i]] + 1.5), threshold=1e9)
        assert abs(float(loss[i] - mean)) < 1e-12
        assert abs(float(lw[i]) - math.log(len(J))) < 1e-12


def test_a_query_without_negatives_has_the_positive_term_alone():
    c, iq, _, _, g = rows(6, 4, 8, seed=2)
    target = torch.tensor([0, 1, 2, 3])
    lists = [np.array([j for j in range(6) if j != t]) for t in target.tolist()]      # everything else is a known partner
    lists[3] = np.arange(6)                                                       # ... the target too
    for alpha in (0.0, 1.0):
        loss, lw, dq, dc, db = negsamp_reference(c[iq], c, target, lists, 1.0, 0.5, alpha, grad=g)
        zt = (c[iq].double() * c[target].double()).sum(1)
        assert torch.allclose(loss, F.softplus(-(zt + 0.5), threshold=1e9), rtol=0, atol=1e-14)
        assert bool(torch.isinf(lw).all()) and bool((lw < 0).all())
        assert torch.isfinite(dq).all() and torch.isfinite(dc).all() and torch.isfinite(db).all()
        want_dq = (-g.double() * torch.sigmoid(-(zt + 0.5)))[:, None] * c[target].double()
        assert torch.allclose(dq, want_dq, rtol=0, atol=1e-14)


# ---- the entry points --------------------------------------------------------------------------------------------------
def test_negsamp_entry_points_are_declared_bound_and_exported():
    with open(os.path.join(_build.INCLUDE, "ghf.h")) as f:
        text = f.read()
    assert re.search(r"#define GHF_ABI_VERSION 15\b", text)            # entry points were added only
    assert "negsamp.hip" in _build.SOURCES
    lib = _native.load()
    assert lib.ghf_abi_version() == 15 and _native.ABI_VERSION == 15
    for name in CALLS:
        assert name in _native.header_symbols() and name in _native.SIGNATURES
        assert hasattr(lib, name), f"libghf_hip.so does not export {name}"
    assert callable(HyperGNN.negative_sampling_loss)
    assert issubclass(autograd.NegSamplingLossFn, torch.autograd.Function)
    assert {"rows", "query", "margin", "alpha", "cand", "bias"} <= set(inspect.signature(autograd.NegSamplingLossFn.forward).parameters)
    params = inspect.signature(HyperGNN.negative_sampling_loss).parameters
    assert [params[k].default for k in ("scale", "margin", "adversarial_temperature")] == [1.0, 0.0, 0.0]
    assert {"known", "filt_ptr", "filt_idx", "query_rows", "query_rel", "candidates", "candidate_bias"} <= set(params)


def test_workspace_queries_without_a_gpu():
    lib = _native.load()
    B, N = 1024, 1_000_000
    fwd = lib.ghf_score_negsamp_workspace_bytes(B, N, 0, 128, 0)
    # a score and a flag per query plus one triple of floats per (query, candidate slab), at most 128 slabs
    assert 8 * B + 12 * B <= fwd <= 8 * B + 12 * 128 * B + 1024
    assert fwd < B * N * 4 // 256
    assert lib.ghf_score_negsamp_workspace_bytes(1, 1, 0, 16, 0) > 0
    per_q = (lib.ghf_score_negsamp_workspace_bytes(4096, N, 0, 128, 0) - lib.ghf_score_negsamp_workspace_bytes(2048, N, 0, 128, 0)) // 2048
    assert per_q == (lib.ghf_score_negsamp_workspace_bytes(8192, N, 0, 128, 0) - lib.ghf_score_negsamp_workspace_bytes(4096, N, 0, 128, 0)) // 4096
    sub = lib.ghf_score_negsamp_workspace_bytes(B, N, 16384, 128, 10 * B)
    assert lib.ghf_score_negsamp_workspace_bytes(B, 16384, 0, 128, 0) + 4 * 16384 <= sub < fwd      # the id map and the gathered bias
    bwd = lib.ghf_score_negsamp_bwd_workspace_bytes(B, N, 0, 128, 0)
    assert bwd == lib.ghf_score_softmax_bwd_workspace_bytes(B, N, 128)                 # the same sweeps, the same partials
    assert lib.ghf_score_negsamp_bwd_workspace_bytes(B, N, 16384, 128, 10 * B) == lib.ghf_score_softmax_bwd_b_workspace_bytes(
        B, N, 16384, 128, 10 * B)
    for bad in ((0, N, 0, 128, 0), (B, 0, 0, 128, 0), (B, N, 0, 0, 0), (B, N, 0, -4, 0), (B, N, 0, 257, 0), (B, N, 64, 257, 0),
                (-1, N, 0, 128, 0), (B, 1 << 31, 0, 128, 0), (1 << 31, N, 0, 128, 0), (B, 100, 101, 128, 0), (B, N, 64, 128, -1)):
        assert lib.ghf_score_negsamp_workspace_bytes(*bad) == 0, bad
        assert lib.ghf_score_negsamp_bwd_workspace_bytes(*bad) == 0, bad


def test_negsamp_entry_points_reject_invalid_arguments_without_a_gpu():
    lib = _native.load()
    fake = ctypes.c_void_p(4096)            # never dereferenced: every call below fails its checks on the host
    ws = ctypes.c_void_p(1 << 20)
    B, N, d = 100, 5000, 64
    nf, nb = lib.ghf_score_negsamp_workspace_bytes(B, N, 0, d, 0), lib.ghf_score_negsamp_bwd_workspace_bytes(B, N, 0, d, 0)

    def fwd(q=fake, c=fake, iq=fake, t=fake, fp=None, fi=None, nnz=0, rows_q=N, N_=N, B_=B, d_=d, scale=1.0, margin=1.0, alpha=0.5,
            ic=None, C=0, bias=None, w=ws, wb=nf, loss=fake, lw=fake):
        return lib.ghf_score_negsamp_fwd(q, c, iq, t, fp, fi, nnz, rows_q, N_, B_, d_, scale, margin, alpha, ic, C, bias, w, wb, loss,
                                         lw, None)

    def bwd(q=fake, c=fake, iq=fake, t=fake, fp=None, fi=None, nnz=0, rows_q=N, N_=N, B_=B, d_=d, scale=1.0, margin=1.0, alpha=0.5,
            lw=fake, g=fake, ic=None, C=0, bias=None, w=ws, wb=nb, dq=fake, dc=fake, db=None):
        return lib.ghf_score_negsamp_bwd(q, c, iq, t, fp, fi, nnz, rows_q, N_, B_, d_, scale, margin, alpha, lw, g, ic, C, bias, w, wb,
                                         dq, dc, db, None)

    for call, nulls in ((fwd, ("q", "c", "t", "w", "loss", "lw")), (bwd, ("q", "c", "t", "lw", "g", "w", "dq", "dc"))):
        for name in nulls:
            assert call(**{name: None}) == -1, name
            assert b"null" in lib.ghf_last_error()
        assert call(nnz=5) == -1 and b"filter list" in lib.ghf_last_error()           # nnz > 0 without lists
        for bad_scale in (0.0, -1.0, float("inf"), float("nan")):
            assert call(scale=bad_scale) == -1 and b"scale" in lib.ghf_last_error(), bad_scale
        for bad_alpha in (-0.5, float("inf"), float("nan")):
            assert call(alpha=bad_alpha) == -1 and b"adv_temperature" in lib.ghf_last_error(), bad_alpha
        for bad_margin in (float("inf"), float("-inf"), float("nan")):
            assert call(margin=bad_margin) == -1 and b"margin" in lib.ghf_last_error(), bad_margin
        assert call(ic=fake, C=N + 1, wb=1 << 30) == -1 and b"C <= N" in lib.ghf_last_error()
        assert call(ic=fake, C=0) == -1 and call(ic=None, C=5) == -1                   # ic and C come together
        assert call(d_=0) == -1 and call(d_=-8) == -1
        assert call(B_=0) == -1 and call(N_=0) == -1 and call(rows_q=0) == -1 and call(nnz=-1) == -1
        assert call(iq=None, rows_q=B - 1) == -1                                       # no index list: B rows of q are needed
        assert call(w=ctypes.c_void_p((1 << 20) + 4)) == -1 and b"aligned" in lib.ghf_last_error()
        assert call(d_=512, wb=1 << 30) == -3                                          # GHF_EUNSUPPORTED
        assert call(d_=512, wb=1 << 30, ic=fake, C=64, bias=fake) == -3
    assert fwd(wb=nf - 1) == -1 and b"workspace" in lib.ghf_last_error()
    assert bwd(wb=nb - 1) == -1 and b"workspace" in lib.ghf_last_error()
    ns = lib.ghf_score_negsamp_workspace_bytes(B, N, 64, d, 0)
    assert fwd(ic=fake, C=64, bias=fake, wb=ns - 1) == -1 and b"workspace" in lib.ghf_last_error()
    nbs = lib.ghf_score_negsamp_bwd_workspace_bytes(B, N, 64, d, 0)
    assert bwd(ic=fake, C=64, bias=fake, wb=nbs - 1) == -1 and b"workspace" in lib.ghf_last_error()


def test_python_arguments_are_checked_before_any_device_work():
    m = HyperGNN(text_dim=32, node_feat_dim=16, hidden_dim=16).eval()
    embs = torch.randn(12, 16)
    q, t = torch.tensor([0, 1]), torch.tensor([2, 3])
    src, dst, rel = torch.tensor([0, 1, 2]), torch.tensor([3, 4, 5]), torch.tensor([0, 1, 2])
    with pytest.raises(ValueError, match=r"\[N, d\]"):
        m.negative_sampling_loss(embs[0], q, t)
    with pytest.raises(ValueError, match="candidate_bias"):
        m.negative_sampling_loss(embs, q, t, candidate_bias=torch.zeros(11))
    with pytest.raises(ValueError, match="candidates is empty"):
        m.negative_sampling_loss(embs, q, t, candidates=torch.zeros(0, dtype=torch.int64))
    with pytest.raises(IndexError):
        m.negative_sampling_loss(embs, q, t, candidates=torch.tensor([12]))
    with pytest.raises(ValueError, match="query_rows"):
        m.negative_sampling_loss(embs, q, t, query_rows=torch.randn(3, 16), scale=-1.0)
    for bad_scale in (0.0, -2.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="scale"):
            m.negative_sampling_loss(embs, torch.tensor([99]), t[:1], scale=bad_scale)
    for bad_margin in (float("inf"), float("-inf"), float("nan")):
        with pytest.raises(ValueError, match="margin"):
            m.negative_sampling_loss(embs, torch.tensor([99]), t[:1], margin=bad_margin)
    for bad_alpha in (-0.1, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="adversarial_temperature"):
            m.negative_sampling_loss(embs, torch.tensor([99]), t[:1], adversarial_temperature=bad_alpha)
    with pytest.raises(IndexError):
        m.negative_sampling_loss(embs, torch.tensor([12]), t[:1])
    with pytest.raises(IndexError):
        m.negative_sampling_loss(embs, q, torch.tensor([0, -13]))
    with pytest.raises(TypeError):
        m.negative_sampling_loss(embs, torch.tensor([0.5]), t[:1])
    with pytest.raises(ValueError, match="queries and"):
        m.negative_sampling_loss(embs, q, t[:1])
    with pytest.raises(RuntimeError, match="HIP device only"):
        m.negative_sampling_loss(embs, q, t, margin=2.0, adversarial_temperature=1.0)
    with pytest.raises(RuntimeError, match="HIP device only"):                              # the lists are built on the device
        m.negative_sampling_loss(embs, q, t, known=(src, dst, rel))
    with pytest.raises(RuntimeError, match="no CPU"):                                       # the typed wrappers refuse host tensors
        _native.score_negsamp_fwd(embs, embs, t, iq=q)
    with pytest.raises(RuntimeError, match="no CPU"):
        _native.score_negsamp_bwd(embs, embs, t, torch.zeros(2), torch.ones(2), iq=q)
