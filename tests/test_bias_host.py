"""Host-side checks of ``candidate_bias=`` (the ghf_score_*_b calls): the float64 restatement
(tests/_bias_ref.py) against torch's own dense formulas on the CPU, the keyword's validation, the new entry points.  No GPU
needed."""

import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _bias_ref as ref
from graph_hypernetwork_forge_amd import HyperGNN, _build, _native, autograd

BIAS_CALLS = ("ghf_score_rank_b", "ghf_score_topk_b", "ghf_score_softmax_fwd_b", "ghf_score_softmax_bwd_b", "ghf_score_bce_fwd_b",
              "ghf_score_bce_bwd_b")
BIAS_SIZES = ("ghf_score_rank_b_workspace_bytes", "ghf_score_topk_b_workspace_bytes", "ghf_score_softmax_b_workspace_bytes",
              "ghf_score_softmax_bwd_b_workspace_bytes", "ghf_score_bce_b_workspace_bytes", "ghf_score_bce_bwd_b_workspace_bytes")


def small(seed=0, N=37, B=9, d=6):
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((N, d)).astype(np.float32)
    q = rng.standard_normal((B, d)).astype(np.float32)
    b = (2.0 * rng.standard_normal(N)).astype(np.float32)
    target = rng.integers(0, N, B)
    lists = [np.unique(rng.integers(0, N, rng.integers(0, 5))) for _ in range(B)]
    return c, q, b, target, lists


def t64(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float64))


def listed_mask(lists, P, B):
    m = torch.zeros(B, len(P), dtype=torch.bool)
    for i, l in enumerate(lists):
        m[i] = torch.from_numpy(np.isin(P, l))
    return m


@pytest.mark.parametrize("subset", (False, True))
def test_softmax_restatement_is_cross_entropy_on_the_biased_logits(subset):
    c, q, b, target, lists = small(1)
    N, B = c.shape[0], q.shape[0]
    P = np.sort(np.unique(np.concatenate([np.random.default_rng(2).choice(N, 15, replace=False), target]))) if subset else np.arange(N)
    lists = [l[l != target[i]] for i, l in enumerate(lists)]                # listed targets stay in: covered on the GPU
    g = np.random.default_rng(3).standard_normal(B)
    bt = t64(b).requires_grad_(True)
    Q, C = t64(q).requires_grad_(True), t64(c).requires_grad_(True)
    logits = 0.3 * Q @ C[torch.from_numpy(P)].T + bt[torch.from_numpy(P)]
    logits = logits.masked_fill(listed_mask(lists, P, B), float("-inf"))
    tpos = torch.from_numpy(np.searchsorted(P, target))
    want = F.cross_entropy(logits, tpos, reduction="none")
    (want * t64(g)).sum().backward()
    loss, lse, dq, dc, db = ref.softmax(q, c, b, target, lists, None if not subset else P, 0.3, grad=g)
    np.testing.assert_allclose(loss, want.detach().numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(lse, torch.logsumexp(logits, 1).detach().numpy(), rtol=1e-12)
    np.testing.assert_allclose(dq, Q.grad.numpy(), rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(dc, C.grad.numpy(), rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(db, bt.grad.numpy(), rtol=1e-10, atol=1e-12)
    outside = np.setdiff1d(np.arange(N), P)
    assert not db[outside].any() and not dc[outside].any()


@pytest.mark.parametrize("subset", (False, True))
def test_bce_restatement_is_bce_with_logits_on_the_smoothed_labels(subset):
    c, q, b, _, lists = small(4)
    N, B = c.shape[0], q.shape[0]
    P = np.sort(np.random.default_rng(5).choice(N, 20, replace=False)) if subset else np.arange(N)
    g = np.random.default_rng(6).standard_normal(B)
    bt = t64(b).requires_grad_(True)
    Q, C = t64(q).requires_grad_(True), t64(c).requires_grad_(True)
    logits = 0.7 * Q @ C[torch.from_numpy(P)].T + bt[torch.from_numpy(P)]
    y = 0.9 * listed_mask(lists, P, B).double() + 0.1 / len(P)
    want = F.binary_cross_entropy_with_logits(logits, y, reduction="none").sum(1)
    (want * t64(g)).sum().backward()
    loss, dq, dc, db = ref.bce(q, c, b, lists, None if not subset else P, 0.7, 0.1, grad=g)
    np.testing.assert_allclose(loss, want.detach().numpy(), rtol=1e-12)
    np.testing.assert_allclose(dq, Q.grad.numpy(), rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(dc, C.grad.numpy(), rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(db, bt.grad.numpy(), rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize("subset", (False, True))
def test_rank_and_topk_restatement_is_compare_and_count_and_torch_topk(subset):
    c, q, b, target, lists = small(7)
    N, B = c.shape[0], q.shape[0]
    P = np.sort(np.random.default_rng(8).choice(N, 18, replace=False)) if subset else np.arange(N)
    b[P[3]] = -np.inf                                                       # a removed candidate (no query's target)
    target = np.where(target == P[3], P[4], target)
    S = t64(q) @ t64(c)[torch.from_numpy(P)].T + t64(b)[torch.from_numpy(P)]
    t = (t64(q) * t64(c)[torch.from_numpy(target)]).sum(1) + t64(b)[torch.from_numpy(target)]
    out = listed_mask(lists, P, B) | (torch.from_numpy(P)[None, :] == torch.from_numpy(target)[:, None])
    greater, equal = ref.rank(q, c, b, target, lists, None if not subset else P)
    assert greater.tolist() == ((S > t[:, None]) & ~out).sum(1).tolist()
    assert equal.tolist() == ((S == t[:, None]) & ~out).sum(1).tolist()
    k = 5
    scores, ids = ref.topk(q, c, b, lists, None if not subset else P, k)
    vals, pos = torch.topk(S.masked_fill(listed_mask(lists, P, B), float("-inf")), k, dim=1)       # random normals: no ties
    np.testing.assert_array_equal(scores, vals.numpy())
    assert ids.tolist() == P[pos.numpy()].tolist()
    assert P[3] not in ids


def test_exact_bias_is_what_the_gpu_tests_say_it_is():
    b = ref.exact_bias(700, 3)
    assert b.dtype == np.float32 and np.abs(b).max() <= 32 and not (b * 64 % 1).any()
    assert not b[::7].any() and np.count_nonzero(b) > 500
    first, last = np.arange(233), np.arange(700 - 233, 700)                 # the copied entries, where neither was zeroed
    both = (first % 7 != 0) & (last % 7 != 0)
    assert np.array_equal(b[first[both]], b[last[both]])


def test_the_keyword_is_validated_from_metadata_before_any_device_work():
    """on CPU tensors: a bad candidate_bias= is a ValueError that names the expected shape, raised before the candidates or
    the device are looked at; a good one reaches the device check"""
    model = HyperGNN(text_dim=8, node_feat_dim=4, hidden_dim=8)
    embs, q = torch.zeros(10, 8), torch.tensor([1, 2])
    good = torch.zeros(10)
    bad = (torch.zeros(9), torch.zeros(10, 1), torch.zeros(10, dtype=torch.float64), torch.zeros(10, dtype=torch.int64),
           [0.0] * 10, torch.zeros(10, device="meta"))
    for call in (lambda **kw: model.rank_candidates(embs, q, q, **kw), lambda **kw: model.topk_candidates(embs, q, 3, **kw),
                 lambda **kw: model.softmax_loss(embs, q, q, **kw), lambda **kw: model.bce_loss(embs, q, **kw)):
        for b in bad:
            with pytest.raises(ValueError, match=r"candidate_bias must be a float32 tensor of shape \[N\] = \[10\]"):
                call(candidate_bias=b, candidates=torch.tensor([3, 10]))    # the bias is reported first
        with pytest.raises(IndexError):
            call(candidate_bias=good, candidates=torch.tensor([3, 10]))
        with pytest.raises(RuntimeError, match="HIP device"):
            call(candidate_bias=good)
    strided = torch.zeros(20)[::2]
    assert HyperGNN._candidate_bias(strided, embs).is_contiguous()
    assert HyperGNN._candidate_bias(None, embs) is None
    p = torch.nn.Parameter(torch.zeros(10))
    assert HyperGNN._candidate_bias(p, embs) is p                           # a parameter stays the leaf autograd knows


def test_bias_entry_points_are_declared_bound_and_exported():
    with open(os.path.join(_build.INCLUDE, "ghf.h")) as f:
        text = f.read()
    assert re.search(r"#define GHF_ABI_VERSION 15\b", text)                 # entry points were added only
    lib = _native.load()
    assert lib.ghf_abi_version() == 15 and _native.ABI_VERSION == 15
    for name in BIAS_CALLS + BIAS_SIZES:
        assert name in _native.header_symbols() and name in _native.SIGNATURES
        assert hasattr(lib, name), f"libghf_hip.so does not export {name}"
    vp, i64 = ctypes.c_void_p, ctypes.c_int64
    for name in BIAS_CALLS:                                                 # the _sub form's arguments plus the bias behind (ic, C)
        sub = _native.SIGNATURES[name[:-2] + "_sub"][1]
        got = _native.SIGNATURES[name][1]
        at = max(i for i in range(len(sub) - 1) if sub[i] == vp and sub[i + 1] == i64) + 2
        extra = [vp] if "_bwd_" in name else []                             # the backwards: db behind dc
        assert got == sub[:at] + [vp] + sub[at:-1] + extra + sub[-1:], name
    for fn in (autograd.SoftmaxLossFn, autograd.BceLossFn):
        assert "bias" in inspect.signature(fn.forward).parameters
    for m in (HyperGNN.rank_candidates, HyperGNN.topk_candidates, HyperGNN.softmax_loss, HyperGNN.bce_loss):
        assert inspect.signature(m).parameters["candidate_bias"].default is None


def test_workspace_queries_without_a_gpu():
    lib = _native.load()
    B, N, C, d, nnz = 1024, 1_000_000, 16_384, 128, 10_240
    # every node: the plain call's workspace; a subset: the _sub call's plus the gathered bias, [C] floats
    assert lib.ghf_score_rank_b_workspace_bytes(B, N, 0, d, nnz) == lib.ghf_score_rank_workspace_bytes(B, N, d)
    assert lib.ghf_score_topk_b_workspace_bytes(B, N, 0, d, 10, nnz) == lib.ghf_score_topk_workspace_bytes(B, N, d, 10)
    assert lib.ghf_score_softmax_b_workspace_bytes(B, N, 0, d, nnz) == lib.ghf_score_softmax_workspace_bytes(B, N, d)
    assert lib.ghf_score_softmax_bwd_b_workspace_bytes(B, N, 0, d, nnz) == lib.ghf_score_softmax_bwd_workspace_bytes(B, N, d)
    assert lib.ghf_score_bce_b_workspace_bytes(B, N, 0, d, nnz) == lib.ghf_score_bce_workspace_bytes(B, N, d)
    assert lib.ghf_score_bce_bwd_b_workspace_bytes(B, N, 0, d, nnz) == lib.ghf_score_bce_bwd_workspace_bytes(B, N, d)
    assert lib.ghf_score_rank_b_workspace_bytes(B, N, C, d, nnz) == lib.ghf_score_rank_sub_workspace_bytes(B, C, d, nnz) + 4 * C
    assert lib.ghf_score_topk_b_workspace_bytes(B, N, C, d, 10, nnz) == lib.ghf_score_topk_sub_workspace_bytes(B, C, d, 10, nnz) + 4 * C
    assert lib.ghf_score_softmax_b_workspace_bytes(B, N, C, d, nnz) == lib.ghf_score_softmax_sub_workspace_bytes(B, C, d, nnz) + 4 * C
    assert (lib.ghf_score_softmax_bwd_b_workspace_bytes(B, N, C, d, nnz)
            == lib.ghf_score_softmax_bwd_sub_workspace_bytes(B, C, d, nnz) + 4 * C)
    assert lib.ghf_score_bce_b_workspace_bytes(B, N, C, d, nnz) == lib.ghf_score_bce_sub_workspace_bytes(B, C, d, nnz) + 4 * C
    assert lib.ghf_score_bce_bwd_b_workspace_bytes(B, N, C, d, nnz) == lib.ghf_score_bce_bwd_sub_workspace_bytes(B, C, d, nnz) + 4 * C
    assert lib.ghf_score_rank_b_workspace_bytes(B, N, 100, d, nnz) % 256 == 0
    assert lib.ghf_score_rank_b_workspace_bytes(B, N, C, 300, nnz) == 0      # d beyond the sweeps' limit


def test_null_bias_and_a_subset_without_its_count_are_refused_without_a_device():
    lib = _native.load()
    buf = (ctypes.c_char * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p).value
    p += (-p) % 256                                                         # the entry checks look at pointers, not through them
    rc = lib.ghf_score_rank_b(p, p, None, p, None, None, 0, 8, 8, 4, 4, None, 0, None, p, 2048, p, p, None)
    assert rc != 0 and "null bias" in _native.load().ghf_last_error().decode()
    rc = lib.ghf_score_topk_b(p, p, None, None, None, 0, 8, 8, 4, 4, 2, None, 3, p, p, 2048, p, p, None)
    assert rc != 0 and "ic" in _native.load().ghf_last_error().decode()
