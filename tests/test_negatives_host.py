"""Per-query negative sets, the part that needs no GPU: the float64 restatement (tests/_negatives_ref.py) against plain torch
autograd formulations written independently of it, the keyword's validation (every error is raised from metadata, before any
device check), and the new header: include/ghf.h keeps its symbols and its ABI version, and every function of
include/ghf_negatives.h is bound in _native.NEG_SIGNATURES and exported by the built library."""

import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _negatives_ref as R
from graph_hypernetwork_forge_amd import HyperGNN, _build, _native

SHAPES = [(257, 65, 20, 9), (70, 9, 64, 33), (5, 3, 8, 1)]         # (N, B, d, K)


def problem(N, B, d, K, seed):
    g = torch.Generator().manual_seed(seed)
    c = torch.randn(N, d, generator=g)
    q = torch.randn(B, d, generator=g)
    target = torch.randint(0, N, (B,), generator=g)
    neg = torch.randint(0, N, (B, K), generator=g)
    neg[torch.rand(B, K, generator=g) < 0.2] = -1                                  # ragged rows
    if K > 2:
        neg[:, 1] = neg[:, 0]                                                      # a repeated id: it counts twice
        neg[::2, 2] = target[::2]                                                  # the target among its own negatives
    rng = np.random.default_rng(seed)
    lists = [np.unique(np.append(rng.integers(0, N, 3), int(neg[i, 0]))) if i % 3 == 0 else np.zeros(0, dtype=np.int64)
             for i in range(B)]
    bias = torch.randn(N, generator=g)
    grad = torch.randn(B, generator=g)
    return c, q, target, neg, lists, bias, grad


def dense_logits(q, c, target, neg, lists, bias, scale):
    """[B, K] logits by one gather and a bmm, -inf where the position drops out; the target's logit [B]."""
    ids = neg.clamp(min=0)
    z = scale * torch.bmm(c[ids], q.unsqueeze(2)).squeeze(2)
    zt = scale * (q * c[target]).sum(1)
    if bias is not None:
        z, zt = z + bias[ids], zt + bias[target]
    drop = (neg == -1) | (neg == target.unsqueeze(1))
    for i, l in enumerate(lists):
        for v in l:
            drop[i] |= neg[i] == int(v)
    return z, zt, drop


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("with_bias", [False, True])
def test_softmax_restatement_is_cross_entropy_over_target_and_negatives(shape, with_bias):
    N, B, d, K = shape
    c, q, target, neg, lists, bias, grad = problem(N, B, d, K, seed=N)
    c64, q64 = c.double().requires_grad_(), q.double().requires_grad_()
    b64 = bias.double().requires_grad_() if with_bias else None
    z, zt, drop = dense_logits(q64, c64, target, neg, lists, b64, 0.7)
    logits = torch.cat([zt.unsqueeze(1), z.masked_fill(drop, -np.inf)], 1)
    want = F.cross_entropy(logits, torch.zeros(B, dtype=torch.int64), reduction="none")
    (want * grad.double()).sum().backward()
    got = R.loss("softmax", q, c, target, neg, lists, bias if with_bias else None, scale=0.7, grad=grad)
    assert torch.allclose(got["loss"], want.detach(), rtol=1e-12, atol=1e-12)
    assert torch.allclose(got["dq"], q64.grad, rtol=1e-10, atol=1e-12)
    assert torch.allclose(got["dc"], c64.grad, rtol=1e-10, atol=1e-12)
    if with_bias:
        assert torch.allclose(got["db"], b64.grad, rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("alpha", [0.0, 1.0])
def test_negsamp_restatement_is_the_nssa_loss_with_detached_weights(shape, alpha):
    N, B, d, K = shape
    c, q, target, neg, lists, bias, grad = problem(N, B, d, K, seed=N + 1)
    c64, q64, b64 = c.double().requires_grad_(), q.double().requires_grad_(), bias.double().requires_grad_()
    z, zt, drop = dense_logits(q64, c64, target, neg, lists, b64, 0.5)
    some = ~drop.all(1)                                                            # (softmax over an empty row is NaN in torch)
    w = torch.softmax((alpha * z).masked_fill(drop, -np.inf)[some], -1).detach()
    negterm = torch.zeros(B, dtype=torch.float64)
    negterm[some] = -(w * F.logsigmoid(-(z[some] + 2.0)).masked_fill(drop[some], 0.0)).sum(1)
    want = -F.logsigmoid(zt + 2.0) + negterm
    (want * grad.double()).sum().backward()
    got = R.loss("negsamp", q, c, target, neg, lists, bias, scale=0.5, margin=2.0, alpha=alpha, grad=grad)
    assert torch.allclose(got["loss"], want.detach(), rtol=1e-12, atol=1e-12)
    assert torch.equal(torch.isinf(got["aux"]), ~some)
    if alpha == 0.0:
        assert torch.allclose(got["aux"][some], torch.log((~drop).sum(1).double())[some], rtol=1e-12, atol=1e-12)
    assert torch.allclose(got["dq"], q64.grad, rtol=1e-10, atol=1e-12)
    assert torch.allclose(got["dc"], c64.grad, rtol=1e-10, atol=1e-12)
    assert torch.allclose(got["db"], b64.grad, rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize("shape", SHAPES)
def test_rank_restatement_is_compare_and_count(shape):
    N, B, d, K = shape
    c, q, target, neg, lists, bias, _ = problem(N, B, d, K, seed=N + 2)
    c = torch.round(c * 2)                                                         # small integers: ties happen
    q = torch.round(q * 2)
    z, zt, drop = dense_logits(q.double(), c.double(), target, neg, lists, None, 1.0)
    greater, equal = R.rank(q, c, target, neg, lists)
    assert torch.equal(greater, ((z > zt.unsqueeze(1)) & ~drop).sum(1))
    assert torch.equal(equal, ((z == zt.unsqueeze(1)) & ~drop).sum(1))
    assert int(equal.sum()) > 0 or K == 1


def test_empty_sets_by_the_formulas():
    c, q, target, neg, lists, bias, grad = problem(30, 4, 8, 5, seed=3)
    neg[0] = -1
    neg[1] = target[1]
    lists = [np.zeros(0, dtype=np.int64)] * 2 + [np.unique(neg[2].numpy())] + [np.zeros(0, dtype=np.int64)]
    sm = R.loss("softmax", q, c, target, neg, lists, grad=grad)
    ns = R.loss("negsamp", q, c, target, neg, lists, margin=1.0, alpha=1.0, grad=grad)
    z, zt = R.scores(q, c, target, neg)
    assert torch.equal(sm["loss"][:3], torch.zeros(3, dtype=torch.float64))
    assert torch.equal(sm["coef"][:3], torch.zeros(3, 6, dtype=torch.float64))
    assert torch.isinf(ns["aux"][:3]).all() and (ns["aux"][:3] < 0).all()
    assert torch.allclose(ns["loss"][:3], F.softplus(-(zt[:3] + 1.0)))
    assert torch.equal(ns["coef"][:3, :5], torch.zeros(3, 5, dtype=torch.float64)) and (ns["coef"][:3, 5] != 0).all()


# ---- the keyword ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model():
    return HyperGNN(text_dim=32, node_feat_dim=16, hidden_dim=16)


def _calls(model):
    return [("rank_candidates", model.rank_candidates), ("softmax_loss", model.softmax_loss),
            ("negative_sampling_loss", model.negative_sampling_loss)]


def test_the_three_methods_take_the_keyword_and_the_other_two_do_not(model):
    import inspect
    for name, fn in _calls(model):
        assert "negatives" in inspect.signature(fn).parameters, name
        assert "do NOT wrap" in fn.__doc__, f"{name}: the docstring must say that negative ids do not wrap"
    for fn in (model.topk_candidates, model.bce_loss):
        assert "negatives" not in inspect.signature(fn).parameters


def test_keyword_validation_needs_no_device(model):
    """CPU tensors throughout: each error below is raised before the "HIP device only" RuntimeError."""
    N, B, K = 50, 6, 4
    embs = torch.randn(N, 16)
    q, t = torch.arange(B), torch.arange(B) + 1
    good = torch.randint(0, N, (B, K))
    for name, fn in _calls(model):
        with pytest.raises(ValueError, match="negatives.*candidates|candidates.*negatives"):
            fn(embs, q, t, negatives=good, candidates=torch.arange(10))
        for bad in (good[0], good[:B - 1], good.reshape(B, 2, 2), torch.zeros(B, 0, dtype=torch.int64), good.tolist()):
            with pytest.raises(ValueError, match="negatives"):
                fn(embs, q, t, negatives=bad)
        for bad in (good.float(), good.bool(), good.to(torch.int16)):
            with pytest.raises(TypeError, match="negatives"):
                fn(embs, q, t, negatives=bad)
        for value in (N, -2, -N):                                                   # -1 is padding, so nothing wraps
            bad = good.clone()
            bad[B - 1, K - 1] = value
            with pytest.raises(IndexError, match="negatives"):
                fn(embs, q, t, negatives=bad)
        padded = good.clone()
        padded[0] = -1
        for ok in (good, good.to(torch.int32), padded):                            # valid: only now the device is asked for
            with pytest.raises(RuntimeError, match="HIP device"):
                fn(embs, q, t, negatives=ok)


def test_query_and_target_are_checked_as_without_the_keyword(model):
    """The same accepted forms and the same errors for query / target with and without negatives=; no queries at all is the
    error of the call without the keyword, not one of torch's."""
    N, B, K = 50, 6, 4
    embs = torch.randn(N, 16)
    q, t = torch.arange(B), torch.arange(B) + 1
    good = torch.randint(0, N, (B, K))
    bad_queries = [(q.reshape(2, 3), ValueError), (q.float(), TypeError), (q + N, IndexError), (q.tolist(), ValueError)]
    for name, fn in _calls(model):
        if name == "rank_candidates":
            continue                                   # (it asks for the device before it looks at query, with or without)
        for bad, err in bad_queries:
            with pytest.raises(err) as without:
                fn(embs, bad, t)
            with pytest.raises(err) as with_kw:
                fn(embs, bad, t, negatives=good)
            assert str(without.value) == str(with_kw.value), name
        with pytest.raises(ValueError, match="queries and"):
            fn(embs, q, t[:-1], negatives=good)
        with pytest.raises(RuntimeError, match="HIP device"):                      # wrapped ids are fine, as without
            fn(embs, q - N, t, negatives=good)
    for name, fn in _calls(model):
        empty = torch.zeros(0, dtype=torch.int64)
        with pytest.raises(RuntimeError, match="HIP device"):                      # (not torch's complaint about an empty aminmax)
            fn(embs, empty, empty, negatives=torch.zeros(0, K, dtype=torch.int64))


# ---- the headers and the library -----------------------------------------------------------------------------------------
NEG_FUNCTIONS = ["ghf_neg_bwd", "ghf_neg_negsamp_fwd", "ghf_neg_rank", "ghf_neg_softmax_fwd", "ghf_neg_workspace_bytes"]


def test_ghf_h_keeps_its_symbols_and_its_abi_version():
    with open(os.path.join(_build.INCLUDE, "ghf.h")) as f:
        text = f.read()
    assert re.search(r"#define GHF_ABI_VERSION 15\b", text) and _native.ABI_VERSION == 15
    assert "ghf_negatives.h" not in text and not [s for s in _native.header_symbols() if s.startswith("ghf_neg_")]
    assert set(_native.header_symbols()) == set(_native.SIGNATURES)
    assert len(_native.header_symbols()) == 113


def test_every_function_of_the_new_header_is_bound_and_exported():
    with open(os.path.join(_build.INCLUDE, "ghf_negatives.h")) as f:
        text = f.read()
    declared = sorted(set(re.findall(r"\b(ghf_[a-z_0-9]+)\s*\(", text)))
    assert declared == NEG_FUNCTIONS == _native.negatives_header_symbols()
    assert set(_native.NEG_SIGNATURES) == set(declared) and not set(declared) & set(_native.SIGNATURES)
    assert os.path.join(_build.INCLUDE, "ghf_negatives.h") in _build.HEADERS and "negatives.hip" in _build.SOURCES
    lib = _native.load()
    for name in declared:
        fn = getattr(lib, name)                                                    # AttributeError: not exported
        assert fn.argtypes == _native.NEG_SIGNATURES[name][1]
    assert lib.ghf_abi_version() == 15


def test_size_query_and_argument_checks_without_a_launch():
    lib = _native.load()
    assert _native.neg_workspace_bytes(5, 7, 128, 0) > 0 and _native.neg_workspace_bytes(5, 7, 128, 0) % 256 == 0
    for B, K, d, nnz in ((0, 7, 128, 0), (5, 0, 128, 0), (5, 7, 0, 0), (5, 7, 257, 0), (5, 7, 128, -1), (1 << 20, 1 << 11, 128, 0),
                         (1 << 31, 1, 128, 0)):
        assert _native.neg_workspace_bytes(B, K, d, nnz) == 0, (B, K, d, nnz)
    assert _native.neg_workspace_bytes((1 << 20) - 1, (1 << 11) - 1, 256, 0) > 0          # B (K + 1) just below 2^31
    # null pointers are refused before anything else is looked at (no device memory is needed to see that)
    assert lib.ghf_neg_rank(None, None, None, None, None, None, 0, 1, 1, 1, 8, None, 1, None, None, 0, None, None, None) == -1
    assert b"null pointer" in lib.ghf_last_error()
    assert lib.ghf_neg_softmax_fwd(None, None, None, None, None, None, 0, 1, 1, 1, 8, 1.0, None, 1, None, None, 0, None, None,
                                   None) == -1
    assert lib.ghf_neg_negsamp_fwd(None, None, None, None, None, None, 0, 1, 1, 1, 8, 1.0, 0.0, 0.0, None, 1, None, None, 0, None,
                                   None, None) == -1
    assert lib.ghf_neg_bwd(0, None, None, None, None, None, None, 0, 1, 1, 1, 8, 1.0, 0.0, 0.0, None, 1, None, None, None, None, 0,
                           None, None, None) == -1
