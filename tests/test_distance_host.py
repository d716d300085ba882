"""Distance scores for per-query negative sets, the part that needs no GPU: the ``distance=`` keyword and its validation
(every error from metadata, before any device check), the third header include/ghf_distance.h against
_native.DIST_SIGNATURES and the built library (ghf.h and ghf_negatives.h as they were), the argument checks that come ahead
of any launch, and the float64 restatement (tests/_distance_ref.py) against torch autograd of an explicit [B, K, d]
formulation written independently of it."""

import ctypes
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _distance_ref as R
from graph_hypernetwork_forge_amd import HyperGNN, _build, _native

EINVAL = -1
DIST_FUNCTIONS = ["ghf_dist_bwd", "ghf_dist_negsamp_fwd", "ghf_dist_rank", "ghf_dist_rows_grad", "ghf_dist_softmax_fwd",
                  "ghf_dist_workspace_bytes"]


# ---- the keyword ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model():
    return HyperGNN(text_dim=32, node_feat_dim=16, hidden_dim=16)


def _calls(model):
    return [("rank_candidates", model.rank_candidates), ("softmax_loss", model.softmax_loss),
            ("negative_sampling_loss", model.negative_sampling_loss)]


def test_the_three_methods_take_the_keyword_and_the_other_two_do_not(model):
    for name, fn in _calls(model):
        p = inspect.signature(fn).parameters
        assert "distance" in p and p["distance"].default is None and p["distance"].kind is inspect.Parameter.KEYWORD_ONLY, name
        assert '``"complex"``' in fn.__doc__, f"{name}: the docstring must name the three distances"
    for fn in (model.topk_candidates, model.bce_loss):
        assert "distance" not in inspect.signature(fn).parameters


def test_keyword_validation_needs_no_device(model):
    """CPU tensors throughout: each error below is raised before the "HIP device only" RuntimeError."""
    N, B, K = 50, 6, 4
    embs = torch.randn(N, 16)
    odd = torch.randn(N, 15)
    q, t = torch.arange(B), torch.arange(B) + 1
    neg = torch.randint(0, N, (B, K))
    for name, fn in _calls(model):
        for metric in R.METRICS:
            with pytest.raises(ValueError, match="dot product"):
                fn(embs, q, t, distance=metric)                                            # the all-node sweep
            with pytest.raises(ValueError, match="dot product"):
                fn(embs, q, t, distance=metric, candidates=torch.arange(10))               # the shared set
            with pytest.raises(ValueError, match="dot product"):
                fn(embs, q, t, distance=metric, negatives=neg, candidates=torch.arange(10))
            with pytest.raises(ValueError, match="dot product"):
                fn(embs, q, t, distance=metric, negatives=neg, candidate_bias=torch.zeros(N))
        for bad in ("L1", "cosine", "", 1, ("l1",)):
            with pytest.raises(ValueError, match="distance must be"):
                fn(embs, q, t, distance=bad, negatives=neg)
        with pytest.raises(ValueError, match="even d"):
            fn(odd, q, t, distance="complex", negatives=neg)
        for metric, e in (("l1", embs), ("l2", embs), ("complex", embs), ("l1", odd), ("l2", odd)):
            with pytest.raises(RuntimeError, match="HIP device"):                          # valid: only now the device is asked for
                fn(e, q, t, distance=metric, negatives=neg)
        with pytest.raises(RuntimeError, match="HIP device"):                              # None is the call without the keyword
            fn(embs, q, t, distance=None, negatives=neg)
        bad = neg.clone()
        bad[0, 0] = N
        with pytest.raises(IndexError, match="negatives"):                                 # negatives= is checked as without it
            fn(embs, q, t, distance="l1", negatives=bad)


# ---- the headers and the library -----------------------------------------------------------------------------------------
def test_the_other_two_headers_are_as_they_were():
    with open(os.path.join(_build.INCLUDE, "ghf.h")) as f:
        text = f.read()
    assert re.search(r"#define GHF_ABI_VERSION 15\b", text) and _native.ABI_VERSION == 15
    assert len(_native.header_symbols()) == 113 and set(_native.header_symbols()) == set(_native.SIGNATURES)
    assert not [s for s in _native.header_symbols() + _native.negatives_header_symbols() if s.startswith("ghf_dist_")]
    assert _native.negatives_header_symbols() == ["ghf_neg_bwd", "ghf_neg_negsamp_fwd", "ghf_neg_rank", "ghf_neg_softmax_fwd",
                                                  "ghf_neg_workspace_bytes"]
    assert set(_native.NEG_SIGNATURES) == set(_native.negatives_header_symbols())


def test_every_function_of_the_header_is_bound_and_exported():
    with open(os.path.join(_build.INCLUDE, "ghf_distance.h")) as f:
        text = f.read()
    declared = sorted(set(re.findall(r"\b(ghf_[a-z_0-9]+)\s*\(", text)))
    assert declared == DIST_FUNCTIONS == _native.distance_header_symbols()
    assert set(_native.DIST_SIGNATURES) == set(declared)
    assert not set(declared) & (set(_native.SIGNATURES) | set(_native.NEG_SIGNATURES))
    assert os.path.join(_build.INCLUDE, "ghf_distance.h") in _build.HEADERS and "distance.hip" in _build.SOURCES
    for name, value in (("GHF_DIST_L1", _native.DIST_L1), ("GHF_DIST_L2", _native.DIST_L2), ("GHF_DIST_COMPLEX", _native.DIST_COMPLEX),
                        ("GHF_DIST_SOFTMAX", _native.NEG_SOFTMAX), ("GHF_DIST_NEGSAMP", _native.NEG_NEGSAMP)):
        assert re.search(rf"#define {name} {value}\b", text), name
    assert _native.DIST_METRICS == {"l1": 1, "l2": 2, "complex": 3}
    lib = _native.load()
    for name in declared:
        fn = getattr(lib, name)                                                    # AttributeError: not exported
        assert fn.argtypes == _native.DIST_SIGNATURES[name][1] and fn.restype is _native.DIST_SIGNATURES[name][0]
    assert lib.ghf_abi_version() == 15
    # the argument count of every declaration is the table's
    flat = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    for name in declared:
        args = re.search(rf"\b{name}\s*\(([^)]*)\)\s*;", flat).group(1)
        assert len(args.split(",")) == len(_native.DIST_SIGNATURES[name][1]), name


def test_the_header_is_plain_c(tmp_path):
    """include/ghf_distance.h compiles as C99 with -Wall -Werror, alone and beside the other two."""
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "use.c"
    src.write_text('#include "ghf_distance.h"\n#include "ghf.h"\n#include "ghf_negatives.h"\n#include "ghf_distance.h"\n'
                   "int use(void) {\n    void* fns[] = {" + ", ".join(f"(void*)(size_t)&{n}" for n in DIST_FUNCTIONS) + "};\n"
                   "    return (int)(sizeof fns / sizeof fns[0]) + GHF_DIST_L1 + GHF_DIST_L2 + GHF_DIST_COMPLEX + GHF_DIST_SOFTMAX"
                   " + GHF_DIST_NEGSAMP;\n}\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", _build.INCLUDE, "-c", str(src), "-o", str(tmp_path / "use.o")],
                   check=True, capture_output=True, text=True)


def test_size_query_and_argument_checks_without_a_launch():
    """Every call below is refused by a check that stands ahead of the launch: the pointers are host buffers that nothing
    dereferences."""
    lib = _native.load()
    assert _native.dist_workspace_bytes(5, 7, 128, 0) > 0 and _native.dist_workspace_bytes(5, 7, 128, 0) % 256 == 0
    for B, K, d, nnz in ((0, 7, 128, 0), (5, 0, 128, 0), (5, 7, 0, 0), (5, 7, 257, 0), (5, 7, 128, -1), (1 << 20, 1 << 11, 128, 0),
                         (1 << 31, 1, 128, 0)):
        assert _native.dist_workspace_bytes(B, K, d, nnz) == 0, (B, K, d, nnz)
    assert _native.dist_workspace_bytes((1 << 20) - 1, (1 << 11) - 1, 256, 0) > 0          # B (K + 1) just below 2^31
    need = _native.dist_workspace_bytes(1, 1, 8, 0)

    raw = (ctypes.c_char * 1024)()
    p = (ctypes.addressof(raw) + 255) & ~255                                               # a 256-byte aligned stand-in
    err = lambda: lib.ghf_last_error().decode()

    def calls(metric, d, ws_bytes):
        return [("rank", lib.ghf_dist_rank(metric, p, p, None, p, None, None, 0, 1, 1, 1, d, p, 1, p, ws_bytes, p, p, None)),
                ("softmax", lib.ghf_dist_softmax_fwd(metric, p, p, None, p, None, None, 0, 1, 1, 1, d, 1.0, p, 1, p, ws_bytes, p, p,
                                                     None)),
                ("negsamp", lib.ghf_dist_negsamp_fwd(metric, p, p, None, p, None, None, 0, 1, 1, 1, d, 1.0, 0.0, 0.0, p, 1, p, ws_bytes,
                                                     p, p, None)),
                ("bwd", lib.ghf_dist_bwd(metric, 0, p, p, None, p, None, None, 0, 1, 1, 1, d, 1.0, 0.0, 0.0, p, 1, p, p, p, ws_bytes, p,
                                         p, None))]

    for metric in (0, 4, -1):                                                              # an unknown metric
        for what, rc in calls(metric, 8, need) + [("rows_grad", lib.ghf_dist_rows_grad(metric, p, p, None, 1, 1, 1, 8, 1, p, p, p, p,
                                                                                       None))]:
            assert rc == EINVAL and "metric" in err(), (what, metric, rc, err())
    for what, rc in calls(_native.DIST_COMPLEX, 7, need) + [("rows_grad", lib.ghf_dist_rows_grad(_native.DIST_COMPLEX, p, p, None, 1, 1,
                                                                                                  1, 7, 1, p, p, p, p, None))]:
        assert rc == EINVAL and "even d" in err(), (what, rc, err())                      # odd d under COMPLEX
    for metric in (_native.DIST_L1, _native.DIST_L2, _native.DIST_COMPLEX):                # a short workspace
        for what, rc in calls(metric, 8, need - 1):
            assert rc == EINVAL and "workspace" in err(), (what, metric, rc, err())
    # null pointers, a bad mode, d beyond the limit
    assert lib.ghf_dist_rank(1, None, None, None, None, None, None, 0, 1, 1, 1, 8, None, 1, None, 0, None, None, None) == EINVAL
    assert "null pointer" in err()
    assert lib.ghf_dist_rows_grad(1, None, None, None, 1, 1, 1, 8, 1, None, None, None, None, None) == EINVAL and "null pointer" in err()
    assert lib.ghf_dist_bwd(1, 2, p, p, None, p, None, None, 0, 1, 1, 1, 8, 1.0, 0.0, 0.0, p, 1, p, p, p, need, p, p, None) == EINVAL
    assert "mode" in err()
    assert lib.ghf_dist_rank(1, p, p, None, p, None, None, 0, 1, 1, 1, 260, p, 1, p, need, p, p, None) == -3     # GHF_EUNSUPPORTED
    assert lib.ghf_dist_rows_grad(1, p, p, None, 1, 1, 1, 260, 1, p, p, p, p, None) == -3


# ---- the restatement against autograd ------------------------------------------------------------------------------------
def explicit_scores(metric, q, c, target, neg):
    """(s [B, K], s_t [B]) through the [B, K, d] tensor, differentiable: L1 by abs, L2 and COMPLEX by a guarded norm (the
    square root is taken of 1 where its argument is 0 and the result put back to 0, so its gradient there is 0, not NaN)."""
    def D(delta):
        if metric == "l1":
            return delta.abs().sum(-1)
        sq = (delta * delta).sum(-1) if metric == "l2" else (delta * delta).reshape(*delta.shape[:-1], -1, 2).sum(-1)
        zero = sq == 0
        root = torch.sqrt(torch.where(zero, torch.ones_like(sq), sq)).masked_fill(zero, 0.0)
        return root if metric == "l2" else root.sum(-1)
    return -D(q.unsqueeze(1) - c[neg.clamp(min=0)]), -D(q - c[target])


def problem(N, B, d, K, seed, integer=False):
    g = torch.Generator().manual_seed(seed)
    c = torch.randn(N, d, generator=g)
    q = torch.randn(B, d, generator=g)
    if integer:
        c, q = torch.round(c), torch.round(q)
    target = torch.randint(0, N, (B,), generator=g)
    neg = torch.randint(0, N, (B, K), generator=g)
    neg[torch.rand(B, K, generator=g) < 0.2] = -1                                  # ragged rows
    if K > 2:
        neg[:, 1] = neg[:, 0]                                                      # a repeated id: it counts twice
        neg[::2, 2] = target[::2]                                                  # the target among its own negatives
    rng = np.random.default_rng(seed)
    lists = [np.unique(np.append(rng.integers(0, N, 3), max(int(neg[i, 0]), 0))) if i % 3 == 0 else np.zeros(0, dtype=np.int64)
             for i in range(B)]
    grad = torch.randn(B, generator=g)
    return c, q, target, neg, lists, grad


def autograd_losses(metric, mode, q64, c64, target, neg, lists, scale, margin, alpha):
    s, st = explicit_scores(metric, q64, c64, target, neg)
    z, zt = scale * s, scale * st
    drop = ~R.live_positions(neg, target, lists)
    if mode == "softmax":
        logits = torch.cat([zt.unsqueeze(1), z.masked_fill(drop, -np.inf)], 1)
        return F.cross_entropy(logits, torch.zeros(len(target), dtype=torch.int64), reduction="none")
    some = ~drop.all(1)
    w = torch.softmax((alpha * z).masked_fill(drop, -np.inf)[some], -1).detach()
    negterm = torch.zeros(len(target), dtype=torch.float64)
    negterm[some] = -(w * F.logsigmoid(-(z[some] + margin)).masked_fill(drop[some], 0.0)).sum(1)
    return -F.logsigmoid(zt + margin) + negterm


@pytest.mark.parametrize("shape", [(257, 65, 20, 9), (70, 9, 64, 33), (5, 3, 8, 1)])
@pytest.mark.parametrize("metric", R.METRICS)
@pytest.mark.parametrize("mode", ["softmax", "negsamp"])
def test_restatement_agrees_with_autograd_of_the_explicit_formulation(shape, metric, mode):
    """Random float rows: no difference is exactly zero (the queries are rows of their own), so autograd's abs and sqrt are
    differentiable everywhere they are used."""
    N, B, d, K = shape
    c, q, target, neg, lists, grad = problem(N, B, d, K, seed=N)
    c64, q64 = c.double().requires_grad_(), q.double().requires_grad_()
    assert bool(((q64.unsqueeze(1) - c64[neg.clamp(min=0)]) != 0).all())
    want = autograd_losses(metric, mode, q64, c64, target, neg, lists, 0.3, 2.0, 0.7)
    (want * grad.double()).sum().backward()
    got = R.loss(mode, metric, q, c, target, neg, lists, scale=0.3, margin=2.0, alpha=0.7, grad=grad)
    assert torch.allclose(got["loss"], want.detach(), rtol=1e-12, atol=1e-12)
    assert torch.allclose(got["dq"], q64.grad, rtol=1e-10, atol=1e-10)
    assert torch.allclose(got["dc"], c64.grad, rtol=1e-10, atol=1e-10)
    assert K == 1 or (float(got["dq"].abs().max()) > 0 and float(got["dc"].abs().max()) > 0)   # (K = 1: every set may be empty)


@pytest.mark.parametrize("metric", R.METRICS)
def test_zero_conventions_on_rows_with_exact_zeros(metric):
    """Integer rows, the query's own row among its negatives and as its target's twin: D = 0 and single zero differences.
    The restatement's gradients are the stated conventions — finite everywhere, 0 where the denominator is 0 — and agree with
    autograd of the guarded formulation (abs' subgradient at 0 is 0 in torch, the guarded root's too)."""
    N, B, d, K = 40, 8, 6, 5
    c, q, target, neg, lists, grad = problem(N, B, d, K, seed=3, integer=True)
    q = c[:B].clone()                                                              # the queries are rows 0 .. B - 1 of c
    neg[:, 0] = torch.arange(B)                                                    # D = 0: the query's own row, first
    neg[:, 3] = torch.arange(B) + B
    c[B:2 * B] = c[:B]
    c[B:2 * B, 0] += 3.0                                                           # differs from the query in one pair only
    c[2 * B] = c[0]
    target[0] = 2 * B                                                              # a target at distance 0
    lists = [np.zeros(0, dtype=np.int64)] * B
    D, g = R.dist(metric, q, c[neg[:, 0]])
    assert torch.equal(D, torch.zeros(B, dtype=torch.float64)) and torch.equal(g, torch.zeros(B, d, dtype=torch.float64))
    D, g = R.dist(metric, q, c[neg[:, 3]])
    assert torch.equal(D, torch.full((B,), 3.0, dtype=torch.float64))
    assert torch.equal(g[:, 0], torch.full((B,), -1.0, dtype=torch.float64)) and torch.equal(g[:, 1:], torch.zeros(B, d - 1, dtype=torch.float64))
    for mode in ("softmax", "negsamp"):
        c64, q64 = c.double().requires_grad_(), q.double().requires_grad_()
        want = autograd_losses(metric, mode, q64, c64, target, neg, lists, 0.5, 1.0, 1.0)
        (want * grad.double()).sum().backward()
        got = R.loss(mode, metric, q, c, target, neg, lists, scale=0.5, margin=1.0, alpha=1.0, grad=grad)
        for k in ("loss", "dq", "dc", "coef"):
            assert bool(torch.isfinite(got[k]).all()), k
        assert bool((got["coef"][:, 0] != 0).all())                                # the zero-distance entries do carry weight
        assert torch.allclose(got["loss"], want.detach(), rtol=1e-12, atol=1e-12)
        assert torch.allclose(got["dq"], q64.grad, rtol=1e-10, atol=1e-10)
        assert torch.allclose(got["dc"], c64.grad, rtol=1e-10, atol=1e-10)


def test_rank_restatement_is_compare_and_count():
    c, q, target, neg, lists, _ = problem(70, 9, 8, 33, seed=5, integer=True)
    for metric in R.METRICS:
        s, st = explicit_scores(metric, q.double(), c.double(), target, neg)
        live = R.live_positions(neg, target, lists)
        greater, equal = R.rank(metric, q, c, target, neg, lists)
        assert torch.equal(greater, ((s > st.unsqueeze(1)) & live).sum(1))
        assert torch.equal(equal, ((s == st.unsqueeze(1)) & live).sum(1))
        assert metric != "l1" or int(equal.sum()) > 0                              # integer L1 distances do tie
