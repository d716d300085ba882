"""Pairwise ranking losses on per-query negative sets, the part that needs no GPU: the sixth header include/ghf_pairwise.h
against _native.PAIR_SIGNATURES and the built library (the five older headers and ABI 15 as they were), the size query and
every refusal in the header's order with nothing launched, every Python-level error of HyperGNN.pairwise_loss from CPU
tensors, the float64 restatement (tests/_pairwise_ref.py) against F.margin_ranking_loss and an explicit [B, K, d]
formulation written independently of it, and — on every problem the GPU parity test runs — that no pair lies in the
near-tie band around the kink and that the same formulas in fp32 pass the project's loss_check / grad_check."""

import ctypes
import functools
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _pairwise_ref as R
from graph_hypernetwork_forge_amd import HyperGNN, _build, _native
from test_softmax_gpu import grad_check, loss_check

EINVAL, EUNSUPPORTED = -1, -3
PAIR_FUNCTIONS = ["ghf_pair_bwd", "ghf_pair_fwd", "ghf_pair_workspace_bytes"]


# ---- the headers and the library -----------------------------------------------------------------------------------------
def test_the_five_older_headers_and_the_abi_are_as_they_were():
    with open(os.path.join(_build.INCLUDE, "ghf.h")) as f:
        text = f.read()
    assert re.search(r"#define GHF_ABI_VERSION 15\b", text) and _native.ABI_VERSION == 15
    assert len(_native.header_symbols()) == 113 and set(_native.header_symbols()) == set(_native.SIGNATURES)
    older = [(_native.negatives_header_symbols, _native.NEG_SIGNATURES, 5), (_native.distance_header_symbols, _native.DIST_SIGNATURES, 6),
             (_native.distance_sweep_header_symbols, _native.DSWEEP_SIGNATURES, 4),
             (_native.distance_loss_header_symbols, _native.DLOSS_SIGNATURES, 5)]
    for symbols, table, count in older:
        assert set(symbols()) == set(table) and len(table) == count
        assert not [s for s in symbols() if s.startswith("ghf_pair_")]
    assert not [s for s in _native.header_symbols() if s.startswith("ghf_pair_")]
    for name in ("ghf.h", "ghf_negatives.h", "ghf_distance.h", "ghf_distance_sweep.h", "ghf_distance_loss.h"):
        with open(os.path.join(_build.INCLUDE, name)) as f:
            assert "pairwise" not in f.read().lower(), name


def test_every_function_of_the_header_is_bound_and_exported():
    with open(os.path.join(_build.INCLUDE, "ghf_pairwise.h")) as f:
        text = f.read()
    flat = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    declared = sorted(set(re.findall(r"\b(ghf_[a-z_0-9]+)\s*\(", flat)))
    assert declared == PAIR_FUNCTIONS == _native.pairwise_header_symbols()
    assert set(_native.PAIR_SIGNATURES) == set(declared)
    assert not set(declared) & (set(_native.SIGNATURES) | set(_native.NEG_SIGNATURES) | set(_native.DIST_SIGNATURES)
                                | set(_native.DSWEEP_SIGNATURES) | set(_native.DLOSS_SIGNATURES))
    assert os.path.join(_build.INCLUDE, "ghf_pairwise.h") in _build.HEADERS and "pairwise.hip" in _build.SOURCES
    for name, value in (("GHF_PAIR_DOT", _native.PAIR_DOT), ("GHF_PAIR_HINGE", _native.PAIR_HINGE),
                        ("GHF_PAIR_LOGISTIC", _native.PAIR_LOGISTIC)):
        assert re.search(rf"#define {name} {value}\b", text), name
    assert (_native.PAIR_DOT, _native.PAIR_HINGE, _native.PAIR_LOGISTIC) == (0, 1, 2)
    assert _native.PAIR_KINDS == {"hinge": 1, "logistic": 2}
    assert _native.PAIR_DOT not in _native.DIST_METRICS.values()
    lib = _native.load()
    for name in declared:
        fn = getattr(lib, name)                                                    # AttributeError: not exported
        assert fn.argtypes == _native.PAIR_SIGNATURES[name][1] and fn.restype is _native.PAIR_SIGNATURES[name][0]
    assert lib.ghf_abi_version() == 15
    for name, count in (("ghf_pair_workspace_bytes", 4), ("ghf_pair_fwd", 25), ("ghf_pair_bwd", 26)):
        args = re.search(rf"\b{name}\s*\(([^)]*)\)\s*;", flat).group(1)
        assert len(args.split(",")) == len(_native.PAIR_SIGNATURES[name][1]) == count, name


def test_the_header_is_plain_c(tmp_path):
    """include/ghf_pairwise.h compiles as C99 with -Wall -Wextra -Werror, alone and beside the other five."""
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "use.c"
    src.write_text('#include "ghf_pairwise.h"\n#include "ghf.h"\n#include "ghf_negatives.h"\n#include "ghf_distance.h"\n'
                   '#include "ghf_distance_sweep.h"\n#include "ghf_distance_loss.h"\n#include "ghf_pairwise.h"\n'
                   "int use(void) {\n    void* fns[] = {" + ", ".join(f"(void*)(size_t)&{n}" for n in PAIR_FUNCTIONS) + "};\n"
                   "    return (int)(sizeof fns / sizeof fns[0]) + GHF_PAIR_DOT + GHF_PAIR_HINGE + GHF_PAIR_LOGISTIC + GHF_DIST_L1;\n}\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", _build.INCLUDE, "-c", str(src), "-o", str(tmp_path / "use.o")],
                   check=True, capture_output=True, text=True)


def test_size_query_and_refusals_in_the_stated_order_without_a_launch():
    """Every call below is refused by a check that stands ahead of the launch: the pointers are host buffers that nothing
    dereferences.  Each call breaks the rule under test AND every later one, so the message says which check came first."""
    lib = _native.load()
    assert _native.pair_workspace_bytes(5, 7, 128, 0) == _native.neg_workspace_bytes(5, 7, 128, 0) == 256
    for B, K, d, nnz in ((0, 7, 128, 0), (5, 0, 128, 0), (5, 7, 0, 0), (5, 7, 257, 0), (5, 7, 128, -1), (1 << 20, 1 << 11, 128, 0),
                         (1 << 31, 1, 128, 0)):
        assert _native.pair_workspace_bytes(B, K, d, nnz) == 0, (B, K, d, nnz)
    assert _native.pair_workspace_bytes((1 << 20) - 1, (1 << 11) - 1, 256, 0) > 0          # B (K + 1) just below 2^31
    need = _native.pair_workspace_bytes(1, 1, 8, 0)

    raw = (ctypes.c_char * 1024)()
    p = (ctypes.addressof(raw) + 255) & ~255                                               # a 256-byte aligned stand-in
    err = lambda: lib.ghf_last_error().decode()
    inf, nan = float("inf"), float("nan")

    def both(metric=0, kind=1, d=8, scale=1.0, margin=1.0, normalize=1, bias=None, ptrs=True, ws=p, ws_bytes=need, N=1, K=1, B=1):
        x = p if ptrs else None
        return [("fwd", lib.ghf_pair_fwd(metric, kind, x, p, None, p, None, None, 0, 1, N, B, d, scale, margin, normalize, p, K, bias, ws,
                                         ws_bytes, p, p, p, None)),
                ("bwd", lib.ghf_pair_bwd(metric, kind, x, p, None, p, None, None, 0, 1, N, B, d, scale, margin, normalize, p, K, bias, p,
                                         p, ws, ws_bytes, p, p, None))]

    def refused(word, code=EINVAL, **kw):
        for what, rc in both(**kw):
            assert rc == code and word in err(), (what, kw, rc, err())

    later = dict(kind=0, scale=-1.0, margin=inf, normalize=2, ptrs=False, ws_bytes=0, d=300)       # everything after the metric
    for metric in (4, -1, 7):
        refused("metric", metric=metric, **later)
    refused("even d", metric=_native.DIST_COMPLEX, **{**later, "d": 7})
    later = dict(scale=-1.0, margin=inf, normalize=2, ptrs=False, ws_bytes=0, d=300)               # ... after the kind
    for kind in (0, 3, -1):                                                                        # 0: no public kind is zero
        for metric in (0, 1, 2, 3):
            refused("kind", metric=metric, kind=kind, bias=p if metric else None, **{**later, "d": 300 if metric != 3 else 302})
    later = dict(margin=nan, normalize=2, bias=p, ptrs=False, ws_bytes=0, d=300)                   # ... after the scale
    for scale in (0.0, -1.0, inf, nan):
        refused("scale", metric=1, scale=scale, **later)
    later = dict(normalize=-1, bias=p, ptrs=False, ws_bytes=0, d=300)                              # ... after the margin
    for margin in (inf, -inf, nan):
        refused("margin", metric=2, margin=margin, **later)
    later = dict(bias=p, ptrs=False, ws_bytes=0, d=300)                                            # ... after normalize
    for normalize in (2, -1):
        refused("normalize", metric=1, normalize=normalize, **later)
    for metric in (1, 2, 3):                                                                       # a bias under a distance
        refused("bias", metric=metric, bias=p, ptrs=False, ws_bytes=0, d=300)
    # the per-query order after that
    refused("null pointer", ptrs=False, ws_bytes=0, d=300)
    refused("aligned", ws=p + 8, ws_bytes=0, d=300)
    refused("K >= 1", K=0, ws_bytes=0, d=300)
    refused("bad shape", N=0, ws_bytes=0, d=300)
    refused("exceeds", code=EUNSUPPORTED, d=300, N=1 << 31, ws_bytes=0)
    refused("N out of range", N=1 << 31, ws_bytes=0)
    refused("B (K + 1)", B=1 << 20, K=1 << 11, ws_bytes=0)
    for metric in (0, 1, 2, 3):
        for kind in (1, 2):
            refused("workspace", metric=metric, kind=kind, ws_bytes=need - 1)
    refused("workspace", bias=p, ws_bytes=need - 1)                                                # (a bias goes with the dot product)


# ---- the method's own checks ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model():
    return HyperGNN(text_dim=32, node_feat_dim=16, hidden_dim=16)


def test_the_signature(model):
    p = inspect.signature(model.pairwise_loss).parameters
    assert list(p)[:3] == ["embs", "query", "target"]
    want = dict(loss="hinge", margin=1.0, scale=1.0, normalize=True, distance=None, known=None, filt_ptr=None, filt_idx=None,
                query_rows=None, query_rel=None, candidate_bias=None, return_active=False)
    for k, v in want.items():
        assert p[k].kind is inspect.Parameter.KEYWORD_ONLY and p[k].default == v, k
    assert p["negatives"].kind is inspect.Parameter.KEYWORD_ONLY and p["negatives"].default is inspect.Parameter.empty
    assert set(p) == {"embs", "query", "target", "negatives"} | set(want)
    assert "TransE" in model.pairwise_loss.__doc__ and "BPR" in model.pairwise_loss.__doc__


def test_every_python_level_error_comes_from_metadata(model):
    """CPU tensors throughout: each error below is raised before the "HIP device only" RuntimeError."""
    N, B, K = 50, 6, 4
    embs, odd = torch.randn(N, 16), torch.randn(N, 15)
    q, t = torch.arange(B), torch.arange(B) + 1
    neg = torch.randint(0, N, (B, K))
    fn = model.pairwise_loss
    with pytest.raises(TypeError):
        fn(embs, q, t)                                                                     # negatives is required
    with pytest.raises(ValueError, match="negatives"):
        fn(embs, q, t, negatives=None)
    with pytest.raises(ValueError, match=r"\[N, d\]"):
        fn(embs[0], q, t, negatives=neg)
    for bad in ("Hinge", "bpr", "", 1, None):
        with pytest.raises(ValueError, match="loss must be"):
            fn(embs, q, t, negatives=neg, loss=bad)
    for bad in ("L1", "cosine", "", 1):
        with pytest.raises(ValueError, match="distance must be"):
            fn(embs, q, t, negatives=neg, distance=bad)
    with pytest.raises(ValueError, match="even d"):
        fn(odd, q, t, negatives=neg, distance="complex")
    for metric in ("l1", "l2", "complex"):
        with pytest.raises(ValueError, match="candidate_bias"):
            fn(embs, q, t, negatives=neg, distance=metric, candidate_bias=torch.zeros(N))
    with pytest.raises(ValueError, match="candidate_bias"):
        fn(embs, q, t, negatives=neg, candidate_bias=torch.zeros(N - 1))
    with pytest.raises(ValueError, match="candidate_bias"):
        fn(embs, q, t, negatives=neg, candidate_bias=torch.zeros(N, dtype=torch.float64))
    for bad in (neg[0], neg[:B - 1], neg[:, :0], [[1, 2]]):
        with pytest.raises(ValueError, match="negatives"):
            fn(embs, q, t, negatives=bad)
    with pytest.raises(TypeError, match="negatives"):
        fn(embs, q, t, negatives=neg.float())
    for entry in (N, -2):
        bad = neg.clone()
        bad[0, 0] = entry                                                                  # -1 alone is the padding: ids do not wrap
        with pytest.raises(IndexError, match="negatives"):
            fn(embs, q, t, negatives=bad)
    with pytest.raises(IndexError, match="query"):
        fn(embs, q + N, t, negatives=neg)
    with pytest.raises(IndexError, match="target"):
        fn(embs, q, t - N - 2, negatives=neg)
    with pytest.raises(TypeError, match="query"):
        fn(embs, q.float(), t, negatives=neg)
    with pytest.raises(ValueError, match="targets"):
        fn(embs, q, t[:B - 1], negatives=neg)
    with pytest.raises(ValueError, match="query_rows"):
        fn(embs, q, t, negatives=neg, query_rows=torch.randn(B, 15))
    with pytest.raises(TypeError, match="query_rows"):
        fn(embs, q, t, negatives=neg, query_rows=torch.randn(B, 16, dtype=torch.float64))
    for scale in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="scale"):
            fn(embs, q, t, negatives=neg, scale=scale)
    for margin in (float("inf"), float("-inf"), float("nan")):
        with pytest.raises(ValueError, match="margin"):
            fn(embs, q, t, negatives=neg, margin=margin)
    with pytest.raises(TypeError, match="bools"):
        fn(embs, q, t, negatives=neg, normalize=1)
    with pytest.raises(TypeError, match="bools"):
        fn(embs, q, t, negatives=neg, return_active="yes")
    for kind in R.KINDS:                                                                   # valid: only now the device is asked for
        for distance in (None, "l1", "l2", "complex"):
            with pytest.raises(RuntimeError, match="HIP device"):
                fn(embs, q, t, negatives=neg, loss=kind, distance=distance, margin=0.0, normalize=False, return_active=True)
    with pytest.raises(RuntimeError, match="HIP device"):
        fn(embs, q, t, negatives=neg, candidate_bias=torch.zeros(N))
    # the lists' checks come behind the device check, as in the siblings; their forms are refused all the same
    with pytest.raises((ValueError, RuntimeError)):
        fn(embs, q, t, negatives=neg, known=(q, t), filt_ptr=torch.zeros(B + 1, dtype=torch.int64), filt_idx=torch.zeros(0, dtype=torch.int64))


def test_the_native_wrappers_check_before_they_load_anything():
    c, q = torch.randn(10, 8), torch.randn(3, 8)
    t, neg = torch.zeros(3, dtype=torch.int64), torch.zeros(3, 2, dtype=torch.int64)
    for fn, extra in ((_native.score_pair_fwd, ()), (_native.score_pair_bwd, (torch.zeros(3, dtype=torch.int32), torch.zeros(3)))):
        with pytest.raises(RuntimeError, match="HIP device"):                              # _req, as in the per-query siblings
            fn(_native.PAIR_DOT, _native.PAIR_HINGE, q, c, t, neg, *extra)


# ---- the restatement against torch's own loss and an explicit formulation --------------------------------------------------
def explicit(kind, score, q, c, target, neg, lists, bias, scale, margin, normalize, dtype):
    """loss [B] through the [B, K, d] tensor in `dtype`, differentiable: L1 by abs, L2 and COMPLEX by a guarded root (its
    gradient at 0 is 0, not NaN), the hinge by a mask."""
    rows = c[neg.clamp(min=0)]                                                         # [B, K, d]
    def S(x, y):
        if score == "dot":
            return (x * y).sum(-1)
        delta = x - y
        if score == "l1":
            return -delta.abs().sum(-1)
        sq = (delta * delta).sum(-1) if score == "l2" else (delta * delta).reshape(*delta.shape[:-1], -1, 2).sum(-1)
        zero = sq == 0
        root = torch.sqrt(torch.where(zero, torch.ones_like(sq), sq)).masked_fill(zero, 0.0)
        return -(root if score == "l2" else root.sum(-1))
    z, zt = scale * S(q.unsqueeze(1), rows), scale * S(q, c[target])
    if bias is not None:
        z, zt = z + bias[neg.clamp(min=0)], zt + bias[target]
    u = z - zt.unsqueeze(1) + margin
    phi = u * (u > 0).to(dtype) if kind == "hinge" else torch.logaddexp(u, torch.zeros_like(u))   # (F.softplus is u beyond 20)
    live = R.live_positions(neg, target, lists)
    total = (phi * live.to(dtype)).sum(1)
    return total / live.sum(1).clamp(min=1).to(dtype) if normalize else total


def test_restatement_at_K_1_is_torch_margin_ranking_loss():
    g = torch.Generator().manual_seed(0)
    N, B, d = 40, 33, 12
    c, q = torch.randn(N, d, generator=g), torch.randn(B, d, generator=g)
    target = torch.randint(0, N, (B,), generator=g)
    neg = (target + 1 + torch.randint(0, N - 1, (B,), generator=g)).remainder(N).unsqueeze(1)     # never the target
    for score in R.SCORES:
        for margin in (0.0, 1.0, 2.5):
            got = R.loss("hinge", score, q, c, target, neg, scale=0.7, margin=margin)
            z, zt = R.scores(score, q.double(), c.double(), target, neg, None, 0.7)
            want = F.margin_ranking_loss(zt, z[:, 0], torch.ones(B, dtype=torch.float64), margin=margin, reduction="none")
            assert torch.allclose(got["loss"], want, rtol=1e-13, atol=1e-13) and float(want.max()) > 0
            soft = R.loss("logistic", score, q, c, target, neg, scale=0.7, margin=margin)
            assert torch.allclose(soft["loss"], F.softplus(z[:, 0] - zt + margin), rtol=1e-12, atol=1e-12)
            assert torch.equal(got["count"], torch.ones(B, dtype=torch.int64))
            assert torch.equal(got["active"], (want > 0).to(torch.int64))


@pytest.mark.parametrize("shape", [(257, 65, 20, 9), (70, 9, 64, 33), (5, 3, 8, 1)])
@pytest.mark.parametrize("score", R.SCORES)
@pytest.mark.parametrize("kind", R.KINDS)
def test_restatement_agrees_with_autograd_of_the_explicit_formulation(shape, score, kind):
    N, B, d, K = shape
    p = R.problem(d, K, B, N, seed=N)
    q = p["embs"][p["query"]]
    bias = p["bias"] if score == "dot" else None
    for normalize in (True, False):
        c64, q64 = p["embs"].double().requires_grad_(), q.double().requires_grad_()
        b64 = None if bias is None else bias.double().requires_grad_()
        want = explicit(kind, score, q64, c64, p["target"], p["neg"], p["lists"], b64, 0.3, 0.8, normalize, torch.float64)
        (want * p["grad"].double()).sum().backward()
        got = R.loss(kind, score, q, p["embs"], p["target"], p["neg"], p["lists"], bias, scale=0.3, margin=0.8, normalize=normalize,
                     grad=p["grad"])
        assert torch.allclose(got["loss"], want.detach(), rtol=1e-12, atol=1e-12)
        assert torch.allclose(got["dq"], q64.grad, rtol=1e-10, atol=1e-10)
        assert torch.allclose(got["dc"], c64.grad, rtol=1e-10, atol=1e-10)
        if b64 is not None:
            assert torch.allclose(got["db"], b64.grad, rtol=1e-10, atol=1e-10)
        # coef is d loss / d s: through it, dq is the per-query siblings' sum
        coef = got["coef"]
        assert torch.allclose(coef[:, K], -coef[:, :K].sum(1), rtol=0, atol=1e-15) and bool((coef[:, :K][~got["live"]] == 0).all())
        if score == "dot":
            dq = coef[:, K:] * p["embs"].double()[p["target"]] + (coef[:, :K].unsqueeze(2) * p["embs"].double()[p["neg"].clamp(min=0)]).sum(1)
            assert torch.allclose(got["dq"], dq, rtol=1e-10, atol=1e-10)
        assert K == 1 or float(got["dq"].abs().max()) > 0


def test_documented_row_sum_is_a_sum_in_every_geometry():
    rng = np.random.default_rng(0)
    for d, vec in ((20, True), (64, True), (128, True), (256, True), (6, False)):
        for K in (1, 7, 64, 65, 256, 257, 1000):
            ints = rng.integers(-8, 9, K).astype(np.float32)                               # exact whatever the order
            assert R.documented_row_sum(ints, d, vec) == ints.sum()
            x = rng.standard_normal(K).astype(np.float32)
            assert abs(float(R.documented_row_sum(x, d, vec)) - float(x.astype(np.float64).sum())) < 1e-4


# ---- the problems of the GPU parity test -----------------------------------------------------------------------------------
CASES = R.parity_cases()
IDS = ["d%d-K%d-B%d-N%d-%s" % (s + (v,)) for s, v, _ in CASES]


def test_the_parity_shapes_cover_what_the_issue_lists():
    assert {s[0] for s in R.SHAPES} == {1, 3, 20, 64, 128, 200, 256}
    assert {s[1] for s in R.SHAPES} == {1, 7, 8, 9, 63, 64, 65, 256, 257, 1000}
    assert {s[2] for s in R.SHAPES} == {1, 5, 129} and {s[3] for s in R.SHAPES} == {300, 5000}
    assert 20 <= len(R.SHAPES) <= 30 and set(R.SEEDS) == set(R.SHAPES)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_no_parity_problem_has_a_pair_in_the_band_and_fp32_passes_the_checks(case):
    """kink_clear >= 1e-4 (1 + |z_it| + |margin|) for every query of the problem: the GPU parity test then needs to excuse no
    pair.  And the explicit formulation in fp32 on the CPU passes loss_check / grad_check at their defaults against the
    float64 restatement: the bounds the GPU is held to are within reach of fp32."""
    (d, K, B, N), variant, seed = case
    score = R.variant_score(variant)
    scale = R.parity_scale(score, d)
    p = R.problem(d, K, B, N, seed)
    q = p["embs"][p["query"]]
    bias = p["bias"] if variant == "dot+bias" else None
    clear, zt = R.kink_clear(score, q, p["embs"], p["target"], p["neg"], p["lists"], bias, scale, R.MARGIN)
    assert bool((clear >= R.band(zt, R.MARGIN)).all()), f"seed {seed}: a pair within {float((clear / R.band(zt, R.MARGIN)).min()):.3f} of the band"
    for kind in R.KINDS:
        for normalize in (True, False):
            want = R.loss(kind, score, q, p["embs"], p["target"], p["neg"], p["lists"], bias, scale, R.MARGIN, normalize, grad=p["grad"])
            c32, q32 = p["embs"].clone().requires_grad_(), q.clone().requires_grad_()
            b32 = None if bias is None else bias.clone().requires_grad_()
            got = explicit(kind, score, q32, c32, p["target"], p["neg"], p["lists"], b32, scale, R.MARGIN, normalize, torch.float32)
            loss_check(f"{kind} fp32 loss", got, want["loss"])
            (got * p["grad"]).sum().backward()
            if float(want["dq"].abs().max()) > 0:
                grad_check(f"{kind} fp32 rows", q32.grad.numpy(), want["dq"].numpy())
                grad_check(f"{kind} fp32 embs", c32.grad.numpy(), want["dc"].numpy())
