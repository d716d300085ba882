"""The pairwise ranking losses by dot product against every node or a shared candidate set (HyperGNN.pairwise_loss_by_dot;
include/ghf_pairwise_dot_sweep.h), the part that needs no GPU: the eighth header against _native.PAIRDOT_SIGNATURES and the
built library (the seven older headers and ABI 15 as they were), the size queries and every refusal in the header's order with
nothing launched, the method's signature and its validation from CPU tensors, the float64 restatement
(tests/_pairwise_dot_sweep_ref.py) against an explicit [B, C] torch-autograd formulation, and the conditions the GPU parity
test puts on its inputs: on the very problems it uses, at most B / 8 queries have a pair in the near-tie band around the
hinge's kink, and the same formulas in fp32 on the CPU pass loss_check / grad_check under the kink rule."""

import ctypes
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import _pairwise_dot_sweep_ref as S
from graph_hypernetwork_forge_amd import HyperGNN, _build, _native
from test_softmax_gpu import grad_check, loss_check

EINVAL, EUNSUPPORTED = -1, -3
PAIRDOT_FUNCTIONS = ["ghf_score_pair_bwd", "ghf_score_pair_bwd_workspace_bytes", "ghf_score_pair_fwd", "ghf_score_pair_fwd_workspace_bytes"]
OLDER = ("ghf.h", "ghf_negatives.h", "ghf_distance.h", "ghf_distance_sweep.h", "ghf_distance_loss.h", "ghf_pairwise.h",
         "ghf_pairwise_sweep.h")


@pytest.fixture(scope="module")
def model():
    return HyperGNN(text_dim=32, node_feat_dim=16, hidden_dim=16)


# ---- the headers and the library -----------------------------------------------------------------------------------------
def test_the_seven_older_headers_and_the_abi_are_as_they_were():
    with open(os.path.join(_build.INCLUDE, "ghf.h")) as f:
        assert re.search(r"#define GHF_ABI_VERSION 15\b", f.read()) and _native.ABI_VERSION == 15
    assert len(_native.header_symbols()) == 113 and set(_native.header_symbols()) == set(_native.SIGNATURES)
    older = [(_native.negatives_header_symbols, _native.NEG_SIGNATURES, 5), (_native.distance_header_symbols, _native.DIST_SIGNATURES, 6),
             (_native.distance_sweep_header_symbols, _native.DSWEEP_SIGNATURES, 4),
             (_native.distance_loss_header_symbols, _native.DLOSS_SIGNATURES, 5), (_native.pairwise_header_symbols, _native.PAIR_SIGNATURES, 3),
             (_native.pairwise_sweep_header_symbols, _native.PAIRSWEEP_SIGNATURES, 4)]
    for symbols, table, count in older:
        assert set(symbols()) == set(table) and len(table) == count
        assert not [s for s in symbols() if s.startswith("ghf_score_pair_")]
    assert not [s for s in _native.header_symbols() if s.startswith("ghf_score_pair_")]
    for name in OLDER:
        with open(os.path.join(_build.INCLUDE, name)) as f:
            assert "pairwise_dot_sweep" not in f.read().lower(), name


def test_every_function_of_the_header_is_bound_and_exported():
    with open(os.path.join(_build.INCLUDE, "ghf_pairwise_dot_sweep.h")) as f:
        text = f.read()
    flat = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    declared = sorted(set(re.findall(r"\b(ghf_[a-z_0-9]+)\s*\(", flat)))
    assert declared == PAIRDOT_FUNCTIONS == _native.pairwise_dot_sweep_header_symbols()
    assert set(_native.PAIRDOT_SIGNATURES) == set(declared)
    assert not set(declared) & (set(_native.SIGNATURES) | set(_native.NEG_SIGNATURES) | set(_native.DIST_SIGNATURES)
                                | set(_native.DSWEEP_SIGNATURES) | set(_native.DLOSS_SIGNATURES) | set(_native.PAIR_SIGNATURES)
                                | set(_native.PAIRSWEEP_SIGNATURES))
    assert os.path.join(_build.INCLUDE, "ghf_pairwise_dot_sweep.h") in _build.HEADERS and "pairwise_dot_sweep.hip" in _build.SOURCES
    assert '#include "ghf_pairwise.h"' in text and "#define" not in flat.replace("#define GHF_PAIRWISE_DOT_SWEEP_H", "")
    lib = _native.load()
    for name in declared:
        fn = getattr(lib, name)                                                    # AttributeError: not exported
        assert fn.argtypes == _native.PAIRDOT_SIGNATURES[name][1] and fn.restype is _native.PAIRDOT_SIGNATURES[name][0]
    assert lib.ghf_abi_version() == 15
    for name, count in (("ghf_score_pair_fwd_workspace_bytes", 5), ("ghf_score_pair_fwd", 25), ("ghf_score_pair_bwd_workspace_bytes", 5),
                        ("ghf_score_pair_bwd", 27)):
        args = re.search(rf"\b{name}\s*\(([^)]*)\)\s*;", flat).group(1)
        assert len(args.split(",")) == len(_native.PAIRDOT_SIGNATURES[name][1]) == count, name


def test_the_header_is_plain_c(tmp_path):
    """include/ghf_pairwise_dot_sweep.h compiles as C99 with -Wall -Wextra -Werror, alone and beside the other seven."""
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    use = ("int use(void) {\n    void* fns[] = {" + ", ".join(f"(void*)(size_t)&{n}" for n in PAIRDOT_FUNCTIONS) + "};\n"
           "    return (int)(sizeof fns / sizeof fns[0]) + GHF_PAIR_HINGE + GHF_PAIR_LOGISTIC;\n}\n")
    beside = '#include "ghf_pairwise_dot_sweep.h"\n' + "".join(f'#include "{n}"\n' for n in OLDER) + '#include "ghf_pairwise_dot_sweep.h"\n'
    for name, head in (("alone.c", '#include "ghf_pairwise_dot_sweep.h"\n'), ("beside.c", beside)):
        src = tmp_path / name
        src.write_text(head + use)
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", _build.INCLUDE, "-c", str(src), "-o",
                        str(tmp_path / (name + ".o"))], check=True, capture_output=True, text=True)


def test_size_queries_and_refusals_in_the_stated_order_without_a_launch():
    """Every call below is refused by a check that stands ahead of the launch: the pointers are host buffers that nothing
    dereferences.  Each call breaks the rule under test AND every later one, so the message says which check came first."""
    lib = _native.load()
    fwd_ws, bwd_ws = _native.score_pair_fwd_workspace_bytes, _native.score_pair_bwd_workspace_bytes
    for B, N, C, d, nnz in ((5, 300, 0, 128, 0), (5, 300, 7, 128, 40), (5, 300, 300, 20, 0), (1, 1, 0, 1, 0), (1024, 1_000_000, 0, 256, 0),
                            (16384, 100_000, 16384, 128, 0)):
        for ws in (fwd_ws, bwd_ws):
            assert ws(B, N, C, d, nnz) > 0 and ws(B, N, C, d, nnz) % 256 == 0
    # nothing of size B x C: at B = C = 16,384 the ids alone would be 2 GiB and the coefficients 1 GiB
    assert fwd_ws(16384, 100_000, 16384, 128, 0) < 64 << 20 and bwd_ws(16384, 100_000, 16384, 128, 0) < 128 << 20
    for B, N, C, d, nnz in ((0, 7, 0, 128, 0), (5, 0, 0, 128, 0), (5, 7, 0, 0, 0), (5, 7, 0, 257, 0), (5, 7, 3, 128, -1), (5, 7, 8, 128, 0),
                            (5, 7, -1, 128, 0), (5, 1 << 31, 0, 128, 0), (1 << 31, 7, 0, 128, 0)):
        assert fwd_ws(B, N, C, d, nnz) == 0 and bwd_ws(B, N, C, d, nnz) == 0, (B, N, C, d, nnz)
    need_f, need_b = fwd_ws(1, 1, 0, 8, 0), bwd_ws(1, 1, 0, 8, 0)

    raw = (ctypes.c_char * 1024)()
    p = (ctypes.addressof(raw) + 255) & ~255                                               # a 256-byte aligned stand-in
    err = lambda: lib.ghf_last_error().decode()
    inf, nan = float("inf"), float("nan")

    def both(kind=1, d=8, scale=1.0, margin=1.0, normalize=1, ptrs=True, ws=p, short=0, N=1, C=0, ic=None, rows_q=1, iq=None, B=1, nnz=0,
             bias=None):
        x = p if ptrs else None
        return [("fwd", lib.ghf_score_pair_fwd(kind, x, p, iq, p, None, None, nnz, rows_q, N, B, d, scale, margin, normalize, ic, C, bias,
                                               ws, need_f - short if short >= 0 else 0, p, p, p, p, None)),
                ("bwd", lib.ghf_score_pair_bwd(kind, x, p, iq, p, None, None, nnz, rows_q, N, B, d, scale, margin, normalize, ic, C, bias,
                                               p, p, p, ws, need_b - short if short >= 0 else 0, p, p, None, None))]

    def refused(word, code=EINVAL, **kw):
        for what, rc in both(**kw):
            assert rc == code and word in err(), (what, kw, rc, err())

    # every rule after the one under test is broken too: a workspace of 0 bytes (short=-1), d beyond the limit, a q table of
    # 2^31 rows, a pairing that cannot be (C != 0 without ic), a misaligned workspace, null pointers, ...
    tail = dict(short=-1, d=300, rows_q=1 << 31, C=2, ws=p + 8, ptrs=False)
    later = dict(scale=-1.0, margin=inf, normalize=2, **tail)                              # everything after the kind
    for kind in (0, 3, -1, 7):
        refused("kind", kind=kind, **later)
    later = dict(margin=nan, normalize=2, **tail)                                          # ... after the scale
    for scale in (0.0, -1.0, inf, nan):
        for kind in (1, 2):
            refused("scale", kind=kind, scale=scale, **later)
    later = dict(normalize=-1, **tail)                                                     # ... after the margin
    for margin in (inf, -inf, nan):
        refused("margin", margin=margin, **later)
    for normalize in (2, -1):                                                              # ... after normalize
        refused("normalize", normalize=normalize, **tail)
    refused("null pointer", **tail)
    refused("filter", nnz=3, **{**tail, "ptrs": True})                                     # nnz > 0 without lists: a null pointer too
    refused("aligned", **{**tail, "ptrs": True})
    tail = dict(short=-1, d=300, rows_q=1 << 31)
    refused("bad shape", N=0, **tail)
    refused("C = 0", N=5, C=4, **tail)                                                     # no ic: C must be 0
    refused("C <= N", N=5, C=6, ic=p, **tail)                                              # more candidates than rows
    refused("C <= N", N=5, C=0, ic=p, **tail)                                              # ic with no candidate
    refused("exceeds the rows", N=5, B=2, short=-1, d=300)                                 # B > rows_q without iq
    for rows_q in (1 << 31, 1 << 40):                                                      # a row number is kept in 32 bits
        for iq in (p, None):
            refused("rows_q", rows_q=rows_q, iq=iq, short=-1, d=300)
    refused("32 bits", N=1 << 31, short=-1, d=300)
    refused("exceeds 256", code=EUNSUPPORTED, d=300, short=-1)
    for kind in (1, 2):
        for normalize in (0, 1):
            for bias in (None, p):
                refused("workspace", kind=kind, normalize=normalize, bias=bias, short=1)   # one byte short


# ---- the method ----------------------------------------------------------------------------------------------------------
def test_signature(model):
    p = inspect.signature(model.pairwise_loss_by_dot).parameters
    lead = ["embs", "query", "target"]
    keys = {"loss": "hinge", "margin": 1.0, "scale": 1.0, "normalize": True, "known": None, "filt_ptr": None, "filt_idx": None,
            "query_rows": None, "query_rel": None, "candidates": None, "candidate_bias": None, "return_active": False}
    assert list(p) == lead + list(keys)
    assert all(p[n].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD and p[n].default is inspect.Parameter.empty for n in lead)
    assert all(p[n].kind is inspect.Parameter.KEYWORD_ONLY and p[n].default == v and type(p[n].default) is type(v) for n, v in keys.items())
    doc = model.pairwise_loss_by_dot.__doc__
    assert "BPR" in doc and "max-margin" in doc
    # the per-query method keeps its form: negatives= is still required there
    with pytest.raises(TypeError):
        model.pairwise_loss(torch.randn(9, 4), torch.arange(3), torch.arange(3))


def test_validation_needs_no_device(model):
    """CPU tensors throughout: each ValueError / IndexError / TypeError below is raised before the "HIP device only"
    RuntimeError."""
    N, B = 50, 6
    embs = torch.randn(N, 16)
    q, t = torch.arange(B), torch.arange(B) + 1
    fn = lambda e, **kw: model.pairwise_loss_by_dot(e, q, t, **kw)
    with pytest.raises(ValueError, match=r"embs must be \[N, d\]"):
        fn(torch.randn(N))
    for bad in ("Hinge", "bpr", "", None, 1, ("hinge",)):
        with pytest.raises(ValueError, match="loss must be one of"):
            fn(embs, loss=bad)
    with pytest.raises(ValueError, match="candidates is empty"):
        fn(embs, candidates=torch.zeros(N, dtype=torch.bool))
    with pytest.raises(ValueError, match="mask must have length"):
        fn(embs, candidates=torch.ones(N + 1, dtype=torch.bool))
    with pytest.raises(IndexError, match="candidates"):
        fn(embs, candidates=torch.tensor([0, N]))
    with pytest.raises(TypeError, match="candidates"):
        fn(embs, candidates=torch.tensor([0.5, 1.0]))
    with pytest.raises(ValueError, match="not both"):
        fn(embs, known=(q, t), filt_ptr=torch.zeros(B + 1, dtype=torch.int64), filt_idx=torch.zeros(0, dtype=torch.int64))
    with pytest.raises(ValueError, match="query_rel"):
        fn(embs, known=(q, t, q))
    with pytest.raises(ValueError, match="query_rel"):
        fn(embs, known=(q, t), query_rel=q)
    for bad in (0.0, -2.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="scale must be finite and positive"):
            fn(embs, scale=bad)
    for bad in (float("inf"), float("-inf"), float("nan")):
        with pytest.raises(ValueError, match="margin must be finite"):
            fn(embs, margin=bad)
    for kw in (dict(normalize=1), dict(normalize=None), dict(return_active=0), dict(return_active="yes")):
        with pytest.raises(TypeError, match="must be bools"):
            fn(embs, **kw)
    with pytest.raises(ValueError, match="query_rows must be"):
        fn(embs, query_rows=torch.randn(B + 1, 16))
    with pytest.raises(TypeError, match="query_rows must be float32"):
        fn(embs, query_rows=torch.randn(B, 16, dtype=torch.float64))
    with pytest.raises((ValueError, TypeError), match="candidate_bias"):
        fn(embs, candidate_bias=torch.zeros(N + 1))
    with pytest.raises((ValueError, TypeError), match="candidate_bias"):
        fn(embs, candidate_bias=torch.zeros(N, dtype=torch.float64))
    for kw in (dict(negatives=torch.zeros(B, 3, dtype=torch.int64)), dict(distance="l1"), dict(adversarial_temperature=1.0)):
        with pytest.raises(TypeError):                                                     # no per-query sets, no distance here
            fn(embs, **kw)
    with pytest.raises(ValueError, match="6 queries and 5 targets"):
        model.pairwise_loss_by_dot(embs, q, t[:5])
    with pytest.raises(IndexError, match="target"):
        model.pairwise_loss_by_dot(embs, q, t + N)
    with pytest.raises(IndexError, match="query"):
        model.pairwise_loss_by_dot(embs, q + N, t)
    with pytest.raises(TypeError, match="query"):
        model.pairwise_loss_by_dot(embs, q.float(), t)
    for kind in S.KINDS:
        for bias in (None, torch.zeros(N)):
            with pytest.raises(RuntimeError, match="HIP device"):                          # valid: only now the device is asked for
                fn(embs, loss=kind, return_active=True, normalize=False, candidates=torch.arange(0, N, 2), candidate_bias=bias)
    # the wrappers of the C ABI refuse CPU tensors too, and check their selectors first
    for call in (lambda **kw: _native.score_pair_sweep_fwd(kw.pop("kind", 1), embs, embs, t, iq=q, **kw),
                 lambda **kw: _native.score_pair_sweep_bwd(kw.pop("kind", 1), embs, embs, t, torch.zeros(B), torch.zeros(B, dtype=torch.int32),
                                                           torch.ones(B), iq=q, **kw)):
        with pytest.raises(RuntimeError, match="HIP device"):
            call()


# ---- the restatement -----------------------------------------------------------------------------------------------------
def explicit(kind, rows, c, target, lists, P, bias, scale, margin, normalize, grad, dtype):
    """(loss, count, active, dsum, d rows, d c, d bias) through the whole [B, C] score matrix and torch autograd in `dtype`,
    written independently of the reference modules: one matmul, the hinge a where (gradient 0 at the kink)."""
    q = rows.detach().to(dtype).requires_grad_()
    cc = c.detach().to(dtype).requires_grad_()
    bb = torch.zeros(c.size(0), dtype=dtype) if bias is None else bias.detach().to(dtype)
    bb.requires_grad_()
    P = torch.as_tensor(P, dtype=torch.int64)
    z = scale * (q @ cc[P].T) + bb[P].unsqueeze(0)
    B = rows.size(0)
    listed = torch.zeros(B, len(P), dtype=torch.bool)
    for i, l in enumerate(lists):
        listed[i] = torch.from_numpy(np.isin(P.numpy(), np.asarray(l, dtype=np.int64)))
    is_t = P.unsqueeze(0) == target.unsqueeze(1)
    assert bool((is_t.sum(1) == 1).all())
    live = ~listed & ~is_t
    u = z - z[is_t].unsqueeze(1) + margin
    zero = torch.zeros_like(u)
    phi = torch.where(u > 0, u, zero) if kind == "hinge" else torch.nn.functional.softplus(u)
    dphi = (u > 0).to(dtype) if kind == "hinge" else torch.sigmoid(u)
    n = live.sum(1)
    total = torch.where(live, phi, zero).sum(1)
    loss = torch.where(n > 0, total / n.clamp(min=1).to(dtype), torch.zeros_like(total)) if normalize else total
    (loss * grad.to(dtype)).sum().backward()
    return loss.detach(), n, ((u > 0) & live).sum(1), torch.where(live, dphi, zero).sum(1).detach(), q.grad, cc.grad, bb.grad


@pytest.mark.parametrize("biased", (False, True))
@pytest.mark.parametrize("kind", S.KINDS)
@pytest.mark.parametrize("normalize", (True, False))
def test_restatement_against_the_explicit_formulation(biased, kind, normalize):
    """Lists, a subset, a target shared by several queries, a listed target and a query whose every negative is listed."""
    i = S.make_problem(8, 40, 15, subset=True, seed=5)
    embs, t, rows, lists, grad = i["embs"], i["t"], i["rows"], list(i["lists"]), i["grad"]
    bias = i["bias"] if biased else None
    for cand in (i["cand"], None):
        P = S.candidate_set(embs.size(0), t, cand)
        ls = list(lists)
        ls[4] = P.copy()                                                            # nothing but the target is left
        want = S.loss(kind, rows, embs, t, ls, cand, bias, scale=0.3, margin=0.7, normalize=normalize, grad=grad)
        loss, n, active, dsum, dq, dc, db = explicit(kind, rows, embs, t, ls, P, bias, 0.3, 0.7, normalize, grad, torch.float64)
        assert torch.allclose(want["loss"], loss, rtol=1e-12, atol=1e-12)
        assert torch.equal(want["count"], n) and torch.equal(want["active"], active)
        assert torch.allclose(want["dsum"], dsum, rtol=1e-12, atol=1e-12)
        assert torch.allclose(want["dq"], dq, rtol=1e-11, atol=1e-12) and torch.allclose(want["dc"], dc, rtol=1e-11, atol=1e-12)
        if biased:
            assert torch.allclose(want["db"], db, rtol=1e-11, atol=1e-12)
            assert torch.allclose(db.sum(), torch.zeros((), dtype=torch.float64), atol=1e-12)      # sum_j G_ij = -G_it, per query
        assert float(loss[4]) == 0.0 and int(n[4]) == 0 and not dq[4].any()
        assert torch.allclose(want["coef"][:, -1], -want["coef"][:, :-1].sum(1))     # G_it = -sum_j G_ij
        w = grad.double() * 0.3 * (torch.where(n > 0, 1.0 / n.clamp(min=1).double(), torch.zeros(len(n), dtype=torch.float64)) if normalize else 1.0)
        assert torch.allclose(want["coef"][:, -1], -w * dsum, rtol=1e-12, atol=1e-15)  # = -w_i dsum_i: what the backward uses
        outside = np.setdiff1d(np.arange(embs.size(0)), P)
        assert not want["dc"][outside].any() and not want["db"][outside].any()


# ---- the parity problems -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", S.SHAPES, ids=S.SHAPE_IDS)
def test_parity_problems_respect_the_kink_condition_and_fp32_passes_the_checks(shape):
    """Conditions on the INPUTS of tests/test_pairwise_dot_sweep_gpu.py's parity test, checked where there is no device.  On its
    very problems, in both forms it runs (all nodes with the queries by id, the subset with given rows), with and without the
    bias: at most B / 8 queries are near (a pair of J_i with float64 |u| < 1e-4 (1 + |z_it| + |margin|)); and the same formulas
    in fp32 pass loss_check / grad_check at their defaults against the float64 restatement, with the kink rule — near queries
    carry grad_loss = 0 under the hinge and their `active` is held to +- their in-band pairs, the logistic kind excuses
    nothing.  A seed that fails this is changed, never a tolerance."""
    d, C, B = shape
    scale = S.scale_for(d)
    for subset, by_id in S.FORMS:
        i = S.problem(shape, subset)
        P = S.candidate_set(i["embs"].size(0), i["t"], i["cand"])
        assert len(P) == C
        rows = i["embs"][i["q"]] if by_id else i["rows"]
        for kind, normalize, biased in S.combos(shape):
            bias = i["bias"] if biased else None
            out, grad, nr, inb = S.reference(shape, subset, kind, normalize, by_id, biased)
            what = f"{kind} {'subset' if subset else 'all'} {'by id' if by_id else 'rows'} bias={biased} normalize={normalize}"
            near_any, _ = S.near(out, S.MARGIN)
            assert torch.equal(near_any, nr) and int(nr.sum()) <= B // 8, f"{what}: {int(nr.sum())} of {B} queries near the kink"
            assert kind == "logistic" or bool((grad[nr] == 0).all())
            loss, n, active, dsum, dq, dc, db = explicit(kind, rows, i["embs"], i["t"], i["lists"], P, bias, scale, S.MARGIN, normalize,
                                                         grad, torch.float32)
            loss_check(f"{what} loss", loss, out["loss"])
            assert torch.equal(n, out["count"]), what
            S.active_check(what, active, out, nr, inb)
            grad_check(f"{what} rows", dq.numpy(), out["dq"].numpy())
            grad_check(f"{what} embs", dc.numpy(), out["dc"].numpy())
            if biased:
                grad_check(f"{what} bias", db.numpy(), out["db"].numpy())
