"""The two losses under a distance against every node or a shared candidate set (HyperGNN.softmax_loss_by_distance /
negative_sampling_loss_by_distance; include/ghf_distance_loss.h), the part that needs no GPU: the fifth header against
_native.DLOSS_SIGNATURES and the built library (the four older headers as they were), the size queries and every refusal that
stands ahead of a launch, the methods' signatures and their validation from CPU tensors, the float64 restatement
(tests/_distance_loss_ref.py) against an explicit [B, C, d] torch-autograd formulation, and the condition the GPU parity test
puts on its inputs: on the very problems it uses, the same formulas in fp32 on the CPU pass loss_check / grad_check."""

import ctypes
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import _distance_loss_ref as L
import _distance_ref as R
from graph_hypernetwork_forge_amd import HyperGNN, _build, _native
from test_distance_gpu import rows_cpu, scale_for
from test_distance_host import DIST_FUNCTIONS
from test_distance_sweep_host import DSWEEP_FUNCTIONS
from test_softmax_gpu import grad_check, loss_check

EINVAL, EUNSUPPORTED = -1, -3
DLOSS_FUNCTIONS = ["ghf_dist_loss_bwd", "ghf_dist_loss_bwd_workspace_bytes", "ghf_dist_loss_fwd_workspace_bytes",
                   "ghf_dist_loss_negsamp_fwd", "ghf_dist_loss_softmax_fwd"]
MODES = (("softmax", _native.NEG_SOFTMAX), ("negsamp", _native.NEG_NEGSAMP))
MARGIN, ALPHA = 1.0, 0.5

# (d, C, B) of the GPU parity test, from the kernels' geometry: the scalar path (d = 1, 3, 6), one ragged 4-group and 16-column
# step, both column halves of the backward (d = 130, 256); candidate tiles of 256 and their edges, three forward slabs with a
# ragged last one (C = 513: dloss_geom gives cdiv(513, 256) = 3 tiles, 3 slabs of one tile, the last holding one candidate; the
# backward's dloss_bwd_geom gives the same 3 slabs of 256 streamed rows for the dq pass), eleven slabs (C = 2600); owner tiles
# of 64 and their edges on both sides (B and C of 63, 64, 65); B past one and two query tiles; and the dc pass, which streams
# the queries, split the same way (B = 513 over C = 70: dloss_bwd_geom gives 2 owner tiles x 3 slabs of 256 queries, the last
# holding one).
SHAPES = [(1, 1, 1), (3, 2, 5), (4, 255, 64), (6, 256, 65), (20, 257, 129), (64, 1023, 5), (130, 1025, 64), (256, 2600, 5),
          (20, 2600, 129), (4, 513, 5), (6, 63, 65), (6, 64, 63), (6, 65, 64), (6, 70, 513)]
CASES = [(m, (2 if m == "complex" and d <= 3 else d, C, B)) for m in R.METRICS for d, C, B in SHAPES]
CASE_IDS = ["%s-d%d-C%d-B%d" % ((m,) + s) for m, s in CASES]


@pytest.fixture(scope="module")
def model():
    return HyperGNN(text_dim=32, node_feat_dim=16, hidden_dim=16)


def parity_problem(d, C, B, subset, seed=None):
    """CPU tensors of one parity case.  `subset`: N = C + 41 nodes and a candidate set of exactly C ids in shuffled order that
    holds every target (so the set the kernels see has C entries); else all N = C nodes.  Queries repeat, several share a
    target, every third node has known partners (so known= and the CSR lists agree), the query rows are translated."""
    seed = 11 * d + C + B if seed is None else seed
    rng = np.random.default_rng(seed)
    N = C + 41 if subset else C
    embs = rows_cpu(N, d, seed)
    cand = rng.permutation(N)[:C].astype(np.int64)
    pool = cand if subset else np.arange(N)
    query, target = rng.integers(0, N, B), pool[rng.integers(0, len(pool), B)]
    if B > 12:
        query[B // 2:B // 2 + 5] = query[:5]
        target[6:12] = target[0]
    node_lists = {}
    for i, v in enumerate(query):
        if v not in node_lists:
            node_lists[v] = np.unique(rng.integers(0, N, 4)) if i % 3 else np.zeros(0, dtype=np.int64)
    if B > 1:
        node_lists[query[1]] = np.unique(np.append(node_lists[query[1]], target[1]))          # a list that holds its target
    lists = [node_lists[v] for v in query]
    src = np.concatenate([np.full(len(l), v) for v, l in node_lists.items()] + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
    dst = np.concatenate(list(node_lists.values()) + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
    v = torch.from_numpy(rng.standard_normal((B, d)).astype(np.float32))
    q = torch.from_numpy(query.astype(np.int64))
    return dict(embs=embs, q=q, t=torch.from_numpy(target.astype(np.int64)), lists=lists,
                known=(torch.from_numpy(src), torch.from_numpy(dst)), cand=torch.from_numpy(cand) if subset else None,
                rows=embs[q] + 0.5 * v, grad=torch.from_numpy((0.5 + rng.random(B)).astype(np.float32)))


def aux_check(what, got, want):
    """lse / lw: -inf (a query without negatives) exactly where the restatement has it, loss_check on the finite entries."""
    got, want = got.detach().cpu(), want.detach().cpu()
    assert torch.equal(torch.isneginf(got), torch.isneginf(want)), what
    fin = torch.isfinite(want)
    assert bool(torch.isfinite(got[fin]).all()), what
    if bool(fin.any()):
        loss_check(what, got[fin], want[fin])


# ---- the headers and the library -----------------------------------------------------------------------------------------
def test_the_four_older_headers_are_as_they_were():
    with open(os.path.join(_build.INCLUDE, "ghf.h")) as f:
        assert re.search(r"#define GHF_ABI_VERSION 15\b", f.read()) and _native.ABI_VERSION == 15
    assert len(_native.header_symbols()) == 113 and set(_native.header_symbols()) == set(_native.SIGNATURES)
    assert _native.negatives_header_symbols() == ["ghf_neg_bwd", "ghf_neg_negsamp_fwd", "ghf_neg_rank", "ghf_neg_softmax_fwd",
                                                  "ghf_neg_workspace_bytes"]
    assert _native.distance_header_symbols() == DIST_FUNCTIONS
    assert _native.distance_sweep_header_symbols() == DSWEEP_FUNCTIONS
    older = (_native.header_symbols() + _native.negatives_header_symbols() + _native.distance_header_symbols()
             + _native.distance_sweep_header_symbols())
    assert not [s for s in older if s.startswith("ghf_dist_loss_")]


def test_every_function_of_the_header_is_bound_and_exported():
    assert _native.distance_loss_header_symbols() == DLOSS_FUNCTIONS and set(_native.DLOSS_SIGNATURES) == set(DLOSS_FUNCTIONS)
    assert not set(DLOSS_FUNCTIONS) & (set(_native.SIGNATURES) | set(_native.NEG_SIGNATURES) | set(_native.DIST_SIGNATURES)
                                       | set(_native.DSWEEP_SIGNATURES))
    assert os.path.join(_build.INCLUDE, "ghf_distance_loss.h") in _build.HEADERS and "distance_loss.hip" in _build.SOURCES
    assert os.path.join(_build.CSRC, "distance_sweep_dev.h") in _build.HEADERS
    lib = _native.load()
    for name in DLOSS_FUNCTIONS:
        fn = getattr(lib, name)                                                    # AttributeError: not exported
        assert fn.argtypes == _native.DLOSS_SIGNATURES[name][1] and fn.restype is _native.DLOSS_SIGNATURES[name][0]
    assert lib.ghf_abi_version() == 15
    with open(os.path.join(_build.INCLUDE, "ghf_distance_loss.h")) as f:
        flat = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    for name in DLOSS_FUNCTIONS:                                                   # the argument counts are the table's
        args = re.search(rf"\b{name}\s*\(([^)]*)\)\s*;", flat).group(1)
        assert len(args.split(",")) == len(_native.DLOSS_SIGNATURES[name][1]), name


def test_the_header_is_plain_c(tmp_path):
    """include/ghf_distance_loss.h compiles as C99 with -Wall -Wextra -Werror, alone and beside the other four."""
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    use = ("int use(void) {\n    void* fns[] = {" + ", ".join(f"(void*)(size_t)&{n}" for n in DLOSS_FUNCTIONS) + "};\n"
           "    return (int)(sizeof fns / sizeof fns[0]) + GHF_DIST_L1 + GHF_DIST_SOFTMAX + GHF_DIST_NEGSAMP;\n}\n")
    for name, head in (("alone.c", '#include "ghf_distance_loss.h"\n'),
                       ("beside.c", '#include "ghf_distance_loss.h"\n#include "ghf.h"\n#include "ghf_negatives.h"\n'
                                    '#include "ghf_distance.h"\n#include "ghf_distance_sweep.h"\n#include "ghf_distance_loss.h"\n')):
        src = tmp_path / name
        src.write_text(head + use)
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", _build.INCLUDE, "-c", str(src), "-o",
                        str(tmp_path / (name + ".o"))], check=True, capture_output=True, text=True)


def test_size_queries_and_argument_checks_without_a_launch():
    """Every call below is refused by a check that stands ahead of the launch: the pointers are host buffers that nothing
    dereferences."""
    lib = _native.load()
    fwd_ws, bwd_ws = _native.dist_loss_fwd_workspace_bytes, _native.dist_loss_bwd_workspace_bytes
    for B, C, d, nnz in ((5, 300, 128, 0), (5, 300, 128, 40), (1, 1, 1, 0), (1024, 1_000_000, 256, 0), (16384, 16384, 128, 0)):
        for ws in (fwd_ws, bwd_ws):
            assert ws(B, C, d, nnz) > 0 and ws(B, C, d, nnz) % 256 == 0
    # nothing of size B x C: at B = C = 16,384, d = 128 the B x C distances alone would be 1 GiB
    assert fwd_ws(16384, 16384, 128, 0) < 32 << 20 and bwd_ws(16384, 16384, 128, 0) < 128 << 20
    for B, C, d, nnz in ((0, 7, 128, 0), (5, 0, 128, 0), (5, 7, 0, 0), (5, 7, 257, 0), (5, 7, 128, -1), (5, 1 << 31, 128, 0),
                         (1 << 31, 7, 128, 0)):
        assert fwd_ws(B, C, d, nnz) == 0 and bwd_ws(B, C, d, nnz) == 0, (B, C, d, nnz)
    need_f, need_b = fwd_ws(1, 1, 8, 0), bwd_ws(1, 1, 8, 0)

    raw = (ctypes.c_char * 1024)()
    p = (ctypes.addressof(raw) + 255) & ~255                                               # a 256-byte aligned stand-in
    err = lambda: lib.ghf_last_error().decode()
    SM, NS = _native.NEG_SOFTMAX, _native.NEG_NEGSAMP

    def calls(metric, d, short=0, N=1, C=1, ic=None, ws=None, scale=1.0, margin=0.0, alpha=0.0, mode=SM, rows_q=1, iq=None, B=1,
              nnz=0):
        ws = p if ws is None else ws
        return [("softmax", lib.ghf_dist_loss_softmax_fwd(metric, p, p, iq, p, None, None, nnz, rows_q, N, B, d, scale, ic, C, ws,
                                                          need_f - short, p, p, None)),
                ("negsamp", lib.ghf_dist_loss_negsamp_fwd(metric, p, p, iq, p, None, None, nnz, rows_q, N, B, d, scale, margin, alpha,
                                                          ic, C, ws, need_f - short, p, p, None)),
                ("bwd", lib.ghf_dist_loss_bwd(metric, mode, p, p, iq, p, None, None, nnz, rows_q, N, B, d, scale, margin, alpha, ic, C,
                                              p, p, ws, need_b - short, p, p, None))]

    for metric in (0, 4, -1):                                                              # an unknown metric, before anything else
        for what, rc in calls(metric, 8) + calls(metric, 260, short=1) + calls(metric, 8, scale=float("nan"), mode=7):
            assert rc == EINVAL and "metric" in err(), (what, metric, rc, err())
    for what, rc in calls(_native.DIST_COMPLEX, 7) + calls(_native.DIST_COMPLEX, 259, short=1):
        assert rc == EINVAL and "even d" in err(), (what, rc, err())                      # odd d under COMPLEX
    for metric in (_native.DIST_L1, _native.DIST_L2, _native.DIST_COMPLEX):
        for what, rc in calls(metric, 8, short=1):                                         # a workspace one byte short
            assert rc == EINVAL and "workspace" in err(), (what, metric, rc, err())
        for what, rc in calls(metric, 260):                                                # d beyond the limit
            assert rc == EUNSUPPORTED, (what, metric, rc, err())
        for what, rc in calls(metric, 8, N=5, C=4):                                        # no ic: C must be N
            assert rc == EINVAL and "C == N" in err(), (what, metric, rc, err())
        for what, rc in calls(metric, 8, N=5, C=6, ic=p):                                  # more candidates than rows
            assert rc == EINVAL, (what, metric, rc, err())
        for what, rc in calls(metric, 8, ws=p + 16):                                       # a misaligned workspace
            assert rc == EINVAL and "aligned" in err(), (what, metric, rc, err())
        for bad in (0.0, -1.0, float("inf"), float("nan")):                                # scale finite and positive
            for what, rc in calls(metric, 8, scale=bad):
                assert rc == EINVAL and "scale" in err(), (what, bad, rc, err())
        for bad in (float("inf"), float("-inf"), float("nan")):                            # margin finite
            for what, rc in calls(metric, 8, margin=bad)[1:]:
                assert rc == EINVAL and "margin" in err(), (what, bad, rc, err())
        for bad in (-0.5, float("inf"), float("nan")):                                     # temperature finite and >= 0
            for what, rc in calls(metric, 8, alpha=bad)[1:]:
                assert rc == EINVAL and "adv_temperature" in err(), (what, bad, rc, err())
        for mode in (-1, 2, 4):                                                            # the backward's mode
            what, rc = calls(metric, 8, mode=mode)[2]
            assert rc == EINVAL and "mode" in err(), (what, mode, rc, err())
        for what, rc in calls(metric, 8, nnz=3):                                           # nnz > 0 without lists
            assert rc == EINVAL and "filter" in err(), (what, rc, err())
        for what, rc in calls(metric, 8, N=5, C=5, B=2):                                   # B > rows_q without iq
            assert rc == EINVAL, (what, rc, err())
        # a q table of 2^31 rows or more: the kernels keep a row number in 32 bits
        for rows_q in (1 << 31, 1 << 40):
            for iq in (p, None):
                for what, rc in calls(metric, 8, rows_q=rows_q, iq=iq):
                    assert rc == EINVAL and "rows_q" in err() and "32 bits" in err(), (what, rc, err())
    assert lib.ghf_dist_loss_softmax_fwd(1, None, None, None, None, None, None, 0, 1, 1, 1, 8, 1.0, None, 1, None, 0, None, None,
                                         None) == EINVAL and "null pointer" in err()
    assert lib.ghf_dist_loss_negsamp_fwd(1, None, None, None, None, None, None, 0, 1, 1, 1, 8, 1.0, 0.0, 0.0, None, 1, None, 0, None,
                                         None, None) == EINVAL and "null pointer" in err()
    assert lib.ghf_dist_loss_bwd(1, 0, None, None, None, None, None, None, 0, 1, 1, 1, 8, 1.0, 0.0, 0.0, None, 1, None, None, None, 0,
                                 None, None, None) == EINVAL and "null pointer" in err()


# ---- the methods ---------------------------------------------------------------------------------------------------------
def test_signatures(model):
    tail = ["known", "filt_ptr", "filt_idx", "query_rows", "query_rel", "candidates"]
    lead = ["embs", "query", "target", "distance"]
    for fn, floats in ((model.softmax_loss_by_distance, {"scale": 1.0}),
                       (model.negative_sampling_loss_by_distance, {"scale": 1.0, "margin": 0.0, "adversarial_temperature": 0.0})):
        p = inspect.signature(fn).parameters
        assert list(p) == lead + list(floats) + tail, fn.__name__
        assert all(p[n].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD and p[n].default is inspect.Parameter.empty for n in lead)
        assert all(p[n].kind is inspect.Parameter.KEYWORD_ONLY and p[n].default == v for n, v in floats.items())
        assert all(p[n].kind is inspect.Parameter.KEYWORD_ONLY and p[n].default is None for n in tail)
    # the older methods keep their forms: distance= without negatives= is still refused there, and says where to go
    for fn in (model.softmax_loss, model.negative_sampling_loss):
        with pytest.raises(ValueError, match="dot product"):
            fn(torch.randn(9, 4), torch.arange(3), torch.arange(3), distance="l1")


def test_validation_needs_no_device(model):
    """CPU tensors throughout: each ValueError / IndexError / TypeError below is raised before the "HIP device only"
    RuntimeError."""
    N, B = 50, 6
    embs, odd = torch.randn(N, 16), torch.randn(N, 15)
    q, t = torch.arange(B), torch.arange(B) + 1
    sm = lambda e, *a, **kw: model.softmax_loss_by_distance(e, q, t, *a, **kw)
    ns = lambda e, *a, **kw: model.negative_sampling_loss_by_distance(e, q, t, *a, **kw)
    for fn in (sm, ns):
        for bad in ("L1", "cosine", "", None, 1, ("l1",)):
            with pytest.raises(ValueError, match="distance must be"):
                fn(embs, bad)
        with pytest.raises(ValueError, match="even d"):
            fn(odd, "complex")
        with pytest.raises(ValueError, match=r"embs must be \[N, d\]"):
            fn(torch.randn(N), "l1")
        with pytest.raises(ValueError, match="candidates is empty"):
            fn(embs, "l1", candidates=torch.zeros(N, dtype=torch.bool))
        with pytest.raises(ValueError, match="mask must have length"):
            fn(embs, "l1", candidates=torch.ones(N + 1, dtype=torch.bool))
        with pytest.raises(IndexError, match="candidates"):
            fn(embs, "l1", candidates=torch.tensor([0, N]))
        with pytest.raises(TypeError, match="candidates"):
            fn(embs, "l1", candidates=torch.tensor([0.5, 1.0]))
        with pytest.raises(ValueError, match="not both"):
            fn(embs, "l1", known=(q, t), filt_ptr=torch.zeros(B + 1, dtype=torch.int64), filt_idx=torch.zeros(0, dtype=torch.int64))
        with pytest.raises(ValueError, match="query_rel"):
            fn(embs, "l1", known=(q, t, q))
        with pytest.raises(ValueError, match="query_rel"):
            fn(embs, "l1", known=(q, t), query_rel=q)
        for bad in (0.0, -2.0, float("inf"), float("nan")):
            with pytest.raises(ValueError, match="scale must be finite and positive"):
                fn(embs, "l1", scale=bad)
        with pytest.raises(ValueError, match="query_rows must be"):
            fn(embs, "l1", query_rows=torch.randn(B + 1, 16))
        with pytest.raises(TypeError, match="query_rows must be float32"):
            fn(embs, "l1", query_rows=torch.randn(B, 16, dtype=torch.float64))
        for metric, e in (("l1", embs), ("l2", embs), ("complex", embs), ("l1", odd), ("l2", odd)):
            with pytest.raises(RuntimeError, match="HIP device"):                          # valid: only now the device is asked for
                fn(e, metric)
        for kw in (dict(candidate_bias=torch.zeros(N)), dict(negatives=torch.zeros(B, 3, dtype=torch.int64)), dict(distance="l1")):
            with pytest.raises(TypeError):                                                 # no bias, no per-query sets here
                fn(embs, "l1", **kw)
    for bad in (float("inf"), float("-inf"), float("nan")):
        with pytest.raises(ValueError, match="margin must be finite"):
            ns(embs, "l1", margin=bad)
    for bad in (-0.1, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="adversarial_temperature must be finite"):
            ns(embs, "l1", adversarial_temperature=bad)
    with pytest.raises(TypeError):
        sm(embs, "l1", margin=1.0)
    with pytest.raises(ValueError, match="6 queries and 5 targets"):
        model.softmax_loss_by_distance(embs, q, t[:5], "l1")
    with pytest.raises(IndexError, match="target"):
        model.negative_sampling_loss_by_distance(embs, q, t + N, "l1")
    with pytest.raises(IndexError, match="query"):
        model.softmax_loss_by_distance(embs, q + N, t, "l1")
    with pytest.raises(TypeError, match="query"):
        model.softmax_loss_by_distance(embs, q.float(), t, "l1")


# ---- the restatement -----------------------------------------------------------------------------------------------------
def explicit(mode, metric, rows, c, target, lists, P, scale, margin, alpha, grad, dtype):
    """(loss, aux, d rows, d c) through the whole [B, C, d] difference tensor and torch autograd in `dtype`, written
    independently of _distance_ref: a root is taken of a positive argument only (its gradient at 0 is the contract's 0)."""
    q = rows.detach().to(dtype).requires_grad_()
    cc = c.detach().to(dtype).requires_grad_()
    P = torch.as_tensor(P, dtype=torch.int64)
    delta = q.unsqueeze(1) - cc[P].unsqueeze(0)

    def root(ss):
        pos = ss > 0
        return torch.where(pos, torch.sqrt(torch.where(pos, ss, torch.ones_like(ss))), torch.zeros_like(ss))
    if metric == "l1":
        D = delta.abs().sum(-1)
    elif metric == "l2":
        D = root((delta * delta).sum(-1))
    else:
        D = root((delta * delta).reshape(*delta.shape[:-1], -1, 2).sum(-1)).sum(-1)
    z = -scale * D
    B = rows.size(0)
    listed = torch.zeros(B, len(P), dtype=torch.bool)
    for i, l in enumerate(lists):
        listed[i] = torch.from_numpy(np.isin(P.numpy(), np.asarray(l, dtype=np.int64)))
    is_t = P.unsqueeze(0) == target.unsqueeze(1)
    assert bool((is_t.sum(1) == 1).all())
    zt = z[is_t]
    if mode == "softmax":
        aux = torch.logsumexp(z.masked_fill(listed & ~is_t, -np.inf), 1)
        loss = aux - zt
    else:
        live = ~listed & ~is_t
        a = (alpha * z).masked_fill(~live, -np.inf)
        aux = torch.logsumexp(a, 1)
        some = live.any(1, keepdim=True)
        w = torch.where(live & some, torch.softmax(torch.where(some, a, torch.zeros_like(a)), 1), torch.zeros_like(a)).detach()
        loss = torch.nn.functional.softplus(-(zt + margin)) + (w * torch.nn.functional.softplus(z + margin)).sum(1)
    (loss * grad.to(dtype)).sum().backward()
    return loss.detach(), aux.detach(), q.grad, cc.grad


@pytest.mark.parametrize("metric", R.METRICS)
@pytest.mark.parametrize("mode", ["softmax", "negsamp"])
def test_restatement_against_the_explicit_formulation(metric, mode):
    """Lists, a subset, a target shared by several queries, a listed target, a candidate equal to a query's row (distance 0)
    and a query whose every negative is listed."""
    i = parity_problem(8, 40, 15, subset=True, seed=5)
    embs, t, rows, lists, grad = i["embs"], i["t"], i["rows"].clone(), list(i["lists"]), i["grad"]
    rows[3] = embs[i["cand"][0]]                                                    # distance 0 to a candidate
    for cand in (i["cand"], None):
        P = L.candidate_set(embs.size(0), t, cand)
        ls = list(lists)
        ls[4] = P.copy()                                                            # nothing but the target is left
        want = L.loss(mode, metric, rows, embs, t, ls, cand, scale=0.3, margin=MARGIN, alpha=ALPHA, grad=grad)
        loss, aux, dq, dc = explicit(mode, metric, rows, embs, t, ls, P, 0.3, MARGIN, ALPHA, grad, torch.float64)
        assert torch.allclose(want["loss"], loss, rtol=1e-12, atol=1e-12)
        assert torch.allclose(want["aux"], aux, rtol=1e-12, atol=1e-12) and torch.equal(torch.isinf(want["aux"]), torch.isinf(aux))
        assert torch.allclose(want["dq"], dq, rtol=1e-11, atol=1e-12) and torch.allclose(want["dc"], dc, rtol=1e-11, atol=1e-12)
        assert (mode == "softmax" and float(loss[4]) == 0.0) or (mode == "negsamp" and bool(torch.isneginf(aux[4])))
        outside = np.setdiff1d(np.arange(embs.size(0)), P)
        assert not want["dc"][outside].any()


@pytest.mark.parametrize("metric,shape", CASES, ids=CASE_IDS)
def test_fp32_on_the_cpu_passes_the_parity_checks(metric, shape):
    """A condition on the INPUTS of tests/test_distance_loss_gpu.py's parity test, checked where there is no device: on its
    very problems the same formulas in fp32 pass loss_check / grad_check at their defaults against the float64 restatement.
    A seed that fails this is changed, never the tolerance."""
    d, C, B = shape
    scale = scale_for(metric, d)
    for subset in (False, True):
        i = parity_problem(d, C, B, subset)
        P = L.candidate_set(i["embs"].size(0), i["t"], i["cand"])
        assert len(P) == C
        for mode, _ in MODES:
            want = L.loss(mode, metric, i["rows"], i["embs"], i["t"], i["lists"], i["cand"], scale=scale, margin=MARGIN, alpha=ALPHA,
                          grad=i["grad"])
            loss, aux, dq, dc = explicit(mode, metric, i["rows"], i["embs"], i["t"], i["lists"], P, scale, MARGIN, ALPHA, i["grad"],
                                         torch.float32)
            what = f"{metric} {mode} {'subset' if subset else 'all'}"
            loss_check(f"{what} loss", loss, want["loss"])
            aux_check(f"{what} aux", aux, want["aux"])
            grad_check(f"{what} rows", dq.numpy(), want["dq"].numpy())
            grad_check(f"{what} embs", dc.numpy(), want["dc"].numpy())
