"""Distance scores against every node (HyperGNN.rank_by_distance / topk_by_distance; include/ghf_distance_sweep.h), the part
that needs no GPU: the fourth header against _native.DSWEEP_SIGNATURES and the built library (the three older headers as they
were), the size queries and every refusal that stands ahead of a launch, the methods' signatures and their validation from
CPU tensors, the float64 restatement (tests/_distance_sweep_ref.py) against an explicit torch formulation, and the cap of what
the GPU tests may excuse: the rank bracket under eps = (d + 8) 2^-24 D."""

import ctypes
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import _distance_ref as R
import _distance_sweep_ref as S
from graph_hypernetwork_forge_amd import HyperGNN, _build, _native
from test_distance_gpu import rows_cpu
from test_distance_host import DIST_FUNCTIONS
from test_rank_gpu import rank_bracket

EINVAL, EUNSUPPORTED = -1, -3
DSWEEP_FUNCTIONS = ["ghf_dist_sweep_rank", "ghf_dist_sweep_rank_workspace_bytes", "ghf_dist_sweep_topk",
                    "ghf_dist_sweep_topk_workspace_bytes"]
DIMS = (1, 2, 3, 4, 6, 64, 130, 256)


@pytest.fixture(scope="module")
def model():
    return HyperGNN(text_dim=32, node_feat_dim=16, hidden_dim=16)


# ---- the headers and the library -----------------------------------------------------------------------------------------
def test_the_three_older_headers_are_as_they_were():
    with open(os.path.join(_build.INCLUDE, "ghf.h")) as f:
        assert re.search(r"#define GHF_ABI_VERSION 15\b", f.read()) and _native.ABI_VERSION == 15
    assert len(_native.header_symbols()) == 113 and set(_native.header_symbols()) == set(_native.SIGNATURES)
    assert _native.negatives_header_symbols() == ["ghf_neg_bwd", "ghf_neg_negsamp_fwd", "ghf_neg_rank", "ghf_neg_softmax_fwd",
                                                  "ghf_neg_workspace_bytes"]
    assert _native.distance_header_symbols() == DIST_FUNCTIONS
    older = _native.header_symbols() + _native.negatives_header_symbols() + _native.distance_header_symbols()
    assert not [s for s in older if s.startswith("ghf_dist_sweep_")]


def test_every_function_of_the_header_is_bound_and_exported():
    assert _native.distance_sweep_header_symbols() == DSWEEP_FUNCTIONS and set(_native.DSWEEP_SIGNATURES) == set(DSWEEP_FUNCTIONS)
    assert not set(DSWEEP_FUNCTIONS) & (set(_native.SIGNATURES) | set(_native.NEG_SIGNATURES) | set(_native.DIST_SIGNATURES))
    assert os.path.join(_build.INCLUDE, "ghf_distance_sweep.h") in _build.HEADERS and "distance_sweep.hip" in _build.SOURCES
    lib = _native.load()
    for name in DSWEEP_FUNCTIONS:
        fn = getattr(lib, name)                                                    # AttributeError: not exported
        assert fn.argtypes == _native.DSWEEP_SIGNATURES[name][1] and fn.restype is _native.DSWEEP_SIGNATURES[name][0]
    assert lib.ghf_abi_version() == 15
    with open(os.path.join(_build.INCLUDE, "ghf_distance_sweep.h")) as f:
        flat = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    for name in DSWEEP_FUNCTIONS:                                                  # the argument counts are the table's
        args = re.search(rf"\b{name}\s*\(([^)]*)\)\s*;", flat).group(1)
        assert len(args.split(",")) == len(_native.DSWEEP_SIGNATURES[name][1]), name


def test_the_header_is_plain_c(tmp_path):
    """include/ghf_distance_sweep.h compiles as C99 with -Wall -Wextra -Werror, alone and beside the other three."""
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "use.c"
    src.write_text('#include "ghf_distance_sweep.h"\n#include "ghf.h"\n#include "ghf_negatives.h"\n#include "ghf_distance.h"\n'
                   '#include "ghf_distance_sweep.h"\n'
                   "int use(void) {\n    void* fns[] = {" + ", ".join(f"(void*)(size_t)&{n}" for n in DSWEEP_FUNCTIONS) + "};\n"
                   "    return (int)(sizeof fns / sizeof fns[0]) + GHF_DIST_L1 + GHF_DIST_L2 + GHF_DIST_COMPLEX;\n}\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", _build.INCLUDE, "-c", str(src), "-o", str(tmp_path / "use.o")],
                   check=True, capture_output=True, text=True)


def test_size_queries_and_argument_checks_without_a_launch():
    """Every call below is refused by a check that stands ahead of the launch: the pointers are host buffers that nothing
    dereferences."""
    lib = _native.load()
    rank_ws, topk_ws = _native.dist_sweep_rank_workspace_bytes, _native.dist_sweep_topk_workspace_bytes
    for B, C, d, nnz in ((5, 300, 128, 0), (5, 300, 128, 40), (1, 1, 1, 0), (1024, 1_000_000, 256, 0)):
        assert rank_ws(B, C, d, nnz) > 0 and rank_ws(B, C, d, nnz) % 256 == 0
        for k in (1, 128):
            assert topk_ws(B, C, d, k, nnz) > 0 and topk_ws(B, C, d, k, nnz) % 256 == 0
    for B, C, d, nnz in ((0, 7, 128, 0), (5, 0, 128, 0), (5, 7, 0, 0), (5, 7, 257, 0), (5, 7, 128, -1), (5, 1 << 31, 128, 0),
                         (1 << 31, 7, 128, 0)):
        assert rank_ws(B, C, d, nnz) == 0 and topk_ws(B, C, d, 10, nnz) == 0, (B, C, d, nnz)
    assert topk_ws(5, 7, 128, 0, 0) == 0 and topk_ws(5, 7, 128, 129, 0) == 0
    need_r, need_t = rank_ws(1, 1, 8, 0), topk_ws(1, 1, 8, 1, 0)

    raw = (ctypes.c_char * 1024)()
    p = (ctypes.addressof(raw) + 255) & ~255                                               # a 256-byte aligned stand-in
    err = lambda: lib.ghf_last_error().decode()

    def calls(metric, d, short=0, N=1, C=1, ic=None, k=1, ws=None):
        ws = p if ws is None else ws
        return [("rank", lib.ghf_dist_sweep_rank(metric, p, p, None, p, None, None, 0, 1, N, 1, d, ic, C, ws, need_r - short, p, p, None)),
                ("topk", lib.ghf_dist_sweep_topk(metric, p, p, None, None, None, 0, 1, N, 1, d, k, ic, C, ws, need_t - short, p, p, None))]

    for metric in (0, 4, -1):                                                              # an unknown metric, before anything else
        for what, rc in calls(metric, 8) + calls(metric, 260, short=1):
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
    for k in (0, 129):
        assert calls(1, 8, k=k)[1][1] == EINVAL and "k =" in err()
    assert lib.ghf_dist_sweep_rank(1, None, None, None, None, None, None, 0, 1, 1, 1, 8, None, 1, None, 0, None, None, None) == EINVAL
    assert "null pointer" in err()
    assert lib.ghf_dist_sweep_topk(1, None, None, None, None, None, 0, 1, 1, 1, 8, 1, None, 1, None, 0, None, None, None) == EINVAL
    assert "null pointer" in err()
    assert lib.ghf_dist_sweep_rank(1, p, p, None, p, None, None, 3, 1, 1, 1, 8, None, 1, p, need_r, p, p, None) == EINVAL
    assert "filter" in err()                                                               # nnz > 0 without lists
    assert lib.ghf_dist_sweep_rank(1, p, p, None, p, None, None, 0, 1, 5, 2, 8, None, 5, p, 1 << 20, p, p, None) == EINVAL
    assert "rows of q" in err()                                                            # B > rows_q without iq
    # a q table of 2^31 rows or more: the sweep keeps a query's row number in 32 bits, so the call is refused, with iq and without
    for rows_q in (1 << 31, 1 << 40):
        for iq in (p, None):
            assert lib.ghf_dist_sweep_rank(1, p, p, iq, p, None, None, 0, rows_q, 1, 1, 8, None, 1, p, need_r, p, p, None) == EINVAL
            assert "rows_q" in err() and "32 bits" in err()
            assert lib.ghf_dist_sweep_topk(1, p, p, iq, None, None, 0, rows_q, 1, 1, 8, 1, None, 1, p, need_t, p, p, None) == EINVAL
            assert "rows_q" in err() and "32 bits" in err()
    with open(os.path.join(_build.INCLUDE, "ghf_distance_sweep.h")) as f:
        assert "rows_q < 2^31" in f.read()


# ---- the methods ---------------------------------------------------------------------------------------------------------
def test_signatures(model):
    want = ["known", "filt_ptr", "filt_idx", "query_rows", "query_rel", "candidates"]
    for fn, lead in ((model.rank_by_distance, ["embs", "query", "target", "distance"]),
                     (model.topk_by_distance, ["embs", "query", "k", "distance"])):
        p = inspect.signature(fn).parameters
        assert list(p) == lead + want, fn.__name__
        assert all(p[n].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD and p[n].default is inspect.Parameter.empty for n in lead)
        assert all(p[n].kind is inspect.Parameter.KEYWORD_ONLY and p[n].default is None for n in want)
        assert '``"complex"``' in fn.__doc__ or "distance`` and every" in fn.__doc__
    # the older methods keep their forms (tests/test_distance_host.py pins them too)
    assert "distance" not in inspect.signature(model.topk_candidates).parameters
    with pytest.raises(ValueError, match="dot product") as exc:
        model.rank_candidates(torch.randn(9, 4), torch.arange(3), torch.arange(3), distance="l1")
    assert "rank_by_distance" in str(exc.value)


def test_validation_needs_no_device(model):
    """CPU tensors throughout: each ValueError / IndexError below is raised before the "HIP device only" RuntimeError."""
    N, B = 50, 6
    embs, odd = torch.randn(N, 16), torch.randn(N, 15)
    q, t = torch.arange(B), torch.arange(B) + 1
    rank = lambda e, *a, **kw: model.rank_by_distance(e, q, t, *a, **kw)
    topk = lambda e, *a, **kw: model.topk_by_distance(e, q, 5, *a, **kw)
    for fn in (rank, topk):
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
        with pytest.raises(ValueError, match="not both"):
            fn(embs, "l1", known=(q, t), filt_ptr=torch.zeros(B + 1, dtype=torch.int64), filt_idx=torch.zeros(0, dtype=torch.int64))
        with pytest.raises(ValueError, match="query_rel"):
            fn(embs, "l1", known=(q, t, q))
        with pytest.raises(ValueError, match="query_rel"):
            fn(embs, "l1", known=(q, t), query_rel=q)
        for metric, e in (("l1", embs), ("l2", embs), ("complex", embs), ("l1", odd), ("l2", odd)):
            with pytest.raises(RuntimeError, match="HIP device"):                          # valid: only now the device is asked for
                fn(e, metric)
        with pytest.raises(TypeError):                                                     # no bias, no per-query sets here
            fn(embs, "l1", candidate_bias=torch.zeros(N))
        with pytest.raises(TypeError):
            fn(embs, "l1", negatives=torch.zeros(B, 3, dtype=torch.int64))
    with pytest.raises(ValueError, match="6 queries and 5 targets"):
        model.rank_by_distance(embs, q, t[:5], "l1")
    with pytest.raises(IndexError, match="target"):
        model.rank_by_distance(embs, q, t + N, "l1")
    with pytest.raises(IndexError, match="query"):
        model.topk_by_distance(embs, q + N, 5, "l1")
    for k in (0, 129):
        with pytest.raises(ValueError, match="outside 1..128"):
            model.topk_by_distance(embs, q, k, "l2")


# ---- the restatement -----------------------------------------------------------------------------------------------------
def explicit_distances(metric, rows, c):
    """[B, N] float64 through the whole [B, N, d] tensor, written independently of _distance_ref.dist."""
    delta = rows.double().unsqueeze(1) - c.double().unsqueeze(0)
    if metric == "l1":
        return torch.linalg.vector_norm(delta, ord=1, dim=-1)
    if metric == "l2":
        return torch.cdist(rows.double(), c.double(), p=2, compute_mode="donot_use_mm_for_euclid_dist")
    return torch.view_as_complex(delta.reshape(*delta.shape[:-1], -1, 2).contiguous()).abs().sum(-1)


@pytest.mark.parametrize("metric", R.METRICS)
def test_restatement_is_compare_count_and_sort(metric):
    N, B, d, k = 300, 9, 8, 12
    g = torch.Generator().manual_seed(11)
    c = torch.round(2 * torch.randn(N, d, generator=g)) / 2                         # coarse rows: distances do tie
    if metric == "complex":
        c[:, 1::2] = 0
    c[200:220] = c[:20]
    query, target = torch.arange(B), torch.arange(B) + 200
    rows = c[query]
    rng = np.random.default_rng(3)
    lists = [np.unique(rng.integers(0, N, 6)) if i % 3 else np.zeros(0, dtype=np.int64) for i in range(B)]
    lists[1] = np.append(lists[1], target[1].item())                                # a list that holds the target
    cand = np.unique(np.concatenate([rng.integers(0, N, 150), np.arange(8), np.arange(200, 208)]))
    D = S.distances(metric, rows, c)
    E = explicit_distances(metric, rows, c)
    assert torch.allclose(torch.from_numpy(D), E, rtol=1e-13, atol=1e-13)
    tn = target.numpy()
    for cd in (None, cand):
        inset = np.ones(N, dtype=bool) if cd is None else np.isin(np.arange(N), cd)
        greater, equal = S.rank(D, tn, lists, cd)
        sc, ids = S.topk(D, k, lists, cd)
        for i in range(B):
            keep = inset.copy()
            keep[lists[i]] = False
            full = keep.copy()
            keep[tn[i]] = False
            s, t = -D[i], -D[i, tn[i]]
            assert greater[i] == int((s[keep] > t).sum()) and equal[i] == int((s[keep] == t).sum())
            order = sorted(np.nonzero(full)[0], key=lambda j: (D[i, j], j))[:k]
            assert ids[i].tolist() == order and np.array_equal(sc[i], -D[i, order])
        assert int(equal.sum()) > 0                                                 # the copies tie with the targets
    short = S.topk(D, k, [np.arange(N - 5)] * B)                                    # fewer than k left
    assert (short[1][:, 5:] == -1).all() and np.isneginf(short[0][:, 5:]).all() and (short[1][:, :5] >= N - 5).all()


def test_l1_chain_in_float32_is_the_stated_chain():
    rng = np.random.default_rng(2)
    rows, c = rng.standard_normal((3, 7)).astype(np.float32), rng.standard_normal((5, 7)).astype(np.float32)
    got = S.l1_chain32(rows, c)
    for i in range(3):
        for j in range(5):
            acc = np.float32(0)
            for k in range(7):
                acc = np.float32(acc + np.abs(np.float32(rows[i, k] - c[j, k])))
            assert got[i, j] == acc
    assert np.abs(got - S.distances("l1", rows, c)).max() <= S.eps(S.distances("l1", rows, c), 7).max()


# ---- the bracket's cap ---------------------------------------------------------------------------------------------------
def cap_problem(d, N=2600, B=65):
    """The problem of the GPU bracket tests (tests/test_distance_sweep_gpu.py imports it, so the cap is checked on the very
    data it is used on): rows_cpu rows, N across three slabs of the sweep, B one query past a query tile, translated queries
    query_rows = embs[q] + 0.5 v with v standard normal."""
    embs = rows_cpu(N, d, 7 * d)
    rng = np.random.default_rng(7 * d)
    query, target = rng.integers(0, N, B), rng.integers(0, N, B)
    v = torch.from_numpy(rng.standard_normal((B, d)).astype(np.float32))
    return embs, query, target, embs[torch.from_numpy(query)] + 0.5 * v


def fp32_distances(metric, rows, c):
    """The same formulas in fp32 on the CPU, a query at a time."""
    out = np.empty((rows.size(0), c.size(0)), dtype=np.float64)
    for i in range(rows.size(0)):
        delta = rows[i].unsqueeze(0) - c
        if metric == "l1":
            D = delta.abs().sum(-1)
        elif metric == "l2":
            D = torch.sqrt((delta * delta).sum(-1))
        else:
            D = torch.sqrt((delta * delta).reshape(c.size(0), -1, 2).sum(-1)).sum(-1)
        assert D.dtype == torch.float32
        out[i] = D.double().numpy()
    return out


CAP_CASES = [(m, d) for m in R.METRICS for d in DIMS if not (m == "complex" and d % 2)]


@pytest.mark.parametrize("metric,d", CAP_CASES, ids=["%s-d%d" % c for c in CAP_CASES])
def test_the_rank_bracket_is_narrow_and_holds_fp32(metric, d):
    """What the GPU tests may excuse on real data is the bracket of test_rank_gpu.rank_bracket on s = -D under eps = (d + 8)
    2^-24 D, and nothing beyond it.  Here, without a GPU: the bracket is at most max(8, N / 100) wide for every query and of
    zero width for at least a quarter of them, and the same formulas in fp32 on the CPU land inside it with an error of at
    most eps.  For k = 10 the k-th and (k + 1)-th distances are separated by more than 2 eps_max for most queries, so the
    top-k rules decide most ids."""
    embs, query, target, rows = cap_problem(d)
    N, B = embs.size(0), rows.size(0)
    D = S.distances(metric, rows, embs)
    E = S.eps(D, d)
    lo, hi = rank_bracket(-D, E, target, None)
    width = hi - lo
    zero = np.count_nonzero(width == 0) / B
    D32 = fp32_distances(metric, rows, embs)
    err = np.abs(D32 - D) / np.maximum(E, 1e-300)
    g32, e32 = S.rank(D32, target)
    ordered = np.sort(D, axis=1)
    apart = np.count_nonzero(ordered[:, 10] - ordered[:, 9] > 2 * E.max(axis=1)) / B
    print(f"{metric} d={d}: bracket width max {width.max()}, zero-width share {zero:.2f}, fp32 error max {err[D > 0].max():.2f} eps, "
          f"k = 10 separated for {apart:.2f}")
    assert width.max() <= max(8, N / 100)
    assert zero >= 0.25
    assert (err[D > 0] <= 1).all() and (D32[D == 0] == 0).all()
    assert (lo <= g32).all() and (g32 + e32 <= hi).all()
