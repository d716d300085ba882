"""Rank and top-k link prediction against every node (HyperGNN.rank_candidates / topk_candidates, ghf_score_rank /
ghf_score_topk) against a float64 numpy restatement of their contract.  All tests need an MI355X.

Two kinds of check:
  * exact: rows are multiples of 2^-6 clipped to [-4, 4]; every product is a multiple of 2^-12 and every partial sum at most
    16 d <= 2^12, so fp32 accumulation is exact in any order and counts, ids and scores must EQUAL the float64 restatement;
  * bracket: for real embeddings, with u = 2^-24 and eps(i, j) = d u sum_k |q_i[k] c_j[k]| (the standard bound of a
    length-d fp32 dot product), lo_i <= greater[i] and greater[i] + equal[i] <= hi_i where lo counts float64 scores above
    t + eps(i, j) + eps(i, target) and hi those at or above t - eps(i, j) - eps(i, target).  For top-k, with
    eps_max(i) = max_j eps(i, j): a returned id's float64 score is at least the k-th float64 score minus eps(i, j) + eps_max(i)
    (if j is returned in place of a true top-k member m, fp32(j) >= fp32(m)), every id whose float64 score exceeds the k-th
    by more than that is returned (same argument with the roles swapped), returned scores are within eps(i, j) of float64.
"""

import numpy as np
import pytest
import torch

import cases
from _util import assert_close
from graph_hypernetwork_forge_amd import HyperGNN, ToyKnowledgeGraph, _native, link_prediction_metrics

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
U = 2.0 ** -24


# ---- the restatement ---------------------------------------------------------------------------------------------------
def csr(lists):
    ptr = np.zeros(len(lists) + 1, dtype=np.int64)
    ptr[1:] = np.cumsum([len(l) for l in lists])
    idx = np.concatenate([np.asarray(l, dtype=np.int64) for l in lists]) if ptr[-1] else np.zeros(0, dtype=np.int64)
    return torch.from_numpy(ptr), torch.from_numpy(idx)


def scores64(q, c):
    """float64 scores [B, N] and eps [B, N] of float32 rows q [B, d], c [N, d]."""
    q64, c64 = q.astype(np.float64), c.astype(np.float64)
    return q64 @ c64.T, q.shape[1] * U * (np.abs(q64) @ np.abs(c64).T)


def allowed_mask(N, lists, i, target=None):
    m = np.ones(N, dtype=bool)
    if lists is not None and len(lists[i]):
        m[np.asarray(lists[i], dtype=np.int64)] = False
    if target is not None:
        m[target[i]] = False
    return m


def rank_exact(S, target, lists):
    g, e = np.zeros(len(target), dtype=np.int64), np.zeros(len(target), dtype=np.int64)
    for i in range(len(target)):
        m = allowed_mask(S.shape[1], lists, i, target)
        t = S[i, target[i]]
        g[i], e[i] = np.count_nonzero(S[i][m] > t), np.count_nonzero(S[i][m] == t)
    return g, e


def rank_bracket(S, E, target, lists):
    lo, hi = np.zeros(len(target), dtype=np.int64), np.zeros(len(target), dtype=np.int64)
    for i in range(len(target)):
        m = allowed_mask(S.shape[1], lists, i, target)
        t, et = S[i, target[i]], E[i, target[i]]
        lo[i] = np.count_nonzero(S[i][m] > t + E[i][m] + et)
        hi[i] = np.count_nonzero(S[i][m] >= t - E[i][m] - et)
    return lo, hi


def check_rank_bracket(greater, equal, S, E, target, lists, what):
    g, e = greater.cpu().numpy(), equal.cpu().numpy()
    lo, hi = rank_bracket(S, E, target, lists)
    width = hi - lo
    print(f"{what}: bracket width mean {width.mean():.2f} max {width.max()}, zero-width {np.count_nonzero(width == 0)} of {len(g)}")
    assert (g >= 0).all() and (e >= 0).all(), what
    bad = np.nonzero((lo > g) | (g + e > hi))[0]
    assert bad.size == 0, f"{what}: queries {bad[:8]} outside the bracket: lo {lo[bad[:8]]} g {g[bad[:8]]} e {e[bad[:8]]} hi {hi[bad[:8]]}"


def topk_exact(S, k, lists):
    B, N = S.shape
    sc, ids = np.full((B, k), -np.inf), np.full((B, k), -1, dtype=np.int64)
    for i in range(B):
        cand = np.nonzero(allowed_mask(N, lists, i))[0]
        order = cand[np.lexsort((cand, -S[i, cand]))][:k]
        sc[i, :len(order)], ids[i, :len(order)] = S[i, order], order
    return sc, ids


def check_topk_bracket(scores, ids, S, E, k, lists, what):
    sc, ids = scores.cpu().numpy().astype(np.float64), ids.cpu().numpy()
    B, N = S.shape
    for i in range(B):
        m = allowed_mask(N, lists, i)
        n_ok = int(m.sum())
        kk = min(k, n_ok)
        assert (ids[i, kk:] == -1).all() and np.isneginf(sc[i, kk:]).all(), f"{what}: tail of query {i}"
        got = ids[i, :kk]
        assert (got >= 0).all() and (got < N).all() and m[got].all() and len(set(got.tolist())) == kk, f"{what}: ids of query {i}"
        assert (np.diff(sc[i, :kk]) <= 0).all(), f"{what}: query {i} not descending"
        assert (np.abs(sc[i, :kk] - S[i, got]) <= E[i, got]).all(), f"{what}: scores of query {i}"
        if kk < k:
            continue
        kth = np.sort(S[i][m])[-k]
        emax = E[i][m].max()
        assert (S[i, got] >= kth - E[i, got] - emax).all(), f"{what}: query {i} returns an id below the k-th score"
        must = np.nonzero(m & (S[i] > kth + E[i] + emax))[0]
        assert np.isin(must, got).all(), f"{what}: query {i} misses an id above the k-th score"


# ---- data --------------------------------------------------------------------------------------------------------------
def exact_rows(N, d, seed):
    g = np.random.default_rng(seed).standard_normal((N, d))
    c = np.clip(np.round(64 * g) / 64, -4, 4).astype(np.float32)
    c[-500:] = c[:500]                       # copies: ties with the target, and between top-k candidates
    return c


def layernorm_rows(N, d, seed):
    """LayerNorm-shaped rows (what the model's last layer emits), built on the device."""
    gen = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(N, d, device=DEV, generator=gen)
    gamma = 1.0 + 0.1 * torch.randn(d, device=DEV, generator=gen)
    beta = 0.1 * torch.randn(d, device=DEV, generator=gen)
    return torch.nn.functional.layer_norm(x, (d,), gamma, beta)


def filter_lists(rng, B, N, target, big=True):
    """Lists that contain the target, hold duplicates, are empty, or name most of the graph; unsorted."""
    lists = []
    for i in range(B):
        kind = i % 5
        if kind == 0:
            l = np.zeros(0, dtype=np.int64)
        elif kind == 1:
            l = np.concatenate([rng.integers(0, N, 7), [target[i]]])
        elif kind == 2:
            l = rng.integers(0, N, 12)
            l = np.concatenate([l, l[:5], [target[i], target[i]]])
        elif kind == 3 and big and i < 20:
            l = rng.permutation(N)[: N - 50]                           # fewer than 128 candidates remain
        else:
            l = rng.integers(0, min(N, 700), 40)                       # the tied rows among them
        lists.append(rng.permutation(l).astype(np.int64))
    return lists


def model_of(d=16):
    return HyperGNN(text_dim=16, node_feat_dim=8, hidden_dim=d, num_layers=1).to(DEV).eval().requires_grad_(False)


# ---- exact case ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [16, 20, 32, 64, 128, 256])
def test_exact_data_equals_the_float64_restatement(d):
    N, B = 20_000, 256
    c = exact_rows(N, d, seed=d)
    rng = np.random.default_rng(1000 + d)
    query = rng.integers(0, N, B)
    query[:40] = rng.integers(0, 500, 40)                              # queries whose copies tie
    target = rng.integers(0, N, B)
    target[:80] = rng.integers(0, 500, 80)                             # targets with a copy: equal >= 1
    S, _ = scores64(c[query], c)
    assert np.array_equal(S, (c[query] @ c.T).astype(np.float64))                 # the data is exact in fp32 as well
    lists = filter_lists(rng, B, N, target)
    fp, fi = csr(lists)
    model, embs = model_of(), torch.from_numpy(c).to(DEV)
    qd, td = torch.from_numpy(query).to(DEV), torch.from_numpy(target).to(DEV)

    g_ref, e_ref = rank_exact(S, target, None)
    print(f"d={d}: max |s| {np.abs(S).max():.1f}, queries with ties {np.count_nonzero(e_ref)} of {B}")
    assert np.count_nonzero(e_ref) >= 40
    g, e = model.rank_candidates(embs, qd, td)
    assert g.dtype == torch.int64 and e.dtype == torch.int64 and not g.requires_grad
    assert np.array_equal(g.cpu().numpy(), g_ref) and np.array_equal(e.cpu().numpy(), e_ref), "unfiltered"
    g_ref, e_ref = rank_exact(S, target, lists)
    g, e = model.rank_candidates(embs, qd, td, filt_ptr=fp.to(DEV), filt_idx=fi.to(DEV))
    assert np.array_equal(g.cpu().numpy(), g_ref) and np.array_equal(e.cpu().numpy(), e_ref), "filtered"
    # queries as their own matrix, no index list
    g, e = _native.score_rank(embs[qd].contiguous(), embs, td)
    g_ref0, e_ref0 = rank_exact(S, target, None)
    assert np.array_equal(g.cpu().numpy(), g_ref0) and np.array_equal(e.cpu().numpy(), e_ref0), "iq omitted"

    for k in (1, 10, 128):
        for ls, fl in ((None, (None, None)), (lists, (fp.to(DEV), fi.to(DEV)))):
            sc_ref, id_ref = topk_exact(S, k, ls)
            sc, ids = model.topk_candidates(embs, qd, k, filt_ptr=fl[0], filt_idx=fl[1])
            assert sc.shape == (B, k) and ids.dtype == torch.int64 and sc.dtype == torch.float32
            assert np.array_equal(ids.cpu().numpy(), id_ref), f"top-{k} ids, filtered={ls is not None}"
            assert np.array_equal(sc.cpu().numpy().astype(np.float64), sc_ref), f"top-{k} scores, filtered={ls is not None}"
            if ls is not None and k == 128:
                assert (id_ref[3] == -1).sum() == 128 - 50              # k > remaining candidates was exercised
    sc, ids = _native.score_topk(embs[qd].contiguous(), embs, 10)
    assert np.array_equal(ids.cpu().numpy(), topk_exact(S, 10, None)[1]), "top-k, iq omitted"


@pytest.mark.parametrize("B,N", [(1, 20_000), (200, 20_000), (129, 777), (5, 100)])
def test_exact_data_odd_batch_and_graph_sizes(B, N):
    d = 128
    c = exact_rows(max(N, 600), d, seed=7)[-N:]
    rng = np.random.default_rng(B * 31 + N)
    query, target = rng.integers(0, N, B), rng.integers(0, N, B)
    lists = filter_lists(rng, B, N, target, big=False)
    fp, fi = csr(lists)
    S, _ = scores64(c[query], c)
    model, embs = model_of(), torch.from_numpy(c).to(DEV)
    qd, td = torch.from_numpy(query).to(DEV), torch.from_numpy(target).to(DEV)
    for ls, fl in ((None, (None, None)), (lists, (fp.to(DEV), fi.to(DEV)))):
        g_ref, e_ref = rank_exact(S, target, ls)
        g, e = model.rank_candidates(embs, qd, td, filt_ptr=fl[0], filt_idx=fl[1])
        assert np.array_equal(g.cpu().numpy(), g_ref) and np.array_equal(e.cpu().numpy(), e_ref)
        for k in (1, 10, 128):
            sc_ref, id_ref = topk_exact(S, k, ls)
            sc, ids = model.topk_candidates(embs, qd, k, filt_ptr=fl[0], filt_idx=fl[1])
            assert np.array_equal(ids.cpu().numpy(), id_ref) and np.array_equal(sc.cpu().numpy().astype(np.float64), sc_ref)


# ---- real embeddings -----------------------------------------------------------------------------------------------------
def test_model_embeddings_of_the_golden_case_every_query():
    (case,) = cases.graph_cases(only=["g6_c3"])
    cfg = cases.MODELS[case.model]
    model = HyperGNN(cfg.text_dim, cfg.node_feat_dim, cfg.hidden_dim, cfg.num_layers, char_emb_dim=cfg.char_emb_dim)
    model.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in cfg.params().items()})
    model = model.to(DEV).eval()
    ei = torch.from_numpy(case.edge_index).to(DEV)
    with torch.no_grad():
        embs = model(torch.from_numpy(case.node_features).to(DEV), ei, case.edge_texts)
    c = embs.cpu().numpy()
    N = c.shape[0]
    B = 300
    src, dst = case.edge_index[0][:B].astype(np.int64), case.edge_index[1][:B].astype(np.int64)
    lists = [np.unique(case.edge_index[1][case.edge_index[0] == s]).astype(np.int64) for s in src]
    S, E = scores64(c[src], c)
    g, e = model.rank_candidates(embs, ei[0][:B], ei[1][:B], known=(ei[0], ei[1]))
    check_rank_bracket(g, e, S, E, dst, lists, "g6_c3 filtered")
    g, e = model.rank_candidates(embs, ei[0][:B], ei[1][:B])
    check_rank_bracket(g, e, S, E, dst, None, "g6_c3 unfiltered")
    for k in (1, 10, 128):
        sc, ids = model.topk_candidates(embs, ei[0][:B], k, known=(ei[0], ei[1]))
        check_topk_bracket(sc, ids, S, E, k, lists, f"g6_c3 top-{k}")
    # against the existing pair kernel, on the returned pairs
    sc, ids = model.topk_candidates(embs, ei[0][:B], 10)
    pair = model.score_edges(embs, ei[0][:B].repeat_interleave(10), ids.reshape(-1))
    assert_close(sc.reshape(-1).cpu().numpy(), pair.cpu().numpy(), "top-k scores against score_edges", atol=1e-4)


def test_layernorm_rows_at_200k_every_query():
    N, d, B = 200_000, 128, 200
    embs = layernorm_rows(N, d, seed=3)
    c = embs.cpu().numpy()
    rng = np.random.default_rng(5)
    query, target = rng.integers(0, N, B), rng.integers(0, N, B)
    lists = filter_lists(rng, B, N, target, big=False)
    fp, fi = csr(lists)
    S, E = scores64(c[query], c)
    model = model_of()
    qd, td = torch.from_numpy(query).to(DEV), torch.from_numpy(target).to(DEV)
    g, e = model.rank_candidates(embs, qd, td, filt_ptr=fp.to(DEV), filt_idx=fi.to(DEV))
    check_rank_bracket(g, e, S, E, target, lists, "LayerNorm rows, N = 200k")
    sc, ids = model.topk_candidates(embs, qd, 10, filt_ptr=fp.to(DEV), filt_idx=fi.to(DEV))
    check_topk_bracket(sc, ids, S, E, 10, lists, "LayerNorm rows, N = 200k, top-10")
    pair = model.score_edges(embs, qd.repeat_interleave(10), ids.reshape(-1))
    assert_close(sc.reshape(-1).cpu().numpy(), pair.cpu().numpy(), "top-k scores against score_edges", atol=1e-4)


def test_no_score_matrix_at_config_3_size():
    N, d, B = 1_000_000, 128, 1024
    embs = layernorm_rows(N, d, seed=1003)
    rng = np.random.default_rng(11)
    query, target = rng.integers(0, N, B), rng.integers(0, N, B)
    ksrc = np.concatenate([query, query, rng.integers(0, N, 5000)])
    kdst = np.concatenate([target, rng.integers(0, N, B), rng.integers(0, N, 5000)])
    qd, td = torch.from_numpy(query).to(DEV), torch.from_numpy(target).to(DEV)
    known = (torch.from_numpy(ksrc).to(DEV), torch.from_numpy(kdst).to(DEV))
    model = model_of()
    limit = B * N * 4 // 16
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    g, e = model.rank_candidates(embs, qd, td, known=known)
    torch.cuda.synchronize()
    rise_rank = torch.cuda.max_memory_allocated() - base
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    sc, ids = model.topk_candidates(embs, qd, 10, known=known)
    torch.cuda.synchronize()
    rise_topk = torch.cuda.max_memory_allocated() - base
    print(f"peak rise: rank {rise_rank / 2**20:.1f} MiB, top-k {rise_topk / 2**20:.1f} MiB, limit {limit / 2**20:.0f} MiB")
    assert rise_rank < limit and rise_topk < limit
    sample = rng.choice(B, 64, replace=False)
    pick = torch.from_numpy(sample).to(DEV)
    c = embs.cpu().numpy()
    S, E = scores64(c[query[sample]], c)
    lists = [np.unique(kdst[ksrc == q]) for q in query[sample]]
    check_rank_bracket(g[pick], e[pick], S, E, target[sample], lists, "N = 1M")
    check_topk_bracket(sc[pick], ids[pick], S, E, 10, lists, "N = 1M top-10")


# ---- reproducibility, graph capture --------------------------------------------------------------------------------------
def test_reproducible_and_graph_capturable():
    N, d, B, k = 50_000, 128, 300, 10
    embs = layernorm_rows(N, d, seed=8)
    rng = np.random.default_rng(8)
    qd = torch.from_numpy(rng.integers(0, N, B)).to(DEV)
    td = torch.from_numpy(rng.integers(0, N, B)).to(DEV)
    lists = [np.sort(rng.integers(0, N, 9)) for _ in range(B)]
    fp, fi = (t.to(DEV) for t in csr(lists))
    first = _native.score_rank(embs, embs, td, iq=qd, filt_ptr=fp, filt_idx=fi)
    again = _native.score_rank(embs, embs, td, iq=qd, filt_ptr=fp, filt_idx=fi)
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])
    tfirst = _native.score_topk(embs, embs, k, iq=qd, filt_ptr=fp, filt_idx=fi)
    tagain = _native.score_topk(embs, embs, k, iq=qd, filt_ptr=fp, filt_idx=fi)
    assert torch.equal(tfirst[0], tagain[0]) and torch.equal(tfirst[1], tagain[1])

    ws_r = torch.empty(_native.score_rank_workspace_bytes(B, N, d), dtype=torch.uint8, device=DEV)
    ws_t = torch.empty(_native.score_topk_workspace_bytes(B, N, d, k), dtype=torch.uint8, device=DEV)
    out_r = (torch.empty(B, dtype=torch.int64, device=DEV), torch.empty(B, dtype=torch.int64, device=DEV))
    out_t = (torch.empty(B, k, dtype=torch.float32, device=DEV), torch.empty(B, k, dtype=torch.int64, device=DEV))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _native.score_rank(embs, embs, td, iq=qd, filt_ptr=fp, filt_idx=fi, workspace=ws_r, out=out_r)
        _native.score_topk(embs, embs, k, iq=qd, filt_ptr=fp, filt_idx=fi, workspace=ws_t, out=out_t)
    for _ in range(2):
        for t in out_r + out_t:
            t.fill_(7)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out_r[0], first[0]) and torch.equal(out_r[1], first[1])
        assert torch.equal(out_t[0], tfirst[0]) and torch.equal(out_t[1], tfirst[1])


# ---- the public path -----------------------------------------------------------------------------------------------------
def test_public_path_on_the_toy_graph():
    kg = ToyKnowledgeGraph(feat_dim=16)
    torch.manual_seed(0)
    model = HyperGNN(text_dim=32, node_feat_dim=16, hidden_dim=32).to(DEV).eval()
    x, ei = kg.node_features.to(DEV), kg.edge_index.to(DEV)
    with torch.no_grad():
        embs = model(x, ei, kg.edge_texts)
    src, dst = ei[0], ei[1]
    g, e = model.rank_candidates(embs, src, dst, known=(src, dst))
    assert not g.requires_grad and g.shape == (src.numel(),)
    m = link_prediction_metrics(g, e)
    c = embs.cpu().numpy()
    s_np, d_np = kg.edge_index[0].numpy(), kg.edge_index[1].numpy()
    lists = [np.unique(d_np[s_np == s]) for s in s_np]
    S, E = scores64(c[s_np], c)
    check_rank_bracket(g, e, S, E, d_np, lists, "toy graph")
    lo, hi = rank_bracket(S, E, d_np, lists)
    g_ref, e_ref = rank_exact(S, d_np, lists)
    tight = hi == lo
    assert np.array_equal(g.cpu().numpy()[tight], g_ref[tight])
    rank = 1 + g.cpu().numpy() + e.cpu().numpy() / 2
    assert m["mrr"] == pytest.approx(float((1 / rank).mean())) and m["mean_rank"] == pytest.approx(float(rank.mean()))
    assert 0 < m["mrr"] <= 1 and m["hits@1"] <= m["hits@3"] <= m["hits@10"] <= 1
    fp, fi = csr(lists)
    g2, e2 = model.rank_candidates(embs, src, dst, filt_ptr=fp.to(DEV), filt_idx=fi.to(DEV))
    assert torch.equal(g, g2) and torch.equal(e, e2)
    sc, ids = model.topk_candidates(embs, src, 3, known=(src, dst))
    sc2, ids2 = model.topk_candidates(embs, src, 3, filt_ptr=fp.to(DEV), filt_idx=fi.to(DEV))
    assert torch.equal(sc, sc2) and torch.equal(ids, ids2)
    check_topk_bracket(sc, ids, S, E, 3, lists, "toy graph top-3")
    # embeddings that carry a graph are read as data
    g3, _ = model.rank_candidates(embs.clone().requires_grad_(True), src, dst, known=(src, dst))
    assert torch.equal(g, g3) and not g3.requires_grad


# ---- errors --------------------------------------------------------------------------------------------------------------
def test_out_of_range_ids():
    N, d, B = 3000, 64, 40
    embs = layernorm_rows(N, d, seed=2)
    model = model_of()
    rng = np.random.default_rng(2)
    query, target = rng.integers(0, N, B), rng.integers(0, N, B)
    qd, td = torch.from_numpy(query).to(DEV), torch.from_numpy(target).to(DEV)
    bad_q, bad_t = qd.clone(), td.clone()
    bad_q[3], bad_t[5] = N, -N - 1
    with pytest.raises(IndexError):
        model.rank_candidates(embs, bad_q, td)
    with pytest.raises(IndexError):
        model.rank_candidates(embs, qd, bad_t)
    with pytest.raises(IndexError):
        model.rank_candidates(embs, qd, td, known=(qd, bad_q))
    with pytest.raises(IndexError):
        model.topk_candidates(embs, bad_q, 5)
    with pytest.raises(ValueError):
        model.topk_candidates(embs, qd, 129)
    with pytest.raises(ValueError):
        model.topk_candidates(embs, qd, 0)
    # negative ids wrap as in indexing
    g, e = model.rank_candidates(embs, qd - N, td - N)
    g0, e0 = model.rank_candidates(embs, qd, td)
    assert torch.equal(g, g0) and torch.equal(e, e0)

    # the raw call: that query's outputs are -1, the others are untouched, nothing faults
    lists = [np.sort(rng.integers(0, N, 4)) for _ in range(B)]
    lists[9] = np.array([1, 2, N + 5])
    lists[11] = np.array([-3, 2, 7])
    fp, fi = (t.to(DEV) for t in csr(lists))
    raw_q, raw_t = qd.clone(), td.clone()
    raw_q[3], raw_q[4], raw_t[5], raw_t[6] = N, -1, N, -2
    bad = [3, 4, 5, 6, 9, 11]
    good = [i for i in range(B) if i not in bad]
    good_lists = [l if i not in (9, 11) else np.zeros(0, dtype=np.int64) for i, l in enumerate(lists)]
    gp, gi = (t.to(DEV) for t in csr(good_lists))
    g, e = _native.score_rank(embs, embs, raw_t, iq=raw_q, filt_ptr=fp, filt_idx=fi)
    gr, er = _native.score_rank(embs, embs, td, iq=qd, filt_ptr=gp, filt_idx=gi)
    assert (g[bad] == -1).all() and (e[bad] == -1).all()
    assert torch.equal(g[good], gr[good]) and torch.equal(e[good], er[good])
    sc, ids = _native.score_topk(embs, embs, 5, iq=raw_q, filt_ptr=fp, filt_idx=fi)
    scr, idr = _native.score_topk(embs, embs, 5, iq=qd, filt_ptr=gp, filt_idx=gi)
    tbad = [3, 4, 9, 11]
    tgood = [i for i in range(B) if i not in tbad]
    assert (ids[tbad] == -1).all() and torch.isnan(sc[tbad]).all()
    assert torch.equal(ids[tgood], idr[tgood]) and torch.equal(sc[tgood], scr[tgood])
