"""Distance scores against every node on the device (HyperGNN.rank_by_distance / topk_by_distance;
include/ghf_distance_sweep.h; csrc/distance_sweep.hip) against the float64 restatement of tests/_distance_sweep_ref.py.

Shapes come from the sweep's tile constants: a workgroup covers TQ = 64 queries (16 per wave) and steps through CT = 256
candidates at a time, a slab is at least 4 tiles = 1,024 candidates, k is walked 16 columns per step and 4 per inner
iteration.  So B is of {1, 63, 65, 131} (TQ - 1, TQ + 1, 2 TQ + 3), N / C of {255, 257} (one tile, short and just over),
{1023, 1025} (one slab, two), 1300 and 2600 (two and three slabs, the last one short), d of {1, 2, 3, 4, 6, 64, 130, 256}
(under one inner iteration, the scalar path, one and several steps, a last step that is short), and a base that is not
16-byte aligned takes the scalar path at d = 64.

What is asserted: on exact data (multiples of 2^-6, copied rows) counts, ids and scores EQUAL float64 — for L2 the scores
are roots of exact sums, which no fp32 holds, and equal float64's root rounded to fp32 to within the 1 ulp the header states
for the hardware root (exactly 0 at distance 0); its counts and ids are float64's.  L1 on real data equals the stated chain emulated in numpy float32 bit for bit.  L2 and the complex modulus
on real data stay inside the bracket of eps = (d + 8) 2^-24 D, whose width tests/test_distance_sweep_host.py caps on this
very data.  The float64 side is computed a query at a time."""

import numpy as np
import pytest
import torch

import _distance_ref as R
import _distance_sweep_ref as S
from graph_hypernetwork_forge_amd import HyperGNN, _native, link_prediction_metrics
from test_distance_sweep_host import DIMS, cap_problem
from test_rank_gpu import check_rank_bracket, check_topk_bracket, csr, filter_lists

gpu = pytest.mark.gpu
DEV = torch.device("cuda:0")
TQ, CT, SLAB = 64, 256, 1024
METRIC = _native.DIST_METRICS
EXACT = [(m, d) for m in R.METRICS for d in DIMS if not (m == "complex" and d % 2)]
EXACT_IDS = ["%s-d%d" % c for c in EXACT]


@pytest.fixture(scope="module")
def model():
    return HyperGNN(text_dim=16, node_feat_dim=8, hidden_dim=16, num_layers=1).to(DEV).eval().requires_grad_(False)


def dev(x):
    return None if x is None else torch.as_tensor(x).to(DEV)


def bits(t):
    return t.detach().contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def lists_dev(lists):
    fp, fi = csr(lists)
    return dict(filt_ptr=fp.to(DEV), filt_idx=fi.to(DEV))


def np_of(pair):
    return tuple(x.cpu().numpy() for x in pair)


# ---- 1. exact data ---------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("metric,d", EXACT, ids=EXACT_IDS)
def test_exact_data_equals_float64(model, metric, d):
    N, B = 2600, 2 * TQ + 3
    c = S.exact_rows(N, d, seed=d, metric=metric)
    rng = np.random.default_rng(500 + d)
    query, target = rng.integers(0, N, B), rng.integers(0, N, B)
    query[:40] = rng.permutation(500)[:40]                              # queries with a copy: two rows at distance 0
    target[:80] = rng.integers(0, 500, 80)                              # targets with a copy: equal >= 1
    # two equal candidates straddling rank k, planted for k = 10 (the last query) and k = 128 (the one before): the first row
    # behind the k-th nearest that is neither a copied row, nor a query's node becomes a copy of the k-th nearest
    query[B - 2:] = rng.permutation(np.arange(500, N - 500))[:2]
    for i, k in ((B - 1, 10), (B - 2, 128)):
        Di = S.distances(metric, c[query[i:i + 1]], c)[0]
        order = np.lexsort((np.arange(N), Di))
        j = next(int(v) for v in order[k:] if 500 <= v < N - 500 and v not in query)
        c[j] = c[order[k - 1]]
    D = S.distances(metric, c[query], c)
    for i, k in ((B - 1, 10), (B - 2, 128)):
        nearest = np.sort(D[i])
        assert nearest[k - 1] == nearest[k], f"the planted tie across the cut at k = {k}"
    if metric != "l2":                                                  # the data is exact in fp32 as well
        assert np.array_equal(D, D.astype(np.float32).astype(np.float64))
    lists = filter_lists(rng, B, N, target)
    embs, qd, td = dev(c), dev(query), dev(target)

    g_ref, e_ref = S.rank(D, target)
    assert np.count_nonzero(e_ref) >= 40, "planted ties with the target"
    g, e = model.rank_by_distance(embs, qd, td, metric)
    assert g.dtype == torch.int64 and e.dtype == torch.int64 and not g.requires_grad
    assert np.array_equal(g.cpu().numpy(), g_ref) and np.array_equal(e.cpu().numpy(), e_ref), "unfiltered"
    g_ref, e_ref = S.rank(D, target, lists)
    g, e = model.rank_by_distance(embs, qd, td, metric, **lists_dev(lists))
    assert np.array_equal(g.cpu().numpy(), g_ref) and np.array_equal(e.cpu().numpy(), e_ref), "filtered"
    m = link_prediction_metrics(g, e)
    assert 0.0 < m["mrr"] <= 1.0
    g, e = _native.score_dist_sweep_rank(METRIC[metric], embs[qd].contiguous(), embs, td)       # queries as their own matrix
    assert np.array_equal(np_of((g, e)), S.rank(D, target)), "iq omitted"

    sc1, id1 = S.topk(D, 1, None)
    # two candidates at distance 0 straddle rank 1: the lower id (at small d further rows of the grid may coincide)
    assert (D[np.arange(40), N - 500 + query[:40]] == 0).all() and (id1[:40, 0] <= query[:40]).all() and (sc1[:40, 0] == 0).all()
    for k in (1, 10, 128):
        for ls, kw in ((None, {}), (lists, lists_dev(lists))):
            sc_ref, id_ref = S.topk(D, k, ls)
            sc, ids = model.topk_by_distance(embs, qd, k, metric, **kw)
            assert sc.shape == (B, k) and ids.dtype == torch.int64 and sc.dtype == torch.float32
            assert np.array_equal(ids.cpu().numpy(), id_ref), f"top-{k} ids, filtered={ls is not None}"
            got = sc.cpu().numpy().astype(np.float64)
            if metric == "l2":
                fin = np.isfinite(sc_ref)
                want32 = np.where(fin, sc_ref, 0.0).astype(np.float32)
                off = np.abs(np.where(fin, got, 0.0) - want32.astype(np.float64))
                assert np.array_equal(np.isfinite(got), fin) and np.isneginf(got[~fin]).all(), f"top-{k} L2 tails"
                assert (off <= np.spacing(np.abs(want32)).astype(np.float64)).all(), f"top-{k} L2 scores: {off.max()}"
                assert (got[sc_ref == 0] == 0).all()
            else:
                assert np.array_equal(got, sc_ref), f"top-{k} scores, filtered={ls is not None}"
            if ls is not None and k == 128:
                assert (id_ref[3] == -1).sum() == 128 - 50              # k > remaining candidates was exercised
    sc, ids = _native.score_dist_sweep_topk(METRIC[metric], embs[qd].contiguous(), embs, 10)
    assert np.array_equal(ids.cpu().numpy(), S.topk(D, 10, None)[1]), "top-k, iq omitted"


@gpu
@pytest.mark.parametrize("metric", R.METRICS)
@pytest.mark.parametrize("B,N", [(1, 255), (TQ - 1, 257), (TQ + 1, SLAB - 1), (1, SLAB + 1), (TQ + 1, 1300)])
def test_exact_data_at_the_tile_and_slab_edges(model, metric, B, N):
    """No copies here (N may be below 500): the edges of a tile and of a slab, every id of the last tile returned."""
    d = 6
    c = S.exact_rows(max(N, 1000), d, seed=N, metric=metric)[:N].copy()
    rng = np.random.default_rng(N)
    query, target = rng.integers(0, N, B), rng.integers(0, N, B)
    target[0] = N - 1                                                   # the last row of the table
    D = S.distances(metric, c[query], c)
    lists = [np.unique(rng.integers(0, N, 5)) if i % 2 else np.zeros(0, dtype=np.int64) for i in range(B)]
    embs, qd, td = dev(c), dev(query), dev(target)
    for ls, kw in ((None, {}), (lists, lists_dev(lists))):
        assert np.array_equal(np_of(model.rank_by_distance(embs, qd, td, metric, **kw)), S.rank(D, target, ls))
        sc, ids = model.topk_by_distance(embs, qd, 128, metric, **kw)
        assert np.array_equal(ids.cpu().numpy(), S.topk(D, 128, ls)[1])
    # the whole table is returned when every other row is listed away: the last tile's ids among them
    keep = np.arange(N - 100, N)
    ls = [np.arange(N - 100)] * B
    sc, ids = model.topk_by_distance(embs, qd, 128, metric, **lists_dev(ls))
    want = S.topk(D, 128, ls)[1]
    assert np.array_equal(ids.cpu().numpy(), want) and (np.sort(want[:, :100], axis=1) == keep).all() and (want[:, 100:] == -1).all()


# ---- 2. L1 on real data: the chain, bit for bit ---------------------------------------------------------------------------
def l1_check(model, embs_d, rows_d, embs, rows, target, lists, what):
    A = S.l1_chain32(rows.numpy(), embs.numpy())
    D = A.astype(np.float64)
    kw = lists_dev(lists)
    got = np_of(model.rank_by_distance(embs_d, dev(np.zeros(len(target), dtype=np.int64)), dev(target), "l1", query_rows=rows_d, **kw))
    assert np.array_equal(got, S.rank(D, target, lists)), f"{what}: counts"
    for k in (1, 10):
        sc, ids = model.topk_by_distance(embs_d, dev(np.zeros(len(target), dtype=np.int64)), k, "l1", query_rows=rows_d, **kw)
        sc_ref, id_ref = S.topk(D, k, lists)
        assert np.array_equal(ids.cpu().numpy(), id_ref), f"{what}: top-{k} ids"
        assert torch.equal(bits(sc.cpu()), bits(torch.from_numpy(sc_ref.astype(np.float32)))), f"{what}: top-{k} score bits"


@gpu
@pytest.mark.parametrize("d", DIMS)
def test_l1_on_real_data_is_the_stated_chain_bit_for_bit(model, d):
    embs, query, target, rows = cap_problem(d)
    lists = filter_lists(np.random.default_rng(d), len(target), embs.size(0), target)
    l1_check(model, embs.to(DEV), rows.to(DEV), embs, rows, target, lists, f"d={d}")


@gpu
def test_an_unaligned_base_takes_the_scalar_path_and_keeps_the_bits(model):
    d = 64
    embs, query, target, rows = cap_problem(d, N=1300)
    lists = filter_lists(np.random.default_rng(d), len(target), embs.size(0), target)
    def off_by_one_float(t):
        buf = torch.empty(t.numel() + 1, dtype=torch.float32, device=DEV)
        out = buf[1:].view(t.shape)
        out.copy_(t)
        assert out.data_ptr() % 16 == 4 and out.is_contiguous()
        return out
    l1_check(model, off_by_one_float(embs), off_by_one_float(rows), embs, rows, target, lists, "both bases unaligned")
    l1_check(model, embs.to(DEV), off_by_one_float(rows), embs, rows, target, lists, "the query rows unaligned")
    l1_check(model, off_by_one_float(embs), rows.to(DEV), embs, rows, target, lists, "the table unaligned")
    for metric in ("l2", "complex"):                                    # the path does not change the bits of the other two
        a = model.topk_by_distance(embs.to(DEV), dev(query), 10, metric, query_rows=rows.to(DEV))
        b = model.topk_by_distance(off_by_one_float(embs), dev(query), 10, metric, query_rows=off_by_one_float(rows))
        assert torch.equal(bits(a[0]), bits(b[0])) and torch.equal(a[1], b[1]), metric


# ---- 3. L2 and the complex modulus on real data: the bracket --------------------------------------------------------------
BRACKET = [(m, d) for m in ("l2", "complex") for d in DIMS if not (m == "complex" and d % 2)]


@gpu
@pytest.mark.parametrize("metric,d", BRACKET, ids=["%s-d%d" % c for c in BRACKET])
def test_l2_and_complex_on_real_data_stay_inside_the_bracket(model, metric, d):
    embs, query, target, rows = cap_problem(d)
    N, B = embs.size(0), len(target)
    D = S.distances(metric, rows, embs)
    E = S.eps(D, d)
    lists = filter_lists(np.random.default_rng(d), B, N, target)
    e_d, r_d, q_d, t_d = embs.to(DEV), rows.to(DEV), dev(query), dev(target)
    for ls, kw in ((None, {}), (lists, lists_dev(lists))):
        g, e = model.rank_by_distance(e_d, q_d, t_d, metric, query_rows=r_d, **kw)
        check_rank_bracket(g, e, -D, E, target, ls, f"{metric} d={d} filtered={ls is not None}")
        for k in (10, 128):
            sc, ids = model.topk_by_distance(e_d, q_d, k, metric, query_rows=r_d, **kw)
            check_topk_bracket(sc, ids, -D, E, k, ls, f"{metric} d={d} top-{k} filtered={ls is not None}")


# ---- 4. consistency with the per-query path ---------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("metric", R.METRICS)
def test_a_shared_set_equals_the_per_query_call_on_exact_data(model, metric):
    N, B, d = 2600, TQ + 1, 64
    c = S.exact_rows(N, d, seed=9, metric=metric)
    rng = np.random.default_rng(9)
    query, target = rng.integers(0, N, B), rng.integers(0, N, B)
    P = np.unique(np.concatenate([rng.integers(0, N, 700), np.arange(20), np.arange(N - 500, N - 480)]))
    target[:10] = P[:10]                                                # targets inside the set, the others mostly outside
    lists = filter_lists(rng, B, N, target, big=False)
    embs, qd, td, kw = dev(c), dev(query), dev(target), lists_dev(lists)
    a = model.rank_by_distance(embs, qd, td, metric, candidates=dev(P), **kw)
    b = model.rank_candidates(embs, qd, td, negatives=dev(P).unsqueeze(0).expand(B, -1).contiguous(), distance=metric, **kw)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert np.array_equal(np_of(a), S.rank(S.distances(metric, c[query], c), target, lists, P))


# ---- 5. subset semantics ---------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("metric", R.METRICS)
@pytest.mark.parametrize("C", [CT - 1, CT + 1, SLAB + 300])
def test_candidates_equal_the_call_on_a_contiguous_copy(model, metric, C):
    d = 64
    embs, query, target, rows = cap_problem(d)
    N, B = embs.size(0), len(target)
    rng = np.random.default_rng(C)
    P = np.unique(np.append(rng.permutation(N - 1)[:C - 1], N - 1))     # the table's last row is a candidate
    assert len(P) == C
    inside = P[rng.integers(0, C, B)]
    lists = filter_lists(rng, B, N, inside, big=False)
    pos = {int(v): j for j, v in enumerate(P)}
    lists_sub = [np.asarray([pos[int(v)] for v in l if int(v) in pos], dtype=np.int64) for l in lists]
    assert sum(len(l) for l in lists_sub) < sum(len(l) for l in lists), "some listed ids are outside the set"
    e_d, r_d, q_d = embs.to(DEV), rows.to(DEV), dev(query)
    sub = embs[torch.from_numpy(P)].contiguous().to(DEV)
    zeros = dev(np.zeros(B, dtype=np.int64))
    # rank: targets inside the set, renumbered for the copy
    a = model.rank_by_distance(e_d, q_d, dev(inside), metric, query_rows=r_d, candidates=dev(P), **lists_dev(lists))
    b = model.rank_by_distance(sub, zeros, dev(np.asarray([pos[int(v)] for v in inside])), metric, query_rows=r_d, **lists_dev(lists_sub))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    mask = torch.zeros(N, dtype=torch.bool)
    mask[torch.from_numpy(P)] = True
    for form in (mask, mask.to(DEV), dev(P[::-1].copy()), torch.from_numpy(P).to(torch.int32)):     # a mask, any order
        a2 = model.rank_by_distance(e_d, q_d, dev(inside), metric, query_rows=r_d, candidates=form, **lists_dev(lists))
        assert torch.equal(a[0], a2[0]) and torch.equal(a[1], a2[1])
    # top-k: bit for bit, ids back in node space
    for k in (10, 128):
        sa, ia = model.topk_by_distance(e_d, q_d, k, metric, query_rows=r_d, candidates=mask, **lists_dev(lists))
        sb, ib = model.topk_by_distance(sub, zeros, k, metric, query_rows=r_d, **lists_dev(lists_sub))
        Pd = dev(P)
        assert torch.equal(bits(sa), bits(sb)) and torch.equal(ia, torch.where(ib >= 0, Pd[ib.clamp(min=0)], ib))
    # a target outside the set: compared, never counted
    outside = np.setdiff1d(np.arange(N), P)[rng.integers(0, N - C, B)]
    g, e = model.rank_by_distance(e_d, q_d, dev(outside), metric, query_rows=r_d, candidates=dev(P), **lists_dev(lists))
    D = S.distances(metric, rows, embs)
    if metric == "l1":
        D = S.l1_chain32(rows.numpy(), embs.numpy()).astype(np.float64)
        assert np.array_equal(np_of((g, e)), S.rank(D, outside, lists, P))
    else:
        lo, hi = np.zeros(B, dtype=np.int64), np.zeros(B, dtype=np.int64)
        E = S.eps(D, d)
        for i in range(B):
            m = S.allowed(N, lists, i, outside, P)
            t, et = D[i, outside[i]], E[i, outside[i]]
            lo[i], hi[i] = np.count_nonzero(D[i][m] < t - E[i][m] - et), np.count_nonzero(D[i][m] <= t + E[i][m] + et)
        gn, en = np_of((g, e))
        assert (gn >= lo).all() and (gn + en <= hi).all()


# ---- 6. lists, typed queries, zero distance -------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("metric", R.METRICS)
def test_typed_known_edges_and_query_rel(model, metric):
    d = 64
    embs, query, target, rows = cap_problem(d, N=1300)
    N, B = embs.size(0), len(target)
    rng = np.random.default_rng(4)
    nrel = 3
    qrel = rng.integers(0, nrel, B)
    src = np.concatenate([query, query, rng.integers(0, N, 200)])
    dst = rng.integers(0, N, len(src))
    rel = np.concatenate([qrel, rng.integers(0, nrel, B), rng.integers(0, nrel, 200)])
    lists = [np.unique(dst[(src == query[i]) & (rel == qrel[i])]) for i in range(B)]
    assert all(len(l) for l in lists)
    e_d, r_d, q_d, t_d = embs.to(DEV), rows.to(DEV), dev(query), dev(target)
    known = (dev(src), dev(dst), dev(rel))
    a = model.rank_by_distance(e_d, q_d, t_d, metric, query_rows=r_d, known=known, query_rel=dev(qrel))
    b = model.rank_by_distance(e_d, q_d, t_d, metric, query_rows=r_d, **lists_dev(lists))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    sa, ia = model.topk_by_distance(e_d, q_d, 10, metric, query_rows=r_d, known=known, query_rel=dev(qrel))
    sb, ib = model.topk_by_distance(e_d, q_d, 10, metric, query_rows=r_d, **lists_dev(lists))
    assert torch.equal(bits(sa), bits(sb)) and torch.equal(ia, ib)
    for i in range(B):
        assert not np.isin(ia[i].cpu().numpy(), lists[i]).any()
    # untyped known=(src, dst): every dst of the query's edges
    a = model.topk_by_distance(e_d, q_d, 10, metric, known=(dev(src), dev(dst)))
    lists2 = [np.unique(dst[src == query[i]]) for i in range(B)]
    b = model.topk_by_distance(e_d, q_d, 10, metric, **lists_dev(lists2))
    assert torch.equal(bits(a[0]), bits(b[0])) and torch.equal(a[1], b[1])


@gpu
@pytest.mark.parametrize("metric", R.METRICS)
def test_distance_zero_the_query_itself_and_a_bit_identical_twin(model, metric):
    d, N, B = 64, 1300, TQ + 1
    embs = cap_problem(d, N=N)[0].clone()
    rng = np.random.default_rng(8)
    query = rng.permutation(np.arange(100, N - 100, 3))[:B]              # ids = 1 mod 3: no twin (0 or 2 mod 3) is a query
    twin_lo, twin_hi = query[:20] - 50, query[20:40] + 50                # a twin below the query's id, a twin above
    embs[torch.from_numpy(twin_lo)] = embs[torch.from_numpy(query[:20])]
    embs[torch.from_numpy(twin_hi)] = embs[torch.from_numpy(query[20:40])]
    e_d, q_d = embs.to(DEV), dev(query)
    sc, ids = model.topk_by_distance(e_d, q_d, 2, metric)
    sc, ids = sc.cpu().numpy(), ids.cpu().numpy()
    assert (sc[:, 0] == 0).all() and not np.signbit(sc[:, 0]).any()      # the query's own node: distance exactly +0
    assert np.array_equal(ids[:20], np.stack([twin_lo, query[:20]], 1)) and (sc[:20] == 0).all()
    assert np.array_equal(ids[20:40], np.stack([query[20:40], twin_hi], 1)) and (sc[20:40] == 0).all()
    assert np.array_equal(ids[40:, 0], query[40:]) and (sc[40:, 1] < 0).all()
    # the twin as the target: nothing is nearer, the query's own node ties with it
    g, e = model.rank_by_distance(e_d, q_d[:20], dev(twin_lo), metric)
    assert (g == 0).all() and (e == 1).all()
    g, e = model.rank_by_distance(e_d, q_d[:20], dev(twin_lo), metric, filt_ptr=dev(np.arange(21)), filt_idx=q_d[:20])
    assert (g == 0).all() and (e == 0).all()                             # ... unless it is listed


# ---- 7. k and invalid ids --------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("metric", R.METRICS)
def test_invalid_ids_make_their_query_alone_invalid_without_a_fault(metric):
    d, N, B = 64, 1300, TQ + 1
    embs, query, target, rows = cap_problem(d, N=N, B=B)
    M = METRIC[metric]
    e_d = embs.to(DEV)
    lists = [np.sort(np.random.default_rng(i).integers(0, N, 4)) for i in range(B)]
    kw = lists_dev(lists)
    good = _native.score_dist_sweep_rank(M, e_d, e_d, dev(target), iq=dev(query), **kw)
    good_k = _native.score_dist_sweep_topk(M, e_d, e_d, 128, iq=dev(query), **kw)
    P = dev(np.arange(0, N, 2))
    good_s = _native.score_dist_sweep_rank(M, e_d, e_d, dev(target), iq=dev(query), ic=P, **kw)
    big = 1 << 40
    for what, bad_q, bad_t, bad_l in (("iq", {0: -1, 5: N, 64: big}, {}, {}), ("target", {}, {1: -1, 63: N, 64: -big}, {}),
                                      ("lists", {}, {}, {2: -1, 64: N, 7: big})):
        q, t = query.copy(), target.copy()
        ls = [l.copy() for l in lists]
        for i, v in bad_q.items():
            q[i] = v
        for i, v in bad_t.items():
            t[i] = v
        for i, v in bad_l.items():
            ls[i][-1 if v > 0 else 0] = v                                # still ascending
        hit = sorted(set(bad_q) | set(bad_t) | set(bad_l))
        rest = np.setdiff1d(np.arange(B), hit)
        for ic, ref in ((None, good), (P, good_s)):
            g, e = _native.score_dist_sweep_rank(M, e_d, e_d, dev(t), iq=dev(q), ic=ic, **lists_dev(ls))
            assert (g[hit] == -1).all() and (e[hit] == -1).all(), f"{what}: the bad queries"
            assert torch.equal(g[rest], ref[0][rest]) and torch.equal(e[rest], ref[1][rest]), f"{what}: the others"
        if what != "target":
            sc, ids = _native.score_dist_sweep_topk(M, e_d, e_d, 128, iq=dev(q), **lists_dev(ls))
            assert torch.isnan(sc[hit]).all() and (ids[hit] == -1).all(), what
            assert torch.equal(bits(sc[rest]), bits(good_k[0][rest])) and torch.equal(ids[rest], good_k[1][rest]), what
    for what, ic in (("not ascending", np.array([3, 2, 9])), ("repeated", np.array([2, 2, 9])), ("out of range", np.array([2, 9, N])),
                     ("negative", np.array([-1, 2, 9])), ("far out of range", np.array([2, 9, big]))):
        g, e = _native.score_dist_sweep_rank(M, e_d, e_d, dev(target), iq=dev(query), ic=dev(ic), **kw)
        assert (g == -1).all() and (e == -1).all(), f"a bad ic ({what}) makes every query invalid"
        sc, ids = _native.score_dist_sweep_topk(M, e_d, e_d, 3, iq=dev(query), ic=dev(ic), **kw)
        assert torch.isnan(sc).all() and (ids == -1).all(), what
    torch.cuda.synchronize()


@gpu
@pytest.mark.parametrize("metric", R.METRICS)
def test_k_of_1_and_128_and_fewer_than_k_left(model, metric):
    d = 6
    embs, query, target, rows = cap_problem(d, N=SLAB + 1, B=5)
    N = embs.size(0)
    D = S.distances(metric, rows, embs) if metric != "l1" else S.l1_chain32(rows.numpy(), embs.numpy()).astype(np.float64)
    E = S.eps(D, d)
    e_d, r_d, q_d = embs.to(DEV), rows.to(DEV), dev(query)
    lists = [np.setdiff1d(np.arange(N), [3, N - 1, 400 + i]) for i in range(5)]               # three candidates left
    lists[4] = np.arange(N)                                                                   # none
    for k in (1, 128):
        sc, ids = model.topk_by_distance(e_d, q_d, k, metric, query_rows=r_d)
        check_topk_bracket(sc, ids, -D, E, k, None, f"{metric} k={k}")
        sc, ids = model.topk_by_distance(e_d, q_d, k, metric, query_rows=r_d, **lists_dev(lists))
        check_topk_bracket(sc, ids, -D, E, k, lists, f"{metric} k={k}, three left")
        assert (ids[4] == -1).all() and torch.isneginf(sc[4]).all()
    assert set(ids[0, :3].tolist()) == {3, N - 1, 400} and (ids[0, 3:] == -1).all()
    for k in (0, 129):
        with pytest.raises(ValueError, match="outside 1..128"):
            _native.score_dist_sweep_topk(METRIC[metric], r_d, e_d, k)
    with pytest.raises(ValueError, match="workspace of 16 bytes"):
        _native.score_dist_sweep_topk(METRIC[metric], r_d, e_d, 3, workspace=torch.zeros(16, dtype=torch.uint8, device=DEV))


# ---- 8. reproducibility ----------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("metric", R.METRICS)
def test_same_bits_twice_and_alone_as_in_the_batch(model, metric):
    d = 130 if metric != "complex" else 64
    embs, query, target, rows = cap_problem(d, B=2 * TQ + 3)
    N, B = embs.size(0), len(target)
    lists = filter_lists(np.random.default_rng(1), B, N, target, big=False)
    e_d, r_d, q_d, t_d, kw = embs.to(DEV), rows.to(DEV), dev(query), dev(target), lists_dev(lists)
    P = dev(np.arange(1, N, 3))
    for cand in (None, P):
        a = model.rank_by_distance(e_d, q_d, t_d, metric, query_rows=r_d, candidates=cand, **kw)
        b = model.rank_by_distance(e_d, q_d, t_d, metric, query_rows=r_d, candidates=cand, **kw)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        sa = model.topk_by_distance(e_d, q_d, 128, metric, query_rows=r_d, candidates=cand, **kw)
        sb = model.topk_by_distance(e_d, q_d, 128, metric, query_rows=r_d, candidates=cand, **kw)
        assert torch.equal(bits(sa[0]), bits(sb[0])) and torch.equal(sa[1], sb[1])
        for i in (0, TQ - 1, TQ, B - 1):
            one = lists_dev([lists[i]])
            g, e = model.rank_by_distance(e_d, q_d[i:i + 1], t_d[i:i + 1], metric, query_rows=r_d[i:i + 1].contiguous(), candidates=cand,
                                          **one)
            assert int(g) == int(a[0][i]) and int(e) == int(a[1][i]), f"query {i} alone"
            sc, ids = model.topk_by_distance(e_d, q_d[i:i + 1], 128, metric, query_rows=r_d[i:i + 1].contiguous(), candidates=cand, **one)
            assert torch.equal(bits(sc[0]), bits(sa[0][i])) and torch.equal(ids[0], sa[1][i]), f"query {i} alone"
