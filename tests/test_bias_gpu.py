"""``candidate_bias=`` of rank_candidates / topk_candidates / softmax_loss / bce_loss (the ghf_score_*_b calls, the BIAS
instantiations of csrc/rank_sweep.h and csrc/softmax.hip) against the float64 restatement of the contract
(tests/_bias_ref.py), against today's entry points run on the extra-column copies ``[c | b]``, ``[q | 1]`` (bit for bit), and
against the call without the keyword (a bias of zeros, bit for bit).

The shapes are test_candidates_gpu's CASES: all-node calls take their N, subset calls their (N, C).  Tolerances are the
project's own, unchanged: losses under tests/_util.assert_close's defaults, gradients (dq, dc and db) under grad_check's rule
(rtol 2e-4, atol 1e-4 * max|want|, relative L2 < 5e-5).  Ranks and top-k run on exact data — rows in multiples of 1/64, the
bias in multiples of 1/64 in [-32, 32]: every s + b is a multiple of 2^-12 below 2^12, exact in fp32 — and are compared for
equality, ties included."""

import numpy as np
import pytest
import torch

import _bias_ref as ref
from graph_hypernetwork_forge_amd import HyperGNN, ToyKnowledgeGraph, _native
from test_candidates_gpu import CASES, IDS, csr, dev, exact_rows, grad_check, layernorm_rows, loss_check, model16, problem

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SUBSET = (False, True)
SUBSET_IDS = ("all-nodes", "candidates")


def normal_bias(N, seed):
    return torch.randn(N, device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed))


def weights(B, seed):
    return torch.randn(B, device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed))


# ---- 1. exact data: rank counts, top-k ids and scores equal the restatement ------------------------------------------------
@pytest.mark.parametrize("subset", SUBSET, ids=SUBSET_IDS)
@pytest.mark.parametrize("N,C,B,d", CASES, ids=IDS)
def test_rank_and_topk_with_a_bias_are_exact(N, C, B, d, subset):
    P, query, t_in, t_any, lists = problem(N, C, B, 1000 + d)
    c, b = exact_rows(N, d, seed=d), ref.exact_bias(N, seed=100 + d)
    e, bias, q = dev(c), dev(b), dev(query)
    ic, Pn = (dev(P), P) if subset else (None, None)
    ptr, idx = csr(lists)
    k = 10
    greater, equal = _native.score_rank(e, e, dev(t_any), iq=q, filt_ptr=ptr, filt_idx=idx, ic=ic, bias=bias)
    want_g, want_e = ref.rank(c[query], c, b, t_any, lists, Pn)
    assert np.array_equal(greater.cpu().numpy(), want_g) and np.array_equal(equal.cpu().numpy(), want_e)
    scores, ids = _native.score_topk(e, e, k, iq=q, filt_ptr=ptr, filt_idx=idx, ic=ic, bias=bias)
    want_s, want_i = ref.topk(c[query], c, b, lists, Pn, k)
    assert np.array_equal(ids.cpu().numpy(), want_i), "top-k ids (node ids, ties to the lower id)"
    assert np.array_equal(scores.cpu().numpy().astype(np.float64), want_s), "top-k returns the biased scores"
    # the bias matters on this data: without it the lists are others (where there is more than one candidate to order)
    if (C if subset else N) > k:
        _, plain = _native.score_topk(e, e, k, iq=q, filt_ptr=ptr, filt_idx=idx, ic=ic)
        assert bool((plain != ids).any(1).all()), "the bias changes the top-10 of every query"


# ---- 2. the extra-column formulation, bit for bit ---------------------------------------------------------------------------
@pytest.mark.parametrize("subset", SUBSET, ids=SUBSET_IDS)
@pytest.mark.parametrize("N,C,B,d", [x for x in CASES if x[3] <= 128], ids=[i for i, x in zip(IDS, CASES) if x[3] <= 128])
def test_rank_and_topk_equal_the_entry_points_without_a_bias_on_an_extra_column(N, C, B, d, subset):
    """[c | b] . [q | 1] continues the chain by fmaf(1, b_j, s) = fl(s + b_j): the contract's single add.  At d = 128 the copy
    (width 129) runs on the other kernel shape, so the result does not depend on the tiling either."""
    P, query, t_in, t_any, lists = problem(N, C, B, 1500 + d)
    embs, bias = layernorm_rows(N, d, seed=d), normal_bias(N, 200 + d)
    cb = torch.cat([embs, bias[:, None]], 1).contiguous()
    q1 = torch.cat([embs, torch.ones(N, 1, device=DEV)], 1).contiguous()
    q, t = dev(query), dev(t_any)
    ic = dev(P) if subset else None
    ptr, idx = csr(lists)
    kw = dict(iq=q, filt_ptr=ptr, filt_idx=idx, ic=ic)
    g0, e0 = _native.score_rank(q1, cb, t, **kw)
    g1, e1 = _native.score_rank(embs, embs, t, bias=bias, **kw)
    assert torch.equal(g0, g1) and torch.equal(e0, e1)
    s0, i0 = _native.score_topk(q1, cb, 16, **kw)
    s1, i1 = _native.score_topk(embs, embs, 16, bias=bias, **kw)
    assert torch.equal(i0, i1) and torch.equal(s0.view(torch.int32), s1.view(torch.int32))


# ---- 3. the two losses and the three gradients against float64 --------------------------------------------------------------
@pytest.mark.parametrize("subset", SUBSET, ids=SUBSET_IDS)
@pytest.mark.parametrize("N,C,B,d", CASES, ids=IDS)
def test_losses_and_gradients_with_a_bias_match_float64(N, C, B, d, subset):
    P, query, t_in, _, lists = problem(N, C, B, 2000 + d)
    embs, bias = layernorm_rows(N, d, seed=d), normal_bias(N, 300 + d)
    c, b = embs.cpu().numpy(), bias.cpu().numpy()
    ic, Pn, M = (dev(P), P, C) if subset else (None, None, N)
    rows = P if subset else np.arange(N)
    q, t = dev(query), dev(t_in)
    ptr, idx = csr(lists)
    g = weights(B, d)
    gn = g.cpu().numpy()
    scale, smoothing = d ** -0.5, 0.1

    want, want_lse, dq64, dc64, db64 = ref.softmax(c[query], c, b, t_in, lists, Pn, scale, grad=gn)
    loss, lse = _native.score_softmax_fwd(embs, embs, t, iq=q, filt_ptr=ptr, filt_idx=idx, scale=scale, ic=ic, bias=bias)
    loss_check("softmax loss", loss, want)
    loss_check("softmax lse", lse, want_lse)
    dq, dc, db = _native.score_softmax_bwd(embs, embs, t, lse, g, iq=q, filt_ptr=ptr, filt_idx=idx, scale=scale, ic=ic, bias=bias)
    assert dc.shape == (M, d) and db.shape == (M,)
    if M == 1:
        # the only candidate is the target: p = 1 and every gradient is identically zero in float64, so a bound relative to
        # it says nothing; the bound of test_candidates_gpu's C = 1 case stands in
        assert not dq64.any() and not dc64.any() and not db64.any()
        assert float(dq.abs().max()) <= 1e-5 and float(dc.abs().max()) <= 1e-5 and float(db.abs().max()) <= 1e-5
    else:
        grad_check("q (softmax)", dq, dq64)
        grad_check("c (softmax)", dc, dc64[rows])
        grad_check("b (softmax)", db, db64[rows])
    dq2, dc2, none = _native.score_softmax_bwd(embs, embs, t, lse, g, iq=q, filt_ptr=ptr, filt_idx=idx, scale=scale, ic=ic, bias=bias,
                                               want_db=False)
    assert none is None and torch.equal(dq, dq2) and torch.equal(dc, dc2), "db = NULL changes nothing else"

    want, dq64, dc64, db64 = ref.bce(c[query], c, b, lists, Pn, scale, smoothing, grad=gn)
    loss = _native.score_bce_fwd(embs, embs, iq=q, pos_ptr=ptr, pos_idx=idx, scale=scale, smoothing=smoothing, ic=ic, bias=bias)
    loss_check("bce loss", loss, want)
    dq, dc, db = _native.score_bce_bwd(embs, embs, loss, g, iq=q, pos_ptr=ptr, pos_idx=idx, scale=scale, smoothing=smoothing, ic=ic,
                                       bias=bias)
    grad_check("q (bce)", dq, dq64)
    grad_check("c (bce)", dc, dc64[rows])
    grad_check("b (bce)", db, db64[rows])


@pytest.mark.parametrize("subset", SUBSET, ids=SUBSET_IDS)
@pytest.mark.parametrize("d", (64, 256))
def test_hub_candidates_that_every_query_lists_with_a_bias(d, subset):
    """test_candidates_gpu's hubs: more listed pairs fall into one candidate tile than the dc sweep keeps in LDS; db comes from
    G after those pairs have been zeroed (softmax) or adjusted (bce)"""
    N, C, B = 1500, 600, 300
    rng = np.random.default_rng(d)
    hubs = np.arange(700, 708)
    P = np.unique(np.concatenate([rng.choice(N, C, replace=False), hubs]))
    embs, bias = layernorm_rows(N, d, seed=70 + d), normal_bias(N, 400 + d)
    c, b = embs.cpu().numpy(), bias.cpu().numpy()
    query = rng.integers(0, N, B)
    target = P[rng.integers(0, len(P), B)]
    target[:20] = 702                                                     # a hub that is some queries' target stays in their sums
    lists = [np.unique(np.concatenate([hubs, rng.integers(0, N, 4)])) for _ in range(B)]
    ptr, idx = csr(lists)
    ic, Pn, rows = (dev(P), P, P) if subset else (None, None, np.arange(N))
    q, t = dev(query), dev(target)
    g = weights(B, d)
    scale = d ** -0.5
    want, _, dq64, dc64, db64 = ref.softmax(c[query], c, b, target, lists, Pn, scale, grad=g.cpu().numpy())
    loss, lse = _native.score_softmax_fwd(embs, embs, t, iq=q, filt_ptr=ptr, filt_idx=idx, scale=scale, ic=ic, bias=bias)
    loss_check(f"hub lists d={d}: softmax", loss, want)
    dq, dc, db = _native.score_softmax_bwd(embs, embs, t, lse, g, iq=q, filt_ptr=ptr, filt_idx=idx, scale=scale, ic=ic, bias=bias)
    grad_check("q (hubs, softmax)", dq, dq64)
    grad_check("c (hubs, softmax)", dc, dc64[rows])
    grad_check("b (hubs, softmax)", db, db64[rows])
    want, dq64, dc64, db64 = ref.bce(c[query], c, b, lists, Pn, scale, 0.1, grad=g.cpu().numpy())
    loss = _native.score_bce_fwd(embs, embs, iq=q, pos_ptr=ptr, pos_idx=idx, scale=scale, smoothing=0.1, ic=ic, bias=bias)
    loss_check(f"hub lists d={d}: bce", loss, want)
    dq, dc, db = _native.score_bce_bwd(embs, embs, loss, g, iq=q, pos_ptr=ptr, pos_idx=idx, scale=scale, smoothing=0.1, ic=ic, bias=bias)
    grad_check("q (hubs, bce)", dq, dq64)
    grad_check("c (hubs, bce)", dc, dc64[rows])
    grad_check("b (hubs, bce)", db, db64[rows])


@pytest.mark.parametrize("subset", SUBSET, ids=SUBSET_IDS)
def test_typed_known_edges_and_query_rows_with_a_bias(subset):
    N, B, d, R = 900, 140, 64, 5
    rng = np.random.default_rng(8)
    model = model16()
    c, b = exact_rows(N, d, seed=81), ref.exact_bias(N, seed=83)
    embs, bias = dev(c), dev(b)
    rows = exact_rows(B, d, seed=82)                                      # the relation decoder's rows stand in for embs[query]
    Q = dev(rows)
    query, qrel = rng.integers(0, N, B), rng.integers(0, R, B)
    src = np.concatenate([np.repeat(query, 6), rng.integers(0, N, 300)])
    dst, rel = rng.integers(0, N, len(src)), rng.integers(0, R, len(src))
    lists = [np.unique(dst[(src == query[i]) & (rel == qrel[i])]) for i in range(B)]
    P = np.unique(np.concatenate([rng.choice(N, 300, replace=False), dst[:200]])) if subset else np.arange(N)
    Pn = P if subset else None
    target = P[rng.integers(0, len(P), B)]
    kw = dict(known=(dev(src), dev(dst), dev(rel)), query_rel=dev(qrel), query_rows=Q, candidate_bias=bias)
    if subset:
        kw["candidates"] = dev(P)
    greater, equal = model.rank_candidates(embs, dev(query), dev(target), **kw)
    want_g, want_e = ref.rank(rows, c, b, target, lists, Pn)
    assert np.array_equal(greater.cpu().numpy(), want_g) and np.array_equal(equal.cpu().numpy(), want_e)
    scores, ids = model.topk_candidates(embs, dev(query), 12, **kw)
    want_s, want_i = ref.topk(rows, c, b, lists, Pn, 12)
    assert np.array_equal(ids.cpu().numpy(), want_i) and np.array_equal(scores.cpu().numpy().astype(np.float64), want_s)
    w = weights(B, 3)
    for name in ("softmax", "bce"):
        e, r, p = embs.clone().requires_grad_(True), Q.clone().requires_grad_(True), bias.clone().requires_grad_(True)
        kw2 = {**kw, "query_rows": r, "candidate_bias": p}
        if name == "softmax":
            loss = model.softmax_loss(e, dev(query), dev(target), scale=0.05, **kw2)
            want, _, dq64, dc64, db64 = ref.softmax(rows, c, b, target, lists, Pn, 0.05, grad=w.cpu().numpy())
        else:
            loss = model.bce_loss(e, dev(query), scale=0.05, smoothing=0.1, normalize=False, **kw2)
            want, dq64, dc64, db64 = ref.bce(rows, c, b, lists, Pn, 0.05, 0.1, grad=w.cpu().numpy())
        loss_check(f"typed {name}", loss, want)
        (loss * w).sum().backward()
        grad_check(f"rows (typed {name})", r.grad, dq64)
        grad_check(f"embs (typed {name})", e.grad, dc64)
        grad_check(f"bias (typed {name})", p.grad, db64)


# ---- 4. a bias of zeros changes no bit ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("subset", SUBSET, ids=SUBSET_IDS)
@pytest.mark.parametrize("d", (20, 64, 128, 256))
def test_a_zero_bias_returns_the_bits_of_the_call_without_the_keyword(d, subset):
    N, C, B = 700, 257, 150
    P, query, t_in, _, lists = problem(N, C, B, 3000 + d)
    embs = layernorm_rows(N, d, seed=5 + d)
    q, t = dev(query), dev(t_in)
    ptr, idx = csr(lists)
    ic = dev(P) if subset else None
    w = weights(B, d)
    zero = torch.zeros(N, device=DEV)
    raw = []
    for bias in (None, zero):
        kw = dict(iq=q, filt_ptr=ptr, filt_idx=idx, ic=ic, bias=bias)
        loss, lse = _native.score_softmax_fwd(embs, embs, t, scale=0.25, **kw)
        bce = _native.score_bce_fwd(embs, embs, iq=q, pos_ptr=ptr, pos_idx=idx, scale=0.25, smoothing=0.05, ic=ic, bias=bias)
        raw.append(_native.score_rank(embs, embs, t, **kw) + _native.score_topk(embs, embs, 10, **kw) + (loss, lse, bce)
                   + _native.score_softmax_bwd(embs, embs, t, lse, w, scale=0.25, **kw)[:2]
                   + _native.score_bce_bwd(embs, embs, bce, w, iq=q, pos_ptr=ptr, pos_idx=idx, scale=0.25, smoothing=0.05, ic=ic,
                                           bias=bias)[:2])
    names = ("greater", "equal", "top-k scores", "top-k ids", "loss", "lse", "bce", "softmax dq", "softmax dc", "bce dq", "bce dc")
    for a, b, name in zip(raw[0], raw[1], names):
        assert torch.equal(a, b), name
    # and through the model methods, recorded: loss and d embs
    model = model16()
    cand = None if ic is None else ic
    for name in ("softmax", "bce"):
        out = []
        for bias in (None, zero):
            e = embs.clone().requires_grad_(True)
            if name == "softmax":
                loss = model.softmax_loss(e, q, t, scale=0.25, filt_ptr=ptr, filt_idx=idx, candidates=cand, candidate_bias=bias)
            else:
                loss = model.bce_loss(e, q, pos_ptr=ptr, pos_idx=idx, scale=0.25, smoothing=0.05, candidates=cand, candidate_bias=bias)
            (loss * w).sum().backward()
            out.append((loss.detach(), e.grad))
        assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1]), name


# ---- 5. -inf removes a candidate -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("subset", SUBSET, ids=SUBSET_IDS)
@pytest.mark.parametrize("N,C,B,d", [CASES[1], CASES[4], CASES[6]], ids=[IDS[1], IDS[4], IDS[6]])
def test_minus_infinity_takes_a_candidate_out(N, C, B, d, subset):
    P, query, t_in, t_any, lists = problem(N, C, B, 1000 + d)
    c, b = exact_rows(N, d, seed=d), ref.exact_bias(N, seed=100 + d)
    free = np.setdiff1d(P, np.concatenate([t_in, t_any]))                 # candidates that are no query's target
    gone = free[:: max(1, len(free) // 9)][:9]
    assert len(gone) >= 3
    b[gone] = -np.inf
    e, bias, q = dev(c), dev(b), dev(query)
    ic, Pn, rows = (dev(P), P, P) if subset else (None, None, np.arange(N))
    ptr, idx = csr(lists)
    left = np.setdiff1d(rows, gone)                                       # the restatement with those nodes removed
    b0 = np.where(np.isinf(b), 0, b).astype(np.float32)
    greater, equal = _native.score_rank(e, e, dev(t_any), iq=q, filt_ptr=ptr, filt_idx=idx, ic=ic, bias=bias)
    want_g, want_e = ref.rank(c[query], c, b0, t_any, lists, left)
    assert np.array_equal(greater.cpu().numpy(), want_g) and np.array_equal(equal.cpu().numpy(), want_e)
    scores, ids = _native.score_topk(e, e, 10, iq=q, filt_ptr=ptr, filt_idx=idx, ic=ic, bias=bias)
    want_s, want_i = ref.topk(c[query], c, b0, lists, left, 10)
    assert np.array_equal(ids.cpu().numpy(), want_i) and np.array_equal(scores.cpu().numpy().astype(np.float64), want_s)
    assert not np.isin(ids.cpu().numpy(), gone).any()
    # softmax: a zero term, and zero gradients for the node, exactly
    g = weights(B, d)
    scale = 1.0 / 64
    t = dev(t_in)
    want, want_lse, dq64, dc64, db64 = ref.softmax(c[query], c, b0, t_in, lists, left, scale, grad=g.cpu().numpy())
    loss, lse = _native.score_softmax_fwd(e, e, t, iq=q, filt_ptr=ptr, filt_idx=idx, scale=scale, ic=ic, bias=bias)
    loss_check("softmax loss with removed candidates", loss, want)
    dq, dc, db = _native.score_softmax_bwd(e, e, t, lse, g, iq=q, filt_ptr=ptr, filt_idx=idx, scale=scale, ic=ic, bias=bias)
    at = torch.from_numpy(np.searchsorted(rows, gone)).to(DEV)
    assert float(dc[at].abs().max()) == 0.0 and float(db[at].abs().max()) == 0.0
    grad_check("q (removed candidates)", dq, dq64)
    grad_check("c (removed candidates)", dc, dc64[rows])
    grad_check("b (removed candidates)", db, db64[rows])


# ---- 6. where the gradient lands ---------------------------------------------------------------------------------------------
def test_the_bias_gradient_is_zero_outside_the_candidates_repeats_and_does_not_depend_on_the_batch():
    N, C, B, d = 6000, 4500, 300, 128
    P, query, t_in, t_any, lists = problem(N, C, B, 7000)
    model = model16()
    embs, bias = layernorm_rows(N, d, seed=71), normal_bias(N, 72)
    q, t = dev(query), dev(t_any)                                         # half of the targets are no candidates: they are added
    ptr, idx = csr(lists)
    w = weights(B, 7)
    c, b = embs.cpu().numpy(), bias.cpu().numpy()
    for name in ("softmax", "bce"):
        part = np.union1d(P, t_any) if name == "softmax" else P
        rest = torch.ones(N, dtype=torch.bool, device=DEV)
        rest[dev(part)] = False
        assert int(rest.sum()) > 100
        runs = []
        for _ in range(2):
            e, p = embs.clone().requires_grad_(True), bias.clone().requires_grad_(True)
            if name == "softmax":
                loss = model.softmax_loss(e, q, t, scale=d ** -0.5, filt_ptr=ptr, filt_idx=idx, candidates=dev(P), candidate_bias=p)
            else:
                loss = model.bce_loss(e, q, pos_ptr=ptr, pos_idx=idx, scale=d ** -0.5, smoothing=0.1, normalize=False,
                                      candidates=dev(P), candidate_bias=p)
            (loss * w).sum().backward()
            runs.append((loss.detach(), e.grad, p.grad))
        for x, y in zip(*runs):
            assert torch.equal(x, y), f"{name}: two runs differ"
        loss, _, db = runs[0]
        assert db.shape == (N,) and float(db[rest].abs().max()) == 0.0, f"{name}: a node outside the candidates has a bias gradient"
        if name == "softmax":
            want, _, _, _, db64 = ref.softmax(c[query], c, b, t_any, lists, part, d ** -0.5, grad=w.cpu().numpy())
        else:
            want, _, _, db64 = ref.bce(c[query], c, b, lists, part, d ** -0.5, 0.1, grad=w.cpu().numpy())
        loss_check(f"{name} through the model", loss, want)
        grad_check(f"bias ({name}, through the model)", db, db64)
        # the bias alone requires grad: embs is data
        p = bias.clone().requires_grad_(True)
        if name == "softmax":
            l2 = model.softmax_loss(embs, q, t, scale=d ** -0.5, filt_ptr=ptr, filt_idx=idx, candidates=dev(P), candidate_bias=p)
        else:
            l2 = model.bce_loss(embs, q, pos_ptr=ptr, pos_idx=idx, scale=d ** -0.5, smoothing=0.1, normalize=False, candidates=dev(P),
                                candidate_bias=p)
        assert l2.requires_grad and torch.equal(l2.detach(), loss)
        (l2 * w).sum().backward()
        assert torch.equal(p.grad, db) and embs.grad is None
        # one query alone has the bits it has inside the batch of 300 (the same candidate set)
        i = 41
        one = dev(query[i:i + 1])
        p1, i1 = csr(lists[i:i + 1])
        if name == "softmax":
            l1 = model.softmax_loss(embs, one, dev(t_any[i:i + 1]), scale=d ** -0.5, filt_ptr=p1, filt_idx=i1, candidates=dev(part),
                                    candidate_bias=bias)
        else:
            l1 = model.bce_loss(embs, one, pos_ptr=p1, pos_idx=i1, scale=d ** -0.5, smoothing=0.1, normalize=False, candidates=dev(P),
                                candidate_bias=bias)
        assert torch.equal(l1, loss[i:i + 1]), f"{name}: a query's loss depends on the batch it is in"


def test_a_learned_entity_bias_trains_with_the_model_s_parameters():
    kg = ToyKnowledgeGraph(feat_dim=16)
    x, ei = kg.node_features.to(DEV), kg.edge_index.to(DEV)
    torch.manual_seed(0)
    model = HyperGNN(text_dim=64, node_feat_dim=16, hidden_dim=32, num_layers=2).to(DEV)
    N = x.size(0)
    entity_bias = torch.nn.Parameter(torch.zeros(N, device=DEV))
    cand = torch.arange(0, N, 2, device=DEV)
    for name in ("softmax", "bce"):
        model.zero_grad()
        entity_bias.grad = None
        embs = model(x, ei, kg.edge_texts)
        if name == "softmax":
            loss = model.softmax_loss(embs, ei[0], ei[1], scale=32 ** -0.5, known=(ei[0], ei[1]), candidates=cand,
                                      candidate_bias=entity_bias)
            part = torch.cat([cand, ei[1]])
        else:
            loss = model.bce_loss(embs, torch.unique(ei[0]), known=(ei[0], ei[1]), scale=32 ** -0.5, smoothing=0.1, candidates=cand,
                                  candidate_bias=entity_bias)
            part = cand
        assert torch.isfinite(loss).all()
        loss.mean().backward()
        trained = [n for n, p in model.named_parameters() if p.grad is not None and bool((p.grad != 0).any())]
        assert len(trained) >= 10, (name, trained)
        rest = torch.ones(N, dtype=torch.bool, device=DEV)
        rest[part] = False
        assert not bool(entity_bias.grad[rest].any()) and bool(entity_bias.grad[~rest].any())


# ---- 7. bad input at the native level ------------------------------------------------------------------------------------------
def test_a_bad_candidate_list_with_a_bias_makes_every_query_invalid_and_db_zero():
    N, C, B, d = 700, 257, 129, 64
    P, query, t_in, _, lists = problem(N, C, B, 8000)
    bad = P.copy()
    bad[-1] = N                                                           # out of range: its bias entry must not be read either
    bad[100] = bad[99]
    embs, bias = layernorm_rows(N, d, seed=81), normal_bias(N, 82)
    before, bias_before = embs.clone(), bias.clone()
    ic, q, t = dev(bad), dev(query), dev(t_in)
    ptr, idx = csr(lists)
    kw = dict(iq=q, filt_ptr=ptr, filt_idx=idx, ic=ic, bias=bias)
    greater, equal = _native.score_rank(embs, embs, t, **kw)
    assert (greater == -1).all() and (equal == -1).all()
    scores, ids = _native.score_topk(embs, embs, 5, **kw)
    assert torch.isnan(scores).all() and (ids == -1).all()
    loss, lse = _native.score_softmax_fwd(embs, embs, t, scale=0.5, **kw)
    assert torch.isnan(loss).all() and torch.isnan(lse).all()
    bce = _native.score_bce_fwd(embs, embs, iq=q, pos_ptr=ptr, pos_idx=idx, scale=0.5, smoothing=0.1, ic=ic, bias=bias)
    assert torch.isnan(bce).all()
    g, fine = torch.ones(B, device=DEV), torch.zeros(B, device=DEV)
    for dq, dc, db in (_native.score_softmax_bwd(embs, embs, t, fine, g, scale=0.5, **kw),
                       _native.score_bce_bwd(embs, embs, fine, g, iq=q, pos_ptr=ptr, pos_idx=idx, scale=0.5, smoothing=0.1, ic=ic,
                                             bias=bias)):
        assert dc.shape == (C, d) and db.shape == (C,)
        assert not bool(dq.any()) and not bool(dc.any()) and not bool(db.any())
    torch.cuda.synchronize()
    assert torch.equal(embs, before) and torch.equal(bias, bias_before)


@pytest.mark.parametrize("subset", SUBSET, ids=SUBSET_IDS)
def test_an_id_out_of_range_with_a_bias_makes_only_its_own_query_invalid(subset):
    N, C, B, d = 700, 257, 129, 64
    P, query, t_in, _, lists = problem(N, C, B, 8500)
    embs, bias = layernorm_rows(N, d, seed=85), normal_bias(N, 86)
    c, b = embs.cpu().numpy(), bias.cpu().numpy()
    target = t_in.copy()
    target[17] = N + 5                                                    # a target out of range
    lists = [l.copy() for l in lists]
    lists[60] = np.sort(np.append(lists[60], N + 9))                      # a listed id out of range
    ok = np.ones(B, dtype=bool)
    ok[[17, 60]] = False
    okd = dev(ok)
    ic, Pn = (dev(P), P) if subset else (None, None)
    q, t = dev(query), dev(target)
    ptr, idx = csr(lists)
    kw = dict(iq=q, filt_ptr=ptr, filt_idx=idx, ic=ic, bias=bias)
    clean = [l[l < N] for l in lists]
    safe_t = np.where(target < N, target, t_in)
    greater, equal = _native.score_rank(embs, embs, t, **kw)
    assert (greater[~okd] == -1).all() and (equal[~okd] == -1).all() and (greater[okd] >= 0).all()
    scores, ids = _native.score_topk(embs, embs, 5, **kw)
    assert torch.isnan(scores[60]).all() and (ids[60] == -1).all() and torch.isfinite(scores[17]).all()
    loss, lse = _native.score_softmax_fwd(embs, embs, t, scale=0.125, **kw)
    assert torch.isnan(loss[~okd]).all() and torch.isnan(lse[~okd]).all()
    want, _ = ref.softmax(c[query], c, b, safe_t, clean, Pn, 0.125)
    loss_check("the other queries (softmax)", loss[okd], want[ok])
    bce = _native.score_bce_fwd(embs, embs, iq=q, pos_ptr=ptr, pos_idx=idx, scale=0.125, smoothing=0.1, ic=ic, bias=bias)
    assert torch.isnan(bce[60]) and torch.isfinite(bce[17])
    want = ref.bce(c[query], c, b, clean, Pn, 0.125, 0.1)
    ok_b = np.ones(B, dtype=bool)
    ok_b[60] = False
    loss_check("the other queries (bce)", bce[dev(ok_b)], want[ok_b])
    g = torch.ones(B, device=DEV)
    dq, dc, db = _native.score_softmax_bwd(embs, embs, t, lse, g, scale=0.125, **kw)
    assert float(dq[17].abs().max()) == 0.0 and float(dq[60].abs().max()) == 0.0
    assert torch.isfinite(dq).all() and torch.isfinite(dc).all() and torch.isfinite(db).all() and bool(db.any())
