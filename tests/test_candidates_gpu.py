"""``candidates=`` of rank_candidates / topk_candidates / softmax_loss / bce_loss (the ghf_score_*_sub calls,
csrc/candidates.hip) against the float64 restatement of the sub-table rule (tests/_candidates_ref.py), against
the all-node entry points run on a contiguous copy ``embs[ic]`` with hand-renumbered ids (bit for bit), and against the call
without the keyword (``candidates = arange(N)``, bit for bit).

Tolerances are the project's own, unchanged: losses under tests/_util.assert_close's defaults, gradients under the rule of
test_softmax_gpu.grad_check (rtol 2e-4, atol 1e-4 * max|want|, relative L2 < 5e-5), restated below.  Ranks and top-k run on
small-integer rows whose fp32 sums are exact, and are compared for equality, ties included."""

import functools

import numpy as np
import pytest
import torch

import _candidates_ref as ref
from _util import assert_close
from graph_hypernetwork_forge_amd import HyperGNN, ToyKnowledgeGraph, _native

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

# (N, C, B, d): row widths 20 (unaligned rows) / 64 / 128 / 256, C at 1 and around the candidate step (256 for d <= 128, 128
# above), B at 1 and around the query tile (128), C = 4,500 (two dq slabs of the backward) and C = 33,000 at d = 64 (more
# than 128 step tiles: forward slabs of more than one tile)
CASES = [(700, 257, 129, 20), (700, 255, 300, 64), (700, 256, 1, 64), (700, 1, 129, 64), (700, 257, 129, 128),
         (500, 127, 129, 256), (500, 129, 300, 256), (6000, 4500, 129, 128), (40000, 33000, 300, 64)]
IDS = [f"N{n}-C{c}-B{b}-d{d}" for n, c, b, d in CASES]


def grad_check(name, got, want, rtol=2e-4, l2=5e-5):
    gw, gg = np.asarray(want, dtype=np.float64), got.detach().cpu().numpy().astype(np.float64)
    assert gg.shape == gw.shape, f"d{name}: shape {gg.shape} vs {gw.shape}"
    assert np.isfinite(gg).all(), f"d{name}: non-finite values"
    scale = float(np.abs(gw).max())
    rel_l2 = np.linalg.norm(gg - gw) / max(np.linalg.norm(gw), 1e-30)
    print(f"d{name}: max abs err {np.abs(gg - gw).max():.3e} at scale {scale:.3e}, relative L2 {rel_l2:.3e}")
    assert np.allclose(gg, gw, rtol=rtol, atol=1e-4 * max(scale, 1e-30)), \
        f"d{name}: max abs err {np.abs(gg - gw).max():.3e} at scale {scale:.3e}"
    assert rel_l2 < l2, f"d{name}: relative L2 {rel_l2:.3e}"


def loss_check(what, got, want):
    got = got.detach().cpu().numpy()
    err = np.abs(got.astype(np.float64) - want)
    print(f"{what}: max abs err {err.max():.3e}, worst err / bound {np.max(err / (1e-5 + 1e-4 * np.abs(want))):.3e}")
    assert_close(got, want, what)


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                         # a copy: the shared problems are read-only


def csr(lists):
    ptr = np.zeros(len(lists) + 1, dtype=np.int64)
    ptr[1:] = np.cumsum([len(l) for l in lists])
    idx = np.concatenate([np.asarray(l, dtype=np.int64) for l in lists]) if ptr[-1] else np.zeros(0, dtype=np.int64)
    return dev(ptr), dev(idx)


def exact_rows(N, d, seed):
    """multiples of 1/64 in [-4, 4]: every fp32 dot product of two rows is exact; copies make ties"""
    g = np.random.default_rng(seed).standard_normal((N, d))
    c = np.clip(np.round(64 * g) / 64, -4, 4).astype(np.float32)
    k = min(500, N // 3)
    c[-k:] = c[:k]
    return c


def layernorm_rows(N, d, seed):
    """LayerNorm-shaped rows (what the model's last layer emits)"""
    gen = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(N, d, device=DEV, generator=gen)
    gamma = 1.0 + 0.1 * torch.randn(d, device=DEV, generator=gen)
    beta = 0.1 * torch.randn(d, device=DEV, generator=gen)
    return torch.nn.functional.layer_norm(x, (d,), gamma, beta).contiguous()


def model16():
    return HyperGNN(text_dim=32, node_feat_dim=16, hidden_dim=16).to(DEV)


@functools.lru_cache(maxsize=None)
def problem(N, C, B, seed):
    """Candidates P (sorted), queries with repeats, targets inside P that several queries share, targets anywhere, and
    lists over ALL nodes: entries outside P, the target, a repeated id, or nothing.  Shared between the tests: read only."""
    rng = np.random.default_rng(seed)
    P = np.sort(rng.choice(N, C, replace=False)) if C < N else np.arange(N)
    query = rng.integers(0, N, B)
    query[B // 2:B // 2 + 5] = query[:5]
    t_in = P[rng.integers(0, C, B)]
    t_in[10:20] = t_in[0]
    t_any = rng.integers(0, N, B)
    t_any[::2] = t_in[::2]
    lists = []
    for i in range(B):
        l = np.unique(np.concatenate([rng.integers(0, N, 6), P[rng.integers(0, C, 6)]])) if i % 7 else np.zeros(0, dtype=np.int64)
        if i % 3 == 0 and len(l):
            l = np.unique(np.concatenate([l, [t_in[i], t_any[i]]]))       # the target is listed: it stays
        if i % 5 == 1 and len(l):
            l = np.sort(np.append(l, l[len(l) // 2]))                       # an id twice
        lists.append(l)
    for a in (P, query, t_in, t_any):
        a.setflags(write=False)
    return P, query, t_in, t_any, lists


def copy_problem(P, N, lists, target):
    """the hand work the keyword replaces: lists and targets renumbered for the all-node call on the copy embs[P]"""
    new_lists, new_target = ref.renumber(lists, target, P, N)
    return csr(new_lists), dev(new_target)


# ---- 1 + 3. ranks and top-k: exact data, the float64 restatement and the contiguous copy ----------------------------------
@pytest.mark.parametrize("N,C,B,d", CASES, ids=IDS)
def test_rank_and_topk_are_exact_and_equal_the_copy(N, C, B, d):
    P, query, t_in, t_any, lists = problem(N, C, B, 1000 + d)
    c = exact_rows(N, d, seed=d)
    e, ic, q = dev(c), dev(P), dev(query)
    ptr, idx = csr(lists)
    k = 16
    # targets anywhere (half of them outside P): counts over P minus list minus target
    greater, equal = _native.score_rank(e, e, dev(t_any), iq=q, filt_ptr=ptr, filt_idx=idx, ic=ic)
    want_g, want_e = ref.rank(c[query], c, t_any, lists, P)
    assert np.array_equal(greater.cpu().numpy(), want_g) and np.array_equal(equal.cpu().numpy(), want_e)
    if C < N and B > 1:
        assert not np.isin(t_any, P).all()
    scores, ids = _native.score_topk(e, e, k, iq=q, filt_ptr=ptr, filt_idx=idx, ic=ic)
    want_s, want_i = ref.topk(c[query], c, lists, P, k)
    assert np.array_equal(ids.cpu().numpy(), want_i), "top-k ids (node ids, ties to the lower id)"
    assert np.array_equal(scores.cpu().numpy().astype(np.float64), want_s)
    if C < k:
        assert (want_i[:, C:] == -1).all() and np.isinf(want_s[:, C:]).all()
    # the all-node entry points on the copy embs[ic], ids renumbered by hand: the same bits
    (cptr, cidx), tpos = copy_problem(P, N, lists, t_in)
    ecopy = e[ic].contiguous()
    g0, e0 = _native.score_rank(e, ecopy, tpos, iq=q, filt_ptr=cptr, filt_idx=cidx)
    g1, e1 = _native.score_rank(e, e, dev(t_in), iq=q, filt_ptr=ptr, filt_idx=idx, ic=ic)
    assert torch.equal(g0, g1) and torch.equal(e0, e1)
    s0, i0 = _native.score_topk(e, ecopy, k, iq=q, filt_ptr=cptr, filt_idx=cidx)
    assert torch.equal(s0, scores) and torch.equal(torch.where(i0 >= 0, ic[i0.clamp(min=0)], i0), ids)


# ---- 1 + 3. the two losses and their gradients ------------------------------------------------------------------------------
@pytest.mark.parametrize("N,C,B,d", CASES, ids=IDS)
def test_losses_and_gradients_match_float64_and_equal_the_copy(N, C, B, d):
    P, query, t_in, _, lists = problem(N, C, B, 2000 + d)
    embs = layernorm_rows(N, d, seed=d)
    c = embs.cpu().numpy()
    ic, q, t = dev(P), dev(query), dev(t_in)
    ptr, idx = csr(lists)
    g = torch.randn(B, device=DEV, generator=torch.Generator(device=DEV).manual_seed(d))
    gn = g.cpu().numpy()
    scale, smoothing = d ** -0.5, 0.1
    (cptr, cidx), tpos = copy_problem(P, N, lists, t_in)
    ecopy = embs[ic].contiguous()

    want, want_lse, dq64, dc64 = ref.softmax(c[query], c, t_in, lists, P, scale, grad=gn)
    loss, lse = _native.score_softmax_fwd(embs, embs, t, iq=q, filt_ptr=ptr, filt_idx=idx, scale=scale, ic=ic)
    loss_check("softmax loss", loss, want)
    loss_check("softmax lse", lse, want_lse)
    dq, dc = _native.score_softmax_bwd(embs, embs, t, lse, g, iq=q, filt_ptr=ptr, filt_idx=idx, scale=scale, ic=ic)
    assert dc.shape == (C, d)
    if C == 1:
        # the only candidate is the target: p = 1 and G = 0, up to the rounding of lse — the float64 gradient is identically
        # zero, so a bound relative to it says nothing; the bound of test_softmax_gpu's N = 1 case stands in
        assert not dq64.any() and not dc64.any()
        assert float(dq.abs().max()) <= 1e-5 and float(dc.abs().max()) <= 1e-5
    else:
        grad_check("q (softmax)", dq, dq64)
        grad_check("c (softmax)", dc, dc64[P])
    loss0, lse0 = _native.score_softmax_fwd(embs, ecopy, tpos, iq=q, filt_ptr=cptr, filt_idx=cidx, scale=scale)
    dq0, dc0 = _native.score_softmax_bwd(embs, ecopy, tpos, lse0, g, iq=q, filt_ptr=cptr, filt_idx=cidx, scale=scale)
    assert torch.equal(loss, loss0) and torch.equal(lse, lse0) and torch.equal(dq, dq0) and torch.equal(dc, dc0)

    want, dq64, dc64 = ref.bce(c[query], c, lists, P, scale, smoothing, grad=gn)
    loss = _native.score_bce_fwd(embs, embs, iq=q, pos_ptr=ptr, pos_idx=idx, scale=scale, smoothing=smoothing, ic=ic)
    loss_check("bce loss", loss, want)
    dq, dc = _native.score_bce_bwd(embs, embs, loss, g, iq=q, pos_ptr=ptr, pos_idx=idx, scale=scale, smoothing=smoothing, ic=ic)
    grad_check("q (bce)", dq, dq64)
    grad_check("c (bce)", dc, dc64[P])
    loss0 = _native.score_bce_fwd(embs, ecopy, iq=q, pos_ptr=cptr, pos_idx=cidx, scale=scale, smoothing=smoothing)
    dq0, dc0 = _native.score_bce_bwd(embs, ecopy, loss0, g, iq=q, pos_ptr=cptr, pos_idx=cidx, scale=scale, smoothing=smoothing)
    assert torch.equal(loss, loss0) and torch.equal(dq, dq0) and torch.equal(dc, dc0)


# ---- 2. candidates = every node ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", (20, 64, 128, 256))
def test_every_node_as_candidate_equals_the_call_without_the_keyword(d):
    N, B = 700, 150
    P, query, t_in, _, lists = problem(N, N, B, 3000 + d)
    model = model16()
    embs = layernorm_rows(N, d, seed=5 + d)
    q, t = dev(query), dev(t_in)
    ptr, idx = csr(lists)
    every = torch.arange(N, device=DEV)
    w = torch.randn(B, device=DEV, generator=torch.Generator(device=DEV).manual_seed(d))
    for a, b in zip(model.rank_candidates(embs, q, t, filt_ptr=ptr, filt_idx=idx),
                    model.rank_candidates(embs, q, t, filt_ptr=ptr, filt_idx=idx, candidates=every)):
        assert torch.equal(a, b)
    for a, b in zip(model.topk_candidates(embs, q, 10, filt_ptr=ptr, filt_idx=idx),
                    model.topk_candidates(embs, q, 10, filt_ptr=ptr, filt_idx=idx, candidates=torch.ones(N, dtype=torch.bool))):
        assert torch.equal(a, b)
    # the native calls: loss, lse and BOTH gradients (dq per query, dc per candidate), each on its own
    raw = []
    for x in (None, every):
        loss, lse = _native.score_softmax_fwd(embs, embs, t, iq=q, filt_ptr=ptr, filt_idx=idx, scale=0.25, ic=x)
        bce = _native.score_bce_fwd(embs, embs, iq=q, pos_ptr=ptr, pos_idx=idx, scale=0.25, smoothing=0.05, ic=x)
        raw.append((loss, lse, bce) + _native.score_softmax_bwd(embs, embs, t, lse, w, iq=q, filt_ptr=ptr, filt_idx=idx, scale=0.25, ic=x)
                   + _native.score_bce_bwd(embs, embs, bce, w, iq=q, pos_ptr=ptr, pos_idx=idx, scale=0.25, smoothing=0.05, ic=x))
    for a, b, name in zip(raw[0], raw[1], ("loss", "lse", "bce", "softmax dq", "softmax dc", "bce dq", "bce dc")):
        assert torch.equal(a, b), name
    for name in ("softmax", "bce"):
        grads, losses = [], []
        for cand in (None, every):
            e = embs.clone().requires_grad_(True)
            if name == "softmax":
                loss = model.softmax_loss(e, q, t, scale=0.25, filt_ptr=ptr, filt_idx=idx, candidates=cand)
            else:
                loss = model.bce_loss(e, q, pos_ptr=ptr, pos_idx=idx, scale=0.25, smoothing=0.05, candidates=cand)
            (loss * w).sum().backward()
            losses.append(loss.detach())
            grads.append(e.grad)
        assert torch.equal(losses[0], losses[1]), f"{name}: loss"
        assert torch.equal(grads[0], grads[1]), f"{name}: d embs"


# ---- 4. lists ----------------------------------------------------------------------------------------------------------------
def test_list_entries_outside_the_candidates_change_nothing():
    N, C, B, d = 700, 257, 129, 64
    P, query, t_in, _, lists = problem(N, C, B, 4000)
    inside = [l[np.isin(l, P)] for l in lists]
    assert sum(len(l) for l in inside) < sum(len(l) for l in lists)
    embs = layernorm_rows(N, d, seed=41)
    ic, q, t = dev(P), dev(query), dev(t_in)
    g = torch.ones(B, device=DEV)
    out = []
    for ls in (lists, inside):
        ptr, idx = csr(ls)
        kw = dict(iq=q, filt_ptr=ptr, filt_idx=idx, ic=ic)
        loss, lse = _native.score_softmax_fwd(embs, embs, t, scale=0.2, **kw)
        bce = _native.score_bce_fwd(embs, embs, iq=q, pos_ptr=ptr, pos_idx=idx, scale=0.2, smoothing=0.1, ic=ic)
        out.append(_native.score_rank(embs, embs, t, **kw) + _native.score_topk(embs, embs, 7, **kw) + (loss, lse, bce)
                   + _native.score_softmax_bwd(embs, embs, t, lse, g, scale=0.2, **kw)
                   + _native.score_bce_bwd(embs, embs, bce, g, iq=q, pos_ptr=ptr, pos_idx=idx, scale=0.2, smoothing=0.1, ic=ic))
    for a, b in zip(*out):
        assert torch.equal(a, b)


@pytest.mark.parametrize("d", (64, 256))
def test_hub_candidates_that_every_query_lists(d):
    """Eight neighbouring candidates on every query's list: more listed pairs (1,024) fall into one candidate tile than the
    dc sweep keeps beside it in LDS, so that tile looks every id up instead (softmax), or subtracts at the looked-up ids
    (bce)."""
    N, C, B = 1500, 600, 300
    rng = np.random.default_rng(d)
    hubs = np.arange(700, 708)
    P = np.unique(np.concatenate([rng.choice(N, C, replace=False), hubs]))
    tile = 128 if d <= 128 else 64                                        # the dc sweep's owner tile, in positions of P
    assert np.bincount(np.searchsorted(P, hubs) // tile).max() * B > 1024
    embs = layernorm_rows(N, d, seed=70 + d)
    c = embs.cpu().numpy()
    query = rng.integers(0, N, B)
    target = P[rng.integers(0, len(P), B)]
    target[:20] = 702                                                     # a hub that is some queries' target stays in their sums
    lists = [np.unique(np.concatenate([hubs, rng.integers(0, N, 4)])) for _ in range(B)]
    ptr, idx = csr(lists)
    ic, q, t = dev(P), dev(query), dev(target)
    g = torch.randn(B, device=DEV, generator=torch.Generator(device=DEV).manual_seed(d))
    scale = d ** -0.5
    want, _, dq64, dc64 = ref.softmax(c[query], c, target, lists, P, scale, grad=g.cpu().numpy())
    loss, lse = _native.score_softmax_fwd(embs, embs, t, iq=q, filt_ptr=ptr, filt_idx=idx, scale=scale, ic=ic)
    loss_check(f"hub lists d={d}: softmax", loss, want)
    dq, dc = _native.score_softmax_bwd(embs, embs, t, lse, g, iq=q, filt_ptr=ptr, filt_idx=idx, scale=scale, ic=ic)
    grad_check(f"q (hub lists, softmax, d={d})", dq, dq64)
    grad_check(f"c (hub lists, softmax, d={d})", dc, dc64[P])
    want, dq64, dc64 = ref.bce(c[query], c, lists, P, scale, 0.1, grad=g.cpu().numpy())
    loss = _native.score_bce_fwd(embs, embs, iq=q, pos_ptr=ptr, pos_idx=idx, scale=scale, smoothing=0.1, ic=ic)
    loss_check(f"hub lists d={d}: bce", loss, want)
    dq, dc = _native.score_bce_bwd(embs, embs, loss, g, iq=q, pos_ptr=ptr, pos_idx=idx, scale=scale, smoothing=0.1, ic=ic)
    grad_check(f"q (hub lists, bce, d={d})", dq, dq64)
    grad_check(f"c (hub lists, bce, d={d})", dc, dc64[P])


def test_listed_candidates_that_dominate_never_enter_the_sum():
    """The construction of test_softmax_gpu's test of this name, with the dominating rows among the candidates: every
    query's 10 listed rows are 2 x its own row, so they score 2 |q|^2 and everything unlisted at most |q|^2."""
    N, B, L, d = 5003, 130, 10, 64
    model = model16()
    embs = layernorm_rows(N, d, seed=50 + d)
    query = np.arange(B)
    lists = [B + L * i + np.arange(L) for i in range(B)]
    rng = np.random.default_rng(d)
    target = rng.integers(B + L * B, N, B)
    target[:8] = target[0]
    for i in range(B):
        embs[dev(lists[i])] = 2.0 * embs[i]
    cand = np.concatenate([np.concatenate(lists), rng.integers(0, N, 900)])
    q, t = dev(query), dev(target)
    ptr, idx = csr(lists)
    w = torch.rand(B, device=DEV, generator=torch.Generator(device=DEV).manual_seed(d)) + 0.5
    c = embs.cpu().numpy()
    P = ref.softmax_set(cand, target, N)
    for scale in (1.0, d ** -0.5):
        want, _, dq64, dc64 = ref.softmax(c[query], c, target, lists, P, scale, grad=w.cpu().numpy())
        np.add.at(dc64, query, dq64)
        e = embs.clone().requires_grad_(True)
        loss = model.softmax_loss(e, q, t, scale=scale, filt_ptr=ptr, filt_idx=idx, candidates=dev(cand))
        loss_check(f"dominating lists scale={scale:.3g}: loss", loss, want)
        (loss * w).sum().backward()
        grad_check(f"embs (dominating lists, scale={scale:.3g})", e.grad, dc64)


def test_typed_known_edges_and_query_rows_with_candidates():
    N, B, d, R = 900, 140, 64, 5
    rng = np.random.default_rng(8)
    model = model16()
    c = exact_rows(N, d, seed=81)
    embs = dev(c)
    rows = exact_rows(B, d, seed=82)                                      # the relation decoder's rows stand in for embs[query]
    Q = dev(rows)
    query, qrel = rng.integers(0, N, B), rng.integers(0, R, B)
    src = np.concatenate([np.repeat(query, 6), rng.integers(0, N, 300)])
    dst, rel = rng.integers(0, N, len(src)), rng.integers(0, R, len(src))
    lists = [np.unique(dst[(src == query[i]) & (rel == qrel[i])]) for i in range(B)]
    assert sum(len(l) for l in lists) > B
    P = np.unique(np.concatenate([rng.choice(N, 300, replace=False), dst[:200]]))
    target = P[rng.integers(0, len(P), B)]
    kw = dict(known=(dev(src), dev(dst), dev(rel)), query_rel=dev(qrel), query_rows=Q, candidates=dev(P))
    greater, equal = model.rank_candidates(embs, dev(query), dev(target), **kw)
    want_g, want_e = ref.rank(rows, c, target, lists, P)
    assert np.array_equal(greater.cpu().numpy(), want_g) and np.array_equal(equal.cpu().numpy(), want_e)
    scores, ids = model.topk_candidates(embs, dev(query), 12, **kw)
    want_s, want_i = ref.topk(rows, c, lists, P, 12)
    assert np.array_equal(ids.cpu().numpy(), want_i) and np.array_equal(scores.cpu().numpy().astype(np.float64), want_s)
    # the two losses, recorded: the per-query gradient is the rows' own
    w = torch.randn(B, device=DEV, generator=torch.Generator(device=DEV).manual_seed(3))
    e, r = embs.clone().requires_grad_(True), Q.clone().requires_grad_(True)
    loss = model.softmax_loss(e, dev(query), dev(target), scale=0.05, **{**kw, "query_rows": r})
    want, _, dq64, dc64 = ref.softmax(rows, c, target, lists, P, 0.05, grad=w.cpu().numpy())
    loss_check("typed softmax", loss, want)
    (loss * w).sum().backward()
    grad_check("rows (typed softmax)", r.grad, dq64)
    grad_check("embs (typed softmax)", e.grad, dc64)
    e, r = embs.clone().requires_grad_(True), Q.clone().requires_grad_(True)
    loss = model.bce_loss(e, dev(query), scale=0.05, smoothing=0.1, **{**kw, "query_rows": r})
    want, dq64, dc64 = ref.bce(rows, c, lists, P, 0.05, 0.1, grad=w.cpu().numpy() / len(P))
    loss_check("typed bce (mean over the candidates)", loss, want / len(P))
    (loss * w).sum().backward()
    grad_check("rows (typed bce)", r.grad, dq64)
    grad_check("embs (typed bce)", e.grad, dc64)


# ---- 5. top-k ----------------------------------------------------------------------------------------------------------------
def test_topk_pads_returns_node_ids_and_selects_in_place_more_than_once():
    N, d = 2100, 64
    model = model16()
    c = exact_rows(N, d, seed=17)
    embs = dev(c)
    rng = np.random.default_rng(17)
    query = rng.integers(0, N, 129)
    q = dev(query)
    # fewer than k left: 20 candidates, 8 of them listed by every query
    P = np.sort(rng.choice(N, 20, replace=False)) + 0
    lists = [np.sort(P[:8])] * len(query)
    ptr, idx = csr(lists)
    scores, ids = model.topk_candidates(embs, q, 16, filt_ptr=ptr, filt_idx=idx, candidates=dev(P[::-1].copy()))
    want_s, want_i = ref.topk(c[query], c, lists, P, 16)
    assert np.array_equal(ids.cpu().numpy(), want_i) and np.array_equal(scores.cpu().numpy().astype(np.float64), want_s)
    assert (ids[:, 12:] == -1).all() and torch.isinf(scores[:, 12:]).all() and (ids[:, :12] >= 0).all()
    assert np.isin(ids[:, :12].cpu().numpy(), P[8:]).all()
    # C = 1,600 with k = 128: the append buffer (k + 256 + 64 entries) fills and is cut back to k several times per query
    P = np.sort(rng.choice(N, 1600, replace=False))
    scores, ids = model.topk_candidates(embs, q, 128, candidates=dev(P))
    want_s, want_i = ref.topk(c[query], c, None, P, 128)
    assert np.array_equal(ids.cpu().numpy(), want_i) and np.array_equal(scores.cpu().numpy().astype(np.float64), want_s)


# ---- 6. targets --------------------------------------------------------------------------------------------------------------
def test_softmax_target_outside_the_candidates():
    N, C, B, d = 700, 257, 129, 64
    P, query, t_in, _, lists = problem(N, C, B, 6000)
    model = model16()
    embs = layernorm_rows(N, d, seed=61)
    c = embs.cpu().numpy()
    target = t_in.copy()
    out = int(np.setdiff1d(np.arange(N), P)[7])
    target[33] = out                                                      # one query's target is no candidate
    ok = np.ones(B, dtype=bool)
    ok[33] = False
    ic, q, t = dev(P), dev(query), dev(target)
    ptr, idx = csr(lists)
    g = torch.randn(B, device=DEV, generator=torch.Generator(device=DEV).manual_seed(6))
    loss, lse = _native.score_softmax_fwd(embs, embs, t, iq=q, filt_ptr=ptr, filt_idx=idx, scale=0.125, ic=ic)
    assert torch.isnan(loss[33]) and torch.isnan(lse[33])
    want, _, dq64, dc64 = ref.softmax(c[query], c, target, lists, P, 0.125, grad=g.cpu().numpy())
    loss_check("the other queries", loss[dev(ok)], want[ok])
    dq, dc = _native.score_softmax_bwd(embs, embs, t, lse, g, iq=q, filt_ptr=ptr, filt_idx=idx, scale=0.125, ic=ic)
    assert float(dq[33].abs().max()) == 0.0
    grad_check("q (one target outside)", dq, dq64)
    grad_check("c (one target outside)", dc, dc64[P])
    # the model method adds the batch's targets to the set: finite, and the restatement over that set
    loss = model.softmax_loss(embs, q, t, scale=0.125, filt_ptr=ptr, filt_idx=idx, candidates=ic)
    assert torch.isfinite(loss).all()
    want, _ = ref.softmax(c[query], c, target, lists, ref.softmax_set(P, target, N), 0.125)
    loss_check("softmax_loss with the target added", loss, want)


# ---- 7. gradients ------------------------------------------------------------------------------------------------------------
def test_gradients_reach_the_parameters_and_only_the_rows_that_took_part():
    kg = ToyKnowledgeGraph(feat_dim=16)
    x, ei = kg.node_features.to(DEV), kg.edge_index.to(DEV)
    torch.manual_seed(0)
    model = HyperGNN(text_dim=64, node_feat_dim=16, hidden_dim=32, num_layers=2).to(DEV)
    N = x.size(0)
    cand = torch.arange(0, N, 2, device=DEV)
    for name in ("softmax", "bce"):
        model.zero_grad()
        embs = model(x, ei, kg.edge_texts)
        embs.retain_grad()
        if name == "softmax":
            loss = model.softmax_loss(embs, ei[0], ei[1], scale=32 ** -0.5, known=(ei[0], ei[1]), candidates=cand)
            part = torch.cat([cand, ei[0], ei[1]])
        else:
            loss = model.bce_loss(embs, torch.unique(ei[0]), known=(ei[0], ei[1]), scale=32 ** -0.5, smoothing=0.1, candidates=cand)
            part = torch.cat([cand, ei[0]])
        assert torch.isfinite(loss).all()
        loss.mean().backward()
        trained = [n for n, p in model.named_parameters() if p.grad is not None and bool((p.grad != 0).any())]
        assert len(trained) >= 10, (name, trained)
        rest = torch.ones(N, dtype=torch.bool, device=DEV)
        rest[part] = False
        assert not bool(embs.grad[rest].any()) and bool(embs.grad[~rest].any())


def test_rows_outside_candidates_and_queries_get_exactly_zero_and_runs_repeat_bit_for_bit():
    N, C, B, d = 6000, 4500, 300, 128
    P, query, t_in, _, lists = problem(N, C, B, 7000)
    model = model16()
    embs = layernorm_rows(N, d, seed=71)
    ic, q, t = dev(P), dev(query), dev(t_in)
    ptr, idx = csr(lists)
    w = torch.randn(B, device=DEV, generator=torch.Generator(device=DEV).manual_seed(7))
    rest = torch.ones(N, dtype=torch.bool, device=DEV)
    rest[ic] = False
    rest[q] = False
    assert int(rest.sum()) > 100
    for name in ("softmax", "bce"):
        runs = []
        for _ in range(2):
            e = embs.clone().requires_grad_(True)
            if name == "softmax":
                loss = model.softmax_loss(e, q, t, scale=d ** -0.5, filt_ptr=ptr, filt_idx=idx, candidates=ic)
            else:
                loss = model.bce_loss(e, q, pos_ptr=ptr, pos_idx=idx, scale=d ** -0.5, smoothing=0.1, candidates=ic)
            (loss * w).sum().backward()
            runs.append((loss.detach(), e.grad))
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), name
        assert not bool(runs[0][1][rest].any()), f"{name}: a row outside the candidates and the queries has a gradient"
        assert bool(runs[0][1][ic].any(1).all())
    # a query's bits do not depend on its batch: two halves against the whole, the same candidates
    kw = dict(scale=d ** -0.5, ic=ic)
    loss, lse = _native.score_softmax_fwd(embs, embs, t, iq=q, filt_ptr=ptr, filt_idx=idx, **kw)
    bce = _native.score_bce_fwd(embs, embs, iq=q, pos_ptr=ptr, pos_idx=idx, smoothing=0.1, **kw)
    # dq's partial sums are cut into candidate slabs whose number depends on B only from 8,192 candidates on (one slab per
    # 4,096, at least one): at C = 4,500 every batch has one slab, and a query's dq has the same bits in any of them
    dq, _ = _native.score_softmax_bwd(embs, embs, t, lse, w, iq=q, filt_ptr=ptr, filt_idx=idx, **kw)
    bdq, _ = _native.score_bce_bwd(embs, embs, bce, w, iq=q, pos_ptr=ptr, pos_idx=idx, smoothing=0.1, **kw)
    g1, e1 = _native.score_rank(embs, embs, t, iq=q, filt_ptr=ptr, filt_idx=idx, ic=ic)
    s1, i1 = _native.score_topk(embs, embs, 10, iq=q, filt_ptr=ptr, filt_idx=idx, ic=ic)
    h = B // 2
    for lo, hi in ((0, h), (h, B)):
        p2, i2 = csr(lists[lo:hi])
        l2, s2 = _native.score_softmax_fwd(embs, embs, t[lo:hi], iq=q[lo:hi], filt_ptr=p2, filt_idx=i2, **kw)
        b2 = _native.score_bce_fwd(embs, embs, iq=q[lo:hi], pos_ptr=p2, pos_idx=i2, smoothing=0.1, **kw)
        assert torch.equal(l2, loss[lo:hi]) and torch.equal(s2, lse[lo:hi]) and torch.equal(b2, bce[lo:hi])
        dq2, _ = _native.score_softmax_bwd(embs, embs, t[lo:hi], s2, w[lo:hi].contiguous(), iq=q[lo:hi], filt_ptr=p2, filt_idx=i2, **kw)
        bdq2, _ = _native.score_bce_bwd(embs, embs, b2, w[lo:hi].contiguous(), iq=q[lo:hi], pos_ptr=p2, pos_idx=i2, smoothing=0.1, **kw)
        assert torch.equal(dq2, dq[lo:hi]) and torch.equal(bdq2, bdq[lo:hi]), "a query's dq depends on the batch it is in"
        g2, e2 = _native.score_rank(embs, embs, t[lo:hi], iq=q[lo:hi], filt_ptr=p2, filt_idx=i2, ic=ic)
        assert torch.equal(g2, g1[lo:hi]) and torch.equal(e2, e1[lo:hi])
        sk, ik = _native.score_topk(embs, embs, 10, iq=q[lo:hi], filt_ptr=p2, filt_idx=i2, ic=ic)
        assert torch.equal(sk, s1[lo:hi]) and torch.equal(ik, i1[lo:hi])


@pytest.mark.parametrize("d", (50, 150))
def test_row_widths_that_are_no_multiple_of_four_train_through_the_model_methods(d):
    """d % 4 != 0 (scalar row loads in the sweeps, the scalar form of the dc scatter), at both owner-tile shapes of the
    backward: the recorded losses and d embs against float64, as without the keyword."""
    N, C, B = 700, 257, 129
    P, query, t_in, _, lists = problem(N, C, B, 9000 + d)
    model = model16()
    embs = layernorm_rows(N, d, seed=91 + d)
    c = embs.cpu().numpy()
    q, t = dev(query), dev(t_in)
    ptr, idx = csr(lists)
    w = torch.randn(B, device=DEV, generator=torch.Generator(device=DEV).manual_seed(d))
    scale = d ** -0.5
    rest = torch.ones(N, dtype=torch.bool, device=DEV)
    rest[dev(P)] = False
    rest[q] = False
    for name in ("softmax", "bce"):
        e = embs.clone().requires_grad_(True)
        if name == "softmax":                                             # the targets are candidates: the set stays P
            loss = model.softmax_loss(e, q, t, scale=scale, filt_ptr=ptr, filt_idx=idx, candidates=dev(P))
            want, _, dq64, dc64 = ref.softmax(c[query], c, t_in, lists, P, scale, grad=w.cpu().numpy())
        else:
            loss = model.bce_loss(e, q, pos_ptr=ptr, pos_idx=idx, scale=scale, smoothing=0.1, normalize=False, candidates=dev(P))
            want, dq64, dc64 = ref.bce(c[query], c, lists, P, scale, 0.1, grad=w.cpu().numpy())
        loss_check(f"{name} d={d}", loss, want)
        (loss * w).sum().backward()
        np.add.at(dc64, query, dq64)
        grad_check(f"embs ({name}, d={d})", e.grad, dc64)
        assert not bool(e.grad[rest].any())
        plain = embs.clone().requires_grad_(True)                         # and the same call without the keyword still trains
        (model.softmax_loss(plain, q, t, scale=scale) if name == "softmax" else model.bce_loss(plain, q, scale=scale)).sum().backward()
        assert torch.isfinite(plain.grad).all()


def test_query_rows_alone_can_require_the_gradient():
    """embs as data, the query rows recorded: the per-query gradient comes back, nothing is built for embs"""
    N, C, B, d = 700, 257, 129, 64
    P, query, t_in, _, lists = problem(N, C, B, 9500)
    model = model16()
    embs = layernorm_rows(N, d, seed=95)
    rows = layernorm_rows(B, d, seed=96)
    ptr, idx = csr(lists)
    w = torch.randn(B, device=DEV, generator=torch.Generator(device=DEV).manual_seed(9))
    r = rows.clone().requires_grad_(True)
    loss = model.softmax_loss(embs, dev(query), dev(t_in), scale=0.125, filt_ptr=ptr, filt_idx=idx, query_rows=r, candidates=dev(P))
    (loss * w).sum().backward()
    want, _, dq64, _ = ref.softmax(rows.cpu().numpy(), embs.cpu().numpy(), t_in, lists, P, 0.125, grad=w.cpu().numpy())
    loss_check("rows only: loss", loss, want)
    grad_check("rows (rows only)", r.grad, dq64)
    assert embs.grad is None


# ---- 8. a bad candidate list at the native level --------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("repeated", "out_of_range", "descending"))
def test_a_bad_candidate_list_makes_every_query_invalid_and_nothing_else_happens(kind):
    N, C, B, d = 700, 257, 129, 64
    P, query, t_in, _, lists = problem(N, C, B, 8000)
    bad = P.copy()
    if kind == "repeated":
        bad[100] = bad[99]
    elif kind == "out_of_range":
        bad[-1] = N
    else:
        bad[[5, 6]] = bad[[6, 5]]
    embs = layernorm_rows(N, d, seed=81)
    before = embs.clone()
    ic, q, t = dev(bad), dev(query), dev(t_in)
    ptr, idx = csr(lists)
    kw = dict(iq=q, filt_ptr=ptr, filt_idx=idx, ic=ic)
    greater, equal = _native.score_rank(embs, embs, t, **kw)
    assert (greater == -1).all() and (equal == -1).all()
    scores, ids = _native.score_topk(embs, embs, 5, **kw)
    assert torch.isnan(scores).all() and (ids == -1).all()
    loss, lse = _native.score_softmax_fwd(embs, embs, t, scale=0.5, **kw)
    assert torch.isnan(loss).all() and torch.isnan(lse).all()
    bce = _native.score_bce_fwd(embs, embs, iq=q, pos_ptr=ptr, pos_idx=idx, scale=0.5, smoothing=0.1, ic=ic)
    assert torch.isnan(bce).all()
    # the backwards check the list themselves: finite values handed in for lse / loss change nothing
    g, fine = torch.ones(B, device=DEV), torch.zeros(B, device=DEV)
    for dq, dc in (_native.score_softmax_bwd(embs, embs, t, fine, g, scale=0.5, **kw),
                   _native.score_bce_bwd(embs, embs, fine, g, iq=q, pos_ptr=ptr, pos_idx=idx, scale=0.5, smoothing=0.1, ic=ic)):
        assert dc.shape == (C, d) and not bool(dq.any()) and not bool(dc.any())
    torch.cuda.synchronize()
    assert torch.equal(embs, before)
    with pytest.raises(ValueError):
        _native.score_rank(embs, embs, t, iq=q, ic=torch.zeros(0, dtype=torch.int64, device=DEV))
