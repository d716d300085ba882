"""Per-query negative sets on the device (HyperGNN.rank_candidates / softmax_loss / negative_sampling_loss with negatives=;
include/ghf_negatives.h; csrc/negatives.hip) against the float64 restatement of tests/_negatives_ref.py.

Tolerances are the project's own, through loss_check / grad_check of tests/test_softmax_gpu.py; ranks must be equal.  The
kernel reads 64 / L rows per wave instruction (L = 8, 16, 32, 64 lanes per row at d <= 32, 64, 128, 256; the scalar path
where d % 4 != 0) and walks its K positions 8 x 64 / L at a time, so the shapes cross d with K around 8, 16, 32 and 64 and
their multiples, and around 256, above which a query's positions are dealt to four waves; B = 129 leaves the last
workgroup (four queries) with one."""

import numpy as np
import pytest
import torch

import _negatives_ref as R
from graph_hypernetwork_forge_amd import ToyKnowledgeGraph, _native
from test_softmax_gpu import csr, grad_check, layernorm_rows, loss_check, model16, problem

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NAN = float("nan")

# (d, K, B, N): every d of {1, 3, 20, 64, 128, 200, 256}, every K of {1, 2, 7, 8, 9, 63, 64, 65, 257, 1000}, B of {1, 5, 129},
# N of {300, 5000}; K = 256 and 257 are the two sides of the split of a query over four waves
SHAPES = [(1, 1, 1, 300), (1, 65, 5, 300), (3, 7, 5, 300), (3, 257, 5, 5000), (20, 8, 5, 300), (20, 63, 129, 5000), (20, 64, 5, 300),
          (20, 65, 5, 300), (20, 256, 5, 300), (20, 1000, 5, 300), (64, 2, 5, 300), (64, 9, 129, 300), (64, 63, 5, 300), (64, 64, 5, 5000),
          (64, 65, 5, 300), (64, 257, 5, 300), (128, 1, 1, 300), (128, 7, 5, 300), (128, 8, 5, 300), (128, 9, 5, 300),
          (128, 63, 5, 300), (128, 65, 129, 5000), (128, 256, 5, 300), (128, 257, 5, 300), (128, 1000, 5, 5000), (200, 9, 5, 300), (200, 65, 5, 300),
          (256, 7, 5, 300), (256, 8, 129, 300), (256, 9, 5, 300), (256, 257, 5, 5000), (256, 1000, 1, 300)]
IDS = ["d%d-K%d-B%d-N%d" % s for s in SHAPES]


def setup(d, K, B, N, seed, pad=True):
    """Rows, queries with per-node lists (test_softmax_gpu.problem), and negatives that hold padding, repeats, the target and
    listed ids."""
    if d > 3:
        embs = layernorm_rows(N, d, seed)
    else:                                       # LayerNorm over one element is its beta: every row the same, every gradient a
        embs = torch.randn(N, d, device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed))    # sum that cancels to 0
    query, target, lists, known = problem(N, max(B, 20), seed + 1, per_list=4)     # (it plants repeats at places up to 20)
    query, target, lists = query[:B], target[:B], lists[:B]                        # known: per node, so it still agrees
    rng = np.random.default_rng(seed + 2)
    neg = rng.integers(0, N, (B, K))
    if pad:
        neg[rng.random((B, K)) < 0.15] = -1
    for i in range(B):
        if K >= 3:
            neg[i, K // 2] = neg[i, 0]                                      # a repeat
        if K >= 4 and i % 2 == 0:
            neg[i, K - 1] = target[i]                                       # the target among its own negatives
        if K >= 2 and len(lists[i]):
            neg[i, 1] = lists[i][0]                                         # a known partner
    bias = torch.from_numpy(rng.standard_normal(N).astype(np.float32)).to(DEV)
    grad = torch.from_numpy(rng.standard_normal(B).astype(np.float32)).to(DEV)
    t = lambda a: torch.from_numpy(np.asarray(a)).to(DEV)
    return embs, t(query), t(target), t(neg), lists, known, bias, grad


def bits(t):
    return t.detach().contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


# ---- 1. the three operations and every gradient against float64 -----------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
@pytest.mark.parametrize("with_bias", [False, True], ids=["plain", "bias"])
def test_forward_and_gradients_match_float64(shape, with_bias):
    d, K, B, N = shape
    model = model16()
    embs, q, t, neg, lists, known, bias, grad = setup(d, K, B, N, seed=7 * d + K)
    b = bias if with_bias else None
    ptr, idx = csr(lists)
    scale = d ** -0.5 if d > 3 else 1.0

    greater, equal = model.rank_candidates(embs, q, t, known=known, negatives=neg, candidate_bias=b)
    live = R.live_positions(neg, t, lists).to(DEV)
    z, zt = R.scores(embs[q], embs, t, neg, b)
    clear = ((z - zt.unsqueeze(1)).abs() > 1e-4 * (1 + zt.abs().unsqueeze(1))).to(DEV)   # float64 says it, with room for fp32
    assert int(greater.min()) >= 0 and bool((greater + equal <= live.sum(1)).all())
    wg, we = R.rank(embs[q], embs, t, neg, lists, b)
    if bool(clear.all()):
        assert torch.equal(greater.cpu(), wg) and torch.equal(equal.cpu(), we)
    else:                                                                                # a near-tie: the count within its reach
        slack = (~clear & live).sum(1).cpu()
        assert bool(((greater.cpu() - wg).abs() <= slack).all())

    for mode, kw in (("softmax", {}), ("negsamp", dict(margin=1.5, adversarial_temperature=0.5))):
        e = embs.clone().requires_grad_()
        bb = None if b is None else b.clone().requires_grad_()
        fn = model.softmax_loss if mode == "softmax" else model.negative_sampling_loss
        loss = fn(e, q, t, scale=scale, known=known, negatives=neg, candidate_bias=bb, **kw)
        want = R.loss(mode, embs[q], embs, t, neg, lists, b, scale=scale, margin=kw.get("margin", 0.0),
                      alpha=kw.get("adversarial_temperature", 0.0), grad=grad)
        loss_check(f"{mode} loss", loss, want["loss"])
        raw = (_native.score_neg_softmax_fwd(embs, embs, t, neg, iq=q, filt_ptr=ptr, filt_idx=idx, scale=scale, bias=b)
               if mode == "softmax" else
               _native.score_neg_negsamp_fwd(embs, embs, t, neg, iq=q, filt_ptr=ptr, filt_idx=idx, scale=scale, bias=b, **kw))
        assert torch.equal(bits(raw[0]), bits(loss))                                     # known= and CSR lists: the same call
        finite = torch.isfinite(want["aux"])
        if bool(finite.any()):
            loss_check(f"{mode} lse / lw", raw[1][finite.to(DEV)], want["aux"][finite])
        assert torch.equal(raw[1].cpu()[~finite], want["aux"][~finite].float())          # -inf: no negatives
        (loss * grad).sum().backward()
        grad_check(f"{mode} embs", e.grad.cpu().numpy(), R.embs_grad(want, q).numpy())
        if bb is not None:
            grad_check(f"{mode} bias", bb.grad.cpu().numpy(), want["db"].numpy())
        dq, coef = _native.score_neg_bwd(_native.NEG_SOFTMAX if mode == "softmax" else _native.NEG_NEGSAMP, embs, embs, t, neg,
                                         raw[1], grad, iq=q, filt_ptr=ptr, filt_idx=idx, scale=scale, bias=b,
                                         margin=kw.get("margin", 0.0), adversarial_temperature=kw.get("adversarial_temperature", 0.0))
        grad_check(f"{mode} dq", dq.cpu().numpy(), want["dq"].numpy())
        grad_check(f"{mode} coef", coef.cpu().numpy(), want["coef"].numpy())
        assert bool((coef[:, :K][~live] == 0).all())                                      # exactly 0 outside J_i


# ---- 2. query_rows and typed lists ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,K", [(20, 9), (128, 65), (200, 8)])
def test_query_rows_and_typed_lists(d, K):
    N, B = 300, 129
    model = model16()
    embs, q, t, neg, _, _, bias, grad = setup(d, K, B, N, seed=d)
    rng = np.random.default_rng(d)
    rows = torch.from_numpy(rng.standard_normal((B, d)).astype(np.float32)).to(DEV)
    E = 400
    src, dst, rel = (torch.from_numpy(rng.integers(0, n, E)).to(DEV) for n in (N, N, 3))
    src[:B] = q
    dst[:B] = neg[:, 0].clamp(min=0)                                        # every query lists its first negative under rel 1
    rel[:B] = 1
    qrel = torch.from_numpy(rng.integers(0, 3, B)).to(DEV)
    lists = [np.unique(dst[(src == q[i]) & (rel == qrel[i])].cpu().numpy()) for i in range(B)]
    for mode in ("softmax", "negsamp"):
        e, r = embs.clone().requires_grad_(), rows.clone().requires_grad_()
        fn = model.softmax_loss if mode == "softmax" else model.negative_sampling_loss
        kw = {} if mode == "softmax" else dict(margin=0.5, adversarial_temperature=1.0)
        loss = fn(e, q, t, scale=0.3, known=(src, dst, rel), query_rel=qrel, query_rows=r, negatives=neg, **kw)
        want = R.loss(mode, rows, embs, t, neg, lists, None, scale=0.3, margin=kw.get("margin", 0.0),
                      alpha=kw.get("adversarial_temperature", 0.0), grad=grad)
        loss_check(f"{mode} typed loss", loss, want["loss"])
        (loss * grad).sum().backward()
        grad_check(f"{mode} typed embs", e.grad.cpu().numpy(), want["dc"].numpy())
        grad_check(f"{mode} typed rows", r.grad.cpu().numpy(), want["dq"].numpy())
    # the counts themselves, on integer data (exact in fp32 whatever the order): ignoring the rows or the typed lists shows
    irows, iembs = integer_rows(B, d, seed=d + 7), integer_rows(N, d, seed=d + 8)
    greater, equal = model.rank_candidates(iembs, q, t, known=(src, dst, rel), query_rel=qrel, query_rows=irows, negatives=neg)
    wg, we = R.rank(irows, iembs, t, neg, lists)
    assert torch.equal(greater.cpu(), wg) and torch.equal(equal.cpu(), we)
    ug, _ = R.rank(irows, iembs, t, neg, None)                               # (the lists do remove something)
    assert int((ug - wg).sum()) > 0 and not torch.equal(wg, R.rank(iembs[q], iembs, t, neg, lists)[0])


# ---- 3. exact-integer data: counts equal float64's, ties included; consistency with candidates= --------------------------
def integer_rows(N, d, seed):
    return torch.from_numpy(np.random.default_rng(seed).integers(-4, 5, (N, d)).astype(np.float32)).to(DEV)


@pytest.mark.parametrize("d,K,B,N", [(1, 65, 5, 300), (3, 9, 129, 300), (20, 257, 5, 300), (64, 63, 129, 300), (128, 64, 129, 5000),
                                     (128, 1000, 5, 300), (200, 65, 5, 300), (256, 9, 129, 300), (256, 257, 5, 300)])
def test_ranks_on_integer_data_equal_float64(d, K, B, N):
    """Entries in {-4..4} and an integer bias: every product and partial sum is an integer below 2^24 (|sum| <= 16 d <= 4,096),
    so the dot product is exact in fp32 whatever its order."""
    model = model16()
    _, q, t, neg, lists, known, _, _ = setup(d, K, B, N, seed=d + K)
    embs = integer_rows(N, d, seed=d)
    embs[N - 40:] = embs[:40]                                                # copies ...
    t = torch.arange(B, device=DEV) % 40
    neg[:, 0] = N - 40 + t                                                   # ... of the target, first in every row: a tie
    bias = torch.from_numpy(np.random.default_rng(K).integers(-3, 4, N).astype(np.float32)).to(DEV)
    for b in (None, bias):
        greater, equal = model.rank_candidates(embs, q, t, known=known, negatives=neg, candidate_bias=b)
        wg, we = R.rank(embs[q], embs, t, neg, lists, b)
        assert torch.equal(greater.cpu(), wg) and torch.equal(equal.cpu(), we)
        assert b is not None or int(we.sum()) >= B // 2


@pytest.mark.parametrize("d,C", [(20, 65), (128, 257), (256, 9)])
def test_the_same_set_for_every_query_is_candidates(d, C):
    N, B = 300, 129
    model = model16()
    _, q, t, _, lists, known, _, _ = setup(d, 4, B, N, seed=d)
    embs = integer_rows(N, d, seed=d + 1)
    S = torch.from_numpy(np.random.default_rng(d).permutation(N)[:C]).to(DEV)            # repeat-free, any order
    t[:B // 2] = S[torch.arange(B // 2, device=DEV) % C]                                   # targets inside S, the rest wherever
    for kn in (None, known):
        got = model.rank_candidates(embs, q, t, known=kn, negatives=S.expand(B, -1))
        want = model.rank_candidates(embs, q, t, known=kn, candidates=S)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


# ---- 4. multisets, padding, empty sets, hubs, untouched rows ----------------------------------------------------------------
def test_an_id_three_times_counts_three_times():
    N, d, B = 300, 128, 5
    model = model16()
    embs = layernorm_rows(N, d, seed=1)
    q = torch.arange(B, device=DEV)
    t = q + 10
    once = torch.tensor([[50, 60, 70, -1, -1]] * B, device=DEV)
    thrice = torch.tensor([[50, 60, 70, 60, 60]] * B, device=DEV)
    for mode in ("softmax", "negsamp"):
        fn = model.softmax_loss if mode == "softmax" else model.negative_sampling_loss
        kw = {} if mode == "softmax" else dict(margin=1.0, adversarial_temperature=1.0)
        kw["scale"] = d ** -0.5                                  # logits of order 1: two more terms move every loss in fp32
        e = embs.clone().requires_grad_()
        loss = fn(e, q, t, negatives=thrice, **kw)
        want = R.loss(mode, embs[q], embs, t, thrice, None, None, grad=torch.ones(B), scale=kw["scale"], margin=kw.get("margin", 0.0),
                      alpha=kw.get("adversarial_temperature", 0.0))
        loss_check(f"{mode} thrice", loss, want["loss"])
        assert bool((loss != fn(embs, q, t, negatives=once, **kw)).all())
        loss.sum().backward()
        grad_check(f"{mode} thrice embs", e.grad.cpu().numpy(), R.embs_grad(want, q).numpy())
        coef = _native.score_neg_bwd(_native.NEG_SOFTMAX if mode == "softmax" else _native.NEG_NEGSAMP, embs, embs, t, thrice,
                                     (_native.score_neg_softmax_fwd(embs, embs, t, thrice, iq=q, **kw) if mode == "softmax" else
                                      _native.score_neg_negsamp_fwd(embs, embs, t, thrice, iq=q, **kw))[1],
                                     torch.ones(B, device=DEV), iq=q, **kw)[1]
        assert torch.equal(bits(coef[:, 1]), bits(coef[:, 3])) and torch.equal(bits(coef[:, 1]), bits(coef[:, 4]))
        # row 60 of d embs: three terms per query, nothing else names it
        three = (3.0 * coef[:, 1].double().unsqueeze(1) * embs[q].double()).sum(0)
        grad_check(f"{mode} row 60", e.grad[60].cpu().numpy(), three.cpu().numpy())
    g1, _ = model.rank_candidates(embs, q, t, negatives=once)
    g3, _ = model.rank_candidates(embs, q, t, negatives=thrice)
    s60 = (embs[q] * embs[60]).sum(1) > (embs[q] * embs[t]).sum(1)
    assert torch.equal(g3 - g1, 2 * s60.to(torch.int64))


@pytest.mark.parametrize("d,K", [(20, 65), (128, 17), (256, 9), (3, 7)])
def test_padding_and_empty_sets(d, K):
    N, B = 300, 6
    model = model16()
    embs, q, t, neg, lists, known, bias, grad = setup(d, K, B, N, seed=K, pad=False)
    neg[0, 0] = -1                                                           # first
    neg[1, K - 1] = -1                                                       # last
    neg[2, ::2] = -1                                                         # scattered
    neg[3] = -1                                                              # a whole row
    neg[4] = t[4]                                                            # every negative is the target
    lists = [l for l in lists]
    lists[5] = np.unique(neg[5].cpu().numpy())                               # every negative is listed
    lists[4], lists[3] = np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    ptr, idx = csr(lists)
    empty = torch.tensor([3, 4, 5], device=DEV)
    loss, lse = _native.score_neg_softmax_fwd(embs, embs, t, neg, iq=q, filt_ptr=ptr, filt_idx=idx, scale=0.5)
    assert torch.equal(bits(loss[empty]), torch.zeros(3, dtype=torch.int32, device=DEV))         # exactly +0
    nl, lw = _native.score_neg_negsamp_fwd(embs, embs, t, neg, iq=q, filt_ptr=ptr, filt_idx=idx, scale=0.5, margin=1.0,
                                           adversarial_temperature=1.0)
    assert bool((lw[empty] == float("-inf")).all())
    greater, equal = _native.score_neg_rank(embs, embs, t, neg, iq=q, filt_ptr=ptr, filt_idx=idx)
    assert int(greater[empty].abs().sum() + equal[empty].abs().sum()) == 0
    for mode, got, aux in (("softmax", loss, lse), ("negsamp", nl, lw)):
        want = R.loss(mode, embs[q], embs, t, neg, lists, None, scale=0.5, margin=1.0, alpha=1.0, grad=grad)
        loss_check(f"{mode} padded loss", got, want["loss"])
        dq, coef = _native.score_neg_bwd(_native.NEG_SOFTMAX if mode == "softmax" else _native.NEG_NEGSAMP, embs, embs, t, neg, aux,
                                         grad, iq=q, filt_ptr=ptr, filt_idx=idx, scale=0.5, margin=1.0, adversarial_temperature=1.0)
        grad_check(f"{mode} padded dq", dq.cpu().numpy(), want["dq"].numpy())
        grad_check(f"{mode} padded coef", coef.cpu().numpy(), want["coef"].numpy())
        assert bool((coef[empty, :K] == 0).all())
        if mode == "softmax":
            assert bool((coef[empty, K] == 0).all()) and bool((dq[empty] == 0).all())    # p_t = 1: nothing to learn
        else:
            assert bool((coef[empty, K] != 0).all())                                      # the positive term alone


def test_hub_one_id_in_every_position():
    """B = 129, K = 65: one segment_axpy segment of 8,385 entries."""
    N, d, B, K = 300, 64, 129, 65
    model = model16()
    embs, q, t, _, _, _, bias, grad = setup(d, K, B, N, seed=5)
    t[t == 17] = 18
    neg = torch.full((B, K), 17, dtype=torch.int64, device=DEV)
    for mode in ("softmax", "negsamp"):
        fn = model.softmax_loss if mode == "softmax" else model.negative_sampling_loss
        kw = {} if mode == "softmax" else dict(margin=0.5, adversarial_temperature=0.5)
        e, b = embs.clone().requires_grad_(), bias.clone().requires_grad_()
        loss = fn(e, q, t, scale=0.2, negatives=neg, candidate_bias=b, **kw)
        (loss * grad).sum().backward()
        want = R.loss(mode, embs[q], embs, t, neg, None, bias, scale=0.2, margin=kw.get("margin", 0.0),
                      alpha=kw.get("adversarial_temperature", 0.0), grad=grad)
        loss_check(f"{mode} hub", loss, want["loss"])
        grad_check(f"{mode} hub embs", e.grad.cpu().numpy(), R.embs_grad(want, q).numpy())
        grad_check(f"{mode} hub bias", b.grad.cpu().numpy(), want["db"].numpy())


def test_untouched_rows_get_exactly_zero():
    N, d, B, K = 5000, 128, 129, 9
    model = model16()
    embs, q, t, neg, lists, known, bias, grad = setup(d, K, B, N, seed=9)
    touched = torch.zeros(N, dtype=torch.bool, device=DEV)
    touched[q] = True
    touched[t] = True
    touched[neg[neg >= 0]] = True
    assert int((~touched).sum()) > 1000 and not bool(touched[0])             # node 0, where a clamped padding id would land
    for mode in ("softmax", "negsamp"):
        fn = model.softmax_loss if mode == "softmax" else model.negative_sampling_loss
        e, b = embs.clone().requires_grad_(), bias.clone().requires_grad_()
        (fn(e, q, t, known=known, negatives=neg, candidate_bias=b) * grad).sum().backward()
        assert int(bits(e.grad[~touched]).abs().sum()) == 0 and int(bits(b.grad[~touched]).abs().sum()) == 0
        assert bool((e.grad[touched].abs().sum(1) > 0).any())


# ---- 5. invalid ids at the raw level, reproducibility, batch independence ----------------------------------------------
def raw_all(embs, q, t, neg, ptr, idx, bias, grad):
    kw = dict(iq=q, filt_ptr=ptr, filt_idx=idx, bias=bias)
    greater, equal = _native.score_neg_rank(embs, embs, t, neg, **kw)
    loss, lse = _native.score_neg_softmax_fwd(embs, embs, t, neg, scale=0.4, **kw)
    nl, lw = _native.score_neg_negsamp_fwd(embs, embs, t, neg, scale=0.4, margin=1.0, adversarial_temperature=0.5, **kw)
    dq1, c1 = _native.score_neg_bwd(_native.NEG_SOFTMAX, embs, embs, t, neg, lse, grad, scale=0.4, **kw)
    dq2, c2 = _native.score_neg_bwd(_native.NEG_NEGSAMP, embs, embs, t, neg, lw, grad, scale=0.4, margin=1.0,
                                    adversarial_temperature=0.5, **kw)
    return dict(greater=greater, equal=equal, loss=loss, lse=lse, nl=nl, lw=lw, dq1=dq1, c1=c1, dq2=dq2, c2=c2)


@pytest.mark.parametrize("d,K", [(128, 65), (20, 9), (3, 7)])
def test_invalid_ids_touch_their_query_alone(d, K):
    N, B = 300, 9
    embs, q, t, neg, lists, _, bias, grad = setup(d, K, B, N, seed=d + 3)
    ptr, idx = csr(lists)
    good = raw_all(embs, q, t, neg, ptr, idx, bias, grad)
    bad_neg = neg.clone()
    bad_neg[2, K - 1] = N                                                    # one past the table
    bad_neg[5, 0] = -2                                                       # not the padding
    bad_q, bad_t = q.clone(), t.clone()
    bad_q[7] = N + 5
    bad_t[1] = -1
    got = raw_all(embs, bad_q, bad_t, bad_neg, ptr, idx, bias, grad)
    torch.cuda.synchronize()
    invalid = torch.tensor([1, 2, 5, 7], device=DEV)
    others = torch.tensor([0, 3, 4, 6, 8], device=DEV)
    for k, v in got.items():
        assert torch.equal(bits(v[others]), bits(good[k][others])), k
    assert bool((got["greater"][invalid] == -1).all()) and bool((got["equal"][invalid] == -1).all())
    for k in ("loss", "lse", "nl", "lw"):
        assert bool(torch.isnan(got[k][invalid]).all()), k
    for k in ("dq1", "c1", "dq2", "c2"):
        assert bool((got[k][invalid] == 0).all()), k
    # a listed id out of range invalidates the query that lists it
    bad_idx = idx.clone()
    owner = int(np.searchsorted(ptr.cpu().numpy(), 0, side="right") - 1)
    bad_idx[0] = N
    l2 = _native.score_neg_softmax_fwd(embs, embs, t, neg, iq=q, filt_ptr=ptr, filt_idx=bad_idx, scale=0.4, bias=bias)[0]
    assert bool(torch.isnan(l2[owner])) and int(torch.isnan(l2).sum()) == 1


@pytest.mark.parametrize("d,K", [(128, 257), (64, 9), (200, 65)])
def test_twice_the_same_bits_and_a_query_alone_as_in_its_batch(d, K):
    N, B = 300, 129
    model = model16()
    embs, q, t, neg, lists, known, bias, grad = setup(d, K, B, N, seed=K)
    ptr, idx = csr(lists)
    one = raw_all(embs, q, t, neg, ptr, idx, bias, grad)
    two = raw_all(embs, q, t, neg, ptr, idx, bias, grad)
    for k in one:
        assert torch.equal(bits(one[k]), bits(two[k])), k
    grads = []
    for _ in range(2):
        e, b = embs.clone().requires_grad_(), bias.clone().requires_grad_()
        (model.negative_sampling_loss(e, q, t, known=known, negatives=neg, candidate_bias=b, adversarial_temperature=1.0) * grad
         ).sum().backward()
        grads.append((e.grad, b.grad))
    assert torch.equal(bits(grads[0][0]), bits(grads[1][0])) and torch.equal(bits(grads[0][1]), bits(grads[1][1]))
    for i in (0, 77, 128):                                                    # alone: B = 1, first place
        pi, xi = csr([lists[i]])
        alone = raw_all(embs, q[i:i + 1], t[i:i + 1], neg[i:i + 1], pi, xi, bias, grad[i:i + 1])
        for k in alone:
            assert torch.equal(bits(alone[k][0]), bits(one[k][i])), (k, i)


# ---- 6. end to end ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["softmax", "negsamp"])
def test_backward_through_the_model_matches_float64_autograd(mode):
    """loss.backward() through HyperGNN on the toy graph: the parameters' gradients against float64 autograd through the
    oracle's forward and a dense formulation of the loss."""
    from oracle import hypergnn_oracle as O
    torch.manual_seed(0)
    kg = ToyKnowledgeGraph(feat_dim=16)
    model = model16().train()
    x, ei, texts = kg.node_features.to(DEV), kg.edge_index.to(DEV), kg.edge_texts
    N = x.size(0)
    rng = np.random.default_rng(4)
    B, K = 7, 5
    q = torch.from_numpy(rng.integers(0, N, B)).to(DEV)
    t = torch.from_numpy(rng.integers(0, N, B)).to(DEV)
    neg = torch.from_numpy(rng.integers(-1, N, (B, K))).to(DEV)
    neg[:, 1] = neg[:, 0]
    kw = {} if mode == "softmax" else dict(margin=1.0, adversarial_temperature=1.0)
    fn = model.softmax_loss if mode == "softmax" else model.negative_sampling_loss
    loss = fn(model(x, ei, texts), q, t, scale=0.5, negatives=neg, **kw).sum()
    loss.backward()

    params = {k: v.detach().cpu().double().requires_grad_(True) for k, v in model.state_dict().items()}
    e64 = O.forward(params, kg.node_features.double(), kg.edge_index.numpy(), texts, variant="factorised", dtype=torch.float64)
    qc, tc, nc = q.cpu(), t.cpu(), neg.cpu()
    z = 0.5 * torch.bmm(e64[nc.clamp(min=0)], e64[qc].unsqueeze(2)).squeeze(2)
    zt = 0.5 * (e64[qc] * e64[tc]).sum(1)
    drop = (nc == -1) | (nc == tc.unsqueeze(1))
    if mode == "softmax":
        want = (torch.logsumexp(torch.cat([zt.unsqueeze(1), z.masked_fill(drop, -np.inf)], 1), 1) - zt).sum()
    else:
        w = torch.nan_to_num(torch.softmax(z.masked_fill(drop, -np.inf), 1).detach())
        want = (torch.nn.functional.softplus(-(zt + 1.0)) + (w * torch.nn.functional.softplus(z + 1.0).masked_fill(drop, 0.0)).sum(1)).sum()
    loss_check(f"{mode} through the model", loss.reshape(1), want.detach().reshape(1))
    want.backward()
    # grad_check's absolute term is 1e-4 of the tensor's largest entry.  A generator's three log-scales are one-element parameters, each
    # the sum sum(dW * W) over one generated tensor: taken alone, one that cancels (here layer 1's W_msg, 1e-3 of layer 0's) has
    # nothing to set that term by.  They are compared as the vector they form per generator.
    checked, scalars = 0, {}
    for k, p in model.named_parameters():
        if params[k].grad is not None and float(params[k].grad.abs().max()) > 0:
            assert p.grad is not None, f"no gradient on {k}"
            if p.numel() == 1:
                scalars.setdefault(k.rsplit(".", 1)[0], []).append((p.grad.cpu().numpy(), params[k].grad.numpy()))
                continue
            grad_check(k, p.grad.cpu().numpy(), params[k].grad.numpy())
            checked += 1
    for k, pairs in scalars.items():
        grad_check(k, np.concatenate([g.reshape(-1) for g, _ in pairs]), np.concatenate([w.reshape(-1) for _, w in pairs]))
        checked += 1
    assert checked >= 10
