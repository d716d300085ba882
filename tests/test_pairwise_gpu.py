"""Pairwise ranking losses on the device (HyperGNN.pairwise_loss; include/ghf_pairwise.h; csrc/pairwise.hip) against the
float64 restatement of tests/_pairwise_ref.py.

Tolerances are the project's own, through loss_check / grad_check of tests/test_softmax_gpu.py; counts must be equal.  The
parity problems and their seeds are _pairwise_ref's: tests/test_pairwise_host.py holds every one of them to "no pair inside
the near-tie band 1e-4 (1 + |z_it| + |margin|) around the kink", so nothing is excused here — `active` and every hinge
coefficient are compared as they are.  The shapes cross every lane-group width (L = 8, 16, 32, 64 at d <= 32, 64, 128, 256;
the scalar path where d % 4 != 0) with K around a step of 8 x 64 / L positions and around 256, above which a query's
positions are dealt to four waves; B = 129 leaves the last workgroup of four queries with one.

Measured on an MI355X, the worst over every case of this file: a loss at 0.022 of loss_check's bound (relative L2 3.6e-7);
gradients at a relative L2 of 1.7e-6 against grad_check's 5e-5."""

import functools

import numpy as np
import pytest
import torch

import _pairwise_ref as R
from graph_hypernetwork_forge_amd import ToyKnowledgeGraph, _native
from test_softmax_gpu import csr, grad_check, loss_check, model16

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
METRIC = {"dot": _native.PAIR_DOT, "l1": _native.DIST_L1, "l2": _native.DIST_L2, "complex": _native.DIST_COMPLEX}
KIND = {"hinge": _native.PAIR_HINGE, "logistic": _native.PAIR_LOGISTIC}
CASES = R.parity_cases()
IDS = ["d%d-K%d-B%d-N%d-%s" % (s + (v,)) for s, v, _ in CASES]


def bits(t):
    t = t.detach().contiguous()
    return t.view({4: torch.int32, 8: torch.int64}[t.element_size()])


def dist_kw(score):
    return {} if score == "dot" else dict(distance=score)


@functools.lru_cache(maxsize=None)
def reference(case, kind, normalize):
    """The float64 restatement of a parity problem, computed once and shared."""
    (d, K, B, N), variant, seed = case
    score = R.variant_score(variant)
    p = R.problem(d, K, B, N, seed)
    return R.loss(kind, score, p["embs"][p["query"]], p["embs"], p["target"], p["neg"], p["lists"],
                  p["bias"] if variant == "dot+bias" else None, R.parity_scale(score, d), R.MARGIN, normalize, grad=p["grad"])


def on_device(p):
    out = {k: v.to(DEV) for k, v in p.items() if isinstance(v, torch.Tensor)}
    out["known"] = tuple(t.to(DEV) for t in p["known"])
    out["lists"] = p["lists"]
    return out


# ---- 1. parity ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_parity_with_float64(case):
    """Both kinds, normalize on and off; by id with known= and by query_rows with CSR lists (the same bits); the loss, the
    counts, coef, dq, d embs, d rows and d bias."""
    (d, K, B, N), variant, seed = case
    score = R.variant_score(variant)
    scale = R.parity_scale(score, d)
    model = model16()
    p = on_device(R.problem(d, K, B, N, seed))
    embs, q, t, neg, grad = p["embs"], p["query"], p["target"], p["neg"], p["grad"]
    bias = p["bias"] if variant == "dot+bias" else None
    ptr, idx = csr(p["lists"])
    for kind in R.KINDS:
        for normalize in (True, False):
            want = reference(case, kind, normalize)
            what = f"{kind} normalize={normalize}"
            e = embs.clone().requires_grad_()
            bb = None if bias is None else bias.clone().requires_grad_()
            loss, active = model.pairwise_loss(e, q, t, negatives=neg, loss=kind, margin=R.MARGIN, scale=scale, normalize=normalize,
                                               known=p["known"], candidate_bias=bb, return_active=True, **dist_kw(score))
            assert loss.dtype == torch.float32 and active.dtype == torch.int32 and not active.requires_grad
            loss_check(f"{what} loss", loss, want["loss"])
            assert torch.equal(active.cpu().long(), want["active"]), what
            (loss * grad).sum().backward()
            grad_check(f"{what} embs", e.grad.cpu().numpy(), R.embs_grad(want, q).numpy())
            if bb is not None:
                grad_check(f"{what} bias", bb.grad.cpu().numpy(), want["db"].numpy())
            # by rows, with CSR lists: the same call underneath
            e2, rows = embs.clone().requires_grad_(), embs[q].clone().requires_grad_()
            loss2 = model.pairwise_loss(e2, q, t, negatives=neg, loss=kind, margin=R.MARGIN, scale=scale, normalize=normalize,
                                        filt_ptr=ptr, filt_idx=idx, query_rows=rows, candidate_bias=bias, **dist_kw(score))
            assert torch.equal(bits(loss2), bits(loss)), what
            (loss2 * grad).sum().backward()
            grad_check(f"{what} rows", rows.grad.cpu().numpy(), want["dq"].numpy())
            grad_check(f"{what} embs by rows", e2.grad.cpu().numpy(), want["dc"].numpy())
            # the two entry points themselves
            kw = dict(iq=q, filt_ptr=ptr, filt_idx=idx, scale=scale, margin=R.MARGIN, normalize=normalize, bias=bias)
            l, count, act = _native.score_pair_fwd(METRIC[score], KIND[kind], embs, embs, t, neg, **kw)
            assert torch.equal(bits(l), bits(loss)) and torch.equal(act, active)
            assert count.dtype == torch.int32 and torch.equal(count.cpu().long(), want["count"])
            dq, coef = _native.score_pair_bwd(METRIC[score], KIND[kind], embs, embs, t, neg, count, grad, **kw)
            grad_check(f"{what} dq", dq.cpu().numpy(), want["dq"].numpy())
            grad_check(f"{what} coef", coef.cpu().numpy(), want["coef"].numpy())
            assert bool((coef[:, :K][~want["live"].to(DEV)] == 0).all())                  # exactly 0 outside J_i
            no_grad = model.pairwise_loss(embs, q, t, negatives=neg, loss=kind, margin=R.MARGIN, scale=scale, normalize=normalize,
                                          known=p["known"], candidate_bias=bias, **dist_kw(score))
            assert torch.equal(bits(no_grad), bits(loss))                                 # recorded or not: the same forward


@pytest.mark.parametrize("score", R.SCORES)
def test_typed_known_lists(score):
    d, K, B, N = 64, 9, 129, 300
    model = model16()
    p = on_device(R.problem(d, K, B, N, seed=11))
    embs, q, t, neg, grad = p["embs"], p["query"], p["target"], p["neg"], p["grad"]
    rng = np.random.default_rng(d)
    E = 400
    src, dst, rel = (torch.from_numpy(rng.integers(0, n, E)).to(DEV) for n in (N, N, 3))
    src[:B], dst[:B], rel[:B] = q, neg[:, 0].clamp(min=0), 1                # every query lists its first negative under rel 1
    qrel = torch.from_numpy(rng.integers(0, 3, B)).to(DEV)
    lists = [np.unique(dst[(src == q[i]) & (rel == qrel[i])].cpu().numpy()) for i in range(B)]
    scale = R.parity_scale(score, d)
    for kind in R.KINDS:
        e = embs.clone().requires_grad_()
        loss, active = model.pairwise_loss(e, q, t, negatives=neg, loss=kind, scale=scale, known=(src, dst, rel), query_rel=qrel,
                                           return_active=True, **dist_kw(score))
        want = R.loss(kind, score, embs[q], embs, t, neg, lists, None, scale, 1.0, True, grad=grad)
        untyped = R.loss(kind, score, embs[q], embs, t, neg, None, None, scale, 1.0, True)
        assert not torch.equal(want["count"], untyped["count"])                         # (the lists do remove something)
        loss_check(f"{kind} typed loss", loss, want["loss"])
        near = (torch.where(want["live"], want["u"].abs(), torch.ones_like(want["u"])) < R.band(want["zt"], 1.0).unsqueeze(1)).sum(1)
        assert bool(((active.cpu().long() - want["active"]).abs() <= near).all())
        if int(near.sum()) == 0 or kind == "logistic":
            (loss * grad).sum().backward()
            grad_check(f"{kind} typed embs", e.grad.cpu().numpy(), R.embs_grad(want, q).numpy())


# ---- 2. exact data -----------------------------------------------------------------------------------------------------------
def integer_rows(N, d, seed):
    return torch.from_numpy(np.random.default_rng(seed).integers(-4, 5, (N, d)).astype(np.float32)).to(DEV)


@pytest.mark.parametrize("d,K,B,N", [(1, 65, 5, 300), (3, 9, 129, 300), (20, 257, 5, 300), (64, 63, 129, 300), (128, 1000, 5, 300),
                                     (200, 65, 5, 300), (256, 9, 129, 300), (256, 257, 5, 300)])
def test_exact_on_integer_rows(d, K, B, N):
    """Entries in {-4..4}, an integer bias and integer margins: every product, difference and partial sum is an integer below
    2^24 (|dot| <= 16 d, L1 <= 8 d, the hinge sum at most K (32 d + 8) < 2^24), so dot and L1 are exact in fp32 whatever the
    order: the unnormalised hinge loss equals float64 bit for bit, `active` equals `greater` at margin 0 and the reference's
    count at margin 2."""
    model = model16()
    p = on_device(R.problem(d, K, B, N, seed=d + K))
    q, t, neg = p["query"], p["target"], p["neg"]
    embs = integer_rows(N, d, seed=d)
    embs[N - 40:] = embs[:40]
    t = torch.arange(B, device=DEV) % 40
    neg[:, 0] = N - 40 + t                                                   # a copy of the target, first in every row: u == margin
    bias = torch.from_numpy(np.random.default_rng(K).integers(-3, 4, N).astype(np.float32)).to(DEV)
    for score, b in (("dot", None), ("dot", bias), ("l1", None), ("l2", None), ("complex", None)):
        if score == "complex" and d % 2:
            continue
        kw = dict(negatives=neg, known=p["known"], candidate_bias=b, **dist_kw(score))
        greater, _ = model.rank_candidates(embs, q, t, **kw)
        for margin in (0.0, 2.0):
            loss, active = model.pairwise_loss(embs, q, t, loss="hinge", margin=margin, normalize=False, return_active=True, **kw)
            want = R.loss("hinge", score, embs[q], embs, t, neg, p["lists"], b, 1.0, margin, False)
            if margin == 0.0:
                assert torch.equal(active.long(), greater), (score, "active is greater at margin 0")
            if score in ("dot", "l1"):
                assert torch.equal(active.cpu().long(), want["active"]), (score, margin)
                assert torch.equal(loss.cpu().double(), want["loss"]), (score, margin)      # bit for bit: float64's value is an fp32
                soft = model.pairwise_loss(embs, q, t, loss="logistic", margin=margin, normalize=False, return_active=True, **kw)[1]
                assert torch.equal(soft, active)                                            # the count does not depend on the kind
        assert int(want["active"].sum()) > 0


# ---- 3. the kink -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,K", [(20, 9), (128, 65), (6, 7), (256, 257)])
def test_the_kink_and_the_sum_behind_the_target_coefficient(d, K):
    """Integer rows under the dot product.  Query 0: its first negative is a copy of the target and margin = 0, so u == 0
    exactly — no loss, no coefficient.  Query 1: every negative scores below the target by more than the margin — loss 0, an
    all-zero coef row and an all-zero dq row.  Every query: coef[i, K] is minus the row's sum in the documented order."""
    N, B = 300, 5
    p = on_device(R.problem(d, K, B, N, seed=K))
    embs = integer_rows(N, d, seed=K + 1)
    grad = p["grad"]
    q, t = torch.arange(B, device=DEV), torch.arange(B, device=DEV) + 10     # queries 0 .. 4, targets 10 .. 14, negatives from 20 on
    neg = torch.where(p["neg"] < 0, p["neg"], 20 + p["neg"] % (N - 20))
    embs[10] = embs[N - 1]
    neg[0] = -1
    neg[0, 0] = N - 1                                                       # the one pair of query 0: a copy of its target
    embs[1] = 0.0
    embs[1, 0] = 1.0                                                        # z = x_0
    embs[11, 0] = 4.0                                                       # z_t = 4; negatives with x_0 <= 2: u <= margin - 2 < 0
    low = ((embs[:, 0] <= 2) & (torch.arange(N, device=DEV) >= 20)).nonzero().flatten()
    neg[1] = low[torch.arange(K, device=DEV) % low.numel()]
    vec = d % 4 == 0
    for kind in R.KINDS:
        for margin, normalize in ((0.0, True), (1.0, False), (0.5, True)):
            kw = dict(iq=q, scale=1.0, margin=margin, normalize=normalize)
            loss, count, active = _native.score_pair_fwd(_native.PAIR_DOT, KIND[kind], embs, embs, t, neg, **kw)
            dq, coef = _native.score_pair_bwd(_native.PAIR_DOT, KIND[kind], embs, embs, t, neg, count, grad, **kw)
            want = R.loss(kind, "dot", embs[q], embs, t, neg, None, None, 1.0, margin, normalize, grad=grad)
            loss_check(f"{kind} {margin} loss", loss, want["loss"])
            grad_check(f"{kind} {margin} coef", coef.cpu().numpy(), want["coef"].numpy())
            if kind == "hinge":
                assert int(count[0]) == 1
                if margin == 0.0:
                    assert int(active[0]) == 0 and int(bits(loss[:1])) == 0 and int(bits(coef[0]).abs().sum()) == 0
                    assert int(bits(dq[0]).abs().sum()) == 0
                else:
                    assert int(active[0]) == 1 and float(loss[0]) == margin
                assert int(count[1]) == K and int(active[1]) == 0 and int(bits(loss[1:2])) == 0
                assert int(bits(coef[1]).abs().sum()) == 0 and int(bits(dq[1]).abs().sum()) == 0
            rows = coef.cpu().numpy()
            for i in range(B):
                s = R.documented_row_sum(rows[i, :K], d, vec)
                assert np.float32(0.0) - s == rows[i, K], (kind, margin, i, s, rows[i, K])


# ---- 4. bits -----------------------------------------------------------------------------------------------------------------
def raw_all(score, embs, q, t, neg, ptr, idx, bias, grad, c=None):
    out = {}
    c = embs if c is None else c
    for kind in R.KINDS:
        kw = dict(iq=q, filt_ptr=ptr, filt_idx=idx, scale=R.parity_scale(score, embs.size(1)), margin=0.7, normalize=True,
                  bias=bias if score == "dot" else None)
        loss, count, active = _native.score_pair_fwd(METRIC[score], KIND[kind], embs, c, t, neg, **kw)
        dq, coef = _native.score_pair_bwd(METRIC[score], KIND[kind], embs, c, t, neg, count, grad, **kw)
        out.update({f"{kind} loss": loss, f"{kind} count": count, f"{kind} active": active, f"{kind} dq": dq, f"{kind} coef": coef})
    return out


@pytest.mark.parametrize("d,K", [(128, 257), (64, 9), (200, 65)])
@pytest.mark.parametrize("score", R.SCORES)
def test_twice_the_same_bits_and_a_query_alone_as_in_its_batch(d, K, score):
    N, B = 300, 129
    model = model16()
    p = on_device(R.problem(d, K, B, N, seed=K))
    embs, q, t, neg, bias, grad = p["embs"], p["query"], p["target"], p["neg"], p["bias"], p["grad"]
    ptr, idx = csr(p["lists"])
    one = raw_all(score, embs, q, t, neg, ptr, idx, bias, grad)
    two = raw_all(score, embs, q, t, neg, ptr, idx, bias, grad)
    for k in one:
        assert torch.equal(bits(one[k]), bits(two[k])), k
    grads = []
    for _ in range(2):
        e = embs.clone().requires_grad_()
        b = bias.clone().requires_grad_() if score == "dot" else None
        (model.pairwise_loss(e, q, t, negatives=neg, known=p["known"], candidate_bias=b, loss="logistic", **dist_kw(score)) * grad
         ).sum().backward()
        grads.append((e.grad, e.grad if b is None else b.grad))
    assert torch.equal(bits(grads[0][0]), bits(grads[1][0])) and torch.equal(bits(grads[0][1]), bits(grads[1][1]))
    for i in (0, 77, 128):                                                    # alone: B = 1, first place
        pi, xi = csr([p["lists"][i]])
        alone = raw_all(score, embs, q[i:i + 1], t[i:i + 1], neg[i:i + 1], pi, xi, bias, grad[i:i + 1])
        for k in alone:
            assert torch.equal(bits(alone[k][0]), bits(one[k][i])), (k, i)


@pytest.mark.parametrize("d,K", [(128, 65), (20, 257), (256, 9)])
@pytest.mark.parametrize("score", R.SCORES)
def test_scalar_path_from_an_unaligned_base_agrees(d, K, score):
    """The same rows four bytes further on: q and c are no longer 16-byte aligned, the scalar path runs.  Parity with float64
    and with the vector path, not bit equality (the order of every sum differs)."""
    N, B = 300, 5
    p = on_device(R.problem(d, K, B, N, seed=3 * K))
    embs, q, t, neg, bias, grad = p["embs"], p["query"], p["target"], p["neg"], p["bias"], p["grad"]
    buf = torch.empty(N * d + 1, dtype=torch.float32, device=DEV)
    shifted = buf[1:].view(N, d)
    shifted.copy_(embs)
    assert embs.data_ptr() % 16 == 0 and shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
    ptr, idx = csr(p["lists"])
    vec = raw_all(score, embs, q, t, neg, ptr, idx, bias, grad)
    sca = raw_all(score, shifted, q, t, neg, ptr, idx, bias, grad)
    for kind in R.KINDS:
        want = R.loss(kind, score, embs[q], embs, t, neg, p["lists"], bias if score == "dot" else None, R.parity_scale(score, d), 0.7,
                      True, grad=grad)
        for got in (vec, sca):
            loss_check(f"{kind} loss", got[f"{kind} loss"], want["loss"])
            grad_check(f"{kind} dq", got[f"{kind} dq"].cpu().numpy(), want["dq"].numpy())
            assert torch.equal(got[f"{kind} count"].cpu().long(), want["count"])
        if kind == "logistic":
            grad_check("logistic coef", sca["logistic coef"].cpu().numpy(), want["coef"].numpy())


@pytest.mark.parametrize("score", R.SCORES)
def test_K_256_against_K_257_with_a_trailing_padding(score):
    """One wave against four over the same J_i: the same counts, the loss within loss_check of each other and of float64."""
    d, N, B = 128, 300, 5
    p = on_device(R.problem(d, 256, B, N, seed=5))
    embs, q, t, neg, grad = p["embs"], p["query"], p["target"], p["neg"], p["grad"]
    wide = torch.cat([neg, torch.full((B, 1), -1, dtype=torch.int64, device=DEV)], 1)
    scale = R.parity_scale(score, d)
    for kind in R.KINDS:
        a = _native.score_pair_fwd(METRIC[score], KIND[kind], embs, embs, t, neg, iq=q, scale=scale, margin=0.7)
        b = _native.score_pair_fwd(METRIC[score], KIND[kind], embs, embs, t, wide, iq=q, scale=scale, margin=0.7)
        assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
        want = R.loss(kind, score, embs[q], embs, t, neg, None, None, scale, 0.7, True)
        loss_check(f"{kind} K 256", a[0], want["loss"])
        loss_check(f"{kind} K 257", b[0], want["loss"])
        loss_check(f"{kind} 256 | 257", b[0], a[0].double())
        ca = _native.score_pair_bwd(METRIC[score], KIND[kind], embs, embs, t, neg, a[1], grad, iq=q, scale=scale, margin=0.7)[1]
        cb = _native.score_pair_bwd(METRIC[score], KIND[kind], embs, embs, t, wide, b[1], grad, iq=q, scale=scale, margin=0.7)[1]
        assert torch.equal(bits(ca[:, :256]), bits(cb[:, :256])) and int(bits(cb[:, 256]).abs().sum()) == 0


# ---- 5. edge cases -----------------------------------------------------------------------------------------------------------
def crossed(shapes):
    """[(d, K, score)]: every shape under every score it admits (complex reads pairs: even d only)."""
    return [(d, K, s) for d, K in shapes for s in R.SCORES if s != "complex" or d % 2 == 0]


@pytest.mark.parametrize("d,K,score", crossed([(20, 65), (128, 17), (256, 9), (3, 7), (64, 257)]))
def test_empty_sets_by_padding_by_the_list_and_by_the_target(d, K, score):
    N, B = 300, 6
    p = on_device(R.problem(d, K, B, N, seed=K))
    embs, q, t, neg, grad = p["embs"], p["query"], p["target"], p["neg"], p["grad"]
    neg = torch.where(neg < 0, (t.unsqueeze(1) + 1) % N, neg)
    neg[3] = -1                                                              # a whole row of padding
    neg[4] = t[4]                                                            # every negative is the target
    lists = [np.zeros(0, dtype=np.int64)] * B
    lists[5] = np.unique(neg[5].cpu().numpy())                               # every negative is listed
    ptr, idx = csr(lists)
    empty = torch.tensor([3, 4, 5], device=DEV)
    scale = R.parity_scale(score, d)
    for kind in R.KINDS:
        for normalize in (True, False):
            kw = dict(iq=q, filt_ptr=ptr, filt_idx=idx, scale=scale, margin=1.0, normalize=normalize)
            loss, count, active = _native.score_pair_fwd(METRIC[score], KIND[kind], embs, embs, t, neg, **kw)
            assert int(bits(loss[empty]).abs().sum()) == 0                   # exactly +0
            assert int(count[empty].abs().sum()) == 0 and int(active[empty].abs().sum()) == 0
            dq, coef = _native.score_pair_bwd(METRIC[score], KIND[kind], embs, embs, t, neg, count, grad, **kw)
            assert int(bits(coef[empty]).abs().sum()) == 0 and int(bits(dq[empty]).abs().sum()) == 0
            want = R.loss(kind, score, embs[q], embs, t, neg, lists, None, scale, 1.0, normalize, grad=grad)
            loss_check(f"{kind} loss", loss, want["loss"])
            assert torch.equal(count.cpu().long(), want["count"])
            if kind == "logistic":
                grad_check(f"{kind} coef", coef.cpu().numpy(), want["coef"].numpy())


@pytest.mark.parametrize("d,K,score", crossed([(128, 65), (20, 9), (3, 7), (64, 300)]))
def test_invalid_ids_touch_their_query_alone(d, K, score):
    N, B = 300, 9
    p = on_device(R.problem(d, K, B, N, seed=d + 3))
    embs, q, t, neg, bias, grad = p["embs"], p["query"], p["target"], p["neg"], p["bias"], p["grad"]
    lists = [l if len(l) else np.array([int(t[i])]) for i, l in enumerate(p["lists"])]
    ptr, idx = csr(lists)
    good = raw_all(score, embs, q, t, neg, ptr, idx, bias, grad)
    bad_neg = neg.clone()
    bad_neg[2, K - 1] = N                                                    # one past the table
    bad_neg[5, 0] = -2                                                       # not the padding
    bad_q, bad_t, bad_idx = q.clone(), t.clone(), idx.clone()
    bad_q[7] = N + 5
    bad_t[1] = -1
    bad_idx[int(ptr[4])] = N                                                 # a listed id out of range: query 4's
    got = raw_all(score, embs, bad_q, bad_t, bad_neg, ptr, bad_idx, bias, grad)
    torch.cuda.synchronize()
    invalid = torch.tensor([1, 2, 4, 5, 7], device=DEV)
    others = torch.tensor([0, 3, 6, 8], device=DEV)
    for k, v in got.items():
        assert torch.equal(bits(v[others]), bits(good[k][others])), k
        if k.endswith("loss"):
            assert bool(torch.isnan(v[invalid]).all()), k
        elif k.endswith(("count", "active")):
            assert bool((v[invalid] == -1).all()), k
        else:
            assert int(bits(v[invalid]).abs().sum()) == 0, k


@pytest.mark.parametrize("score", ["l1", "l2", "complex"])
@pytest.mark.parametrize("d", [128, 6])
def test_a_candidate_equal_to_the_query_row_has_zero_gradient(score, d):
    """D = 0: g is 0 by the conventions of include/ghf_distance.h.  The pair is violated (u = margin + D_t > 0), so its
    coefficient is not 0 — yet it moves neither the query's row nor the candidate's."""
    N, B, K = 50, 3, 4
    p = on_device(R.problem(d, K, B, N, seed=d))
    embs, grad = p["embs"], p["grad"]
    q = torch.tensor([0, 1, 2], device=DEV)
    t = torch.tensor([10, 11, 12], device=DEV)
    neg = torch.full((B, K), -1, dtype=torch.int64, device=DEV)
    neg[:, 0] = q + 20
    embs[20:23] = embs[0:3]                                                  # copies of the query rows, named by no one else
    model = model16()
    e = embs.clone().requires_grad_()
    loss = model.pairwise_loss(e, q, t, negatives=neg, distance=score, margin=1.0)
    (loss * grad).sum().backward()
    count = torch.ones(B, dtype=torch.int32, device=DEV)
    dq, coef = _native.score_pair_bwd(METRIC[score], _native.PAIR_HINGE, embs, embs, t, neg, count, grad, iq=q, margin=1.0)
    assert bool((coef[:, 0] != 0).all()) and int(bits(e.grad[20:23]).abs().sum()) == 0
    want = R.loss("hinge", score, embs[q], embs, t, neg, None, None, 1.0, 1.0, True, grad=grad)
    grad_check("dq", dq.cpu().numpy(), want["dq"].numpy())
    grad_check("embs", e.grad.cpu().numpy(), R.embs_grad(want, q).numpy())


# ---- 6. through the model ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.KINDS)
def test_transe_through_the_model_matches_float64_autograd(kind):
    """The published TransE objective on a 2-layer HyperGNN over the toy graph: rows = embs[head] + rel_vec[rel], L1 distance,
    the pairwise loss; the gradients of every parameter and of rel_vec against float64 autograd through the oracle's forward
    and a dense formulation of the loss."""
    from oracle import hypergnn_oracle as O
    torch.manual_seed(0)
    kg = ToyKnowledgeGraph(feat_dim=16)
    model = model16().train()
    x, ei, texts = kg.node_features.to(DEV), kg.edge_index.to(DEV), kg.edge_texts
    N = x.size(0)
    rng = np.random.default_rng(4)
    B, K, nrel = 7, 5, 3
    head = torch.from_numpy(rng.integers(0, N, B)).to(DEV)
    tail = torch.from_numpy(rng.integers(0, N, B)).to(DEV)
    rel = torch.from_numpy(rng.integers(0, nrel, B)).to(DEV)
    neg = torch.from_numpy(rng.integers(-1, N, (B, K))).to(DEV)
    neg[:, 1] = neg[:, 0]
    rel_vec = torch.from_numpy(rng.standard_normal((nrel, 16)).astype(np.float32)).to(DEV).requires_grad_()
    embs = model(x, ei, texts)
    rows = embs[head] + rel_vec[rel]
    loss = model.pairwise_loss(embs, head, tail, negatives=neg, query_rows=rows, distance="l1", margin=2.0, loss=kind).sum()
    loss.backward()

    params = {k: v.detach().cpu().double().requires_grad_(True) for k, v in model.state_dict().items()}
    r64 = rel_vec.detach().cpu().double().requires_grad_()
    e64 = O.forward(params, kg.node_features.double(), kg.edge_index.numpy(), texts, variant="factorised", dtype=torch.float64)
    hc, tc, rc, nc = head.cpu(), tail.cpu(), rel.cpu(), neg.cpu()
    q64 = e64[hc] + r64[rc]
    z = -(q64.unsqueeze(1) - e64[nc.clamp(min=0)]).abs().sum(-1)
    zt = -(q64 - e64[tc]).abs().sum(-1)
    live = (nc != -1) & (nc != tc.unsqueeze(1))
    u = z - zt.unsqueeze(1) + 2.0
    assert float(torch.where(live, u.abs(), torch.ones_like(u)).detach().min()) > 1e-3   # no pair at the kink
    phi = torch.relu(u) if kind == "hinge" else torch.nn.functional.softplus(u)
    want = ((phi * live).sum(1) / live.sum(1).clamp(min=1)).sum()
    loss_check(f"{kind} through the model", loss.reshape(1), want.detach().reshape(1))
    want.backward()
    grad_check("rel_vec", rel_vec.grad.cpu().numpy(), r64.grad.numpy())
    checked, scalars = 0, {}
    for k, p in model.named_parameters():                                            # (one-element parameters: as one vector per
        if params[k].grad is not None and float(params[k].grad.abs().max()) > 0:    # generator, as in test_negatives_gpu.py)
            assert p.grad is not None, f"no gradient on {k}"
            # A distance depends on differences of rows alone, so the loss does not move when every row moves together: the
            # last LayerNorm's bias has gradient exactly 0 (float64 gives 1e-16, fp32 1e-7), which taken alone leaves grad_check
            # no scale.  A LayerNorm's weight and bias are compared as the one vector they form.
            if p.numel() == 1 or k.startswith("layer_norms."):
                scalars.setdefault(k.rsplit(".", 1)[0], []).append((p.grad.cpu().numpy(), params[k].grad.numpy()))
                continue
            grad_check(k, p.grad.cpu().numpy(), params[k].grad.numpy())
            checked += 1
    for k, pairs in scalars.items():
        grad_check(k, np.concatenate([g.reshape(-1) for g, _ in pairs]), np.concatenate([w.reshape(-1) for _, w in pairs]))
        checked += 1
    assert checked >= 10
