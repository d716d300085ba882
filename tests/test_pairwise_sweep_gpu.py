"""The pairwise ranking losses under a distance against every node or a shared candidate set
(HyperGNN.pairwise_loss_by_distance, ghf_dist_pair_*, csrc/pairwise_sweep.hip) on the GPU, against the float64 restatement of
tests/_pairwise_sweep_ref.py.

Tolerances are the project's own and no new number is introduced: losses (and the logistic dsum) under
test_softmax_gpu.loss_check, gradients under test_softmax_gpu.grad_check, both at their defaults; counts are exact.  The
hinge's gradient and `active` jump at u = 0, so the parity problems carry the kink rule of tests/_pairwise_sweep_ref.py: a
query with a pair inside the near-tie band takes grad_loss = 0 in the call and in the reference and its `active` is held to
+- its in-band pairs; tests/test_pairwise_sweep_host.py checks, without a device, that at most B / 8 queries of any problem are
such and that fp32 on the CPU passes the same checks on these very problems.  The integer tests need no tolerance at all.

Shapes come from the kernels' geometry (test_distance_loss_host.SHAPES says which edge each one sits on)."""

import numpy as np
import pytest
import torch

import _distance_ref as R
import _pairwise_sweep_ref as S
from graph_hypernetwork_forge_amd import HyperGNN, ToyKnowledgeGraph, _native
from test_distance_gpu import rows_cpu, scale_for
from test_distance_loss_host import CASES, CASE_IDS, parity_problem
from test_softmax_gpu import csr, grad_check, loss_check

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
METRIC = _native.DIST_METRICS
KIND = _native.PAIR_KINDS
MARGIN = S.MARGIN


@pytest.fixture(scope="module")
def model():
    return HyperGNN(text_dim=32, node_feat_dim=16, hidden_dim=16).to(DEV)


def dev(x):
    return None if x is None else (tuple(dev(v) for v in x) if isinstance(x, tuple) else x.to(DEV))


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def raw_fwd(kind, M, q, c, t, scale, margin=MARGIN, normalize=True, **kw):
    return _native.score_dist_pair_sweep_fwd(M, KIND[kind], q, c, t, scale=scale, margin=margin, normalize=normalize, **kw)


def raw_all(kind, M, q, c, t, grad, scale, margin=MARGIN, normalize=True, **kw):
    """(loss, dsum, count, active, dq, dc)"""
    f = raw_fwd(kind, M, q, c, t, scale, margin, normalize, **kw)
    return f + _native.score_dist_pair_sweep_bwd(M, KIND[kind], q, c, t, f[1], f[2], grad, scale=scale, margin=margin,
                                                 normalize=normalize, **kw)


def integer_rows(N, d, seed):
    return torch.from_numpy(np.random.default_rng(seed).integers(-3, 4, (N, d)).astype(np.float32))


# ---- 1. parity -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric,shape", CASES, ids=CASE_IDS)
def test_losses_counts_and_gradients_match_float64(model, metric, shape):
    """Both kinds, normalize on and off, in two forms: all nodes with queries by id and known= pairs — equal bit for bit to the
    CSR lists — and a candidate subset (shuffled ids) with translated query_rows and CSR lists.  Loss, count, active, dsum,
    d embs, d query_rows."""
    d, C, B = shape
    scale, M = scale_for(metric, d), METRIC[metric]
    for subset, by_id in S.FORMS:
        i = S.problem(metric, shape, subset)
        embs, q, t, rows, known, cand = (dev(i[k]) for k in ("embs", "q", "t", "rows", "known", "cand"))
        ptr, idx = csr(i["lists"])
        P = S.candidate_set(embs.size(0), i["t"], i["cand"])
        ic = None if cand is None else torch.from_numpy(P).to(DEV)
        for kind in S.KINDS:
            for normalize in (True, False):
                kw = dict(loss=kind, margin=MARGIN, scale=scale, normalize=normalize, candidates=cand, return_active=True)
                what = f"{metric} {kind} {'subset' if subset else 'all'} normalize={normalize}"
                want, grad, nr, inb = S.reference(metric, shape, subset, kind, normalize, by_id)
                if by_id:               # the query's own row is a candidate at distance 0
                    e = embs.clone().requires_grad_()
                    loss, active = model.pairwise_loss_by_distance(e, q, t, metric, known=known, **kw)
                    (loss * dev(grad)).sum().backward()
                    grad_check(f"{what} by id: embs", e.grad.cpu().numpy(), S.embs_grad(want, i["q"]).numpy())
                    listed = model.pairwise_loss_by_distance(embs, q, t, metric, filt_ptr=ptr, filt_idx=idx, **kw)
                    assert same_bits(loss, listed[0]) and torch.equal(active, listed[1]), f"{what}: CSR lists equal to known= bit for bit"
                    raw = raw_fwd(kind, M, embs, embs, t, scale, normalize=normalize, iq=q, filt_ptr=ptr, filt_idx=idx, ic=ic)
                else:                   # translated rows
                    e, r = embs.clone().requires_grad_(), rows.clone().requires_grad_()
                    loss, active = model.pairwise_loss_by_distance(e, q, t, metric, filt_ptr=ptr, filt_idx=idx, query_rows=r, **kw)
                    (loss * dev(grad)).sum().backward()
                    grad_check(f"{what} rows: embs", e.grad.cpu().numpy(), want["dc"].numpy())
                    grad_check(f"{what} rows: query_rows", r.grad.cpu().numpy(), want["dq"].numpy())
                    raw = raw_fwd(kind, M, rows, embs, t, scale, normalize=normalize, filt_ptr=ptr, filt_idx=idx, ic=ic)
                loss_check(f"{what}: loss", loss, want["loss"])
                S.active_check(what, active, want, nr, inb)
                rl, dsum, count, ra = raw
                assert same_bits(rl, loss) and torch.equal(ra, active), f"{what}: the method is the C call"
                assert torch.equal(count.cpu().long(), want["count"]), f"{what}: count"
                if kind == "hinge":
                    assert torch.equal(dsum, active.float()), f"{what}: the hinge's dsum is float(active)"
                else:
                    loss_check(f"{what}: dsum", dsum, want["dsum"])
                if cand is not None:    # rows that are neither candidate, target nor query: exactly zero
                    outside = np.setdiff1d(np.arange(embs.size(0)), P)
                    assert not e.grad[torch.from_numpy(outside).to(DEV)].any()


@pytest.mark.parametrize("metric", R.METRICS)
def test_typed_known_with_query_rel(model, metric):
    d, N, B = 20, 300, 40
    rng = np.random.default_rng(17)
    embs = rows_cpu(N, d, 17)
    q, t, qrel = rng.integers(0, N, B), rng.integers(0, N, B), rng.integers(0, 3, B)
    src, dst, rel = np.repeat(q, 3), rng.integers(0, N, 3 * B), rng.integers(0, 3, 3 * B)
    lists = [np.unique(dst[(src == q[i]) & (rel == qrel[i])]) for i in range(B)]
    T = lambda a: torch.from_numpy(a.astype(np.int64))
    scale = scale_for(metric, d)
    for kind in S.KINDS:
        want = S.loss(kind, metric, embs[T(q)], embs, T(t), lists, None, scale=scale, margin=MARGIN)
        got, active = model.pairwise_loss_by_distance(dev(embs), dev(T(q)), dev(T(t)), metric, loss=kind, scale=scale, margin=MARGIN,
                                                      known=dev((T(src), T(dst), T(rel))), query_rel=dev(T(qrel)), return_active=True)
        loss_check(f"{metric} {kind} typed", got, want["loss"])
        nr, inb = S.near(want, MARGIN)
        S.active_check(f"{metric} {kind} typed", active, want, nr, inb)


# ---- 2. exact ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,C,B", [(4, 513, 5), (6, 70, 513), (20, 257, 129), (130, 1025, 64), (3, 2, 5), (256, 2600, 5)])
def test_exact_on_integer_rows_under_l1(d, C, B):
    """Entries in {-3..3} under L1, scale = 1, margin = k + 0.5 and integer grad_loss: every distance is an integer <= 6 d, every
    u a half-integer that is never 0, every sum below 2^24 — exact in fp32 whatever the order.  The unnormalised hinge loss,
    count, active, dq and dc equal float64 bit for bit: this pins G_it = -w active and the whole backward with no tolerance.  At
    the integer margin k some pairs sit at u == 0 exactly: no loss and no coefficient there, still bit for bit."""
    rng = np.random.default_rng(d + C + B)
    for subset in (False, True):
        N = C + 41 if subset else C
        embs = integer_rows(N, d, d + C)
        embs[N - N // 3:] = embs[:N // 3][:N - (N - N // 3)]                               # copies: distances tie and repeat
        P = np.sort(rng.permutation(N)[:C]).astype(np.int64) if subset else np.arange(N, dtype=np.int64)
        t = torch.from_numpy(P[rng.integers(0, C, B)])
        rows = integer_rows(B, d, B) + embs[torch.from_numpy(rng.integers(0, N, B))]
        lists = [np.unique(rng.integers(0, N, 4)) if i % 3 else np.zeros(0, dtype=np.int64) for i in range(B)]
        lists[0] = np.unique(np.append(lists[0], int(t[0])))                               # a listed target still receives G_it
        grad = torch.from_numpy(rng.integers(-3, 4, B).astype(np.float32))
        ptr, idx = csr(lists)
        ic = torch.from_numpy(P).to(DEV) if subset else None
        zeros = 0
        for margin in (2.5, 2.0, 0.5 - 2 * d):
            want = S.loss("hinge", "l1", rows, embs, t, lists, P if subset else None, scale=1.0, margin=margin, normalize=False,
                          grad=grad, add_targets=False)
            zeros += int(((want["u"] == 0) & want["live"]).sum())
            loss, dsum, count, active, dq, dc = raw_all("hinge", METRIC["l1"], dev(rows), dev(embs), dev(t), dev(grad), 1.0, margin, False,
                                                        filt_ptr=ptr, filt_idx=idx, ic=ic)
            what = (d, C, B, subset, margin)
            assert torch.equal(count.cpu().long(), want["count"]) and torch.equal(active.cpu().long(), want["active"]), what
            assert torch.equal(dsum.cpu().double(), want["active"].double()), what
            assert torch.equal(loss.cpu().double(), want["loss"]), what
            assert torch.equal(dq.cpu().double(), want["dq"]), what
            assert torch.equal(dc.cpu().double(), want["dc"][torch.from_numpy(P)]), what
            soft = raw_fwd("logistic", METRIC["l1"], dev(rows), dev(embs), dev(t), 1.0, margin, False, filt_ptr=ptr, filt_idx=idx, ic=ic)
            assert torch.equal(soft[2], count) and torch.equal(soft[3], active), "the counts do not depend on the kind"
        assert zeros > 0 or C < 3, "the integer margin puts pairs at u == 0"
        assert int(want["count"].sum()) > 0


@pytest.mark.parametrize("metric", R.METRICS)
def test_active_is_the_rank_sweeps_greater_at_margin_zero(model, metric):
    """margin = 0, scale = 1: u > 0 is z_ij > z_it by the very chain and J_i of rank_by_distance — exact under every metric."""
    for d, C, B in ((20, 1025, 70), (6, 257, 65), (130, 513, 9)):
        for subset in (False, True):
            i = parity_problem(d, C, B, subset)
            embs, q, t, rows, known, cand = (dev(i[k]) for k in ("embs", "q", "t", "rows", "known", "cand"))
            kw = dict(known=known, candidates=cand, query_rows=rows)
            greater, _ = model.rank_by_distance(embs, q, t, metric, **kw)
            want = S.loss("hinge", metric, i["rows"], i["embs"], i["t"], i["lists"], i["cand"], scale=1.0, margin=0.0)
            for kind in S.KINDS:
                _, active = model.pairwise_loss_by_distance(embs, q, t, metric, loss=kind, margin=0.0, return_active=True, **kw)
                assert torch.equal(active.long(), greater), (metric, kind, d, C, B, subset)
            ptr, idx = csr(i["lists"])
            P = S.candidate_set(embs.size(0), i["t"], i["cand"])
            ic = None if cand is None else torch.from_numpy(P).to(DEV)
            _, dsum, count, active = raw_fwd("hinge", METRIC[metric], rows, embs, t, 1.0, 0.0, filt_ptr=ptr, filt_idx=idx, ic=ic)
            assert torch.equal(count.cpu().long(), want["count"]) and torch.equal(dsum, active.float())


# ---- 3. against the per-query kernel -------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", R.METRICS)
def test_shared_set_agrees_with_per_query_negatives(model, metric):
    """candidates=P against pairwise_loss(negatives=P per row, distance=): to rounding, not in bits — the per-query kernel sums
    across a lane group."""
    d, C, B = 64, 700, 33
    i = parity_problem(d, C, B, True)
    embs, q, t, known, cand = (dev(i[k]) for k in ("embs", "q", "t", "known", "cand"))
    P = torch.from_numpy(S.candidate_set(embs.size(0), i["t"], i["cand"])).to(DEV)
    neg = P.unsqueeze(0).expand(B, -1).contiguous()
    scale = scale_for(metric, d)
    for kind in S.KINDS:
        for normalize in (True, False):
            a = model.pairwise_loss_by_distance(embs, q, t, metric, loss=kind, scale=scale, margin=MARGIN, normalize=normalize, known=known,
                                                candidates=cand)
            b = model.pairwise_loss(embs, q, t, negatives=neg, loss=kind, scale=scale, margin=MARGIN, normalize=normalize, known=known,
                                    distance=metric)
            loss_check(f"{metric} {kind} vs per-query", a, b.double().cpu())


# ---- 4. bits -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric,d", [("l1", 20), ("l2", 130), ("complex", 64), ("l1", 6)])
def test_bits(model, metric, d):
    C, B = 1025, 70
    M, scale = METRIC[metric], scale_for(metric, d)
    i = parity_problem(d, C, B, True)
    embs, q, t, rows, grad, cand = (dev(i[k]) for k in ("embs", "q", "t", "rows", "grad", "cand"))
    lists = i["lists"]
    ptr, idx = csr(lists)
    P = torch.from_numpy(S.candidate_set(embs.size(0), i["t"], i["cand"])).to(DEV)
    kw = dict(filt_ptr=ptr, filt_idx=idx)
    for kind in S.KINDS:
        one = raw_all(kind, M, rows, embs, t, grad, scale, ic=P, **kw)
        two = raw_all(kind, M, rows, embs, t, grad, scale, ic=P, **kw)
        assert all(same_bits(a, b) for a, b in zip(one, two)), "the same call twice"
        grads = []
        for _ in range(2):
            e = embs.clone().requires_grad_()
            (model.pairwise_loss_by_distance(e, q, t, metric, loss=kind, scale=scale, candidates=cand, **kw) * grad).sum().backward()
            grads.append(e.grad)
        assert same_bits(*grads), "the final gradients twice"
        # the two halves of a batch
        h = B // 2
        lo = raw_fwd(kind, M, rows[:h].contiguous(), embs, t[:h].contiguous(), scale, ic=P, **dict(zip(("filt_ptr", "filt_idx"), csr(lists[:h]))))
        hi = raw_fwd(kind, M, rows[h:].contiguous(), embs, t[h:].contiguous(), scale, ic=P, **dict(zip(("filt_ptr", "filt_idx"), csr(lists[h:]))))
        assert all(same_bits(torch.cat([lo[k], hi[k]]), one[k]) for k in range(4)), "halves of a batch"
        # the subset against the all-node call on the contiguous copy embs[P]: positions instead of ids
        pos = {int(v): j for j, v in enumerate(P.tolist())}
        lists_p = [np.array(sorted(pos[v] for v in l.tolist() if v in pos), dtype=np.int64) for l in lists]
        tp = torch.tensor([pos[int(v)] for v in i["t"]], device=DEV)
        copy = raw_all(kind, M, rows, embs[P].contiguous(), tp, grad, scale, **dict(zip(("filt_ptr", "filt_idx"), csr(lists_p))))
        assert all(same_bits(a, b) for a, b in zip(one, copy)), "candidates=P equals the call on embs[P]"
        # shuffled against sorted candidates
        a = model.pairwise_loss_by_distance(embs, q, t, metric, loss=kind, scale=scale, candidates=cand, **kw)
        b = model.pairwise_loss_by_distance(embs, q, t, metric, loss=kind, scale=scale, candidates=torch.sort(cand).values, **kw)
        assert same_bits(a, b), "candidates in any order"
        # an unaligned base: the scalar path gives the aligned call's forward bits
        if d % 4 == 0:
            buf = torch.empty(embs.numel() + 1, device=DEV)
            off = buf[1:].view_as(embs).copy_(embs)
            rbuf = torch.empty(rows.numel() + 1, device=DEV)
            roff = rbuf[1:].view_as(rows).copy_(rows)
            assert off.data_ptr() % 16 and roff.data_ptr() % 16
            un = raw_fwd(kind, M, roff, off, t, scale, ic=P, **kw)
            assert all(same_bits(un[k], one[k]) for k in range(4)), "the load path does not change the forward's bits"
            dq, dc = _native.score_dist_pair_sweep_bwd(M, KIND[kind], roff, off, t, un[1], un[2], grad, scale=scale, margin=MARGIN, ic=P, **kw)
            grad_check("unaligned dq", dq.cpu().numpy(), one[4].cpu().numpy())
            grad_check("unaligned dc", dc.cpu().numpy(), one[5].cpu().numpy())


# ---- 5. edge semantics ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", R.METRICS)
def test_the_target_alone(model, metric):
    """C = 1: J_i is empty — loss exactly 0, count 0, active 0, and not one gradient."""
    d, N, B = 6, 40, 5
    embs = rows_cpu(N, d, 3).to(DEV)
    rows = rows_cpu(B, d, 4).to(DEV)
    t = torch.full((B,), 7, device=DEV)
    ic = torch.tensor([7], device=DEV)
    grad = torch.ones(B, device=DEV)
    for kind in S.KINDS:
        for normalize in (True, False):
            loss, dsum, count, active, dq, dc = raw_all(kind, METRIC[metric], rows, embs, t, grad, 0.7, normalize=normalize, ic=ic)
            assert not loss.any() and not dsum.any() and not count.any() and not active.any() and same_bits(loss, torch.zeros_like(loss))
            assert not dq.any() and not dc.any() and tuple(dc.shape) == (1, d)
        e = embs.clone().requires_grad_()
        out = model.pairwise_loss_by_distance(e, t[:1], t[:1], metric, loss=kind, candidates=ic)
        out.sum().backward()
        assert float(out.detach().abs().max()) == 0.0 and not e.grad.any()


@pytest.mark.parametrize("metric", R.METRICS)
def test_distance_zero_contributes_exactly_nothing(model, metric):
    d, N = 8, 90
    embs = rows_cpu(N, d, 5).to(DEV)
    rows = embs[11:12].clone()                                                             # bit-identical to candidate 11
    t = torch.tensor([40], device=DEV)
    for kind in S.KINDS:
        out = raw_all(kind, METRIC[metric], rows, embs, t, torch.ones(1, device=DEV), 0.5)
        assert int(out[3]) > 0 and not out[5][11].any(), "the pair at distance 0 is violated and adds exactly 0 to dc"
        e, r = embs.clone().requires_grad_(), rows.clone().requires_grad_()
        model.pairwise_loss_by_distance(e, torch.tensor([11], device=DEV), t, metric, loss=kind, scale=0.5, query_rows=r).sum().backward()
        assert not e.grad[11].any(), "with B = 1 and query_rows, the twin's row of d embs is exactly zero"
        want = S.loss(kind, metric, rows.cpu(), embs.cpu(), t.cpu(), None, None, scale=0.5, margin=MARGIN, grad=torch.ones(1))
        grad_check("dq", out[4].cpu().numpy(), want["dq"].numpy())


@pytest.mark.parametrize("metric", R.METRICS)
def test_listed_target_and_listed_ids_outside_the_subset(model, metric):
    d, N, B = 12, 400, 6
    embs = rows_cpu(N, d, 21)
    rng = np.random.default_rng(21)
    cand = np.arange(0, N, 3)
    t = cand[rng.integers(0, len(cand), B)]
    q = rng.integers(0, N, B)
    lists = [np.unique(np.concatenate([[t[i]], [1, 2, 4, 5], cand[rng.integers(0, len(cand), 3)]])) for i in range(B)]
    ptr, idx = csr(lists)
    T = torch.from_numpy
    grad = torch.ones(B)
    for kind in S.KINDS:
        want = S.loss(kind, metric, embs[T(q)], embs, T(t), lists, cand, scale=0.3, margin=MARGIN, grad=grad)
        e = dev(embs).requires_grad_()
        got = model.pairwise_loss_by_distance(e, dev(T(q)), dev(T(t)), metric, loss=kind, scale=0.3, filt_ptr=ptr, filt_idx=idx,
                                              candidates=dev(T(cand)))
        loss_check(f"{metric} {kind}", got, want["loss"])
        if kind == "logistic":                                                             # the listed target's pair carries G_it
            got.sum().backward()
            grad_check(f"{metric} {kind} embs", e.grad.cpu().numpy(), S.embs_grad(want, T(q)).numpy())
            assert bool(want["coef"][:, -1].abs().min() > 0)
        inside = [np.intersect1d(l, cand) for l in lists]                                  # the ids outside the set take no part
        same = model.pairwise_loss_by_distance(dev(embs), dev(T(q)), dev(T(t)), metric, loss=kind, scale=0.3, candidates=dev(T(cand)),
                                               **dict(zip(("filt_ptr", "filt_idx"), csr(inside))))
        assert same_bits(got, same)


# ---- 6. invalid ids: ordinary calls whose contract is "no fault" ----------------------------------------------------------
@pytest.mark.parametrize("metric", R.METRICS)
def test_an_invalid_id_makes_its_query_alone_nan(metric):
    d, N, B = 20, 700, 70
    M, big = METRIC[metric], 1 << 40
    i = parity_problem(d, N, B, False)
    embs, q, t, grad = (dev(i[k]) for k in ("embs", "q", "t", "grad"))
    lists = i["lists"]
    ic_np = np.unique(np.concatenate([np.arange(0, N, 2), i["t"].numpy()]))
    outside = next(v for v in range(1, N, 2) if v not in ic_np)                           # a node that is no candidate
    for kind in S.KINDS:
        for ic in (None, torch.from_numpy(ic_np).to(DEV)):
            ptr, idx = csr(lists)
            good = raw_all(kind, M, embs, embs, t, grad, 0.2, iq=q, filt_ptr=ptr, filt_idx=idx, ic=ic)
            assert all(bool(torch.isfinite(x).all()) for x in (good[0], good[1], good[4], good[5])) and bool((good[2] >= 0).all())
            kinds = [("iq", 3, N + 5), ("iq", 64, -2), ("iq", 5, big), ("target", 9, N), ("target", 65, -1), ("target", 2, big),
                     ("list", 4, N + 1), ("list", 66, -7), ("list", 7, big)]
            if ic is not None:
                kinds.append(("target", 11, outside))                                      # a node, but no candidate
            for what_bad, b, value in kinds:
                q2, t2, l2 = q.clone(), t.clone(), [l.copy() for l in lists]
                if what_bad == "iq":
                    q2[b] = value
                elif what_bad == "target":
                    t2[b] = value
                else:
                    l2[b] = np.sort(np.append(l2[b], value))
                ptr2, idx2 = csr(l2)
                bad = raw_all(kind, M, embs, embs, t2, grad, 0.2, iq=q2, filt_ptr=ptr2, filt_idx=idx2, ic=ic)
                what = f"{metric} {kind} {what_bad} {value} {'sub' if ic is not None else 'all'}"
                assert bool(torch.isnan(bad[0][b])) and bool(torch.isnan(bad[1][b])) and int(bad[2][b]) == -1 and int(bad[3][b]) == -1, what
                assert not bad[4][b].any(), what
                keep = torch.arange(B, device=DEV) != b
                for k in range(5):
                    assert same_bits(bad[k][keep], good[k][keep]), (what, k)
                # the same call without the bad query
                qk, tk = q[keep].contiguous(), t[keep].contiguous()
                ptrk, idxk = csr([l for j, l in enumerate(lists) if j != b])
                rest = raw_all(kind, M, embs, embs, tk, grad[keep].contiguous(), 0.2, iq=qk, filt_ptr=ptrk, filt_idx=idxk, ic=ic)
                assert same_bits(bad[5], rest[5]), f"{what}: the bad query adds nothing to dc"
    torch.cuda.synchronize()


@pytest.mark.parametrize("metric", R.METRICS)
def test_a_bad_ic_makes_every_query_invalid(metric):
    d, N, B = 8, 300, 5
    M, big = METRIC[metric], 1 << 40
    i = parity_problem(d, N, B, False)
    embs, q, grad = dev(i["embs"]), dev(i["q"]), dev(i["grad"])
    t = torch.full((B,), 2, device=DEV)
    for kind in S.KINDS:
        for what, ic in (("not ascending", np.array([3, 2, 9])), ("repeated", np.array([2, 2, 9])), ("out of range", np.array([2, 9, N])),
                         ("negative", np.array([-1, 2, 9])), ("far out of range", np.array([2, 9, big]))):
            loss, dsum, count, active, dq, dc = raw_all(kind, M, embs, embs, t, grad, 0.3, iq=q, ic=torch.from_numpy(ic).to(DEV))
            assert bool(torch.isnan(loss).all()) and bool(torch.isnan(dsum).all()), f"a bad ic ({what}) makes every query invalid"
            assert bool((count == -1).all()) and bool((active == -1).all()), what
            assert not dq.any() and not dc.any(), what
    torch.cuda.synchronize()


# ---- 7. through the model ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", S.KINDS)
def test_transe_through_the_model_matches_float64_autograd(kind):
    """The published TransE objective with ONE negative set shared by the batch, on a 2-layer HyperGNN over the toy graph: rows =
    embs[head] + rel_vec[rel], L1 distance, the pairwise loss against candidates=; the gradients of every parameter and of
    rel_vec against float64 autograd through the oracle's forward and a dense formulation of the loss."""
    from oracle import hypergnn_oracle as O
    torch.manual_seed(0)
    kg = ToyKnowledgeGraph(feat_dim=16)
    model = HyperGNN(text_dim=32, node_feat_dim=16, hidden_dim=16).to(DEV).train()
    x, ei, texts = kg.node_features.to(DEV), kg.edge_index.to(DEV), kg.edge_texts
    N = x.size(0)
    rng = np.random.default_rng(4)
    B, nrel = 7, 3
    head = torch.from_numpy(rng.integers(0, N, B)).to(DEV)
    tail = torch.from_numpy(rng.integers(0, N, B)).to(DEV)
    rel = torch.from_numpy(rng.integers(0, nrel, B)).to(DEV)
    cand = torch.from_numpy(rng.permutation(N)[:max(2, N // 2)]).to(DEV)
    rel_vec = torch.from_numpy(rng.standard_normal((nrel, 16)).astype(np.float32)).to(DEV).requires_grad_()
    embs = model(x, ei, texts)
    rows = embs[head] + rel_vec[rel]
    loss = model.pairwise_loss_by_distance(embs, head, tail, "l1", loss=kind, margin=2.0, query_rows=rows, candidates=cand).sum()
    loss.backward()

    params = {k: v.detach().cpu().double().requires_grad_(True) for k, v in model.state_dict().items()}
    r64 = rel_vec.detach().cpu().double().requires_grad_()
    e64 = O.forward(params, kg.node_features.double(), kg.edge_index.numpy(), texts, variant="factorised", dtype=torch.float64)
    hc, tc, rc = head.cpu(), tail.cpu(), rel.cpu()
    P = torch.from_numpy(S.candidate_set(N, tc, cand.cpu()))
    q64 = e64[hc] + r64[rc]
    z = -(q64.unsqueeze(1) - e64[P].unsqueeze(0)).abs().sum(-1)
    zt = -(q64 - e64[tc]).abs().sum(-1)
    live = P.unsqueeze(0) != tc.unsqueeze(1)
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
            # last LayerNorm's bias has gradient exactly 0 in exact arithmetic, which taken alone leaves grad_check no scale.
            # A LayerNorm's weight and bias are compared as the one vector they form.
            if p.numel() == 1 or k.startswith("layer_norms."):
                scalars.setdefault(k.rsplit(".", 1)[0], []).append((p.grad.cpu().numpy(), params[k].grad.numpy()))
                continue
            grad_check(k, p.grad.cpu().numpy(), params[k].grad.numpy())
            checked += 1
    for k, pairs in scalars.items():
        grad_check(k, np.concatenate([g.reshape(-1) for g, _ in pairs]), np.concatenate([w.reshape(-1) for _, w in pairs]))
        checked += 1
    assert checked >= 10
