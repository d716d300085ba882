"""The softmax and the negative-sampling loss under a distance against every node or a shared candidate set
(HyperGNN.softmax_loss_by_distance / negative_sampling_loss_by_distance, ghf_dist_loss_*, csrc/distance_loss.hip) on the GPU,
against the float64 restatement of tests/_distance_loss_ref.py.

Tolerances are the project's own and no new number is introduced: losses and lse / lw under test_softmax_gpu.loss_check,
gradients under test_softmax_gpu.grad_check, both at their defaults (DESIGN.md §22 uses them for the same formulas).
tests/test_distance_loss_host.py checks, without a device, that fp32 on the CPU passes them on these very problems.

Shapes come from the kernels' geometry (test_distance_loss_host.SHAPES says which edge each one sits on)."""

import numpy as np
import pytest
import torch

import _distance_loss_ref as L
import _distance_ref as R
from graph_hypernetwork_forge_amd import HyperGNN, ToyKnowledgeGraph, _native
from test_distance_gpu import rows_cpu, scale_for
from test_distance_loss_host import ALPHA, CASES, CASE_IDS, MARGIN, MODES, aux_check, parity_problem
from test_softmax_gpu import csr, grad_check, loss_check

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
METRIC = _native.DIST_METRICS
NAN = float("nan")


@pytest.fixture(scope="module")
def model():
    return HyperGNN(text_dim=32, node_feat_dim=16, hidden_dim=16).to(DEV)


def dev(x):
    return None if x is None else (tuple(dev(v) for v in x) if isinstance(x, tuple) else x.to(DEV))


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def method(model, mode):
    if mode == "softmax":
        return lambda *a, **kw: model.softmax_loss_by_distance(*a, **kw)
    return lambda *a, **kw: model.negative_sampling_loss_by_distance(*a, margin=MARGIN, adversarial_temperature=ALPHA, **kw)


def raw_fwd(mode, M, q, c, t, scale, **kw):
    if mode == "softmax":
        return _native.score_dist_loss_softmax_fwd(M, q, c, t, scale=scale, **kw)
    return _native.score_dist_loss_negsamp_fwd(M, q, c, t, scale=scale, margin=MARGIN, adversarial_temperature=ALPHA, **kw)


def raw_bwd(mode, M, q, c, t, saved, grad, scale, **kw):
    code = _native.NEG_SOFTMAX if mode == "softmax" else _native.NEG_NEGSAMP
    return _native.score_dist_loss_bwd(M, code, q, c, t, saved, grad, scale=scale, margin=MARGIN, adversarial_temperature=ALPHA, **kw)


def raw_all(mode, M, q, c, t, grad, scale, **kw):
    loss, aux = raw_fwd(mode, M, q, c, t, scale, **kw)
    dq, dc = raw_bwd(mode, M, q, c, t, aux, grad, scale, **kw)
    return loss, aux, dq, dc


# ---- 1. parity -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric,shape", CASES, ids=CASE_IDS)
def test_losses_and_gradients_match_float64(model, metric, shape):
    """All nodes with queries by id and known= pairs; a candidate subset (shuffled ids) with query_rows and CSR lists.  Loss,
    lse / lw, d embs and d query_rows.  Slabs, from the routines: C = 513 is the smallest C that dloss_geom (forward) and
    dloss_bwd_geom (dq pass) split into 3 slabs with a ragged last one — 3 tiles of 256, the last holding 1 candidate —; the dc
    pass streams the queries, and B = 513 is the smallest B it splits into 3 slabs (256, 256, 1); C = 2600 is 11 forward slabs."""
    d, C, B = shape
    scale, M = scale_for(metric, d), METRIC[metric]
    for subset in (False, True):
        i = parity_problem(d, C, B, subset)
        embs, q, t, rows, grad, known, cand = (dev(i[k]) for k in ("embs", "q", "t", "rows", "grad", "known", "cand"))
        ptr, idx = csr(i["lists"])
        P = L.candidate_set(embs.size(0), i["t"], i["cand"])
        ic = None if cand is None else torch.from_numpy(P).to(DEV)
        for mode, _ in MODES:
            fn, what = method(model, mode), f"{metric} {mode} {'subset' if subset else 'all'}"
            # queries by id: the query's own row is a candidate at distance 0 unless the subset leaves it out
            want = L.loss(mode, metric, i["embs"][i["q"]], i["embs"], i["t"], i["lists"], i["cand"], scale=scale, margin=MARGIN,
                          alpha=ALPHA, grad=i["grad"])
            e = embs.clone().requires_grad_()
            loss = fn(e, q, t, metric, scale=scale, known=known, candidates=cand)
            loss_check(f"{what} by id: loss", loss, want["loss"])
            (loss * grad).sum().backward()
            grad_check(f"{what} by id: embs", e.grad.cpu().numpy(), L.embs_grad(want, i["q"]).numpy())
            listed = fn(embs, q, t, metric, scale=scale, filt_ptr=ptr, filt_idx=idx, candidates=cand)
            assert same_bits(loss, listed), f"{what}: CSR lists equal to known= bit for bit"
            _, aux = raw_fwd(mode, M, embs, embs, t, scale, iq=q, filt_ptr=ptr, filt_idx=idx, ic=ic)
            aux_check(f"{what} by id: aux", aux, want["aux"])
            # translated rows
            want = L.loss(mode, metric, i["rows"], i["embs"], i["t"], i["lists"], i["cand"], scale=scale, margin=MARGIN, alpha=ALPHA,
                          grad=i["grad"])
            e, r = embs.clone().requires_grad_(), rows.clone().requires_grad_()
            loss = fn(e, q, t, metric, scale=scale, filt_ptr=ptr, filt_idx=idx, query_rows=r, candidates=cand)
            loss_check(f"{what} rows: loss", loss, want["loss"])
            (loss * grad).sum().backward()
            grad_check(f"{what} rows: embs", e.grad.cpu().numpy(), want["dc"].numpy())
            grad_check(f"{what} rows: query_rows", r.grad.cpu().numpy(), want["dq"].numpy())
            _, aux = raw_fwd(mode, M, rows, embs, t, scale, filt_ptr=ptr, filt_idx=idx, ic=ic)
            aux_check(f"{what} rows: aux", aux, want["aux"])
            if cand is not None:                        # rows that are neither candidate, target nor query: exactly zero
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
    for mode, _ in MODES:
        want = L.loss(mode, metric, embs[T(q)], embs, T(t), lists, None, scale=scale, margin=MARGIN, alpha=ALPHA)
        got = method(model, mode)(dev(embs), dev(T(q)), dev(T(t)), metric, scale=scale, known=dev((T(src), T(dst), T(rel))),
                                  query_rel=dev(T(qrel)))
        loss_check(f"{metric} {mode} typed", got, want["loss"])


# ---- 2. against the per-query kernels --------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", R.METRICS)
def test_shared_set_agrees_with_per_query_negatives(model, metric):
    """candidates=P against softmax_loss / negative_sampling_loss(negatives=P per row, distance=): to rounding, not in bits —
    the per-query kernel sums across a lane group."""
    d, C, B = 64, 700, 33
    i = parity_problem(d, C, B, True)
    embs, q, t, known, cand = (dev(i[k]) for k in ("embs", "q", "t", "known", "cand"))
    P = torch.from_numpy(L.candidate_set(embs.size(0), i["t"], i["cand"])).to(DEV)
    neg = P.unsqueeze(0).expand(B, -1).contiguous()
    scale = scale_for(metric, d)
    a = model.softmax_loss_by_distance(embs, q, t, metric, scale=scale, known=known, candidates=cand)
    b = model.softmax_loss(embs, q, t, scale=scale, known=known, negatives=neg, distance=metric)
    loss_check(f"{metric} softmax vs per-query", a, b.double().cpu())
    a = model.negative_sampling_loss_by_distance(embs, q, t, metric, scale=scale, margin=MARGIN, adversarial_temperature=ALPHA,
                                                 known=known, candidates=cand)
    b = model.negative_sampling_loss(embs, q, t, scale=scale, margin=MARGIN, adversarial_temperature=ALPHA, known=known,
                                     negatives=neg, distance=metric)
    loss_check(f"{metric} negsamp vs per-query", a, b.double().cpu())


# ---- 3. bits ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric,d", [("l1", 20), ("l2", 130), ("complex", 64), ("l1", 6)])
def test_bits(model, metric, d):
    C, B = 1025, 70
    M, scale = METRIC[metric], scale_for(metric, d)
    i = parity_problem(d, C, B, True)
    embs, q, t, rows, grad, cand = (dev(i[k]) for k in ("embs", "q", "t", "rows", "grad", "cand"))
    ptr, idx = csr(i["lists"])
    P = torch.from_numpy(L.candidate_set(embs.size(0), i["t"], i["cand"])).to(DEV)
    kw = dict(filt_ptr=ptr, filt_idx=idx)
    for mode, _ in MODES:
        fn = method(model, mode)
        one = raw_all(mode, M, rows, embs, t, grad, scale, ic=P, **kw)
        two = raw_all(mode, M, rows, embs, t, grad, scale, ic=P, **kw)
        assert all(same_bits(a, b) for a, b in zip(one, two)), "the same call twice"
        grads = []
        for _ in range(2):
            e = embs.clone().requires_grad_()
            (fn(e, q, t, metric, scale=scale, candidates=cand, **kw) * grad).sum().backward()
            grads.append(e.grad)
        assert same_bits(*grads), "the final gradients twice"
        # the two halves of a batch
        h = B // 2
        lists = i["lists"]
        lo = raw_fwd(mode, M, rows[:h].contiguous(), embs, t[:h].contiguous(), scale, ic=P, **dict(zip(("filt_ptr", "filt_idx"), csr(lists[:h]))))
        hi = raw_fwd(mode, M, rows[h:].contiguous(), embs, t[h:].contiguous(), scale, ic=P, **dict(zip(("filt_ptr", "filt_idx"), csr(lists[h:]))))
        assert same_bits(torch.cat([lo[0], hi[0]]), one[0]) and same_bits(torch.cat([lo[1], hi[1]]), one[1]), "halves of a batch"
        # the subset against the all-node call on the contiguous copy embs[P]: positions instead of ids
        pos = {int(v): j for j, v in enumerate(P.tolist())}
        lists_p = [np.array(sorted(pos[v] for v in l.tolist() if v in pos), dtype=np.int64) for l in lists]
        tp = torch.tensor([pos[int(v)] for v in i["t"]], device=DEV)
        copy = raw_all(mode, M, rows, embs[P].contiguous(), tp, grad, scale, **dict(zip(("filt_ptr", "filt_idx"), csr(lists_p))))
        assert all(same_bits(a, b) for a, b in zip(one, copy)), "candidates=P equals the call on embs[P]"
        # shuffled against sorted candidates
        a = fn(embs, q, t, metric, scale=scale, candidates=cand, **kw)
        b = fn(embs, q, t, metric, scale=scale, candidates=torch.sort(cand).values, **kw)
        assert same_bits(a, b), "candidates in any order"
        # an unaligned base: the scalar path gives the aligned call's loss bits
        if d % 4 == 0:
            buf = torch.empty(embs.numel() + 1, device=DEV)
            off = buf[1:].view_as(embs).copy_(embs)
            rbuf = torch.empty(rows.numel() + 1, device=DEV)
            roff = rbuf[1:].view_as(rows).copy_(rows)
            assert off.data_ptr() % 16 and roff.data_ptr() % 16
            un = raw_fwd(mode, M, roff, off, t, scale, ic=P, **kw)
            assert same_bits(un[0], one[0]) and same_bits(un[1], one[1]), "the load path does not change the forward's bits"
            dq, dc = raw_bwd(mode, M, roff, off, t, un[1], grad, scale, ic=P, **kw)
            grad_check("unaligned dq", dq.cpu().numpy(), one[2].cpu().numpy())
            grad_check("unaligned dc", dc.cpu().numpy(), one[3].cpu().numpy())


# ---- 4. edge semantics -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", R.METRICS)
def test_the_target_alone(model, metric):
    """C = 1: softmax loss exactly 0; negsamp lw = -inf and the positive term alone; the backward touches the target pair."""
    d, N, B = 6, 40, 5
    embs = rows_cpu(N, d, 3).to(DEV)
    rows = rows_cpu(B, d, 4).to(DEV)
    t = torch.full((B,), 7, device=DEV)
    ic = torch.tensor([7], device=DEV)
    grad = torch.ones(B, device=DEV)
    M = METRIC[metric]
    loss, lse, dq, dc = raw_all("softmax", M, rows, embs, t, grad, 0.7, ic=ic)
    assert not loss.any() and not dq.any() and not dc.any() and tuple(dc.shape) == (1, d)
    loss, lw, dq, dc = raw_all("negsamp", M, rows, embs, t, grad, 0.7, ic=ic)
    assert bool(torch.isneginf(lw).all())
    D, g = R.dist(metric, rows.cpu(), embs.cpu()[7].unsqueeze(0))
    z = -0.7 * D
    loss_check("positive term", loss, torch.nn.functional.softplus(-(z + MARGIN)))
    Gt = -0.7 * torch.sigmoid(-(z + MARGIN))
    grad_check("dq", dq.cpu().numpy(), (-Gt.unsqueeze(1) * g).numpy())
    grad_check("dc", dc.cpu().numpy(), (Gt.unsqueeze(1) * g).sum(0, keepdim=True).numpy())
    assert float(model.softmax_loss_by_distance(embs, t[:1], t[:1], metric, candidates=ic).abs().max()) == 0.0


@pytest.mark.parametrize("metric", R.METRICS)
def test_distance_zero_contributes_exactly_nothing(model, metric):
    d, N = 8, 90
    embs = rows_cpu(N, d, 5).to(DEV)
    M = METRIC[metric]
    # one query whose row is bit-identical to candidate 11; the target is another node
    rows = embs[11:12].clone()
    t = torch.tensor([40], device=DEV)
    for mode, _ in MODES:
        fn = method(model, mode)
        loss, aux, dq, dc = raw_all(mode, M, rows, embs, t, torch.ones(1, device=DEV), 0.5)
        assert not dc[11].any(), "the pair at distance 0 adds exactly 0 to dc"
        e, r = embs.clone().requires_grad_(), rows.clone().requires_grad_()
        fn(e, torch.tensor([11], device=DEV), t, metric, scale=0.5, query_rows=r).sum().backward()
        assert not e.grad[11].any(), "with B = 1 and query_rows, the twin's row of d embs is exactly zero"
        want = L.loss(mode, metric, rows.cpu(), embs.cpu(), t.cpu(), None, None, scale=0.5, margin=MARGIN, alpha=ALPHA,
                      grad=torch.ones(1))
        grad_check("dq", dq.cpu().numpy(), want["dq"].numpy())


@pytest.mark.parametrize("metric", R.METRICS)
def test_listed_candidates_dominate(model, metric):
    """Copies of the query row are listed, at a scale at which exp(z) of every other candidate underflows against them: a loss
    that subtracted listed terms afterwards would be inf - inf or log 0.  Masked before the sum, it is finite and the
    restatement's."""
    d, N, B = 16, 600, 9
    embs = rows_cpu(N, d, 9)
    rng = np.random.default_rng(9)
    q = rng.integers(300, N, B)
    copies = np.array([3, 255, 256, 299])
    embs[copies] = embs[3].clone()                                                         # four rows the queries sit on exactly
    rows = embs[3].unsqueeze(0).repeat(B, 1)
    lists = [copies.copy() for _ in range(B)]
    t = torch.from_numpy(rng.integers(300, N, B))
    # z = 0 for the listed copies and about -35 for every other node: exp(z) of the others is below 2^-24 of the copies' sum
    scale = {"l1": 2.0, "l2": 7.0, "complex": 2.5}[metric]
    ptr, idx = csr(lists)
    for mode, _ in MODES:
        want = L.loss(mode, metric, rows, embs, t, lists, None, scale=scale, margin=MARGIN, alpha=ALPHA)
        got = method(model, mode)(dev(embs), dev(torch.from_numpy(q)), dev(t), metric, scale=scale, query_rows=dev(rows), filt_ptr=ptr,
                                  filt_idx=idx)
        assert bool(torch.isfinite(got).all())
        loss_check(f"{metric} {mode} listed copies", got, want["loss"])


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
    for mode, _ in MODES:
        fn = method(model, mode)
        want = L.loss(mode, metric, embs[T(q)], embs, T(t), lists, cand, scale=0.3, margin=MARGIN, alpha=ALPHA)
        got = fn(dev(embs), dev(T(q)), dev(T(t)), metric, scale=0.3, filt_ptr=ptr, filt_idx=idx, candidates=dev(T(cand)))
        loss_check(f"{metric} {mode}", got, want["loss"])
        inside = [np.intersect1d(l, cand) for l in lists]                                  # the ids outside the set take no part
        same = fn(dev(embs), dev(T(q)), dev(T(t)), metric, scale=0.3, candidates=dev(T(cand)), **dict(zip(("filt_ptr", "filt_idx"), csr(inside))))
        assert same_bits(got, same)


@pytest.mark.parametrize("metric", R.METRICS)
def test_alpha_zero_is_the_uniform_mean(model, metric):
    d, C, B = 20, 513, 9
    i = parity_problem(d, C, B, False)
    scale = scale_for(metric, d)
    want = L.loss("negsamp", metric, i["rows"], i["embs"], i["t"], i["lists"], None, scale=scale, margin=MARGIN, alpha=0.0, grad=i["grad"])
    ptr, idx = csr(i["lists"])
    e, r = dev(i["embs"]).requires_grad_(), dev(i["rows"]).requires_grad_()
    got = model.negative_sampling_loss_by_distance(e, dev(i["q"]), dev(i["t"]), metric, scale=scale, margin=MARGIN, query_rows=r,
                                                   filt_ptr=ptr, filt_idx=idx)
    loss_check(f"{metric} alpha = 0", got, want["loss"])
    (got * dev(i["grad"])).sum().backward()
    grad_check("embs", e.grad.cpu().numpy(), want["dc"].numpy())
    grad_check("query_rows", r.grad.cpu().numpy(), want["dq"].numpy())
    z = -scale * R.distances(metric, i["rows"], i["embs"], i["t"], torch.arange(C).unsqueeze(0).expand(B, C))[0]
    live = R.live_positions(torch.arange(C).unsqueeze(0).expand(B, C), i["t"], i["lists"])
    mean = torch.stack([torch.nn.functional.softplus(z[b][live[b]] + MARGIN).mean() for b in range(B)])
    zt = -scale * R.dist(metric, i["rows"], i["embs"][i["t"]])[0]
    loss_check("the mean, written out", got, torch.nn.functional.softplus(-(zt + MARGIN)) + mean)


# ---- 5. invalid ids: ordinary calls whose contract is "no fault" ------------------------------------------------------------
@pytest.mark.parametrize("metric", R.METRICS)
def test_an_invalid_id_makes_its_query_alone_nan(metric):
    d, N, B = 20, 700, 70
    M, big = METRIC[metric], 1 << 40
    i = parity_problem(d, N, B, False)
    embs, q, t, grad = (dev(i[k]) for k in ("embs", "q", "t", "grad"))
    lists = i["lists"]
    ic_np = np.unique(np.concatenate([np.arange(0, N, 2), i["t"].numpy()]))
    outside = next(v for v in range(1, N, 2) if v not in ic_np)                           # a node that is no candidate
    for mode, _ in MODES:
        for ic in (None, torch.from_numpy(ic_np).to(DEV)):
            ptr, idx = csr(lists)
            good = raw_all(mode, M, embs, embs, t, grad, 0.2, iq=q, filt_ptr=ptr, filt_idx=idx, ic=ic)
            assert all(bool(torch.isfinite(x).all()) for x in (good[0], good[2], good[3]))
            kinds = [("iq", 3, N + 5), ("iq", 64, -2), ("iq", 5, big), ("target", 9, N), ("target", 65, -1), ("target", 2, big),
                     ("list", 4, N + 1), ("list", 66, -7), ("list", 7, big)]
            if ic is not None:
                kinds.append(("target", 11, outside))                                      # a node, but no candidate
            for kind, b, value in kinds:
                q2, t2, l2 = q.clone(), t.clone(), [l.copy() for l in lists]
                if kind == "iq":
                    q2[b] = value
                elif kind == "target":
                    t2[b] = value
                else:
                    l2[b] = np.sort(np.append(l2[b], value))
                ptr2, idx2 = csr(l2)
                bad = raw_all(mode, M, embs, embs, t2, grad, 0.2, iq=q2, filt_ptr=ptr2, filt_idx=idx2, ic=ic)
                what = f"{metric} {mode} {kind} {value} {'sub' if ic is not None else 'all'}"
                assert bool(torch.isnan(bad[0][b])) and bool(torch.isnan(bad[1][b])), what
                assert not bad[2][b].any(), what
                keep = torch.arange(B, device=DEV) != b
                for k in range(3):
                    assert same_bits(bad[k][keep], good[k][keep]), (what, k)
                # the same call without the bad query
                qk, tk = q[keep].contiguous(), t[keep].contiguous()
                ptrk, idxk = csr([l for j, l in enumerate(lists) if j != b])
                rest = raw_all(mode, M, embs, embs, tk, grad[keep].contiguous(), 0.2, iq=qk, filt_ptr=ptrk, filt_idx=idxk, ic=ic)
                assert same_bits(bad[3], rest[3]), f"{what}: the bad query adds nothing to dc"
    torch.cuda.synchronize()


@pytest.mark.parametrize("metric", R.METRICS)
def test_a_bad_ic_makes_every_query_invalid(metric):
    d, N, B = 8, 300, 5
    M, big = METRIC[metric], 1 << 40
    i = parity_problem(d, N, B, False)
    embs, q, grad = dev(i["embs"]), dev(i["q"]), dev(i["grad"])
    t = torch.full((B,), 2, device=DEV)
    for mode, _ in MODES:
        for what, ic in (("not ascending", np.array([3, 2, 9])), ("repeated", np.array([2, 2, 9])), ("out of range", np.array([2, 9, N])),
                         ("negative", np.array([-1, 2, 9])), ("far out of range", np.array([2, 9, big]))):
            loss, aux, dq, dc = raw_all(mode, M, embs, embs, t, grad, 0.3, iq=q, ic=torch.from_numpy(ic).to(DEV))
            assert bool(torch.isnan(loss).all()) and bool(torch.isnan(aux).all()), f"a bad ic ({what}) makes every query invalid"
            assert not dq.any() and not dc.any(), what
    torch.cuda.synchronize()


# ---- 6. through the model --------------------------------------------------------------------------------------------------
def test_gradients_reach_the_model_parameters():
    kg = ToyKnowledgeGraph(feat_dim=16)
    model = HyperGNN(text_dim=32, node_feat_dim=16, hidden_dim=16).to(DEV).train()
    x, ei, texts = kg.node_features.to(DEV), kg.edge_index.to(DEV), kg.edge_texts
    N = x.size(0)
    q, t = ei[0][:6].contiguous(), ei[1][:6].contiguous()
    r = torch.zeros(16, device=DEV, requires_grad=True)
    for loss_of in (lambda e: model.softmax_loss_by_distance(e, q, t, "l1", query_rows=e[q] + r, scale=0.2),
                    lambda e: model.negative_sampling_loss_by_distance(e, q, t, "complex", margin=2.0, adversarial_temperature=1.0,
                                                                       candidates=torch.arange(0, N, 2, device=DEV))):
        model.zero_grad()
        loss = loss_of(model(x, ei, texts))
        assert bool(torch.isfinite(loss).all())
        loss.mean().backward()
        grads = [p.grad for p in model.parameters() if p.grad is not None]
        assert grads and all(bool(torch.isfinite(g).all()) for g in grads) and any(bool(g.any()) for g in grads)
