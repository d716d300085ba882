"""Distance scores for per-query negative sets on the device (HyperGNN.rank_candidates / softmax_loss /
negative_sampling_loss with negatives= and distance=; include/ghf_distance.h; csrc/distance.hip) against the float64
restatement of tests/_distance_ref.py.

Tolerances are the project's own, loss_check / grad_check of tests/test_softmax_gpu.py at their defaults; ranks are equal
where float64 separates the scores by more than 1e-4 (1 + |t|) and within the count of near-ties otherwise, the rule of
tests/test_negatives_gpu.py.  The kernels have negatives.hip's geometry: 64 / L rows per wave instruction (L = 8, 16, 32, 64
lanes per row at d <= 32, 64, 128, 256 on the vector path; the scalar path where d % 4 != 0 or a base is not 16-byte
aligned), K walked 8 x 64 / L positions at a time, four waves per query above K = 256.  The shapes cross each (path, waves)
pair with K around those steps; B = 129 leaves the last workgroup of four queries with one.  The inputs are built on the
CPU (so that the float64 side can be looked at without a device) the way test_negatives_gpu.setup builds them: padding, a
repeat, the target among its own negatives, a listed partner."""

import numpy as np
import pytest
import torch

import _distance_ref as R
from graph_hypernetwork_forge_amd import ToyKnowledgeGraph, _native
from test_distance_host import explicit_scores
from test_softmax_gpu import csr, grad_check, loss_check, model16

gpu = pytest.mark.gpu
DEV = torch.device("cuda:0")
MODES = (("softmax", {}), ("negsamp", dict(margin=1.5, adversarial_temperature=0.5)))
METRIC = _native.DIST_METRICS

# (d, K, B, N): d of {1, 3, 20, 64, 128, 200, 256} ({2, 6, ...} for "complex"), K of {1, 7, 8, 9, 63, 64, 65, 256, 257, 1000},
# B of {1, 5, 129}, N of {300, 5000}; every path — scalar (d = 1, 3), L = 8 (20), 16 (64), 32 (128), 64 (200, 256) — with one
# wave (K <= 256) and with four (K > 256)
SHAPES = [(1, 1, 1, 300), (3, 7, 5, 300), (3, 257, 5, 5000), (20, 8, 5, 300), (20, 63, 129, 5000), (20, 1000, 5, 300),
          (64, 9, 129, 300), (64, 65, 5, 300), (64, 257, 5, 300), (128, 64, 5, 5000), (128, 256, 5, 300), (128, 257, 5, 300),
          (200, 65, 5, 300), (256, 9, 5, 300), (256, 1000, 1, 300)]
CASES = [(m, (2 * d if m == "complex" and d <= 3 else d, K, B, N)) for m in R.METRICS for d, K, B, N in SHAPES]
CASE_IDS = ["%s-d%d-K%d-B%d-N%d" % ((m,) + s) for m, s in CASES]


def scale_for(metric, d):
    """Logits of order 1: an L1 / complex distance of LayerNorm rows grows like d, an L2 distance like sqrt(d)."""
    return 1.0 if d <= 6 else (d ** -0.5 if metric == "l2" else 2.0 / d)


def rows_cpu(N, d, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, d, generator=g)
    if d > 6:                                   # LayerNorm-shaped rows, what the model's last layer emits
        x = torch.nn.functional.layer_norm(x, (d,), 1.0 + 0.1 * torch.randn(d, generator=g), 0.1 * torch.randn(d, generator=g))
    return x


def setup(d, K, B, N, seed, pad=True):
    """CPU tensors: rows, queries with per-node known partners (so known= and CSR lists agree), negatives that hold padding,
    a repeat, the target and a listed id."""
    rng = np.random.default_rng(seed)
    embs = rows_cpu(N, d, seed)
    query, target = rng.integers(0, N, B), rng.integers(0, N, B)
    if B > 12:
        query[B // 2:B // 2 + 5] = query[:5]                                   # repeated queries
        target[6:12] = target[0]                                               # queries sharing a target
    node_lists = {}
    for i, v in enumerate(query):
        if v not in node_lists:
            node_lists[v] = np.unique(rng.integers(0, N, 4)) if i % 7 else np.zeros(0, dtype=np.int64)
    lists = [node_lists[v] for v in query]
    src = np.concatenate([np.full(len(l), v) for v, l in node_lists.items()] + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
    dst = np.concatenate(list(node_lists.values()) + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
    neg = rng.integers(0, N, (B, K))
    if pad:
        neg[rng.random((B, K)) < 0.15] = -1
    for i in range(B):
        if K >= 3:
            neg[i, K // 2] = neg[i, 0]                                          # a repeat
        if K >= 4 and i % 2 == 0:
            neg[i, K - 1] = target[i]                                           # the target among its own negatives
        if K >= 2 and len(lists[i]):
            neg[i, 1] = lists[i][0]                                             # a known partner
    grad = torch.from_numpy(rng.standard_normal(B).astype(np.float32))
    t = lambda a: torch.from_numpy(np.asarray(a))
    return dict(embs=embs, q=t(query), t=t(target), neg=t(neg), lists=lists, known=(t(src), t(dst)), grad=grad)


def dev(x):
    return tuple(dev(v) for v in x) if isinstance(x, tuple) else x.to(DEV)


def bits(t):
    return t.detach().contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def check_ranks(what, got, metric, rows, c, t, neg, lists):
    """Equal to float64's where it separates every score from the target's; else off by no more than the near-ties."""
    greater, equal = (x.cpu() for x in got)
    live = R.live_positions(neg, t, lists)
    wg, we = R.rank(metric, rows, c, t, neg, lists)
    clear, slack = R.near_ties(metric, rows, c, t, neg, lists)
    assert int(greater.min()) >= 0 and bool((greater + equal <= live.sum(1)).all()), what
    if bool((clear | ~live).all()):
        assert torch.equal(greater, wg) and torch.equal(equal, we), what
    else:
        assert bool(((greater - wg).abs() <= slack).all()) and bool(((equal - we).abs() <= slack).all()), what


def test_the_float64_side_stays_inside_its_near_tie_cap():
    """No GPU: on the seeds below, the positions that float64 cannot separate from the target by 1e-4 (1 + |t|) — what
    check_ranks may excuse — are few (at most 2 % of the live positions, 3 for a small set), and the same formulas in fp32
    on the CPU already land inside that cap."""
    for metric, (d, K, B, N) in CASES:
        i = setup(d, K, B, N, seed=7 * d + K)
        rows = i["embs"][i["q"]]
        live = R.live_positions(i["neg"], i["t"], i["lists"])
        clear, slack = R.near_ties(metric, rows, i["embs"], i["t"], i["neg"], i["lists"])
        assert bool((slack <= torch.clamp(live.sum(1) // 50, min=3)).all()), (metric, d, K, int(slack.max()))
        D32 = torch.stack([R.dist(metric, rows, i["embs"][i["neg"][:, j].clamp(min=0)])[0].float() for j in range(K)], 1)
        Dt32 = R.dist(metric, rows, i["embs"][i["t"]])[0].float()
        wg, _ = R.rank(metric, rows, i["embs"], i["t"], i["neg"], i["lists"])
        assert bool(((((D32 < Dt32.unsqueeze(1)) & live).sum(1) - wg).abs() <= slack).all()), (metric, d, K)


# ---- the three operations and every gradient against float64 -----------------------------------------------------------
@gpu
@pytest.mark.parametrize("metric,shape", CASES, ids=CASE_IDS)
def test_forward_and_gradients_match_float64(metric, shape):
    d, K, B, N = shape
    model = model16()
    i = setup(d, K, B, N, seed=7 * d + K)
    embs, q, t, neg, known, grad = (dev(i[k]) for k in ("embs", "q", "t", "neg", "known", "grad"))
    lists, M = i["lists"], METRIC[metric]
    ptr, idx = csr(lists)
    scale = scale_for(metric, d)
    rows = i["embs"][i["q"]]

    check_ranks("ranks", model.rank_candidates(embs, q, t, known=known, negatives=neg, distance=metric), metric, rows, i["embs"],
                i["t"], i["neg"], lists)
    live = R.live_positions(i["neg"], i["t"], lists).to(DEV)
    for mode, kw in MODES:
        e = embs.clone().requires_grad_()
        fn = model.softmax_loss if mode == "softmax" else model.negative_sampling_loss
        loss = fn(e, q, t, scale=scale, known=known, negatives=neg, distance=metric, **kw)
        want = R.loss(mode, metric, rows, i["embs"], i["t"], i["neg"], lists, scale=scale, margin=kw.get("margin", 0.0),
                      alpha=kw.get("adversarial_temperature", 0.0), grad=i["grad"])
        loss_check(f"{metric} {mode} loss", loss, want["loss"])
        raw = (_native.score_dist_softmax_fwd(M, embs, embs, t, neg, iq=q, filt_ptr=ptr, filt_idx=idx, scale=scale)
               if mode == "softmax" else
               _native.score_dist_negsamp_fwd(M, embs, embs, t, neg, iq=q, filt_ptr=ptr, filt_idx=idx, scale=scale, **kw))
        assert torch.equal(bits(raw[0]), bits(loss))                                     # known= and CSR lists: the same call
        finite = torch.isfinite(want["aux"])
        if bool(finite.any()):
            loss_check(f"{metric} {mode} lse / lw", raw[1][finite.to(DEV)], want["aux"][finite])
        assert torch.equal(raw[1].cpu()[~finite], want["aux"][~finite].float())          # -inf: no negatives
        (loss * grad).sum().backward()
        grad_check(f"{metric} {mode} embs", e.grad.cpu().numpy(), R.embs_grad(want, i["q"]).numpy())
        mode_id = _native.NEG_SOFTMAX if mode == "softmax" else _native.NEG_NEGSAMP
        dq, coef = _native.score_dist_bwd(M, mode_id, embs, embs, t, neg, raw[1], grad, iq=q, filt_ptr=ptr, filt_idx=idx, scale=scale,
                                          margin=kw.get("margin", 0.0), adversarial_temperature=kw.get("adversarial_temperature", 0.0))
        grad_check(f"{metric} {mode} dq", dq.cpu().numpy(), want["dq"].numpy())
        grad_check(f"{metric} {mode} coef", coef.cpu().numpy(), want["coef"].numpy())
        assert bool((coef[:, :K][~live] == 0).all())                                      # exactly 0 outside J_i
        keys = torch.cat([torch.where(neg < 0, t.unsqueeze(1), neg), t.unsqueeze(1)], 1).reshape(-1)
        dc = _native.dist_rows_grad(M, embs, embs, coef, *_native.group_edges(keys, N), iq=q)
        grad_check(f"{metric} {mode} dc", dc.cpu().numpy(), want["dc"].numpy())


def raw_all(M, rows, embs, q, t, neg, ptr, idx, grad, with_dc=True, scale=0.4):
    """Every entry point of the header on one input (q = None: `rows` are the queries' own)."""
    kw = dict(iq=q, filt_ptr=ptr, filt_idx=idx)
    greater, equal = _native.score_dist_rank(M, rows, embs, t, neg, **kw)
    loss, lse = _native.score_dist_softmax_fwd(M, rows, embs, t, neg, scale=scale, **kw)
    nl, lw = _native.score_dist_negsamp_fwd(M, rows, embs, t, neg, scale=scale, margin=1.0, adversarial_temperature=0.5, **kw)
    dq1, c1 = _native.score_dist_bwd(M, _native.NEG_SOFTMAX, rows, embs, t, neg, lse, grad, scale=scale, **kw)
    dq2, c2 = _native.score_dist_bwd(M, _native.NEG_NEGSAMP, rows, embs, t, neg, lw, grad, scale=scale, margin=1.0,
                                     adversarial_temperature=0.5, **kw)
    out = dict(greater=greater, equal=equal, loss=loss, lse=lse, nl=nl, lw=lw, dq1=dq1, c1=c1, dq2=dq2, c2=c2)
    if with_dc:
        N = embs.size(0)
        keys = torch.cat([torch.where(neg < 0, t.unsqueeze(1), neg), t.unsqueeze(1)], 1).reshape(-1).clamp(0, N - 1)
        group = _native.group_edges(keys, N)
        out.update(dc1=_native.dist_rows_grad(M, rows, embs, c1, *group, iq=q), dc2=_native.dist_rows_grad(M, rows, embs, c2, *group, iq=q))
    return out


def check_all(what, got, metric, rows, c, t, neg, lists, grad, scale=0.4):
    """raw_all's outputs (margin 1, temperature 0.5) against the restatement."""
    check_ranks(what, (got["greater"], got["equal"]), metric, rows, c, t, neg, lists)
    for mode, lk, ak, dqk, ck, dck in (("softmax", "loss", "lse", "dq1", "c1", "dc1"), ("negsamp", "nl", "lw", "dq2", "c2", "dc2")):
        want = R.loss(mode, metric, rows, c, t, neg, lists, scale=scale, margin=1.0, alpha=0.5, grad=grad)
        for k in (lk, dqk, ck, dck):
            assert bool(torch.isfinite(got[k]).all()), (what, k)
        loss_check(f"{what} {mode} loss", got[lk], want["loss"])
        grad_check(f"{what} {mode} dq", got[dqk].cpu().numpy(), want["dq"].numpy())
        grad_check(f"{what} {mode} coef", got[ck].cpu().numpy(), want["coef"].numpy())
        grad_check(f"{what} {mode} dc", got[dck].cpu().numpy(), want["dc"].numpy())


# ---- 1. a base pointer that is not 16-byte aligned ---------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("metric", R.METRICS)
def test_unaligned_base_takes_the_scalar_path(metric):
    d, K, B, N = 128, 9, 5, 300
    i = setup(d, K, B, N, seed=11)
    buf = torch.zeros(N * d + 4, device=DEV)
    embs = buf[1:1 + N * d].view(N, d)                                       # one float into a larger buffer
    embs.copy_(i["embs"])
    assert embs.data_ptr() % 16 == 4 and embs.is_contiguous()
    q, t, neg, grad = (dev(i[k]) for k in ("q", "t", "neg", "grad"))
    ptr, idx = csr(i["lists"])
    sc = scale_for(metric, d)
    one = raw_all(METRIC[metric], embs, embs, q, t, neg, ptr, idx, grad, scale=sc)
    two = raw_all(METRIC[metric], embs, embs, q, t, neg, ptr, idx, grad, scale=sc)
    for k in one:
        assert torch.equal(bits(one[k]), bits(two[k])), k
    check_all(f"{metric} unaligned", one, metric, i["embs"][i["q"]], i["embs"], i["t"], i["neg"], i["lists"], i["grad"], scale=sc)


# ---- 2. exact data -------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("d,K,B", [(3, 9, 129), (20, 257, 5), (64, 63, 129), (128, 64, 129), (200, 65, 5), (256, 9, 129), (256, 257, 5)])
def test_exact_integer_rows(d, K, B):
    """Integer rows in [-8, 8]: every difference, |.|, square and partial sum is an integer below 2^24 (sums of squares stay
    <= 256 x 16^2 = 2^16), so L1 distances are exact in fp32 whatever the order, and sums of squares too — distinct sums then
    have roots more than 2^-18 apart relatively, far more than an ulp, and equal sums give equal bits.  Each query gets, first
    in its row, the MIRROR of its target through its own row (2 q - c[t]: every difference negated, the same distance under
    every metric) and a copy of its target: two ties.  L1 and L2 counts equal float64's exactly; for the complex modulus, a
    sum of roots, the ties are still exact."""
    N = 600
    model = model16()
    i = setup(d, K, B, N, seed=d + K)
    rng = np.random.default_rng(d)
    embs = torch.from_numpy(rng.integers(-8, 9, (N, d)).astype(np.float32))
    q = torch.from_numpy(rng.integers(0, 40, B))
    t = torch.from_numpy(rng.integers(40, 80, B))
    rows = torch.from_numpy(rng.integers(-8, 9, (B, d)).astype(np.float32))              # B <= 129 planted nodes each, from the top
    embs[N - B:] = 2 * rows - embs[t]
    embs[N - 2 * B:N - B] = embs[t]
    neg = i["neg"].clone()
    neg[neg >= N - 2 * B] -= 2 * B                                                        # (no planted node by chance)
    neg[:, 0] = N - B + torch.arange(B)
    if K > 4:
        neg[:, 3] = N - 2 * B + torch.arange(B)
    for metric in R.METRICS:
        if metric == "complex" and d % 2:
            continue
        greater, equal = model.rank_candidates(dev(embs), dev(q), dev(t), query_rows=dev(rows), negatives=dev(neg), distance=metric)
        wg, we = R.rank(metric, rows, embs, t, neg, None)
        assert int(we.min()) >= (2 if K > 4 else 1)
        if metric == "complex":
            check_ranks("complex", (greater, equal), metric, rows, embs, t, neg, None)
            assert bool((equal.cpu() >= (2 if K > 4 else 1)).all())
        else:
            assert torch.equal(greater.cpu(), wg) and torch.equal(equal.cpu(), we), metric


@gpu
@pytest.mark.parametrize("d", [3, 20, 128, 200])
def test_l1_backward_on_integer_rows_is_exact(d):
    """K = 1: dq[i] = -(G_i1 sign(q - c[n]) + G_it sign(q - c[t])), one fp32 addition of two of the call's own coefficients —
    exact where float64 is: the kernel's dq equals that sum formed in float64 from its coef and rounded once."""
    N, B, K = 300, 129, 1
    rng = np.random.default_rng(d)
    embs = torch.from_numpy(rng.integers(-8, 9, (N, d)).astype(np.float32))
    rows = torch.from_numpy(rng.integers(-8, 9, (B, d)).astype(np.float32))
    t, neg = torch.from_numpy(rng.integers(0, N // 2, B)), torch.from_numpy(rng.integers(N // 2, N, (B, K)))
    grad = torch.from_numpy(rng.standard_normal(B).astype(np.float32))
    M = _native.DIST_L1
    for mode, fwd in ((_native.NEG_SOFTMAX, _native.score_dist_softmax_fwd), (_native.NEG_NEGSAMP, _native.score_dist_negsamp_fwd)):
        loss, aux = fwd(M, dev(rows), dev(embs), dev(t), dev(neg), scale=1.0 / d)
        want = R.loss("softmax" if mode == _native.NEG_SOFTMAX else "negsamp", "l1", rows, embs, t, neg, None, scale=1.0 / d)
        loss_check("integer L1 loss", loss, want["loss"])
        dq, coef = _native.score_dist_bwd(M, mode, dev(rows), dev(embs), dev(t), dev(neg), aux, dev(grad), scale=1.0 / d)
        c64 = coef.cpu().double()
        exact = -(c64[:, :1] * R.dist("l1", rows, embs[neg[:, 0]])[1] + c64[:, 1:] * R.dist("l1", rows, embs[t])[1])
        assert torch.equal(dq.cpu(), exact.float())
        assert int((dq != 0).sum()) > B * d // 2


# ---- 3. zero distance ----------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("metric", R.METRICS)
@pytest.mark.parametrize("d,K", [(6, 9), (20, 9), (128, 65), (200, 257)])
def test_zero_distance_is_finite_and_follows_the_conventions(metric, d, K):
    """The queries are embs' own rows; each has its own node first among its negatives (D = 0, and the same row on both
    sides of every difference), a bit-identical twin second, and third a row that differs from its own in one pair only."""
    N, B = 300, 5
    i = setup(d, K, B, N, seed=K + d)
    embs, neg = i["embs"].clone(), i["neg"].clone()
    q = torch.arange(B) + 20
    t = torch.arange(B) + 40
    embs[N - B:] = embs[q]                                                    # twins
    embs[N - 2 * B:N - B] = embs[q]
    embs[N - 2 * B:N - B, 2] += 0.75                                          # one pair differs (pair 1: floats 2, 3)
    neg[neg >= N - 2 * B] -= 2 * B
    neg[:, 0], neg[:, 1], neg[:, 2] = q, N - B + torch.arange(B), N - 2 * B + torch.arange(B)
    lists = [np.zeros(0, dtype=np.int64)] * B
    ptr, idx = csr(lists)
    sc = scale_for(metric, d)
    got = raw_all(METRIC[metric], dev(embs), dev(embs), dev(q), dev(t), dev(neg), ptr, idx, dev(i["grad"]), scale=sc)
    check_all(f"{metric} zero", got, metric, embs[q], embs, t, neg, lists, i["grad"], scale=sc)
    D, g = R.dist(metric, embs[q], embs[neg[:, 2]])
    assert torch.allclose(D, torch.full((B,), 0.75, dtype=torch.float64)) and int((g != 0).sum()) == B
    assert bool((got["c1"][:, :2] != 0).all()) and bool((got["c2"][:, :2] != 0).all())       # zero distance, yet weight
    # through the method: d embs, with the fold of dq through the queries' own rows
    model = model16()
    for mode, kw in MODES:
        e = dev(embs).requires_grad_()
        fn = model.softmax_loss if mode == "softmax" else model.negative_sampling_loss
        (fn(e, dev(q), dev(t), scale=sc, negatives=dev(neg), distance=metric, **kw) * dev(i["grad"])).sum().backward()
        want = R.loss(mode, metric, embs[q], embs, t, neg, lists, scale=sc, margin=kw.get("margin", 0.0),
                      alpha=kw.get("adversarial_temperature", 0.0), grad=i["grad"])
        grad_check(f"{metric} {mode} zero embs", e.grad.cpu().numpy(), R.embs_grad(want, q).numpy())


# ---- 4. query_rows and typed lists ---------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("metric", R.METRICS)
@pytest.mark.parametrize("d,K", [(20, 9), (128, 65), (200, 8)])
def test_query_rows_and_typed_lists(metric, d, K):
    """rows = embs[h] + v recorded in torch (a translation): v's gradient is dq, embs' is dc plus dq folded through h."""
    N, B = 300, 129
    model = model16()
    i = setup(d, K, B, N, seed=d)
    rng = np.random.default_rng(d)
    v0 = torch.from_numpy((0.3 * rng.standard_normal((B, d))).astype(np.float32))
    E = 400
    src, dst, rel = (torch.from_numpy(rng.integers(0, n, E)) for n in (N, N, 3))
    src[:B], dst[:B], rel[:B] = i["q"], i["neg"][:, 0].clamp(min=0), 1                     # every query lists its first negative under rel 1
    qrel = torch.from_numpy(rng.integers(0, 3, B))
    lists = [np.unique(dst[(src == i["q"][n]) & (rel == qrel[n])].numpy()) for n in range(B)]
    rows0 = i["embs"][i["q"]] + v0
    scale = scale_for(metric, d)
    for mode, kw in MODES:
        e, v = dev(i["embs"]).requires_grad_(), dev(v0).requires_grad_()
        fn = model.softmax_loss if mode == "softmax" else model.negative_sampling_loss
        loss = fn(e, dev(i["q"]), dev(i["t"]), scale=scale, known=dev((src, dst, rel)), query_rel=dev(qrel), query_rows=e[dev(i["q"])] + v,
                  negatives=dev(i["neg"]), distance=metric, **kw)
        want = R.loss(mode, metric, rows0, i["embs"], i["t"], i["neg"], lists, scale=scale, margin=kw.get("margin", 0.0),
                      alpha=kw.get("adversarial_temperature", 0.0), grad=i["grad"])
        loss_check(f"{metric} {mode} typed loss", loss, want["loss"])
        (loss * dev(i["grad"])).sum().backward()
        grad_check(f"{metric} {mode} typed rows", v.grad.cpu().numpy(), want["dq"].numpy())
        grad_check(f"{metric} {mode} typed embs", e.grad.cpu().numpy(), R.embs_grad(want, i["q"]).numpy())
    check_ranks("typed ranks", model.rank_candidates(dev(i["embs"]), dev(i["q"]), dev(i["t"]), known=dev((src, dst, rel)), query_rel=dev(qrel),
                                                     query_rows=dev(rows0), negatives=dev(i["neg"]), distance=metric),
                metric, rows0, i["embs"], i["t"], i["neg"], lists)
    ug, _ = R.rank(metric, rows0, i["embs"], i["t"], i["neg"], None)                        # (the lists do remove something)
    assert int((ug - R.rank(metric, rows0, i["embs"], i["t"], i["neg"], lists)[0]).sum()) > 0


# ---- 5. untouched rows, 6. a hub, 7. padding and empty sets ------------------------------------------------------------
@gpu
@pytest.mark.parametrize("metric", R.METRICS)
def test_untouched_rows_get_exactly_zero(metric):
    N, d, B, K = 5000, 128, 129, 9
    model = model16()
    i = setup(d, K, B, N, seed=9)
    q, t, neg = dev(i["q"]), dev(i["t"]), dev(i["neg"])
    touched = torch.zeros(N, dtype=torch.bool, device=DEV)
    touched[q] = True
    touched[t] = True
    touched[neg[neg >= 0]] = True
    assert int((~touched).sum()) > 1000 and not bool(touched[0])             # node 0, where a clamped padding id would land
    for mode, kw in MODES:
        fn = model.softmax_loss if mode == "softmax" else model.negative_sampling_loss
        e = dev(i["embs"]).requires_grad_()
        (fn(e, q, t, scale=scale_for(metric, d), known=dev(i["known"]), negatives=neg, distance=metric, **kw) * dev(i["grad"])).sum().backward()
        assert int(bits(e.grad[~touched]).abs().sum()) == 0
        assert bool((e.grad[touched].abs().sum(1) > 0).any())


@gpu
@pytest.mark.parametrize("metric", R.METRICS)
def test_hub_one_id_in_every_position(metric):
    """B = 129, K = 65: node 17's segment holds 8,385 entries, walked by one wave in order."""
    N, d, B, K = 300, 64, 129, 65
    model = model16()
    i = setup(d, K, B, N, seed=5)
    t = i["t"].clone()
    t[t == 17] = 18
    neg = torch.full((B, K), 17, dtype=torch.int64)
    for mode, kw in MODES:
        fn = model.softmax_loss if mode == "softmax" else model.negative_sampling_loss
        e = dev(i["embs"]).requires_grad_()
        loss = fn(e, dev(i["q"]), dev(t), scale=scale_for(metric, d), negatives=dev(neg), distance=metric, **kw)
        (loss * dev(i["grad"])).sum().backward()
        want = R.loss(mode, metric, i["embs"][i["q"]], i["embs"], t, neg, None, scale=scale_for(metric, d), margin=kw.get("margin", 0.0),
                      alpha=kw.get("adversarial_temperature", 0.0), grad=i["grad"])
        loss_check(f"{metric} {mode} hub", loss, want["loss"])
        grad_check(f"{metric} {mode} hub embs", e.grad.cpu().numpy(), R.embs_grad(want, i["q"]).numpy())


@gpu
@pytest.mark.parametrize("metric", R.METRICS)
@pytest.mark.parametrize("d,K", [(20, 65), (128, 17), (256, 9), (6, 7)])
def test_padding_and_empty_sets(metric, d, K):
    N, B = 300, 6
    i = setup(d, K, B, N, seed=K, pad=False)
    neg, t = i["neg"].clone(), i["t"]
    neg[0, 0] = -1                                                           # first
    neg[1, K - 1] = -1                                                       # last
    neg[2, ::2] = -1                                                         # scattered
    neg[3] = -1                                                              # a whole row
    neg[4] = t[4]                                                            # every negative is the target
    lists = list(i["lists"])
    lists[5] = np.unique(neg[5].numpy())                                     # every negative is listed
    lists[4], lists[3] = np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    ptr, idx = csr(lists)
    sc = scale_for(metric, d)
    got = raw_all(METRIC[metric], dev(i["embs"]), dev(i["embs"]), dev(i["q"]), dev(t), dev(neg), ptr, idx, dev(i["grad"]), scale=sc)
    empty = torch.tensor([3, 4, 5], device=DEV)
    assert torch.equal(bits(got["loss"][empty]), torch.zeros(3, dtype=torch.int32, device=DEV))         # exactly +0
    assert bool((got["lw"][empty] == float("-inf")).all())
    assert int(got["greater"][empty].abs().sum() + got["equal"][empty].abs().sum()) == 0
    check_all(f"{metric} padded", got, metric, i["embs"][i["q"]], i["embs"], t, neg, lists, i["grad"], scale=sc)
    Dt = R.dist(metric, i["embs"][i["q"]], i["embs"][t])[0]
    want_pos = torch.nn.functional.softplus(-(-sc * Dt + 1.0))
    loss_check("the positive term alone", got["nl"][empty], want_pos[empty.cpu()])
    assert bool((got["c1"][empty] == 0).all()) and bool((got["dq1"][empty] == 0).all())   # p_t = 1: nothing to learn
    assert bool((got["c2"][empty, :K] == 0).all()) and bool((got["c2"][empty, K] != 0).all())


# ---- 8. invalid ids, 9. reproducibility and batch independence ----------------------------------------------------------
@gpu
@pytest.mark.parametrize("metric", R.METRICS)
@pytest.mark.parametrize("d,K", [(128, 65), (20, 9), (6, 7)])
def test_invalid_ids_touch_their_query_alone(metric, d, K):
    N, B = 300, 9
    i = setup(d, K, B, N, seed=d + 3)
    embs, q, t, neg, grad = (dev(i[k]) for k in ("embs", "q", "t", "neg", "grad"))
    ptr, idx = csr(i["lists"])
    M = METRIC[metric]
    good = raw_all(M, embs, embs, q, t, neg, ptr, idx, grad, with_dc=False)
    bad_neg = neg.clone()
    bad_neg[2, K - 1] = N                                                    # one past the table
    bad_neg[5, 0] = -2                                                       # not the padding
    bad_q, bad_t = q.clone(), t.clone()
    bad_q[7] = N + 5
    bad_t[1] = -1
    got = raw_all(M, embs, embs, bad_q, bad_t, bad_neg, ptr, idx, grad, with_dc=False)
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
    # the scatter with ids outside their ranges: such entries are skipped, the others' sums are unchanged
    keys = torch.cat([torch.where(neg < 0, t.unsqueeze(1), neg), t.unsqueeze(1)], 1).reshape(-1)
    perm, off = _native.group_edges(keys, N)
    dc = _native.dist_rows_grad(M, embs, embs, good["c1"], perm, off, iq=q)
    bad_perm = perm.clone()
    bad_perm[0], bad_perm[1] = -1, B * (K + 1)
    dropped = good["c1"].clone().reshape(-1)
    dropped[perm[:2]] = 0.0
    want = _native.dist_rows_grad(M, embs, embs, dropped.reshape(B, K + 1), perm, off, iq=q)
    assert torch.equal(bits(_native.dist_rows_grad(M, embs, embs, good["c1"], bad_perm, off, iq=q)), bits(want))
    zeroed = good["c1"].clone()
    zeroed[7] = 0.0
    assert torch.equal(bits(_native.dist_rows_grad(M, embs, embs, good["c1"], perm, off, iq=bad_q)),
                       bits(_native.dist_rows_grad(M, embs, embs, zeroed, perm, off, iq=q)))
    assert bool(torch.isfinite(dc).all())


@gpu
@pytest.mark.parametrize("metric", R.METRICS)
@pytest.mark.parametrize("d,K", [(128, 257), (128, 256), (64, 9), (200, 65)])
def test_twice_the_same_bits_and_a_query_alone_as_in_its_batch(metric, d, K):
    N, B = 300, 129
    model = model16()
    i = setup(d, K, B, N, seed=K)
    embs, q, t, neg, grad = (dev(i[k]) for k in ("embs", "q", "t", "neg", "grad"))
    ptr, idx = csr(i["lists"])
    M = METRIC[metric]
    one = raw_all(M, embs, embs, q, t, neg, ptr, idx, grad)
    two = raw_all(M, embs, embs, q, t, neg, ptr, idx, grad)
    for k in one:
        assert torch.equal(bits(one[k]), bits(two[k])), k
    grads = []
    for _ in range(2):
        e = embs.clone().requires_grad_()
        (model.negative_sampling_loss(e, q, t, scale=scale_for(metric, d), known=dev(i["known"]), negatives=neg, distance=metric,
                                      margin=1.0, adversarial_temperature=1.0) * grad).sum().backward()
        grads.append(e.grad)
    assert torch.equal(bits(grads[0]), bits(grads[1]))
    for n in (0, 77, 128):                                                    # alone: B = 1, first place
        pi, xi = csr([i["lists"][n]])
        alone = raw_all(M, embs, embs, q[n:n + 1], t[n:n + 1], neg[n:n + 1], pi, xi, grad[n:n + 1], with_dc=False)
        for k in alone:
            assert torch.equal(bits(alone[k][0]), bits(one[k][n])), (k, n)


# ---- 10. end to end ------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("metric", R.METRICS)
def test_backward_through_the_model_matches_float64_autograd(metric):
    """loss.backward() through HyperGNN on the toy graph (hidden 16): the parameters' gradients against float64 autograd
    through the oracle's forward and the explicit [B, K, d] formulation of the negative-sampling loss under the distance."""
    from oracle import hypergnn_oracle as O
    torch.manual_seed(0)
    kg = ToyKnowledgeGraph(feat_dim=16)
    model = model16().train()
    x, ei, texts = kg.node_features.to(DEV), kg.edge_index.to(DEV), kg.edge_texts
    N = x.size(0)
    rng = np.random.default_rng(4)
    B, K = 7, 5
    q = torch.from_numpy(rng.integers(0, N, B))
    t = torch.from_numpy(rng.integers(0, N, B))
    neg = torch.from_numpy(rng.integers(-1, N, (B, K)))
    neg[:, 1] = neg[:, 0]
    loss = model.negative_sampling_loss(model(x, ei, texts), dev(q), dev(t), scale=0.5, negatives=dev(neg), distance=metric, margin=2.0,
                                        adversarial_temperature=1.0).sum()
    loss.backward()

    params = {k: v.detach().cpu().double().requires_grad_(True) for k, v in model.state_dict().items()}
    e64 = O.forward(params, kg.node_features.double(), kg.edge_index.numpy(), texts, variant="factorised", dtype=torch.float64)
    s, st = explicit_scores(metric, e64[q], e64, t, neg)
    z, zt = 0.5 * s, 0.5 * st
    drop = (neg == -1) | (neg == t.unsqueeze(1))
    w = torch.nan_to_num(torch.softmax(z.masked_fill(drop, -np.inf), 1).detach())
    want = (torch.nn.functional.softplus(-(zt + 2.0)) + (w * torch.nn.functional.softplus(z + 2.0).masked_fill(drop, 0.0)).sum(1)).sum()
    loss_check(f"{metric} through the model", loss.reshape(1), want.detach().reshape(1))
    want.backward()
    # A distance sees differences of rows only, so the last LayerNorm's bias, which moves every row alike, has a gradient that is
    # a sum cancelling to zero: float64 leaves 1e-16 of it, fp32 1e-7, and grad_check's tolerance, relative to the tensor's own
    # largest entry, has nothing to hold on to.  Such a tensor (below 1e-10 of the largest gradient entry of the model in
    # float64) is held to 1e-5 of that entry instead — fp32's rounding of the terms that cancel, not a looser rule: grad_check
    # allows 1e-4 of a tensor's scale.
    top = max(float(v.grad.abs().max()) for v in params.values() if v.grad is not None)
    checked, scalars = 0, {}                       # one-element parameters compared as the vector they form per generator, as
    for k, p in model.named_parameters():          # test_negatives_gpu does and explains
        if params[k].grad is not None and 0 < float(params[k].grad.abs().max()) < 1e-10 * top:
            print(f"d{k}: cancels in float64 ({float(params[k].grad.abs().max()):.1e}), got max {float(p.grad.abs().max()):.3e}, top {top:.3e}")
            assert float(p.grad.abs().max()) <= 1e-5 * top, k
            continue
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


# ---- 11. without the keyword nothing changed ---------------------------------------------------------------------------
class _Names:
    """The loaded library, noting which entry points are reached."""

    def __init__(self, lib):
        self._lib, self.called = lib, []

    def __getattr__(self, name):
        if name.startswith("ghf_"):
            self.called.append(name)
        return getattr(self._lib, name)


@gpu
def test_without_the_keyword_the_methods_reach_the_dot_product_calls(monkeypatch):
    d, K, B, N = 128, 65, 129, 300
    model = model16()
    i = setup(d, K, B, N, seed=3)
    embs, q, t, neg, known, grad = (dev(i[k]) for k in ("embs", "q", "t", "neg", "known", "grad"))
    ptr, idx = csr(i["lists"])
    rec = _Names(_native.load())
    monkeypatch.setattr(_native, "_lib", rec)
    greater, equal = model.rank_candidates(embs, q, t, known=known, negatives=neg)
    sm = model.softmax_loss(embs, q, t, scale=0.3, known=known, negatives=neg)
    ns = model.negative_sampling_loss(embs, q, t, scale=0.3, known=known, negatives=neg, margin=1.0, adversarial_temperature=0.5)
    e = embs.clone().requires_grad_()
    (model.negative_sampling_loss(e, q, t, scale=0.3, known=known, negatives=neg, margin=1.0, adversarial_temperature=0.5) * grad).sum().backward()
    assert not [n for n in rec.called if n.startswith("ghf_dist_")]
    assert {"ghf_neg_rank", "ghf_neg_softmax_fwd", "ghf_neg_negsamp_fwd", "ghf_neg_bwd", "ghf_segment_axpy"} <= set(rec.called)
    kw = dict(iq=q, filt_ptr=ptr, filt_idx=idx)
    rg, re_ = _native.score_neg_rank(embs, embs, t, neg, **kw)
    assert torch.equal(greater, rg) and torch.equal(equal, re_)
    assert torch.equal(bits(sm), bits(_native.score_neg_softmax_fwd(embs, embs, t, neg, scale=0.3, **kw)[0]))
    nl, lw = _native.score_neg_negsamp_fwd(embs, embs, t, neg, scale=0.3, margin=1.0, adversarial_temperature=0.5, **kw)
    assert torch.equal(bits(ns), bits(nl))
    dq, coef = _native.score_neg_bwd(_native.NEG_NEGSAMP, embs, embs, t, neg, lw, grad, scale=0.3, margin=1.0, adversarial_temperature=0.5,
                                     **kw)
    keys = torch.cat([torch.where(neg < 0, t.unsqueeze(1), neg), t.unsqueeze(1)], 1).reshape(-1)
    perm, off = _native.group_edges(keys, N)
    owner = q.index_select(0, torch.div(perm, K + 1, rounding_mode="floor"))
    want = _native.segment_axpy(coef.reshape(-1), perm, embs, owner, off)
    fperm, foff = _native.group_edges(q, N)
    want = _native.add3(want, _native.segment_axpy(torch.ones(B, device=DEV), fperm, dq, fperm, foff))
    assert torch.equal(bits(e.grad), bits(want))
    # and with it, the distance calls — on the same input the two differ
    rec.called.clear()
    model.softmax_loss(embs, q, t, scale=0.3, known=known, negatives=neg, distance="l2")
    assert "ghf_dist_softmax_fwd" in rec.called and not [n for n in rec.called if n.startswith("ghf_neg_")]
