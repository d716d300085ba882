"""The pairwise ranking losses by dot product against every node or a shared candidate set (HyperGNN.pairwise_loss_by_dot,
ghf_score_pair_*, csrc/pairwise_dot_sweep.hip + rank_sweep.h + softmax.hip) on the GPU, against the float64 restatement of
tests/_pairwise_dot_sweep_ref.py.

Tolerances are the project's own and no new number is introduced: losses (and the logistic dsum) under
test_softmax_gpu.loss_check, gradients under test_softmax_gpu.grad_check, both at their defaults, as the other dot-product
losses (tests/test_negsamp_gpu.py); counts are exact.  The hinge's gradient and `active` jump at u = 0, so the parity problems
carry the kink rule of tests/_pairwise_sweep_ref.py: a query with a pair inside the near-tie band takes grad_loss = 0 in the
call and in the reference and its `active` is held to +- its in-band pairs; tests/test_pairwise_dot_sweep_host.py checks,
without a device, that at most B / 8 queries of any problem are such and that fp32 on the CPU passes the same checks on these
very problems.  The integer tests and the bias-gradient tests need no tolerance at all.

Shapes come from the sweeps' geometry (tests/_pairwise_dot_sweep_ref.SHAPES says which edge each one sits on)."""

import numpy as np
import pytest
import torch

import _pairwise_dot_sweep_ref as S
from graph_hypernetwork_forge_amd import HyperGNN, RelationDecoder, ToyKnowledgeGraph, _native
from test_distance_gpu import rows_cpu
from test_softmax_gpu import csr, grad_check, loss_check

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
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
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def raw_fwd(kind, q, c, t, scale, margin=MARGIN, normalize=True, **kw):
    return _native.score_pair_sweep_fwd(KIND[kind], q, c, t, scale=scale, margin=margin, normalize=normalize, **kw)


def raw_all(kind, q, c, t, grad, scale, margin=MARGIN, normalize=True, **kw):
    """(loss, dsum, count, active, dq, dc[, db])"""
    f = raw_fwd(kind, q, c, t, scale, margin, normalize, **kw)
    return f + _native.score_pair_sweep_bwd(KIND[kind], q, c, t, f[1], f[2], grad, scale=scale, margin=margin, normalize=normalize, **kw)


def integer_rows(N, d, seed, lo=-3, hi=4):
    return torch.from_numpy(np.random.default_rng(seed).integers(lo, hi, (N, d)).astype(np.float32))


def positions(P, lists, t):
    """lists and targets of node ids as positions in the ascending id set P (ids outside P dropped)"""
    pos = {int(v): j for j, v in enumerate(P.tolist())}
    lists_p = [np.array(sorted(pos[v] for v in np.asarray(l).tolist() if v in pos), dtype=np.int64) for l in lists]
    return lists_p, torch.tensor([pos[int(v)] for v in t], device=DEV)


# ---- 1. parity -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", S.SHAPES, ids=S.SHAPE_IDS)
def test_losses_counts_and_gradients_match_float64(model, shape):
    """Both kinds, normalize on and off, with and without candidate_bias (S.combos), in two forms: all nodes with queries by id
    and known= pairs — equal bit for bit to the CSR lists — and a candidate subset (shuffled ids) with given query_rows and CSR
    lists.  Loss, count, active, dsum, d embs, d query_rows, d candidate_bias."""
    d, C, B = shape
    scale = S.scale_for(d)
    for subset, by_id in S.FORMS:
        i = S.problem(shape, subset)
        embs, q, t, rows, known, cand, bias = (dev(i[k]) for k in ("embs", "q", "t", "rows", "known", "cand", "bias"))
        ptr, idx = csr(i["lists"])
        P = S.candidate_set(embs.size(0), i["t"], i["cand"])
        ic = None if cand is None else torch.from_numpy(P).to(DEV)
        for kind, normalize, biased in S.combos(shape):
            kw = dict(loss=kind, margin=MARGIN, scale=scale, normalize=normalize, candidates=cand, return_active=True)
            what = f"{kind} {'subset' if subset else 'all'} normalize={normalize} bias={biased}"
            want, grad, nr, inb = S.reference(shape, subset, kind, normalize, by_id, biased)
            b = bias.clone().requires_grad_() if biased else None
            if by_id:
                e = embs.clone().requires_grad_()
                loss, active = model.pairwise_loss_by_dot(e, q, t, known=known, candidate_bias=b, **kw)
                (loss * dev(grad)).sum().backward()
                grad_check(f"{what} by id: embs", e.grad.cpu().numpy(), S.embs_grad(want, i["q"]).numpy())
                listed = model.pairwise_loss_by_dot(embs, q, t, filt_ptr=ptr, filt_idx=idx, candidate_bias=bias if biased else None, **kw)
                assert same_bits(loss, listed[0]) and torch.equal(active, listed[1]), f"{what}: CSR lists equal to known= bit for bit"
                raw = raw_fwd(kind, embs, embs, t, scale, normalize=normalize, iq=q, filt_ptr=ptr, filt_idx=idx, ic=ic,
                              bias=bias if biased else None)
            else:
                e, r = embs.clone().requires_grad_(), rows.clone().requires_grad_()
                loss, active = model.pairwise_loss_by_dot(e, q, t, filt_ptr=ptr, filt_idx=idx, query_rows=r, candidate_bias=b, **kw)
                (loss * dev(grad)).sum().backward()
                grad_check(f"{what} rows: embs", e.grad.cpu().numpy(), want["dc"].numpy())
                grad_check(f"{what} rows: query_rows", r.grad.cpu().numpy(), want["dq"].numpy())
                raw = raw_fwd(kind, rows, embs, t, scale, normalize=normalize, filt_ptr=ptr, filt_idx=idx, ic=ic,
                              bias=bias if biased else None)
            if biased:
                grad_check(f"{what}: candidate_bias", b.grad.cpu().numpy(), want["db"].numpy())
            loss_check(f"{what}: loss", loss, want["loss"])
            S.active_check(what, active, want, nr, inb)
            rl, dsum, count, ra = raw
            assert same_bits(rl, loss) and torch.equal(ra, active), f"{what}: the method is the C call"
            assert torch.equal(count.cpu().long(), want["count"]), f"{what}: count"
            if kind == "hinge":
                assert torch.equal(dsum, active.float()), f"{what}: the hinge's dsum is float(active)"
            else:
                loss_check(f"{what}: dsum", dsum, want["dsum"])
            if cand is not None:    # rows (and bias entries) that are neither candidate, target nor query: exactly zero
                outside = torch.from_numpy(np.setdiff1d(np.arange(embs.size(0)), P)).to(DEV)
                assert not e.grad[outside].any() and (b is None or not b.grad[outside].any())


def test_typed_known_with_query_rel(model):
    d, N, B = 20, 300, 40
    rng = np.random.default_rng(17)
    embs = rows_cpu(N, d, 17)
    q, t, qrel = rng.integers(0, N, B), rng.integers(0, N, B), rng.integers(0, 3, B)
    src, dst, rel = np.repeat(q, 3), rng.integers(0, N, 3 * B), rng.integers(0, 3, 3 * B)
    lists = [np.unique(dst[(src == q[i]) & (rel == qrel[i])]) for i in range(B)]
    T = lambda a: torch.from_numpy(a.astype(np.int64))
    scale = S.scale_for(d)
    for kind in S.KINDS:
        want = S.loss(kind, embs[T(q)], embs, T(t), lists, None, None, scale=scale, margin=MARGIN)
        got, active = model.pairwise_loss_by_dot(dev(embs), dev(T(q)), dev(T(t)), loss=kind, scale=scale, margin=MARGIN,
                                                 known=dev((T(src), T(dst), T(rel))), query_rel=dev(T(qrel)), return_active=True)
        loss_check(f"{kind} typed", got, want["loss"])
        nr, inb = S.near(want, MARGIN)
        S.active_check(f"{kind} typed", active, want, nr, inb)


# ---- 2. exact ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,C,B", [(4, 513, 5), (6, 70, 513), (20, 257, 129), (130, 1025, 64), (3, 2, 5), (256, 300, 5)])
def test_exact_on_integer_rows(d, C, B):
    """Entries in {-2..2}, scale = 1, an integer margin, an integer bias and integer grad_loss: every dot product is an integer
    of at most 4 d, every u an integer, every sum far below 2^24 — exact in fp32 whatever the order.  The unnormalised hinge
    loss, count, active, dsum, dq, dc and db equal float64 bit for bit, pairs at u == 0 exactly (no loss, no coefficient)
    included: this pins G_it = -w active and the whole backward with no tolerance."""
    rng = np.random.default_rng(d + C + B)
    for subset in (False, True):
        N = C + 41 if subset else C
        embs = integer_rows(N, d, d + C, -2, 3)
        embs[N - N // 3:] = embs[:N // 3][:N - (N - N // 3)]                               # copies: scores tie and repeat
        P = np.sort(rng.permutation(N)[:C]).astype(np.int64) if subset else np.arange(N, dtype=np.int64)
        t = torch.from_numpy(P[rng.integers(0, C, B)])
        rows = integer_rows(B, d, B, -2, 3)
        lists = [np.unique(rng.integers(0, N, 4)) if i % 3 else np.zeros(0, dtype=np.int64) for i in range(B)]
        lists[0] = np.unique(np.append(lists[0], int(t[0])))                               # a listed target still receives G_it
        grad = torch.from_numpy(rng.integers(-3, 4, B).astype(np.float32))
        ptr, idx = csr(lists)
        ic = torch.from_numpy(P).to(DEV) if subset else None
        zeros = 0
        for margin, bias in ((2.0, None), (0.0, torch.from_numpy(rng.integers(-2, 3, N).astype(np.float32))), (-3.0, None)):
            want = S.loss("hinge", rows, embs, t, lists, P if subset else None, bias, scale=1.0, margin=margin, normalize=False, grad=grad,
                          add_targets=False)
            zeros += int(((want["u"] == 0) & want["live"]).sum())
            out = raw_all("hinge", dev(rows), dev(embs), dev(t), dev(grad), 1.0, margin, False, filt_ptr=ptr, filt_idx=idx, ic=ic,
                          bias=dev(bias))
            loss, dsum, count, active, dq, dc = out[:6]
            what = (d, C, B, subset, margin)
            assert torch.equal(count.cpu().long(), want["count"]) and torch.equal(active.cpu().long(), want["active"]), what
            assert torch.equal(dsum.cpu().double(), want["active"].double()), what
            assert torch.equal(loss.cpu().double(), want["loss"]), what
            assert torch.equal(dq.cpu().double(), want["dq"]), what
            assert torch.equal(dc.cpu().double(), want["dc"][torch.from_numpy(P)]), what
            if bias is not None:
                assert torch.equal(out[6].cpu().double(), want["db"][torch.from_numpy(P)]), what
            soft = raw_fwd("logistic", dev(rows), dev(embs), dev(t), 1.0, margin, False, filt_ptr=ptr, filt_idx=idx, ic=ic, bias=dev(bias))
            assert torch.equal(soft[2], count) and torch.equal(soft[3], active), "the counts do not depend on the kind"
        assert zeros > 0 or C < 3, "integer scores put pairs at u == 0"
        assert int(want["count"].sum()) > 0


# ---- 3. cross-checks -----------------------------------------------------------------------------------------------------
def test_active_is_rank_candidates_greater_at_margin_zero(model):
    """margin = 0, scale = 1, no bias: u > 0 is z_ij > z_it by the very chain and J_i of rank_candidates — exact."""
    for d, C, B in ((20, 1025, 70), (64, 257, 65), (200, 513, 9)):
        for subset in (False, True):
            i = S.make_problem(d, C, B, subset)
            embs, q, t, rows, known, cand = (dev(i[k]) for k in ("embs", "q", "t", "rows", "known", "cand"))
            kw = dict(known=known, candidates=cand, query_rows=rows)
            greater, _ = model.rank_candidates(embs, q, t, **kw)
            want = S.loss("hinge", i["rows"], i["embs"], i["t"], i["lists"], i["cand"], None, scale=1.0, margin=0.0)
            for kind in S.KINDS:
                _, active = model.pairwise_loss_by_dot(embs, q, t, loss=kind, margin=0.0, return_active=True, **kw)
                assert torch.equal(active.long(), greater), (kind, d, C, B, subset)
            ptr, idx = csr(i["lists"])
            P = S.candidate_set(embs.size(0), i["t"], i["cand"])
            ic = None if cand is None else torch.from_numpy(P).to(DEV)
            _, dsum, count, active = raw_fwd("hinge", rows, embs, t, 1.0, 0.0, filt_ptr=ptr, filt_idx=idx, ic=ic)
            assert torch.equal(count.cpu().long(), want["count"]) and torch.equal(dsum, active.float())


def test_shared_set_agrees_with_per_query_negatives(model):
    """candidates=P against pairwise_loss(negatives=P per row): count exact; loss and gradients to rounding, not in bits — the
    per-query kernel's chain runs across a lane group (include/ghf_negatives.h)."""
    d, C, B = 64, 700, 33
    i = S.make_problem(d, C, B, True)
    embs, q, t, known, cand, bias, grad = (dev(i[k]) for k in ("embs", "q", "t", "known", "cand", "bias", "grad"))
    P = torch.from_numpy(S.candidate_set(embs.size(0), i["t"], i["cand"])).to(DEV)
    neg = P.unsqueeze(0).expand(B, -1).contiguous()
    scale = S.scale_for(d)
    for kind in S.KINDS:
        for normalize, biased in ((True, False), (False, True)):
            kw = dict(loss=kind, scale=scale, margin=MARGIN, normalize=normalize, known=known, return_active=True)
            ea, eb = embs.clone().requires_grad_(), embs.clone().requires_grad_()
            ba, bb = (bias.clone().requires_grad_(), bias.clone().requires_grad_()) if biased else (None, None)
            a, act_a = model.pairwise_loss_by_dot(ea, q, t, candidates=cand, candidate_bias=ba, **kw)
            b, act_b = model.pairwise_loss(eb, q, t, negatives=neg, candidate_bias=bb, **kw)
            loss_check(f"{kind} vs per-query", a, b.double().cpu())
            want = S.loss(kind, i["embs"][i["q"]], i["embs"], i["t"], i["lists"], i["cand"], i["bias"] if biased else None, scale=scale,
                          margin=MARGIN, normalize=normalize)
            nr, _ = S.near(want, MARGIN)
            g = grad.clone()
            if kind == "hinge":
                g[dev(nr)] = 0.0
            (a * g).sum().backward()
            (b * g).sum().backward()
            grad_check(f"{kind} vs per-query: embs", ea.grad.cpu().numpy(), eb.grad.cpu().numpy().astype(np.float64))
            if biased:
                grad_check(f"{kind} vs per-query: bias", ba.grad.cpu().numpy(), bb.grad.cpu().numpy().astype(np.float64))
            _, _, count, _ = raw_fwd(kind, embs, embs, t, scale, normalize=normalize, iq=q, ic=P,
                                     **dict(zip(("filt_ptr", "filt_idx"), csr(i["lists"]))))
            assert torch.equal(count.cpu().long(), want["count"])
            assert bool(((act_a - act_b).abs().cpu() <= S.near(want, MARGIN)[1]).all())


# ---- 4. the backward's scores have the forward's bits --------------------------------------------------------------------
@pytest.mark.parametrize("d,C,B", [(64, 700, 1), (200, 300, 1), (20, 2600, 1), (64, 700, 129), (256, 513, 129)])
def test_hinge_bias_gradient_counts_the_forwards_active_pairs(d, C, B):
    """General float rows, hinge, normalize = False, scale = 1, grad = 1, a bias of zeros: G_ij is exactly 1 or 0.  The
    backward's u has the forward's bits, so with B = 1 db holds exactly +1 at `active` entries and -active at the target; with
    B = 129 every query's row of G sums to zero and so does db, exactly (integers below 2^24)."""
    for subset in (False, True):
        i = S.make_problem(d, C, B, subset)
        embs, t, rows = (dev(i[k]) for k in ("embs", "t", "rows"))
        P = S.candidate_set(embs.size(0), i["t"], i["cand"])
        ic = torch.from_numpy(P).to(DEV) if subset else None
        ptr, idx = csr(i["lists"])
        zero = torch.zeros(embs.size(0), device=DEV)
        out = raw_all("hinge", rows, embs, t, torch.ones(B, device=DEV), 1.0, MARGIN, False, filt_ptr=ptr, filt_idx=idx, ic=ic, bias=zero)
        active, db = out[3], out[6]
        assert int(active.sum()) > 0
        assert float(db.sum()) == 0.0, (d, C, B, subset)
        if B == 1:
            tp = int(np.searchsorted(P, int(i["t"][0])))
            assert float(db[tp]) == -float(active[0]), (d, C, subset)
            others = torch.cat([db[:tp], db[tp + 1:]])
            assert int((others == 1).sum()) == int(active[0]) and bool(((others == 0) | (others == 1)).all()), (d, C, subset)


# ---- 5. bits -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [20, 64, 200])
def test_bits(model, d):
    C, B = 1025, 70
    scale = S.scale_for(d)
    i = S.make_problem(d, C, B, True)
    embs, q, t, rows, grad, cand, bias = (dev(i[k]) for k in ("embs", "q", "t", "rows", "grad", "cand", "bias"))
    lists = i["lists"]
    ptr, idx = csr(lists)
    P = torch.from_numpy(S.candidate_set(embs.size(0), i["t"], i["cand"])).to(DEV)
    kw = dict(filt_ptr=ptr, filt_idx=idx)
    for kind in S.KINDS:
        one = raw_all(kind, rows, embs, t, grad, scale, ic=P, bias=bias, **kw)
        two = raw_all(kind, rows, embs, t, grad, scale, ic=P, bias=bias, **kw)
        assert all(same_bits(a, b) for a, b in zip(one, two)), "the same call twice"
        grads = []
        for _ in range(2):
            e = embs.clone().requires_grad_()
            (model.pairwise_loss_by_dot(e, q, t, loss=kind, scale=scale, candidates=cand, **kw) * grad).sum().backward()
            grads.append(e.grad)
        assert same_bits(*grads), "the final gradients twice"
        # the two halves of a batch
        h = B // 2
        lo = raw_fwd(kind, rows[:h].contiguous(), embs, t[:h].contiguous(), scale, ic=P, bias=bias,
                     **dict(zip(("filt_ptr", "filt_idx"), csr(lists[:h]))))
        hi = raw_fwd(kind, rows[h:].contiguous(), embs, t[h:].contiguous(), scale, ic=P, bias=bias,
                     **dict(zip(("filt_ptr", "filt_idx"), csr(lists[h:]))))
        assert all(same_bits(torch.cat([lo[k], hi[k]]), one[k]) for k in range(4)), "halves of a batch"
        # the subset against the all-node call on the contiguous copy embs[P]: positions instead of ids
        lists_p, tp = positions(P, lists, i["t"])
        copy = raw_all(kind, rows, embs[P].contiguous(), tp, grad, scale, bias=bias[P].contiguous(),
                       **dict(zip(("filt_ptr", "filt_idx"), csr(lists_p))))
        assert all(same_bits(a, b) for a, b in zip(one, copy)), "candidates=P equals the call on embs[P]"
        # a bias of zeros against no bias
        none = raw_all(kind, rows, embs, t, grad, scale, ic=P, **kw)
        zero = raw_all(kind, rows, embs, t, grad, scale, ic=P, bias=torch.zeros_like(bias), **kw)
        assert all(same_bits(a, b) for a, b in zip(none, zero[:6])), "a bias of zeros keeps the bits"
        # shuffled against sorted candidates
        a = model.pairwise_loss_by_dot(embs, q, t, loss=kind, scale=scale, candidates=cand, **kw)
        b = model.pairwise_loss_by_dot(embs, q, t, loss=kind, scale=scale, candidates=torch.sort(cand).values, **kw)
        assert same_bits(a, b), "candidates in any order"
        # an unaligned base: the scalar load path gives the aligned call's bits, forward and backward
        buf = torch.empty(embs.numel() + 1, device=DEV)
        off = buf[1:].view_as(embs).copy_(embs)
        rbuf = torch.empty(rows.numel() + 1, device=DEV)
        roff = rbuf[1:].view_as(rows).copy_(rows)
        assert off.data_ptr() % 16 and roff.data_ptr() % 16
        un = raw_all(kind, roff, off, t, grad, scale, ic=P, bias=bias, **kw)
        assert all(same_bits(a, b) for a, b in zip(one, un)), "the load path does not change the bits"


# ---- 6. edge semantics ---------------------------------------------------------------------------------------------------
def test_the_target_alone(model):
    """C = 1: J_i is empty — loss exactly 0, count 0, active 0, and not one gradient."""
    d, N, B = 20, 40, 5
    embs = rows_cpu(N, d, 3).to(DEV)
    rows = rows_cpu(B, d, 4).to(DEV)
    t = torch.full((B,), 7, device=DEV)
    ic = torch.tensor([7], device=DEV)
    grad = torch.ones(B, device=DEV)
    bias = torch.ones(N, device=DEV)
    for kind in S.KINDS:
        for normalize in (True, False):
            loss, dsum, count, active, dq, dc, db = raw_all(kind, rows, embs, t, grad, 0.7, normalize=normalize, ic=ic, bias=bias)
            assert not loss.any() and not dsum.any() and not count.any() and not active.any() and same_bits(loss, torch.zeros_like(loss))
            assert not dq.any() and not dc.any() and not db.any() and tuple(dc.shape) == (1, d) and tuple(db.shape) == (1,)
        e = embs.clone().requires_grad_()
        out = model.pairwise_loss_by_dot(e, t[:1], t[:1], loss=kind, candidates=ic)
        out.sum().backward()
        assert float(out.detach().abs().max()) == 0.0 and not e.grad.any()
        one = raw_all(kind, embs[:1].contiguous(), embs[:1].contiguous(), torch.zeros(1, dtype=torch.int64, device=DEV), grad[:1], 1.0)
        assert float(one[0]) == 0.0 and int(one[2]) == 0 and not one[4].any() and not one[5].any()       # N = 1, every node


def test_an_empty_j_a_listed_target_and_listed_ids_outside_the_subset(model):
    d, N, B = 20, 400, 6
    embs = rows_cpu(N, d, 21)
    rng = np.random.default_rng(21)
    cand = np.arange(0, N, 3)
    t = cand[rng.integers(0, len(cand), B)]
    q = rng.integers(0, N, B)
    lists = [np.unique(np.concatenate([[t[i]], [1, 2, 4, 5], cand[rng.integers(0, len(cand), 3)]])) for i in range(B)]
    lists[3] = np.unique(np.concatenate([cand, [1, 2]]))                                   # every candidate listed: J_3 is empty
    ptr, idx = csr(lists)
    T = torch.from_numpy
    grad = torch.ones(B)
    scale = S.scale_for(d)
    for kind in S.KINDS:
        want = S.loss(kind, embs[T(q)], embs, T(t), lists, cand, None, scale=scale, margin=MARGIN, grad=grad)
        assert int(want["count"][3]) == 0
        e = dev(embs).requires_grad_()
        got, active = model.pairwise_loss_by_dot(e, dev(T(q)), dev(T(t)), loss=kind, scale=scale, filt_ptr=ptr, filt_idx=idx,
                                                 candidates=dev(T(cand)), return_active=True)
        loss_check(f"{kind}", got, want["loss"])
        assert float(got.detach()[3]) == 0.0 and int(active[3]) == 0
        if kind == "logistic":                                                             # the listed target's pair carries G_it
            got.sum().backward()
            grad_check(f"{kind} embs", e.grad.cpu().numpy(), S.embs_grad(want, T(q)).numpy())
            assert bool(want["coef"][[0, 1, 2, 4, 5], -1].abs().min() > 0)
        inside = [np.intersect1d(l, cand) for l in lists]                                  # the ids outside the set take no part
        same = model.pairwise_loss_by_dot(dev(embs), dev(T(q)), dev(T(t)), loss=kind, scale=scale, candidates=dev(T(cand)),
                                          **dict(zip(("filt_ptr", "filt_idx"), csr(inside))))
        assert same_bits(got, same)


def test_a_large_bias(model):
    """A finite bias of the size of the scores' whole range on some nodes: the logits stay finite and the checks hold."""
    d, C, B = 64, 300, 9
    i = S.make_problem(d, C, B, False)
    bias = i["bias"].clone()
    bias[::7] = -1e4
    bias[3::11] = 50.0
    scale = S.scale_for(d)
    for kind in S.KINDS:
        nr, inb = S.near(S.loss(kind, i["rows"], i["embs"], i["t"], i["lists"], None, bias, scale=scale, margin=MARGIN), MARGIN)
        grad = i["grad"].clone()
        if kind == "hinge":                                                                # the kink rule
            grad[nr] = 0.0
        want = S.loss(kind, i["rows"], i["embs"], i["t"], i["lists"], None, bias, scale=scale, margin=MARGIN, grad=grad)
        ptr, idx = csr(i["lists"])
        loss, dsum, count, active, dq, dc, db = raw_all(kind, dev(i["rows"]), dev(i["embs"]), dev(i["t"]), dev(grad), scale,
                                                        filt_ptr=ptr, filt_idx=idx, bias=dev(bias))
        loss_check(f"{kind} large bias", loss, want["loss"])
        S.active_check(f"{kind} large bias", active, want, nr, inb)
        assert torch.equal(count.cpu().long(), want["count"])
        grad_check(f"{kind} large bias dq", dq.cpu().numpy(), want["dq"].numpy())
        grad_check(f"{kind} large bias dc", dc.cpu().numpy(), want["dc"].numpy())
        grad_check(f"{kind} large bias db", db.cpu().numpy(), want["db"].numpy())


def test_one_candidate_listed_by_every_query_takes_the_overflow_path():
    """B = 1,100 queries all list candidate 5: more than the 1,024 pairs a candidate tile of the dc pass keeps, so the tile looks
    every id up instead."""
    d, N, B = 20, 300, 1100
    rng = np.random.default_rng(9)
    embs = rows_cpu(N, d, 9)
    rows = rows_cpu(B, d, 10)
    t = torch.from_numpy(rng.integers(6, N, B))
    lists = [np.array([5]) if k % 2 else np.array([5, 6 + k % 200]) for k in range(B)]
    grad = torch.from_numpy((0.5 + rng.random(B)).astype(np.float32))
    ptr, idx = csr(lists)
    scale = S.scale_for(d)
    want = S.loss("logistic", rows, embs, t, lists, None, None, scale=scale, margin=MARGIN, grad=grad)
    loss, dsum, count, active, dq, dc = raw_all("logistic", dev(rows), dev(embs), dev(t), dev(grad), scale, filt_ptr=ptr, filt_idx=idx)
    loss_check("overflow loss", loss, want["loss"])
    assert torch.equal(count.cpu().long(), want["count"])
    grad_check("overflow dq", dq.cpu().numpy(), want["dq"].numpy())
    grad_check("overflow dc", dc.cpu().numpy(), want["dc"].numpy())
    assert not dc[5].any(), "the candidate every query lists receives exactly nothing"


# ---- 7. invalid ids: ordinary calls whose contract is "no fault" ----------------------------------------------------------
def test_an_invalid_id_makes_its_query_alone_nan():
    d, N, B = 20, 700, 70
    big = 1 << 40
    i = S.make_problem(d, N, B, False)
    embs, q, t, grad, bias = (dev(i[k]) for k in ("embs", "q", "t", "grad", "bias"))
    lists = [l[:6] for l in i["lists"]]
    ic_np = np.unique(np.concatenate([np.arange(0, N, 2), i["t"].numpy()]))
    outside = next(v for v in range(1, N, 2) if v not in ic_np)                           # a node that is no candidate
    for kind in S.KINDS:
        for ic in (None, torch.from_numpy(ic_np).to(DEV)):
            ptr, idx = csr(lists)
            good = raw_all(kind, embs, embs, t, grad, 0.2, iq=q, filt_ptr=ptr, filt_idx=idx, ic=ic, bias=bias)
            assert all(bool(torch.isfinite(x).all()) for x in (good[0], good[1], good[4], good[5], good[6])) and bool((good[2] >= 0).all())
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
                bad = raw_all(kind, embs, embs, t2, grad, 0.2, iq=q2, filt_ptr=ptr2, filt_idx=idx2, ic=ic, bias=bias)
                what = f"{kind} {what_bad} {value} {'sub' if ic is not None else 'all'}"
                assert bool(torch.isnan(bad[0][b])) and bool(torch.isnan(bad[1][b])) and int(bad[2][b]) == -1 and int(bad[3][b]) == -1, what
                assert not bad[4][b].any(), what
                keep = torch.arange(B, device=DEV) != b
                for k in range(5):
                    assert same_bits(bad[k][keep], good[k][keep]), (what, k)
                # the same call without the bad query
                qk, tk = q[keep].contiguous(), t[keep].contiguous()
                ptrk, idxk = csr([l for j, l in enumerate(lists) if j != b])
                rest = raw_all(kind, embs, embs, tk, grad[keep].contiguous(), 0.2, iq=qk, filt_ptr=ptrk, filt_idx=idxk, ic=ic, bias=bias)
                assert same_bits(bad[5], rest[5]) and same_bits(bad[6], rest[6]), f"{what}: the bad query adds nothing to dc or db"
    torch.cuda.synchronize()


def test_a_bad_ic_makes_every_query_invalid():
    d, N, B = 20, 300, 5
    big = 1 << 40
    i = S.make_problem(d, N, B, False)
    embs, q, grad, bias = dev(i["embs"]), dev(i["q"]), dev(i["grad"]), dev(i["bias"])
    t = torch.full((B,), 2, device=DEV)
    for kind in S.KINDS:
        for what, ic in (("not ascending", np.array([3, 2, 9])), ("repeated", np.array([2, 2, 9])), ("out of range", np.array([2, 9, N])),
                         ("negative", np.array([-1, 2, 9])), ("far out of range", np.array([2, 9, big]))):
            for b in (None, bias):
                out = raw_all(kind, embs, embs, t, grad, 0.3, iq=q, ic=torch.from_numpy(ic).to(DEV), bias=b)
                loss, dsum, count, active, dq, dc = out[:6]
                assert bool(torch.isnan(loss).all()) and bool(torch.isnan(dsum).all()), f"a bad ic ({what}) makes every query invalid"
                assert bool((count == -1).all()) and bool((active == -1).all()), what
                assert not dq.any() and not dc.any() and (b is None or not out[6].any()), what
    torch.cuda.synchronize()


# ---- 8. through the model ------------------------------------------------------------------------------------------------
def test_bpr_through_the_model_a_decoder_and_an_entity_bias_matches_float64_autograd():
    """BPR (logistic, margin 0) with ONE negative set shared by the batch, on a 2-layer HyperGNN over the toy graph, the query
    rows from a RelationDecoder, an entity-bias parameter: the gradients of every model parameter and of the bias against
    float64 autograd through the oracle's forward and a dense formulation of the loss (the decoder's generated matrices taken
    as data there; its own parameters must receive finite, non-zero gradients)."""
    from oracle import hypergnn_oracle as O
    from test_relation_gpu import restate
    torch.manual_seed(0)
    kg = ToyKnowledgeGraph(feat_dim=16)
    hidden = 16
    model = HyperGNN(text_dim=32, node_feat_dim=16, hidden_dim=hidden, num_layers=2).to(DEV).train()
    dec = RelationDecoder(text_dim=32, hidden_dim=hidden).to(DEV)
    x, ei, texts = kg.node_features.to(DEV), kg.edge_index.to(DEV), kg.edge_texts
    N = x.size(0)
    rel_texts = kg.relation_types
    rng = np.random.default_rng(4)
    B = 7
    head = torch.from_numpy(rng.integers(0, N, B)).to(DEV)
    tail = torch.from_numpy(rng.integers(0, N, B)).to(DEV)
    rel = torch.from_numpy(rng.integers(0, len(rel_texts), B)).to(DEV)
    cand = torch.from_numpy(rng.permutation(N)[:max(2, N // 2)]).to(DEV)
    ent_bias = torch.from_numpy((0.3 * rng.standard_normal(N)).astype(np.float32)).to(DEV).requires_grad_()
    with torch.no_grad():
        rel_embs = model.text_encoder(rel_texts, DEV)
    scale = hidden ** -0.5
    embs = model(x, ei, texts)
    rows = dec(embs, head, rel, rel_embs)
    loss = model.pairwise_loss_by_dot(embs, head, tail, loss="logistic", margin=0.0, scale=scale, query_rows=rows, candidates=cand,
                                      candidate_bias=ent_bias).sum()
    loss.backward()

    params = {k: v.detach().cpu().double().requires_grad_(True) for k, v in model.state_dict().items()}
    b64 = ent_bias.detach().cpu().double().requires_grad_()
    e64 = O.forward(params, kg.node_features.double(), kg.edge_index.numpy(), texts, variant="factorised", dtype=torch.float64)
    with torch.no_grad():
        heads = dec.generator(rel_embs)
    hc, tc, rc = head.cpu(), tail.cpu(), rel.cpu()
    P = torch.from_numpy(S.candidate_set(N, tc, cand.cpu()))
    q64 = restate(e64, hc, rc, heads["W_msg"].cpu(), heads["bias"].cpu())
    z = scale * (q64 @ e64[P].T) + b64[P].unsqueeze(0)
    zt = scale * (q64 * e64[tc]).sum(-1) + b64[tc]
    live = P.unsqueeze(0) != tc.unsqueeze(1)
    u = z - zt.unsqueeze(1)
    want = ((torch.nn.functional.softplus(u) * live).sum(1) / live.sum(1).clamp(min=1)).sum()
    loss_check("BPR through the model", loss.reshape(1), want.detach().reshape(1))
    want.backward()
    grad_check("entity bias", ent_bias.grad.cpu().numpy(), b64.grad.numpy())
    checked, scalars = 0, {}
    for k, p in model.named_parameters():                                            # (one-element parameters: as one vector per
        if params[k].grad is not None and float(params[k].grad.abs().max()) > 0:    # generator, as in test_negatives_gpu.py)
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
    used = [p.grad for n, p in dec.named_parameters() if ".W_msg." in n or ".bias." in n]
    assert used and all(g is not None and bool(torch.isfinite(g).all()) for g in used) and any(bool((g != 0).any()) for g in used)
