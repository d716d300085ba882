"""The fused negative-sampling loss with self-adversarial weighting (HyperGNN.negative_sampling_loss; ghf_score_negsamp_fwd /
_bwd, csrc/negsamp.hip, csrc/softmax.hip) against its float64 restatement (tests/_negsamp_ref.py, itself checked on the host
against a PyKEEN-style autograd formulation).

Tolerances are the project's own, taken from tests/test_softmax_gpu.py: loss and lw under tests/_util.assert_close's
defaults (rtol 1e-4, atol 1e-5, relative L2 1e-5), gradients under its grad_check (rtol 2e-4, atol 1e-4 * max|want|, relative
L2 < 5e-5).  An lw of -inf (a query without negatives) is compared exactly."""

import numpy as np
import pytest
import torch

from _negsamp_ref import negsamp_reference
from test_softmax_gpu import csr, grad_check, layernorm_rows, loss_check, model16, problem
from graph_hypernetwork_forge_amd import HyperGNN, RelationDecoder, ToyKnowledgeGraph, _native

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
DIMS = (20, 64, 128, 256)
ALPHAS, MARGINS = (0.0, 0.5, 1.0), (0.0, 2.0, -1.0)


def weights(B, seed=0):
    return torch.rand(B, device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed)) + 0.5


def dev(a):
    return torch.from_numpy(np.asarray(a)).to(DEV)


def native(q, c, t, g, **kw):
    """(loss, lw, dq, dc, db-or-None) of the two raw calls."""
    loss, lw = _native.score_negsamp_fwd(q, c, t, **kw)
    res = _native.score_negsamp_bwd(q, c, t, lw, g, **kw)
    return (loss, lw) + tuple(res) + ((None,) if len(res) == 2 else ())


def check(what, got, want, grads=True):
    """loss, lw (and dq, dc, db) against the float64 restatement: the same NaNs, the same -inf in lw, the rest in tolerance."""
    loss, lw, dq, dc, db = got
    wl, ww, wq, wc, wb = want
    ok = ~torch.isnan(wl)
    assert torch.equal(torch.isnan(loss), ~ok) and torch.equal(torch.isnan(lw), ~ok), f"{what}: NaNs differ"
    if ok.any():
        loss_check(f"{what}: loss", loss[ok], wl[ok])
    fin = ok & torch.isfinite(ww)
    assert torch.equal(lw[ok & ~fin], ww[ok & ~fin].float()), f"{what}: lw of the queries without negatives"
    if fin.any():
        loss_check(f"{what}: lw", lw[fin], ww[fin])
    if grads:
        grad_check(f"q ({what})", dq.cpu().numpy(), wq.cpu().numpy())
        grad_check(f"c ({what})", dc.cpu().numpy(), wc.cpu().numpy())
        if db is not None:
            grad_check(f"b ({what})", db.cpu().numpy(), wb.cpu().numpy())


def same_bits(a, b, what):
    for x, y, name in zip(a, b, ("loss", "lw", "dq", "dc", "db")):
        if x is None or y is None:
            continue
        assert torch.equal(torch.isnan(x), torch.isnan(y)) and torch.equal(torch.nan_to_num(x), torch.nan_to_num(y)), f"{what}: {name}"


# ---- 1. parity ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", DIMS)
def test_forward_and_backward_match_float64(d):
    N, B = 5003, 150                                  # neither a multiple of a tile; problem(): repeated queries, a listed target
    model = model16()
    embs = layernorm_rows(N, d, seed=d)
    query, target, lists, known = problem(N, B, seed=300 + d)
    target[B // 2:B // 2 + 5] = target[:5]            # the repeated queries share their targets: the same negatives
    q, t = dev(query), dev(target)
    ptr, idx = csr(lists)
    g = weights(B, d)
    for scale in (1.0, d ** -0.5):
        for alpha in ALPHAS:
            for margin in MARGINS:
                kw = dict(scale=scale, margin=margin, adversarial_temperature=alpha)
                tag = f"d={d} scale={scale:.3g} alpha={alpha} margin={margin}"
                got = native(embs, embs, t, g, iq=q, **kw)
                check(f"{tag} no lists", got, negsamp_reference(embs[q], embs, t, None, scale, margin, alpha, grad=g))
                assert torch.equal(got[1][B // 2:B // 2 + 5], got[1][:5])        # a repeated (query, target): the same sum, bit for bit
                assert torch.equal(model.negative_sampling_loss(embs, q, t, **kw), got[0])
                got = native(embs, embs, t, g, iq=q, filt_ptr=ptr, filt_idx=idx, **kw)
                check(f"{tag} lists", got, negsamp_reference(embs[q], embs, t, lists, scale, margin, alpha, grad=g))
                by_csr = model.negative_sampling_loss(embs, q, t, filt_ptr=ptr, filt_idx=idx, **kw)
                assert torch.equal(by_csr, got[0]) and not by_csr.requires_grad
        by_known = model.negative_sampling_loss(embs, q, t, known=known, **kw)
        wrapped = model.negative_sampling_loss(embs, q - N, t - N, known=known, **kw)      # negative ids wrap
        assert torch.equal(by_known, got[0]) and torch.equal(wrapped, got[0])


def test_gradient_through_the_model_method_matches_the_raw_calls():
    N, B, d = 2003, 130, 64
    model = model16()
    embs = layernorm_rows(N, d, seed=4)
    query, target, lists, known = problem(N, B, seed=41)
    q, t = dev(query), dev(target)
    ptr, idx = csr(lists)
    g = weights(B, 1)
    kw = dict(scale=d ** -0.5, margin=1.0, adversarial_temperature=0.5)
    loss, lw, dq, dc, _ = native(embs, embs, t, g, iq=q, filt_ptr=ptr, filt_idx=idx, **kw)
    e = embs.clone().requires_grad_(True)
    out = model.negative_sampling_loss(e, q, t, known=known, **kw)
    assert out.requires_grad and torch.equal(out, loss)
    (out * g).sum().backward()
    want = dc.double().index_add(0, q, dq.double())                     # d embs = dc + dq scattered to the query rows
    grad_check("embs through the method", e.grad.cpu().numpy(), want.cpu().numpy())
    _, _, wq, wc, _ = negsamp_reference(embs[q], embs, t, lists, grad=g, **{"scale": kw["scale"], "margin": 1.0, "alpha": 0.5})
    grad_check("embs against float64", e.grad.cpu().numpy(), wc.index_add(0, q, wq).cpu().numpy())


# ---- 2. tile edges -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", (20, 128, 256))
def test_tile_edges(d):
    for N in (1, 127, 128, 129, 255, 256, 257):
        embs = layernorm_rows(N, d, seed=N + d)
        for B in (1, 65, 129):
            rng = np.random.default_rng(N * 1000 + B)
            query, target = rng.integers(0, N, B), rng.integers(0, N, B)
            target[0] = N - 1                                             # the target is the last candidate
            lists = [np.unique(rng.integers(0, N, 3)) if i % 3 else np.zeros(0, dtype=np.int64) for i in range(B)]
            q, t, g = dev(query), dev(target), weights(B, B)
            ptr, idx = csr(lists)
            got = native(embs, embs, t, g, iq=q, filt_ptr=ptr, filt_idx=idx, scale=d ** -0.5, margin=1.0, adversarial_temperature=0.5)
            want = negsamp_reference(embs[q], embs, t, lists, d ** -0.5, 1.0, 0.5, grad=g)
            check(f"N={N} B={B} d={d}", got, want)
            if N == 1:                                                    # no negatives: the positive term, lw = -inf
                assert bool(torch.isinf(got[1]).all()) and bool((got[1] < 0).all())
                assert torch.isfinite(got[0]).all() and torch.isfinite(got[2]).all() and torch.isfinite(got[3]).all()


# ---- 3. the online rescale ---------------------------------------------------------------------------------------------
def test_the_running_max_rescales_across_tiles_and_slabs():
    """alpha z spans +-30 along the candidates: ascending with the id for query 0, descending for query 1, flat but for one
    planted top scorer in the last tile of the last slab for query 2; query 3 is query 2 with that scorer listed, where it must
    not matter.  N = 33,000 at d = 64: 129 candidate tiles in 65 slabs forward, 8 dq slabs backward."""
    N, d = 33_000, 64
    c = 0.05 * layernorm_rows(N, d, seed=3)
    c[:, 0] = torch.linspace(-30, 30, N, device=DEV)
    c[:, 1] = 0
    top = N - 5
    c[top, 1] = 30.0
    rows = torch.zeros(40, d, device=DEV)
    rows[0, 0], rows[1, 0], rows[2, 1], rows[3, 1] = 1.0, -1.0, 1.0, 1.0
    rows[2:4, 2:] = 1.0
    rows[4:] = layernorm_rows(36, d, seed=8)
    rows[4:, :2] = 0
    B = rows.size(0)
    rng = np.random.default_rng(0)
    target = rng.integers(0, N, B)
    lists = [np.unique(rng.integers(0, N, 10)) for _ in range(B)]
    lists[3] = np.unique(np.append(lists[3], top))
    t, g = dev(target), weights(B, 3)
    ptr, idx = csr(lists)
    for alpha, margin in ((1.0, 0.0), (1.0, 2.0), (0.5, -1.0), (0.0, 0.0)):
        got = native(rows, c, t, g, filt_ptr=ptr, filt_idx=idx, scale=1.0, margin=margin, adversarial_temperature=alpha)
        check(f"rescale alpha={alpha} margin={margin}", got, negsamp_reference(rows, c, t, lists, 1.0, margin, alpha, grad=g))
    no_top = negsamp_reference(rows[3:4], torch.cat([c[:top], c[top + 1:]]), t[3:4] - (1 if target[3] > top else 0),
                               [np.where(lists[3] > top, lists[3] - 1, lists[3])[lists[3] != top]], 1.0, 0.0, 1.0)
    loss, lw = _native.score_negsamp_fwd(rows, c, t, filt_ptr=ptr, filt_idx=idx, adversarial_temperature=1.0)
    loss_check("the listed top scorer does not matter", loss[3:4], no_top[0])
    loss_check("the listed top scorer does not matter: lw", lw[3:4], no_top[1])
    assert float(lw[2]) > float(lw[3]) + 5                                # unlisted it dominates


# ---- 4. subsets --------------------------------------------------------------------------------------------------------
def subset_problem(N, C, B, seed):
    rng = np.random.default_rng(seed)
    ic = np.sort(rng.choice(N, C, replace=False))
    query = rng.integers(0, N, B)
    target = ic[rng.integers(0, C, B)]                                    # every target a candidate
    lists = [np.unique(np.concatenate([rng.integers(0, N, 6), ic[rng.integers(0, C, 3)]])) if i % 4 else np.zeros(0, dtype=np.int64)
             for i in range(B)]
    return ic, query, target, lists


@pytest.mark.parametrize("N,C,B,d", [(700, 257, 129, 20), (700, 255, 300, 64), (700, 1, 129, 64), (700, 257, 129, 128),
                                     (700, 256, 129, 256), (33_000, 4500, 70, 64)])
def test_a_subset_has_the_bits_of_the_call_on_a_contiguous_copy(N, C, B, d):
    embs = layernorm_rows(N, d, seed=N + C + d)
    ic, query, target, lists = subset_problem(N, C, B, seed=C + d)
    q, t, cand, g = dev(query), dev(target), dev(ic), weights(B, C)
    ptr, idx = csr(lists)
    kw = dict(scale=d ** -0.5, margin=1.0, adversarial_temperature=1.0)
    got = native(embs, embs, t, g, iq=q, filt_ptr=ptr, filt_idx=idx, ic=cand, **kw)
    check(f"subset N={N} C={C} B={B} d={d}", got, negsamp_reference(embs[q], embs, t, lists, d ** -0.5, 1.0, 1.0, grad=g, ic=cand))
    pos = {int(v): j for j, v in enumerate(ic)}
    rlists = [np.array(sorted(pos[int(v)] for v in l if int(v) in pos), dtype=np.int64) for l in lists]
    rptr, ridx = csr(rlists)
    rt = dev(np.array([pos[int(v)] for v in target]))
    copy = native(embs, embs[cand].contiguous(), rt, g, iq=q, filt_ptr=rptr, filt_idx=ridx, **kw)
    same_bits(got, copy, "subset against the contiguous copy")
    assert got[3].shape == (C, d)


def test_subset_rules_through_the_method_and_at_the_c_abi():
    N, C, B, d = 700, 257, 129, 64
    model = model16()
    embs = layernorm_rows(N, d, seed=77)
    ic, query, target, lists = subset_problem(N, C, B, seed=5)
    q, t, cand, g = dev(query), dev(target), dev(ic), weights(B, 9)
    ptr, idx = csr(lists)
    kw = dict(scale=d ** -0.5, margin=0.5, adversarial_temperature=0.5)
    # candidates=arange(N) is the call without the keyword
    e1, e2 = embs.clone().requires_grad_(True), embs.clone().requires_grad_(True)
    l1 = model.negative_sampling_loss(e1, q, t, filt_ptr=ptr, filt_idx=idx, **kw)
    l2 = model.negative_sampling_loss(e2, q, t, filt_ptr=ptr, filt_idx=idx, candidates=torch.arange(N), **kw)
    (l1 * g).sum().backward()
    (l2 * g).sum().backward()
    assert torch.equal(l1, l2) and torch.equal(e1.grad, e2.grad)
    # the method adds the batch's targets; rows that are neither candidates, targets nor queries get exactly zero
    far = dev(np.setdiff1d(np.arange(N), ic)[:B])                        # targets outside the given candidates
    e3 = embs.clone().requires_grad_(True)
    l3 = model.negative_sampling_loss(e3, q, far, filt_ptr=ptr, filt_idx=idx, candidates=cand[torch.randperm(C, device=DEV)], **kw)
    assert torch.isfinite(l3).all()
    full = torch.unique(torch.cat([cand, far]))
    raw = native(embs, embs, far, g, iq=q, filt_ptr=ptr, filt_idx=idx, ic=full, **kw)
    assert torch.equal(l3, raw[0])
    (l3 * g).sum().backward()
    touched = torch.zeros(N, dtype=torch.bool, device=DEV)
    touched[full] = True
    touched[q] = True
    assert not e3.grad[~touched].any() and bool(e3.grad[touched].any())
    # at the C ABI a target outside P: NaN, and the query takes no part
    base = native(embs, embs, t, g, iq=q, filt_ptr=ptr, filt_idx=idx, ic=cand, **kw)
    t_bad = t.clone()
    t_bad[7] = far[0]
    got = native(embs, embs, t_bad, g, iq=q, filt_ptr=ptr, filt_idx=idx, ic=cand, **kw)
    keep = torch.arange(B, device=DEV) != 7
    assert torch.isnan(got[0][7]) and torch.isnan(got[1][7]) and not got[2][7].any()
    assert torch.equal(got[0][keep], base[0][keep]) and torch.equal(got[2][keep], base[2][keep])
    check("a target outside P", got, negsamp_reference(embs[q], embs, t_bad, lists, kw["scale"], 0.5, 0.5, grad=g, ic=cand))
    # a bad ic (not ascending; an id outside the table): every query NaN, zero gradients, nothing faults
    for bad in (torch.flip(cand, (0,)), torch.cat([cand[:-1], dev(np.array([N + 5]))])):
        loss, lw, dq, dc, _ = native(embs, embs, t, g, iq=q, filt_ptr=ptr, filt_idx=idx, ic=bad, **kw)
        assert torch.isnan(loss).all() and torch.isnan(lw).all() and not dq.any() and not dc.any()


# ---- 5. bias -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", (20, 128, 256))
def test_candidate_bias(d):
    N, C, B = 700, 257, 129
    model = model16()
    embs = layernorm_rows(N, d, seed=50 + d)
    ic, query, target, lists = subset_problem(N, C, B, seed=d)
    q, t, cand, g = dev(query), dev(target), dev(ic), weights(B, d)
    ptr, idx = csr(lists)
    kw = dict(iq=q, filt_ptr=ptr, filt_idx=idx, scale=d ** -0.5, margin=1.0, adversarial_temperature=0.5)
    bias = torch.randn(N, device=DEV, generator=torch.Generator(device=DEV).manual_seed(d))
    for sub in (None, cand):
        plain = native(embs, embs, t, g, ic=sub, **kw)
        zeros = native(embs, embs, t, g, ic=sub, bias=torch.zeros(N, device=DEV), **kw)
        same_bits(plain, zeros, "a bias of zeros")
        assert zeros[4] is not None and zeros[4].shape == ((N,) if sub is None else (C,))
        got = native(embs, embs, t, g, ic=sub, bias=bias, **kw)
        check(f"bias d={d} subset={sub is not None}", got,
              negsamp_reference(embs[q], embs, t, lists, d ** -0.5, 1.0, 0.5, grad=g, ic=sub, bias=bias))
    # the bias alone requires grad: the loss is recorded, and the [N] gradient is zero outside the candidates
    b = bias.clone().requires_grad_(True)
    loss = model.negative_sampling_loss(embs, q, t, filt_ptr=ptr, filt_idx=idx, scale=d ** -0.5, margin=1.0, adversarial_temperature=0.5,
                                        candidates=cand, candidate_bias=b)
    assert loss.requires_grad and torch.equal(loss, got[0])
    (loss * g).sum().backward()
    assert torch.equal(b.grad[cand], got[4])
    outside = torch.ones(N, dtype=torch.bool, device=DEV)
    outside[cand] = False
    assert not b.grad[outside].any()


# ---- 6. properties -----------------------------------------------------------------------------------------------------
def test_results_are_bit_reproducible_and_independent_of_the_batch():
    N, B, d = 50_000, 300, 128                        # several candidate slabs
    embs = layernorm_rows(N, d, seed=11)
    query, target, lists, _ = problem(N, B, seed=12)
    q, t, g = dev(query), dev(target), weights(B, 2)
    ptr, idx = csr(lists)
    kw = dict(scale=d ** -0.5, margin=1.0, adversarial_temperature=1.0)
    first = native(embs, embs, t, g, iq=q, filt_ptr=ptr, filt_idx=idx, **kw)
    for _ in range(2):
        same_bits(first, native(embs, embs, t, g, iq=q, filt_ptr=ptr, filt_idx=idx, **kw), "a repeated call")
    sl = slice(37, 171)                                                  # the same queries in another batch: the same bits
    sptr, sidx = csr(lists[sl])
    loss, lw = _native.score_negsamp_fwd(embs, embs, t[sl], iq=q[sl], filt_ptr=sptr, filt_idx=sidx, **kw)
    assert torch.equal(loss, first[0][sl]) and torch.equal(lw, first[1][sl])


def test_out_of_range_ids_give_nan_for_their_query_only():
    N, B, d = 2500, 140, 64
    embs = layernorm_rows(N, d, seed=21)
    query, target, lists, _ = problem(N, B, seed=22)
    g = weights(B, 4)
    kw = dict(scale=d ** -0.5, margin=1.0, adversarial_temperature=0.5)
    ptr, idx = csr(lists)
    base = native(embs, embs, dev(target), g, iq=dev(query), filt_ptr=ptr, filt_idx=idx, **kw)
    bq, bt, bl = query.copy(), target.copy(), [l.copy() for l in lists]
    bq[3], bq[4], bt[5], bt[6] = N, -1, N + 7, -2
    bl[8] = np.append(bl[8], N + 1)
    bl[9] = np.append(-3, bl[9])
    bad = [3, 4, 5, 6, 8, 9]
    bptr, bidx = csr(bl)
    got = native(embs, embs, dev(bt), g, iq=dev(bq), filt_ptr=bptr, filt_idx=bidx, **kw)
    keep = torch.ones(B, dtype=torch.bool, device=DEV)
    keep[bad] = False
    assert torch.isnan(got[0][~keep]).all() and torch.isnan(got[1][~keep]).all() and not got[2][~keep].any()
    assert torch.equal(got[0][keep], base[0][keep]) and torch.equal(got[1][keep], base[1][keep])
    assert torch.equal(got[2][keep], base[2][keep]) and torch.isfinite(got[3]).all()
    g0 = g.clone()
    g0[bad] = 0                                                          # the rest of dc: the base call without those queries
    want = native(embs, embs, dev(target), g0, iq=dev(query), filt_ptr=ptr, filt_idx=idx, **kw)
    assert torch.equal(got[3], want[3])


def test_query_rows_of_zeros_and_an_empty_batch():
    N, d = 300, 64
    embs = layernorm_rows(N, d, seed=31)
    rows = torch.zeros(3, d, device=DEV)
    t = dev(np.array([0, 5, N - 1]))
    lists = [np.array([1, 2]), np.zeros(0, dtype=np.int64), np.array([7, N - 1])]
    ptr, idx = csr(lists)
    g = weights(3)
    got = native(rows, embs, t, g, filt_ptr=ptr, filt_idx=idx, margin=0.5, adversarial_temperature=1.0)
    check("zero rows", got, negsamp_reference(rows, embs, t, lists, 1.0, 0.5, 1.0, grad=g))
    counts = torch.tensor([N - 3, N - 1, N - 2], device=DEV, dtype=torch.float32)   # z = 0 everywhere: lw = log |J|
    loss_check("zero rows: lw = log |J|", got[1], torch.log(counts.double()))
    model = model16()
    with pytest.raises(ValueError):
        model.negative_sampling_loss(embs, t[:0], t[:0])


def test_typed_queries_through_a_relation_decoder_and_a_node_batch():
    kg = ToyKnowledgeGraph(feat_dim=16)
    x, ei = kg.node_features.to(DEV), kg.edge_index.to(DEV)
    rel_texts = kg.relation_types
    edge_rel = torch.tensor([rel_texts.index(t) for t in kg.edge_texts], device=DEV)
    hidden = 16
    torch.manual_seed(0)
    model = HyperGNN(text_dim=32, node_feat_dim=16, hidden_dim=hidden).to(DEV)
    dec = RelationDecoder(text_dim=32, hidden_dim=hidden).to(DEV)
    embs = model(x, ei, kg.edge_texts)
    N = embs.size(0)
    head, rel, tail = ei[0], edge_rel, ei[1]
    Q = dec(embs, head, rel, model.text_encoder(rel_texts, embs.device))
    kw = dict(scale=hidden ** -0.5, margin=1.0, adversarial_temperature=1.0)
    loss = model.negative_sampling_loss(embs, head, tail, query_rows=Q, known=(ei[0], ei[1], edge_rel), query_rel=rel, **kw)
    assert loss.shape == (head.numel(),) and loss.requires_grad
    lists = [sorted({int(t) for s, r, t in zip(ei[0].tolist(), edge_rel.tolist(), ei[1].tolist()) if s == h and r == u})
             for h, u in zip(head.tolist(), rel.tolist())]
    want = negsamp_reference(Q.detach(), embs.detach(), tail, lists, hidden ** -0.5, 1.0, 1.0)
    loss_check("toy graph, typed queries", loss, want[0])
    loss.mean().backward()

    def usable(gr):
        return gr is not None and bool(torch.isfinite(gr).all()) and bool((gr != 0).any())

    assert usable(dec.generator.generators["W_msg"][-1].weight.grad) and usable(dec.generator.generators["bias"][-1].weight.grad)
    for n, p in model.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), f"{n} has no finite gradient"
    # rows of a forward_nodes batch: ids are positions in the batch
    model.zero_grad()
    nodes = torch.unique(torch.cat([head[:6], tail[:6]]))
    sub = model.forward_nodes(x, ei, kg.edge_texts, nodes)
    where = {int(v): j for j, v in enumerate(nodes.tolist())}
    bq = dev(np.array([where[int(v)] for v in head[:6]]))
    bt = dev(np.array([where[int(v)] for v in tail[:6]]))
    bl = model.negative_sampling_loss(sub, bq, bt, **kw)
    want = negsamp_reference(sub.detach()[bq], sub.detach(), bt, None, hidden ** -0.5, 1.0, 1.0)
    loss_check("a forward_nodes batch", bl, want[0])
    bl.mean().backward()
    assert any(usable(p.grad) for p in model.parameters())


def test_training_on_the_negative_sampling_loss_end_to_end():
    kg = ToyKnowledgeGraph(feat_dim=16)
    x, ei = kg.node_features.to(DEV), kg.edge_index.to(DEV)
    hidden = 32
    torch.manual_seed(0)
    model = HyperGNN(text_dim=64, node_feat_dim=16, hidden_dim=hidden, num_layers=2).to(DEV)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    losses = []
    for step in range(21):
        opt.zero_grad()
        loss = model.negative_sampling_loss(model(x, ei, kg.edge_texts), ei[0], ei[1], known=(ei[0], ei[1]), scale=hidden ** -0.5,
                                            margin=1.0, adversarial_temperature=1.0).mean()
        losses.append(loss.item())
        if step == 20:
            break
        loss.backward()
        opt.step()
    print("negative-sampling loss over 20 Adam steps:", " ".join(f"{v:.4f}" for v in losses))
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]
