"""The 1-vs-all softmax link-prediction loss against every node (HyperGNN.softmax_loss, ghf_score_softmax_fwd / _bwd,
csrc/softmax.hip) against a float64 restatement of its contract on the float32 rows: the dense [B, N] logits,
masked_fill(-inf) over each query's filter list (the target always kept), logsumexp, autograd.

Tolerances are the project's own: the loss under tests/_util.assert_close's defaults (rtol 1e-4, atol 1e-5, relative L2
1e-5), gradients under the rule of test_hip_parity._grad_check (rtol 2e-4, atol 1e-4 * max|want|, relative L2 < 5e-5),
restated below."""

import numpy as np
import pytest
import torch

from _util import assert_close
from graph_hypernetwork_forge_amd import HyperGNN, ToyKnowledgeGraph, _native

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
DIMS = (20, 64, 128, 256)


def grad_check(name, got, want, rtol=2e-4, l2=5e-5):
    gw, gg = want.astype(np.float64), got.astype(np.float64)
    assert gg.shape == gw.shape, f"d{name}: shape {gg.shape} vs {gw.shape}"
    assert np.isfinite(gg).all(), f"d{name}: non-finite values"
    scale = float(np.abs(gw).max())
    rel_l2 = np.linalg.norm(gg - gw) / max(np.linalg.norm(gw), 1e-30)
    print(f"d{name}: max abs err {np.abs(gg - gw).max():.3e} at scale {scale:.3e}, relative L2 {rel_l2:.3e}")
    assert np.allclose(gg, gw, rtol=rtol, atol=1e-4 * max(scale, 1e-30)), \
        f"d{name}: max abs err {np.abs(gg - gw).max():.3e} at scale {scale:.3e}"
    assert rel_l2 < l2, f"d{name}: relative L2 {rel_l2:.3e}"


def loss_check(what, got, want):
    got, want = got.detach().cpu().numpy(), want.detach().cpu().numpy()
    err = np.abs(got.astype(np.float64) - want)
    print(f"{what}: max abs err {err.max():.3e}, worst err / bound {np.max(err / (1e-5 + 1e-4 * np.abs(want))):.3e}, "
          f"relative L2 {np.linalg.norm(got - want) / max(np.linalg.norm(want), 1e-30):.3e}")
    assert_close(got, want, what)


# ---- the restatement ---------------------------------------------------------------------------------------------------
def csr(lists):
    ptr = np.zeros(len(lists) + 1, dtype=np.int64)
    ptr[1:] = np.cumsum([len(l) for l in lists])
    idx = np.concatenate([np.asarray(l, dtype=np.int64) for l in lists]) if ptr[-1] else np.zeros(0, dtype=np.int64)
    return torch.from_numpy(ptr).to(DEV), torch.from_numpy(idx).to(DEV)


def reference(qrows, c, target, lists, scale, grad=None):
    """float64 (loss, lse[, dq, dc]) for gathered query rows qrows [B, d] and candidates c [N, d] (float32 tensors)."""
    B, N = qrows.size(0), c.size(0)
    q64 = qrows.double().detach().requires_grad_(grad is not None)
    c64 = c.double().detach().requires_grad_(grad is not None)
    S = scale * (q64 @ c64.T)
    mask = torch.zeros(B, N, dtype=torch.bool, device=c.device)
    if lists is not None:
        for i, l in enumerate(lists):
            if len(l):
                mask[i, torch.as_tensor(np.asarray(l, dtype=np.int64), device=c.device)] = True
    ar = torch.arange(B, device=c.device)
    mask[ar, target] = False                                             # the target always stays
    lse = S.masked_fill(mask, -np.inf).logsumexp(1)
    loss = lse - S[ar, target]
    if grad is None:
        return loss, lse
    (loss * grad.double()).sum().backward()
    return loss.detach(), lse.detach(), q64.grad, c64.grad


def layernorm_rows(N, d, seed):
    """LayerNorm-shaped rows (what the model's last layer emits), built on the device."""
    gen = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(N, d, device=DEV, generator=gen)
    gamma = 1.0 + 0.1 * torch.randn(d, device=DEV, generator=gen)
    beta = 0.1 * torch.randn(d, device=DEV, generator=gen)
    return torch.nn.functional.layer_norm(x, (d,), gamma, beta)


def exact_rows(N, d, seed):
    g = np.random.default_rng(seed).standard_normal((N, d))
    c = np.clip(np.round(64 * g) / 64, -4, 4).astype(np.float32)
    c[-500:] = c[:500]                       # copies: ties with the target
    return c


def model16():
    return HyperGNN(text_dim=32, node_feat_dim=16, hidden_dim=16).to(DEV)


def problem(N, B, seed, per_list=10):
    """Queries with repeats, targets that several queries share, and per-NODE known partners (so that known= and CSR lists
    agree): some lists hold the target, one id twice, or nothing."""
    rng = np.random.default_rng(seed)
    query = rng.integers(0, N, B)
    query[B // 2:B // 2 + 5] = query[:5]                                  # repeated queries
    target = rng.integers(0, N, B)
    target[10:20] = target[0]                                             # queries sharing a target
    node_lists = {}
    for i, v in enumerate(query):
        if v not in node_lists:
            l = np.unique(rng.integers(0, N, per_list)) if i % 7 else np.zeros(0, dtype=np.int64)
            if i % 3 == 0 and len(l):
                l = np.unique(np.append(l, target[i]))                    # the target is listed: it stays in the sum
            node_lists[v] = l
    lists = [node_lists[v] for v in query]
    src = np.concatenate([np.full(len(l), v) for v, l in node_lists.items()] + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
    dst = np.concatenate(list(node_lists.values()) + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
    return query, target, lists, (torch.from_numpy(src).to(DEV), torch.from_numpy(dst).to(DEV))


# ---- 1. loss and lse ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", DIMS)
def test_loss_and_lse_match_float64(d):
    N, B = 5003, 150                                  # neither a multiple of a tile
    model = model16()
    embs = layernorm_rows(N, d, seed=d)
    query, target, lists, known = problem(N, B, seed=100 + d)
    q, t = torch.from_numpy(query).to(DEV), torch.from_numpy(target).to(DEV)
    ptr, idx = csr(lists)
    rep_lists = [np.sort(np.append(l, l[:1])) for l in lists]            # a repeated id changes nothing
    rptr, ridx = csr(rep_lists)
    for scale in (1.0, d ** -0.5):
        want, want_lse = reference(embs[q], embs, t, None, scale)
        loss, lse = _native.score_softmax_fwd(embs, embs, t, iq=q, scale=scale)
        loss_check(f"d={d} scale={scale:.3g} no lists: loss", loss, want)
        loss_check(f"d={d} scale={scale:.3g} no lists: lse", lse, want_lse)
        assert torch.equal(model.softmax_loss(embs, q, t, scale=scale), loss)
        assert torch.equal(lse[B // 2:B // 2 + 5], lse[:5])                  # a repeated query: the same sum, bit for bit
        want, want_lse = reference(embs[q], embs, t, lists, scale)
        loss, lse = _native.score_softmax_fwd(embs, embs, t, iq=q, filt_ptr=ptr, filt_idx=idx, scale=scale)
        loss_check(f"d={d} scale={scale:.3g} lists: loss", loss, want)
        loss_check(f"d={d} scale={scale:.3g} lists: lse", lse, want_lse)
        by_csr = model.softmax_loss(embs, q, t, scale=scale, filt_ptr=ptr, filt_idx=idx)
        by_known = model.softmax_loss(embs, q, t, scale=scale, known=known)
        assert torch.equal(by_csr, loss) and torch.equal(by_known, loss)
        assert torch.equal(model.softmax_loss(embs, q, t, scale=scale, filt_ptr=rptr, filt_idx=ridx), loss)
        wrapped = model.softmax_loss(embs, q - N, t - N, scale=scale, known=known)                  # negative ids wrap
        assert torch.equal(wrapped, loss)
        assert not loss.requires_grad


def test_duplicate_queries_and_a_single_candidate():
    d = 64
    embs = layernorm_rows(700, d, seed=3)
    q = torch.tensor([5, 5, 9, 5], device=DEV)
    t = torch.tensor([8, 8, 8, 1], device=DEV)
    loss, lse = _native.score_softmax_fwd(embs, embs, t, iq=q, scale=0.125)
    assert torch.equal(loss[0], loss[1]) and torch.equal(lse[0], lse[1]) and torch.equal(lse[0], lse[3])
    want, _ = reference(embs[q], embs, t, None, 0.125)
    loss_check("duplicates", loss, want)
    # N = 1: the only candidate is the target, listed or not: lse = scale t, loss = 0
    one = layernorm_rows(1, d, seed=4)
    z = torch.zeros(3, dtype=torch.int64, device=DEV)
    for lists in (None, [[0], [], [0, 0]]):
        ptr, idx = csr(lists) if lists else (None, None)
        loss, lse = _native.score_softmax_fwd(one, one, z, iq=z, filt_ptr=ptr, filt_idx=idx, scale=0.5)
        s = 0.5 * float((one.double() ** 2).sum())
        assert_close(lse.cpu().numpy(), np.full(3, s), "N = 1: lse")
        assert_close(loss.cpu().numpy(), np.zeros(3), "N = 1: loss")
        g = torch.ones(3, device=DEV)
        dq, dc = _native.score_softmax_bwd(one, one, z, lse, g, iq=z, filt_ptr=ptr, filt_idx=idx, scale=0.5)
        assert float(dq.abs().max()) <= 1e-5 and float(dc.abs().max()) <= 1e-5        # p = 1: G = 0 up to the rounding of lse


# ---- 2. listed candidates dominate --------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", (64, 128))
def test_listed_candidates_that_dominate_never_enter_the_sum(d):
    """Every query's ~10 listed rows are 2 x its own row: they score 2 |q|^2, everything unlisted at most |q|^2.  Subtracting
    their terms from a total afterwards fails here (infinite loss at scale 1); masking them before the sum does not."""
    N, B, L = 5003, 130, 10
    model = model16()
    embs = layernorm_rows(N, d, seed=50 + d)
    query = np.arange(B)
    lists = [B + L * i + np.arange(L) for i in range(B)]
    rng = np.random.default_rng(d)
    target = rng.integers(B + L * B, N, B)
    target[:8] = target[0]
    for i in range(B):
        embs[torch.from_numpy(lists[i]).to(DEV)] = 2.0 * embs[i]
    q, t = torch.from_numpy(query).to(DEV), torch.from_numpy(target).to(DEV)
    ptr, idx = csr(lists)
    w = torch.rand(B, device=DEV, generator=torch.Generator(device=DEV).manual_seed(d)) + 0.5
    for scale in (1.0, d ** -0.5):
        want, _, dq64, dc64 = reference(embs[q], embs, t, lists, scale, grad=w)
        e = embs.clone().requires_grad_(True)
        loss = model.softmax_loss(e, q, t, scale=scale, filt_ptr=ptr, filt_idx=idx)
        loss_check(f"dominating lists d={d} scale={scale:.3g}: loss", loss, want)
        (loss * w).sum().backward()
        want_g = dc64.clone()
        want_g.index_add_(0, q, dq64)
        grad_check(f"embs (dominating lists, d={d}, scale={scale:.3g})", e.grad.cpu().numpy(), want_g.cpu().numpy())


# ---- 3. gradients -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", DIMS)
def test_raw_backward_dq_and_dc_match_float64(d):
    N, M, B = 3001, 517, 200
    c = layernorm_rows(N, d, seed=7 + d)
    qm = layernorm_rows(M, d, seed=8 + d)                                 # q != c
    rng = np.random.default_rng(d)
    iq = rng.integers(0, M, B)
    iq[50:60] = iq[0]
    target = rng.integers(0, N, B)
    target[:12] = target[100]
    lists = [np.unique(rng.integers(0, N, 12)) if i % 5 else np.zeros(0, dtype=np.int64) for i in range(B)]
    lists[3] = np.unique(np.append(lists[3], target[3]))
    ptr, idx = csr(lists)
    q_i, t = torch.from_numpy(iq).to(DEV), torch.from_numpy(target).to(DEV)
    g = torch.randn(B, device=DEV, generator=torch.Generator(device=DEV).manual_seed(d))
    for scale, with_lists in ((1.0, True), (d ** -0.5, True), (0.25, False)):
        fp, fi, ls = (ptr, idx, lists) if with_lists else (None, None, None)
        want, want_lse, dq64, dc64 = reference(qm[q_i], c, t, ls, scale, grad=g)
        loss, lse = _native.score_softmax_fwd(qm, c, t, iq=q_i, filt_ptr=fp, filt_idx=fi, scale=scale)
        loss_check(f"q != c, d={d}, scale={scale:.3g}: loss", loss, want)
        dq, dc = _native.score_softmax_bwd(qm, c, t, lse, g, iq=q_i, filt_ptr=fp, filt_idx=fi, scale=scale)
        grad_check(f"q (d={d}, scale={scale:.3g}, lists={with_lists})", dq.cpu().numpy(), dq64.cpu().numpy())
        grad_check(f"c (d={d}, scale={scale:.3g}, lists={with_lists})", dc.cpu().numpy(), dc64.cpu().numpy())


@pytest.mark.parametrize("d", (64, 256))
def test_backward_with_hub_candidates_that_every_query_lists(d):
    """Six neighbouring candidates on every query's list: more listed pairs fall into one candidate tile than the dc sweep
    keeps beside its tile, so it looks every id up instead; the result is the same contract."""
    N, B = 1500, 300
    c = layernorm_rows(N, d, seed=70 + d)
    rng = np.random.default_rng(d)
    iq, target = rng.integers(0, N, B), rng.integers(0, N, B)
    hubs = np.arange(700, 706)
    target[:20] = 702                                                     # a hub that is some queries' target stays in their sums
    lists = [np.unique(np.append(hubs, rng.integers(0, N, 4))) for _ in range(B)]
    ptr, idx = csr(lists)
    q_i, t = torch.from_numpy(iq).to(DEV), torch.from_numpy(target).to(DEV)
    g = torch.randn(B, device=DEV, generator=torch.Generator(device=DEV).manual_seed(d))
    scale = d ** -0.5
    want, _, dq64, dc64 = reference(c[q_i], c, t, lists, scale, grad=g)
    loss, lse = _native.score_softmax_fwd(c, c, t, iq=q_i, filt_ptr=ptr, filt_idx=idx, scale=scale)
    loss_check(f"hub lists d={d}: loss", loss, want)
    dq, dc = _native.score_softmax_bwd(c, c, t, lse, g, iq=q_i, filt_ptr=ptr, filt_idx=idx, scale=scale)
    grad_check(f"q (hub lists, d={d})", dq.cpu().numpy(), dq64.cpu().numpy())
    grad_check(f"c (hub lists, d={d})", dc.cpu().numpy(), dc64.cpu().numpy())


@pytest.mark.parametrize("d", DIMS)
def test_gradient_through_the_model_method_matches_float64(d):
    N, B = 4099, 260
    model = model16()
    embs = layernorm_rows(N, d, seed=21 + d)
    query, target, lists, known = problem(N, B, seed=300 + d)
    q, t = torch.from_numpy(query).to(DEV), torch.from_numpy(target).to(DEV)
    w = torch.randn(B, device=DEV, generator=torch.Generator(device=DEV).manual_seed(d))
    scale = d ** -0.5
    want, _, dq64, dc64 = reference(embs[q], embs, t, lists, scale, grad=w)
    want_g = dc64.clone()
    want_g.index_add_(0, q, dq64)
    e = embs.clone().requires_grad_(True)
    loss = model.softmax_loss(e, q, t, scale=scale, known=known)
    assert loss.requires_grad and loss.dtype == torch.float32 and loss.shape == (B,)
    loss_check(f"recorded loss d={d}", loss, want)
    (loss * w).sum().backward()
    grad_check(f"embs (d={d})", e.grad.cpu().numpy(), want_g.cpu().numpy())
    # rows no query names get exactly the dc term
    ptr, idx = csr(lists)
    _, lse = _native.score_softmax_fwd(embs, embs, t, iq=q, filt_ptr=ptr, filt_idx=idx, scale=scale)
    dq, dc = _native.score_softmax_bwd(embs, embs, t, lse, w, iq=q, filt_ptr=ptr, filt_idx=idx, scale=scale)
    untouched = torch.ones(N, dtype=torch.bool, device=DEV)
    untouched[q] = False
    assert int(untouched.sum()) > N // 2 and torch.equal(e.grad[untouched], dc[untouched])
    # a second backward through the same graph is refused, and so is a double backward
    e2 = embs.clone().requires_grad_(True)
    l2 = model.softmax_loss(e2, q, t, scale=scale, known=known).sum()
    (g2,) = torch.autograd.grad(l2, e2, create_graph=True)
    with pytest.raises(RuntimeError):
        g2.sum().backward()
    with torch.no_grad():
        assert not model.softmax_loss(e2, q, t, scale=scale, known=known).requires_grad


# ---- 4. reproducibility -------------------------------------------------------------------------------------------------
def test_results_are_bit_reproducible_and_independent_of_the_batch():
    N, B, d = 50_000, 300, 128
    embs = layernorm_rows(N, d, seed=11)
    query, target, lists, _ = problem(N, B, seed=12)
    q, t = torch.from_numpy(query).to(DEV), torch.from_numpy(target).to(DEV)
    ptr, idx = csr(lists)
    g = torch.randn(B, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    scale = d ** -0.5
    runs = []
    for _ in range(2):
        loss, lse = _native.score_softmax_fwd(embs, embs, t, iq=q, filt_ptr=ptr, filt_idx=idx, scale=scale)
        dq, dc = _native.score_softmax_bwd(embs, embs, t, lse, g, iq=q, filt_ptr=ptr, filt_idx=idx, scale=scale)
        runs.append((loss, lse, dq, dc))
    for a, b, name in zip(runs[0], runs[1], ("loss", "lse", "dq", "dc")):
        assert torch.equal(a, b), f"{name} differs between two calls on the same inputs"
    want, _ = reference(embs[q], embs, t, lists, scale)
    loss_check("N = 50k: loss", runs[0][0], want)
    h = B // 2
    for lo, hi in ((0, h), (h, B)):
        p2, i2 = csr(lists[lo:hi])
        half, _ = _native.score_softmax_fwd(embs, embs, t[lo:hi], iq=q[lo:hi], filt_ptr=p2, filt_idx=i2, scale=scale)
        assert torch.equal(half, runs[0][0][lo:hi]), "a query's loss depends on the batch it is in"


# ---- 5. raw-call id errors ----------------------------------------------------------------------------------------------
def test_out_of_range_ids_give_nan_for_their_query_only():
    N, M, B, d = 2500, 400, 140, 64
    c = layernorm_rows(N, d, seed=31)
    qm = layernorm_rows(M, d, seed=32)
    rng = np.random.default_rng(5)
    iq, target = rng.integers(0, M, B), rng.integers(0, N, B)
    lists = [np.unique(rng.integers(0, N, 8)) for _ in range(B)]
    bad_iq, bad_iq2, bad_t, bad_t2, bad_f, bad_f2 = 3, 131, 17, 64, 40, 129
    dirty_iq, dirty_t, dirty_lists = iq.copy(), target.copy(), [l.copy() for l in lists]
    dirty_iq[bad_iq], dirty_iq[bad_iq2] = M, -1
    dirty_t[bad_t], dirty_t[bad_t2] = N, -7
    dirty_lists[bad_f] = np.append(dirty_lists[bad_f], N + 5)             # still sorted
    dirty_lists[bad_f2] = np.append(-3, dirty_lists[bad_f2])
    bad = np.array([bad_iq, bad_iq2, bad_t, bad_t2, bad_f, bad_f2])
    g = torch.randn(B, device=DEV, generator=torch.Generator(device=DEV).manual_seed(2))
    g_clean = g.clone()
    g_clean[torch.from_numpy(bad).to(DEV)] = 0.0          # the clean call keeps the queries in place, with no weight
    scale = 0.125

    def run(iq_, t_, lists_, g_):
        ptr, idx = csr(lists_)
        a, b = torch.from_numpy(iq_).to(DEV), torch.from_numpy(t_).to(DEV)
        loss, lse = _native.score_softmax_fwd(qm, c, b, iq=a, filt_ptr=ptr, filt_idx=idx, scale=scale)
        dq, dc = _native.score_softmax_bwd(qm, c, b, lse, g_, iq=a, filt_ptr=ptr, filt_idx=idx, scale=scale)
        torch.cuda.synchronize()
        return loss, lse, dq, dc

    loss0, lse0, dq0, dc0 = run(iq, target, lists, g_clean)
    loss1, lse1, dq1, dc1 = run(dirty_iq, dirty_t, dirty_lists, g)
    ok = np.ones(B, dtype=bool)
    ok[bad] = False
    ok_t, bad_tt = torch.from_numpy(ok).to(DEV), torch.from_numpy(~ok).to(DEV)
    assert torch.isnan(loss1[bad_tt]).all() and torch.isnan(lse1[bad_tt]).all()
    assert torch.isfinite(loss0).all()
    assert torch.equal(loss1[ok_t], loss0[ok_t]) and torch.equal(lse1[ok_t], lse0[ok_t])
    assert torch.equal(dq1[ok_t], dq0[ok_t]) and float(dq1[bad_tt].abs().max()) == 0.0
    assert torch.isfinite(dc1).all() and torch.equal(dc1, dc0)


# ---- 6. consistency with evaluation -------------------------------------------------------------------------------------
def test_the_loss_agrees_with_rank_candidates_on_what_filtered_means():
    N, B, d = 3000, 200, 64
    model = model16()
    c = exact_rows(N, d, seed=9)
    embs = torch.from_numpy(c).to(DEV)
    query, target, lists, known = problem(N, B, seed=13)
    q, t = torch.from_numpy(query).to(DEV), torch.from_numpy(target).to(DEV)
    ptr, idx = csr(lists)
    scale = 0.125
    loss, lse = _native.score_softmax_fwd(embs, embs, t, iq=q, filt_ptr=ptr, filt_idx=idx, scale=scale)
    S = embs[q].double() @ embs.double().T                                # exact in float64, and in the kernel's fp32 chain
    tsc = S[torch.arange(B, device=DEV), t]
    want, want_lse = reference(embs[q], embs, t, lists, scale)
    prob = torch.exp(scale * tsc.float() - lse)
    loss_check("probability of the target", prob, torch.exp(-want))
    loss_check("exact rows: loss", loss, want)
    # a target that is the strict unfiltered maximum, by a margin: the loss vanishes as the scale grows
    top2 = S.topk(2, dim=1)
    sure = torch.nonzero(top2.values[:, 0] - top2.values[:, 1] >= 0.5).flatten()
    assert sure.numel() >= B // 4                    # a node's best partner under the dot product is usually itself
    qs, ts = q[sure], top2.indices[sure, 0]
    greater, equal = model.rank_candidates(embs, qs, ts)
    assert int(greater.abs().max()) == 0 and int(equal.abs().max()) == 0
    sharp = model.softmax_loss(embs, qs, ts, scale=64.0)
    assert torch.isfinite(sharp).all() and float(sharp.max()) < 1e-3, float(sharp.max())


# ---- 7. end to end ------------------------------------------------------------------------------------------------------
def test_training_on_the_softmax_loss_end_to_end():
    kg = ToyKnowledgeGraph(feat_dim=16)
    x, ei = kg.node_features.to(DEV), kg.edge_index.to(DEV)
    src, dst = ei[0], ei[1]
    hidden = 32

    def fresh():
        torch.manual_seed(0)
        return HyperGNN(text_dim=64, node_feat_dim=16, hidden_dim=hidden, num_layers=2).to(DEV)

    # what the hinge-loss demo trains: the parameters its loss reaches
    model = fresh()
    embs = model(x, ei, kg.edge_texts)
    perm = torch.randperm(dst.size(0), generator=torch.Generator().manual_seed(0)).to(DEV)
    hinge = torch.clamp(1.0 - model.score_edges(embs, src, dst) + model.score_edges(embs, src, dst[perm]), min=0.0).mean()
    hinge.backward()
    trained = [n for n, p in model.named_parameters() if p.grad is not None and bool((p.grad != 0).any())]
    assert len(trained) >= 10

    model = fresh()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    losses = []
    for step in range(31):
        opt.zero_grad()
        loss = model.softmax_loss(model(x, ei, kg.edge_texts), src, dst, scale=hidden ** -0.5, known=(ei[0], ei[1])).mean()
        losses.append(loss.item())
        if step == 30:
            break
        loss.backward()
        if step == 0:
            grads = dict(model.named_parameters())
            for n in trained:
                gr = grads[n].grad
                assert gr is not None and torch.isfinite(gr).all() and bool((gr != 0).any()), f"{n}: no usable gradient"
        opt.step()
    print("softmax loss over 30 Adam steps:", " ".join(f"{l:.4f}" for l in losses[::5]))
    assert np.isfinite(losses).all() and losses[30] < losses[0], losses
