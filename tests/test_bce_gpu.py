"""The multi-label 1-vs-all BCE link-prediction loss against every node (HyperGNN.bce_loss, ghf_score_bce_fwd / _bwd,
csrc/bce.hip and the loss mode of csrc/softmax.hip's backward) against a float64 restatement of its contract on the float32
rows: the dense [B, N] logits, the dense labels y = (1 - smoothing) [j listed] + smoothing / N,
binary_cross_entropy_with_logits(reduction="none").sum(1), autograd.

Tolerances are the project's own, taken from tests/test_softmax_gpu.py: the loss under tests/_util.assert_close's defaults
(rtol 1e-4, atol 1e-5, relative L2 1e-5), gradients under its grad_check (rtol 2e-4, atol 1e-4 * max|want|, relative L2 <
5e-5)."""

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_softmax_gpu import csr, grad_check, layernorm_rows, loss_check, model16
from graph_hypernetwork_forge_amd import HyperGNN, RelationDecoder, ToyKnowledgeGraph, _native

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
DIMS = (20, 64, 128, 256)


# ---- the restatement ---------------------------------------------------------------------------------------------------
def reference(qrows, c, lists, scale, smoothing, grad=None):
    """float64 loss [B] (and dq, dc for the weights `grad`) for gathered query rows qrows [B, d] and candidates c [N, d]."""
    B, N = qrows.size(0), c.size(0)
    q64 = qrows.double().detach().requires_grad_(grad is not None)
    c64 = c.double().detach().requires_grad_(grad is not None)
    Z = scale * (q64 @ c64.T)
    Y = torch.full((B, N), smoothing / N, dtype=torch.float64, device=c.device)
    if lists is not None:
        for i, l in enumerate(lists):
            if len(l):
                Y[i, torch.as_tensor(np.asarray(l, dtype=np.int64), device=c.device)] = (1.0 - smoothing) + smoothing / N
    loss = F.binary_cross_entropy_with_logits(Z, Y, reduction="none").sum(1)
    if grad is None:
        return loss.detach()
    (loss * grad.double()).sum().backward()
    return loss.detach(), q64.grad, c64.grad


def problem(N, B, seed, per_list=10):
    """Queries with repeats and per-NODE positives (so that known= and CSR lists agree); every seventh first-seen node has
    none."""
    rng = np.random.default_rng(seed)
    query = rng.integers(0, N, B)
    query[B // 2:B // 2 + 5] = query[:5]                                  # repeated queries
    node_lists = {}
    for i, v in enumerate(query):
        if v not in node_lists:
            node_lists[v] = np.unique(rng.integers(0, N, per_list)) if i % 7 else np.zeros(0, dtype=np.int64)
    lists = [node_lists[v] for v in query]
    src = np.concatenate([np.full(len(l), v) for v, l in node_lists.items()] + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
    dst = np.concatenate(list(node_lists.values()) + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
    return query, lists, (torch.from_numpy(src).to(DEV), torch.from_numpy(dst).to(DEV))


def weights(B, seed):
    return torch.randn(B, device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed))


# ---- 1. loss parity ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", DIMS)
def test_loss_matches_float64(d):
    N, B = 5003, 150                                  # neither a multiple of a tile
    model = model16()
    embs = layernorm_rows(N, d, seed=d)
    query, lists, known = problem(N, B, seed=100 + d)
    assert any(len(l) == 0 for l in lists)
    q = torch.from_numpy(query).to(DEV)
    ptr, idx = csr(lists)
    rep_lists = [np.sort(np.append(l, l[:1])) for l in lists]            # an id twice in a list: it counts once
    rptr, ridx = csr(rep_lists)
    for scale in (1.0, d ** -0.5):
        for smoothing in (0.0, 0.1):
            tag = f"d={d} scale={scale:.3g} smoothing={smoothing}"
            want = reference(embs[q], embs, None, scale, smoothing)
            loss = _native.score_bce_fwd(embs, embs, iq=q, scale=scale, smoothing=smoothing)
            loss_check(f"{tag} no lists", loss, want)
            assert torch.equal(model.bce_loss(embs, q, scale=scale, smoothing=smoothing, normalize=False), loss)
            assert torch.equal(loss[B // 2:B // 2 + 5], loss[:5])            # a repeated query: the same sums, bit for bit
            want = reference(embs[q], embs, lists, scale, smoothing)
            loss = _native.score_bce_fwd(embs, embs, iq=q, pos_ptr=ptr, pos_idx=idx, scale=scale, smoothing=smoothing)
            loss_check(f"{tag} lists", loss, want)
            kw = dict(scale=scale, smoothing=smoothing, normalize=False)
            assert torch.equal(model.bce_loss(embs, q, pos_ptr=ptr, pos_idx=idx, **kw), loss)
            assert torch.equal(model.bce_loss(embs, q, known=known, **kw), loss)                  # known= agrees with CSR
            assert torch.equal(model.bce_loss(embs, q, pos_ptr=rptr, pos_idx=ridx, **kw), loss)  # the repeated id
            assert torch.equal(model.bce_loss(embs, q - N, known=known, **kw), loss)              # negative ids wrap
            mean = model.bce_loss(embs, q, known=known, scale=scale, smoothing=smoothing)
            assert torch.equal(mean, loss * (1.0 / N))
            loss_check(f"{tag} mean over the candidates", mean, want / N)
            assert not loss.requires_grad and not mean.requires_grad


# ---- 2. tile edges -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", (20, 128))
def test_tile_edges_and_padding(d):
    """Candidates past N must contribute nothing: a padded row scored as zeros would leak ln 2 each."""
    for N in (1, 255, 256, 257):
        c = layernorm_rows(N, d, seed=N + d)
        for B in (1, 65, 129):
            qm = layernorm_rows(B, d, seed=N + d + B)
            rng = np.random.default_rng(N + B)
            lists = [np.unique(np.append(rng.integers(0, N, 2), N - 1)) if i % 2 == 0 else np.zeros(0, dtype=np.int64)
                     for i in range(B)]                                   # one positive is the last candidate
            ptr, idx = csr(lists)
            g = weights(B, N + B)
            for smoothing in (0.0, 0.1):
                tag = f"N={N} B={B} d={d} smoothing={smoothing}"
                want, dq64, dc64 = reference(qm, c, lists, 0.5, smoothing, grad=g)
                loss = _native.score_bce_fwd(qm, c, pos_ptr=ptr, pos_idx=idx, scale=0.5, smoothing=smoothing)
                loss_check(tag, loss, want)
                dq, dc = _native.score_bce_bwd(qm, c, loss, g, pos_ptr=ptr, pos_idx=idx, scale=0.5, smoothing=smoothing)
                grad_check(f"q ({tag})", dq.cpu().numpy(), dq64.cpu().numpy())
                grad_check(f"c ({tag})", dc.cpu().numpy(), dc64.cpu().numpy())


# ---- 3. far-negative logits --------------------------------------------------------------------------------------------
def test_far_negative_logits_keep_their_softplus_tail():
    """Every logit is near -6.4, -12.8, -19.2: exp(z) falls to 5e-9, where log(1 + t) computed as log of the rounded 1 + t is
    0 (it already loses 2 % at t = 6e-6).  The losses are about 8.33, 1.4e-2 and 2.4e-5."""
    N, d = 5003, 64
    gen = torch.Generator(device=DEV).manual_seed(3)
    c = 1.0 + 0.1 * torch.randn(N, d, device=DEV, generator=gen)
    Q = torch.tensor([-0.1, -0.2, -0.3], device=DEV)[:, None] * torch.ones(3, d, device=DEV)
    want = reference(Q, c, None, 1.0, 0.0)
    print("expected losses:", want.tolist())
    assert 7.0 < float(want[0]) < 10.0 and 1.0e-2 < float(want[1]) < 2.0e-2 and 1.5e-5 < float(want[2]) < 3.5e-5
    model = model16()
    loss = model.bce_loss(c, torch.zeros(3, dtype=torch.int64, device=DEV), query_rows=Q, normalize=False)
    print("losses:", loss.tolist(), "relative errors:", ((loss.double() - want) / want).tolist())
    loss_check("far-negative logits", loss, want)
    for i in range(3):                                                   # and each row on its own
        loss_check(f"far-negative logits, row {i}", loss[i:i + 1], want[i:i + 1])


# ---- 4. positives dominate ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", (64, 128))
def test_positives_that_dominate(d):
    """Every query's 10 listed rows are 2 x its own row: they score 2 |q|^2 (about 2 d at scale 1), where sigma = 1 to the
    last bit and softplus(z) - z vanishes.  Loss and gradients stay finite and within tolerance."""
    N, B, L = 5003, 130, 10
    model = model16()
    embs = layernorm_rows(N, d, seed=50 + d)
    query = np.arange(B)
    lists = [B + L * i + np.arange(L) for i in range(B)]
    for i in range(B):
        embs[torch.from_numpy(lists[i]).to(DEV)] = 2.0 * embs[i]
    q = torch.from_numpy(query).to(DEV)
    ptr, idx = csr(lists)
    w = torch.rand(B, device=DEV, generator=torch.Generator(device=DEV).manual_seed(d)) + 0.5
    for smoothing in (0.0, 0.1):
        want, dq64, dc64 = reference(embs[q], embs, lists, 1.0, smoothing, grad=w)
        e = embs.clone().requires_grad_(True)
        loss = model.bce_loss(e, q, pos_ptr=ptr, pos_idx=idx, scale=1.0, smoothing=smoothing, normalize=False)
        assert torch.isfinite(loss).all()
        loss_check(f"dominating positives d={d} smoothing={smoothing}: loss", loss, want)
        (loss * w).sum().backward()
        want_g = dc64.clone()
        want_g.index_add_(0, q, dq64)
        grad_check(f"embs (dominating positives, d={d}, smoothing={smoothing})", e.grad.cpu().numpy(), want_g.cpu().numpy())


# ---- 5. gradients ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", (20, 128, 256))
def test_raw_backward_dq_and_dc_match_float64(d):
    N, M, B = 3001, 517, 200
    c = layernorm_rows(N, d, seed=7 + d)
    qm = layernorm_rows(M, d, seed=8 + d)                                 # q != c
    rng = np.random.default_rng(d)
    iq = rng.integers(0, M, B)
    iq[50:60] = iq[0]
    lists = [np.unique(rng.integers(0, N, 12)) if i % 5 else np.zeros(0, dtype=np.int64) for i in range(B)]
    lists[3] = np.sort(np.append(lists[3], lists[3][:2]))                 # two ids twice
    ptr, idx = csr(lists)
    q_i = torch.from_numpy(iq).to(DEV)
    g = weights(B, d)
    for scale, smoothing, with_lists in ((1.0, 0.1, True), (d ** -0.5, 0.0, True), (0.25, 0.1, False), (0.25, 0.0, False)):
        pp, pi, ls = (ptr, idx, lists) if with_lists else (None, None, None)
        tag = f"d={d}, scale={scale:.3g}, smoothing={smoothing}, lists={with_lists}"
        want, dq64, dc64 = reference(qm[q_i], c, ls, scale, smoothing, grad=g)
        loss = _native.score_bce_fwd(qm, c, iq=q_i, pos_ptr=pp, pos_idx=pi, scale=scale, smoothing=smoothing)
        loss_check(f"q != c, {tag}: loss", loss, want)
        dq, dc = _native.score_bce_bwd(qm, c, loss, g, iq=q_i, pos_ptr=pp, pos_idx=pi, scale=scale, smoothing=smoothing)
        grad_check(f"q ({tag})", dq.cpu().numpy(), dq64.cpu().numpy())
        grad_check(f"c ({tag})", dc.cpu().numpy(), dc64.cpu().numpy())


@pytest.mark.parametrize("d", (20, 128, 256))
def test_gradient_through_the_model_method_matches_float64(d):
    N, B = 4099, 260
    model = model16()
    embs = layernorm_rows(N, d, seed=21 + d)
    query, lists, known = problem(N, B, seed=300 + d)
    q = torch.from_numpy(query).to(DEV)
    w = weights(B, d)
    scale = d ** -0.5
    for smoothing, kn, ls in ((0.1, known, lists), (0.0, None, None)):
        want, dq64, dc64 = reference(embs[q], embs, ls, scale, smoothing, grad=w)
        want_g = dc64.clone()
        want_g.index_add_(0, q, dq64)
        e = embs.clone().requires_grad_(True)
        loss = model.bce_loss(e, q, known=kn, scale=scale, smoothing=smoothing, normalize=False)
        assert loss.requires_grad and loss.dtype == torch.float32 and loss.shape == (B,)
        loss_check(f"recorded loss d={d} smoothing={smoothing}", loss, want)
        (loss * w).sum().backward()
        grad_check(f"embs (d={d}, smoothing={smoothing})", e.grad.cpu().numpy(), want_g.cpu().numpy())
    # the mean over the candidates carries 1 / N into the gradient
    e1 = embs.clone().requires_grad_(True)
    (model.bce_loss(e1, q, known=known, scale=scale, smoothing=0.1) * w).sum().backward()
    want, dq64, dc64 = reference(embs[q], embs, lists, scale, 0.1, grad=w / N)
    want_g = dc64.clone()
    want_g.index_add_(0, q, dq64)
    grad_check(f"embs (d={d}, normalized)", e1.grad.cpu().numpy(), want_g.cpu().numpy())
    # rows no query names get exactly the dc term
    ptr, idx = csr(lists)
    raw = _native.score_bce_fwd(embs, embs, iq=q, pos_ptr=ptr, pos_idx=idx, scale=scale, smoothing=0.1)
    dq, dc = _native.score_bce_bwd(embs, embs, raw, w / N, iq=q, pos_ptr=ptr, pos_idx=idx, scale=scale, smoothing=0.1)
    untouched = torch.ones(N, dtype=torch.bool, device=DEV)
    untouched[q] = False
    assert int(untouched.sum()) > N // 2 and torch.equal(e1.grad[untouched], dc[untouched])
    with torch.no_grad():
        assert not model.bce_loss(e1, q, known=known, scale=scale).requires_grad


@pytest.mark.parametrize("d", (20, 128))
def test_gradient_through_query_rows_matches_float64(d):
    N, B = 2050, 140
    model = model16()
    embs = layernorm_rows(N, d, seed=40 + d)
    rows = layernorm_rows(B, d, seed=41 + d)
    query, lists, known = problem(N, B, seed=400 + d)
    q = torch.from_numpy(query).to(DEV)
    w = weights(B, d)
    want, dq64, dc64 = reference(rows, embs, lists, 0.25, 0.1, grad=w)
    e, r = embs.clone().requires_grad_(True), rows.clone().requires_grad_(True)
    loss = model.bce_loss(e, q, known=known, scale=0.25, smoothing=0.1, normalize=False, query_rows=r)
    loss_check(f"query_rows d={d}: loss", loss, want)
    (loss * w).sum().backward()
    grad_check(f"query_rows (d={d})", r.grad.cpu().numpy(), dq64.cpu().numpy())
    grad_check(f"embs under query_rows (d={d})", e.grad.cpu().numpy(), dc64.cpu().numpy())
    only_rows = model.bce_loss(embs, q, known=known, scale=0.25, smoothing=0.1, normalize=False, query_rows=r)
    assert only_rows.requires_grad and torch.equal(only_rows, loss)


def test_the_gradient_reaches_a_relation_decoder_on_the_toy_graph():
    kg = ToyKnowledgeGraph(feat_dim=16)
    x, ei = kg.node_features.to(DEV), kg.edge_index.to(DEV)
    rel_texts = kg.relation_types
    edge_rel = torch.tensor([rel_texts.index(t) for t in kg.edge_texts], device=DEV)
    hidden = 16
    torch.manual_seed(0)
    model = HyperGNN(text_dim=32, node_feat_dim=16, hidden_dim=hidden).to(DEV)
    dec = RelationDecoder(text_dim=32, hidden_dim=hidden).to(DEV)
    embs = model(x, ei, kg.edge_texts)
    N, R = embs.size(0), len(rel_texts)
    pair = torch.unique(ei[0] * R + edge_rel)                            # the distinct (head, relation) queries
    head, rel = pair // R, pair % R
    Q = dec(embs, head, rel, model.text_encoder(rel_texts, embs.device))
    loss = model.bce_loss(embs, head, query_rows=Q, known=(ei[0], ei[1], edge_rel), query_rel=rel, scale=hidden ** -0.5,
                          smoothing=0.1)
    assert loss.shape == (pair.numel(),) and loss.requires_grad and torch.isfinite(loss).all()
    # against the dense statement, labels built from the triples
    lists = [sorted({int(t) for s, r, t in zip(ei[0].tolist(), edge_rel.tolist(), ei[1].tolist()) if s == h and r == u})
             for h, u in zip(head.tolist(), rel.tolist())]
    assert all(len(l) >= 1 for l in lists)
    want = reference(Q.detach(), embs.detach(), lists, hidden ** -0.5, 0.1) / N
    loss_check("toy graph, typed queries", loss, want)
    loss.mean().backward()

    def usable(g):
        return g is not None and bool(torch.isfinite(g).all()) and bool((g != 0).any())

    assert usable(dec.generator.generators["W_msg"][-1].weight.grad) and usable(dec.generator.generators["bias"][-1].weight.grad)
    for n, p in model.text_encoder.named_parameters():
        assert usable(p.grad), f"text encoder {n}"
    for n, p in model.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), f"{n} has no finite gradient"


# ---- 6. hub positives --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", (64, 256))
def test_hub_positives_that_every_query_lists(d):
    """Every query lists the same three neighbouring candidates: more listed pairs fall into one candidate tile than the dc
    sweep keeps beside it, so it looks every id up instead; the same contract, and a list that carries each id twice changes
    nothing."""
    N, B = 1500, 1200
    c = layernorm_rows(N, d, seed=70 + d)
    rng = np.random.default_rng(d)
    iq = rng.integers(0, N, B)
    hubs = np.arange(700, 703)
    lists = [np.unique(np.append(hubs, rng.integers(0, N, 2))) for _ in range(B)]
    twice = [np.sort(np.concatenate([l, l])) for l in lists]
    q_i = torch.from_numpy(iq).to(DEV)
    g = weights(B, d)
    scale, smoothing = d ** -0.5, 0.1
    want, dq64, dc64 = reference(c[q_i], c, lists, scale, smoothing, grad=g)
    out = []
    for ls in (lists, twice):
        ptr, idx = csr(ls)
        loss = _native.score_bce_fwd(c, c, iq=q_i, pos_ptr=ptr, pos_idx=idx, scale=scale, smoothing=smoothing)
        dq, dc = _native.score_bce_bwd(c, c, loss, g, iq=q_i, pos_ptr=ptr, pos_idx=idx, scale=scale, smoothing=smoothing)
        out.append((loss, dq, dc))
    loss, dq, dc = out[0]
    loss_check(f"hub positives d={d}: loss", loss, want)
    grad_check(f"q (hub positives, d={d})", dq.cpu().numpy(), dq64.cpu().numpy())
    grad_check(f"c (hub positives, d={d})", dc.cpu().numpy(), dc64.cpu().numpy())
    for a, b, name in zip(out[0], out[1], ("loss", "dq", "dc")):
        assert torch.equal(a, b), f"{name} changes when every listed id appears twice"


# ---- 7. reproducibility ------------------------------------------------------------------------------------------------
def test_results_are_bit_reproducible_and_independent_of_the_batch():
    N, B, d = 50_000, 300, 128                        # several candidate slabs
    embs = layernorm_rows(N, d, seed=11)
    query, lists, _ = problem(N, B, seed=12)
    q = torch.from_numpy(query).to(DEV)
    ptr, idx = csr(lists)
    g = weights(B, 1)
    scale, smoothing = d ** -0.5, 0.1
    runs = []
    for _ in range(2):
        loss = _native.score_bce_fwd(embs, embs, iq=q, pos_ptr=ptr, pos_idx=idx, scale=scale, smoothing=smoothing)
        dq, dc = _native.score_bce_bwd(embs, embs, loss, g, iq=q, pos_ptr=ptr, pos_idx=idx, scale=scale, smoothing=smoothing)
        runs.append((loss, dq, dc))
    for a, b, name in zip(runs[0], runs[1], ("loss", "dq", "dc")):
        assert torch.equal(a, b), f"{name} differs between two calls on the same inputs"
    loss_check("N = 50k: loss", runs[0][0], reference(embs[q], embs, lists, scale, smoothing))
    h = B // 2
    for lo, hi in ((0, h), (h, B)):
        p2, i2 = csr(lists[lo:hi])
        half = _native.score_bce_fwd(embs, embs, iq=q[lo:hi], pos_ptr=p2, pos_idx=i2, scale=scale, smoothing=smoothing)
        assert torch.equal(half, runs[0][0][lo:hi]), "a query's loss depends on the batch it is in"


# ---- 8. raw-call id errors ---------------------------------------------------------------------------------------------
def test_out_of_range_ids_give_nan_for_their_query_only():
    N, M, B, d = 2500, 400, 140, 64
    c = layernorm_rows(N, d, seed=31)
    qm = layernorm_rows(M, d, seed=32)
    rng = np.random.default_rng(5)
    iq = rng.integers(0, M, B)
    lists = [np.unique(rng.integers(0, N, 8)) for _ in range(B)]
    bad_iq, bad_iq2, bad_f, bad_f2 = 3, 131, 40, 129
    dirty_iq, dirty_lists = iq.copy(), [l.copy() for l in lists]
    dirty_iq[bad_iq], dirty_iq[bad_iq2] = M, -1
    dirty_lists[bad_f] = np.append(dirty_lists[bad_f], N + 5)             # still sorted
    dirty_lists[bad_f2] = np.append(-3, dirty_lists[bad_f2])
    bad = np.array([bad_iq, bad_iq2, bad_f, bad_f2])
    g = weights(B, 2)
    g_clean = g.clone()
    g_clean[torch.from_numpy(bad).to(DEV)] = 0.0          # the clean call keeps the queries in place, with no weight

    def run(iq_, lists_, g_):
        ptr, idx = csr(lists_)
        a = torch.from_numpy(iq_).to(DEV)
        loss = _native.score_bce_fwd(qm, c, iq=a, pos_ptr=ptr, pos_idx=idx, scale=0.125, smoothing=0.1)
        dq, dc = _native.score_bce_bwd(qm, c, loss, g_, iq=a, pos_ptr=ptr, pos_idx=idx, scale=0.125, smoothing=0.1)
        torch.cuda.synchronize()
        return loss, dq, dc

    loss0, dq0, dc0 = run(iq, lists, g_clean)
    loss1, dq1, dc1 = run(dirty_iq, dirty_lists, g)
    ok = np.ones(B, dtype=bool)
    ok[bad] = False
    ok_t, bad_tt = torch.from_numpy(ok).to(DEV), torch.from_numpy(~ok).to(DEV)
    assert torch.isnan(loss1[bad_tt]).all() and torch.isfinite(loss0).all()
    assert torch.equal(loss1[ok_t], loss0[ok_t])
    assert torch.equal(dq1[ok_t], dq0[ok_t]) and float(dq1[bad_tt].abs().max()) == 0.0
    assert torch.isfinite(dc1).all() and torch.equal(dc1, dc0)


# ---- 9. graph capture --------------------------------------------------------------------------------------------------
def test_the_raw_calls_are_capturable_into_a_hip_graph():
    N, B, d = 20_000, 200, 128
    embs = layernorm_rows(N, d, seed=61)
    query, lists, _ = problem(N, B, seed=62)
    q = torch.from_numpy(query).to(DEV)
    ptr, idx = csr(lists)
    g = weights(B, 3)
    kw = dict(iq=q, pos_ptr=ptr, pos_idx=idx, scale=d ** -0.5, smoothing=0.1)
    loss = _native.score_bce_fwd(embs, embs, **kw)                         # also the warm-up (the kernels' LDS limits)
    dq, dc = _native.score_bce_bwd(embs, embs, loss, g, **kw)
    ws_f = torch.empty(_native.score_bce_workspace_bytes(B, N, d), dtype=torch.uint8, device=DEV)
    ws_b = torch.empty(_native.score_bce_bwd_workspace_bytes(B, N, d), dtype=torch.uint8, device=DEV)
    o_loss = torch.empty(B, device=DEV)
    o_dq, o_dc = torch.empty(B, d, device=DEV), torch.empty(N, d, device=DEV)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _native.score_bce_fwd(embs, embs, workspace=ws_f, out=o_loss, **kw)
        _native.score_bce_bwd(embs, embs, o_loss, g, workspace=ws_b, out=(o_dq, o_dc), **kw)
    for _ in range(2):
        for t in (o_loss, o_dq, o_dc):
            t.fill_(7)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(o_loss, loss) and torch.equal(o_dq, dq) and torch.equal(o_dc, dc)


# ---- 10. end to end ----------------------------------------------------------------------------------------------------
def test_training_on_the_bce_loss_end_to_end():
    kg = ToyKnowledgeGraph(feat_dim=16)
    x, ei = kg.node_features.to(DEV), kg.edge_index.to(DEV)
    hidden = 32
    torch.manual_seed(0)
    model = HyperGNN(text_dim=64, node_feat_dim=16, hidden_dim=hidden, num_layers=2).to(DEV)
    heads = torch.unique(ei[0])                                          # one row per distinct query, all its partners at once
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    losses = []
    for step in range(21):
        opt.zero_grad()
        loss = model.bce_loss(model(x, ei, kg.edge_texts), heads, known=(ei[0], ei[1]), scale=hidden ** -0.5, smoothing=0.1).mean()
        losses.append(loss.item())
        if step == 20:
            break
        loss.backward()
        if step == 0:
            grads = [p.grad for p in model.parameters() if p.grad is not None and bool((p.grad != 0).any())]
            assert len(grads) >= 10 and all(bool(torch.isfinite(gr).all()) for gr in grads)
        opt.step()
    print("bce loss over 20 Adam steps:", " ".join(f"{l:.5f}" for l in losses[::4]))
    assert np.isfinite(losses).all() and losses[20] < losses[0], losses
