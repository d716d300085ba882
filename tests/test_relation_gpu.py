"""Relation-typed link prediction on the GPU: ghf_relation_rows (csrc/relation.hip), autograd.RelationRowsFn / ScoreRowsFn /
SoftmaxLossFn with the query rows given, RelationDecoder and the query_rows / query_rel arguments of HyperGNN.rank_candidates, topk_candidates
and softmax_loss, against a float64 restatement:  out_i = x[ix_i] + x[ix_i] @ op(W[rel_i]) + b[rel_i].

Tolerances are the project's own: values under tests/_util.assert_close's defaults (rtol 1e-4, atol 1e-5, relative L2
1e-5), gradients under the standing gradient rule (rtol 2e-4, atol 1e-4 * max|want|, relative L2 < 5e-5), restated below as
in tests/test_softmax_gpu.py."""

import math

import numpy as np
import pytest
import torch

from _util import assert_close
from graph_hypernetwork_forge_amd import HyperGNN, RelationDecoder, ToyKnowledgeGraph, _native
from graph_hypernetwork_forge_amd.autograd import RelationRowsFn, ScoreRowsFn

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
N, B, R = 5003, 150, 7                      # relation 0 has no query, relation 1 exactly one, relation 2 more than a 64-row tile


def grad_check(name, got, want, rtol=2e-4, l2=5e-5):
    gw, gg = want.detach().cpu().numpy().astype(np.float64), got.detach().cpu().numpy().astype(np.float64)
    assert gg.shape == gw.shape, f"d{name}: shape {gg.shape} vs {gw.shape}"
    assert np.isfinite(gg).all(), f"d{name}: non-finite values"
    scale = float(np.abs(gw).max())
    rel_l2 = np.linalg.norm(gg - gw) / max(np.linalg.norm(gw), 1e-30)
    print(f"d{name}: max abs err {np.abs(gg - gw).max():.3e} at scale {scale:.3e}, relative L2 {rel_l2:.3e}")
    assert np.allclose(gg, gw, rtol=rtol, atol=1e-4 * max(scale, 1e-30)), \
        f"d{name}: max abs err {np.abs(gg - gw).max():.3e} at scale {scale:.3e}"
    assert rel_l2 < l2, f"d{name}: relative L2 {rel_l2:.3e}"


def value_check(what, got, want):
    got, want = got.detach().cpu().numpy(), want.detach().cpu().numpy()
    err = np.abs(got.astype(np.float64) - want)
    print(f"{what}: max abs err {err.max():.3e}, worst err / bound {np.max(err / (1e-5 + 1e-4 * np.abs(want))):.3e}, "
          f"relative L2 {np.linalg.norm(got - want) / max(np.linalg.norm(want), 1e-30):.3e}")
    assert_close(got, want, what)


# ---- the problem and the restatement --------------------------------------------------------------------------------------
def queries(seed):
    """(nodes, rel) int64 [B] on the device: heads repeat; relation 0 unused, relation 1 once, relation 2 seventy times."""
    rng = np.random.default_rng(seed)
    rel = np.concatenate([[1], np.full(70, 2), rng.integers(3, R, B - 71)]).astype(np.int64)
    rng.shuffle(rel)
    nodes = rng.integers(0, N, B).astype(np.int64)
    nodes[B // 2:B // 2 + 5] = nodes[:5]
    nodes[7] = N - 1
    assert (rel == 0).sum() == 0 and (rel == 1).sum() == 1 and (rel == 2).sum() == 70
    return torch.from_numpy(nodes).to(DEV), torch.from_numpy(rel).to(DEV)


def layernorm_rows(n, d, seed):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(n, d, device=DEV, generator=gen)
    gamma = 1.0 + 0.1 * torch.randn(d, device=DEV, generator=gen)
    beta = 0.1 * torch.randn(d, device=DEV, generator=gen)
    return torch.nn.functional.layer_norm(x, (d,), gamma, beta)


def weights(d, seed):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    return 0.05 * torch.randn(R, d, d, device=DEV, generator=gen), 0.1 * torch.randn(R, d, device=DEV, generator=gen)


def restate(x, ix, rel, W, b, add_x=True, transpose=False, dtype=torch.float64):
    """The torch formulation: one gathered matrix per query, in `dtype`."""
    xr = (x[:rel.numel()] if ix is None else x[ix]).to(dtype)
    Wr = W.to(dtype)[rel]
    out = torch.bmm(xr.unsqueeze(1), Wr.transpose(1, 2) if transpose else Wr).squeeze(1)
    if add_x:
        out = out + xr
    if b is not None:
        out = out + b.to(dtype)[rel]
    return out


def typed_known(nodes, rel, seed):
    """Known triples around the queries: true tails under the query's relation, the same pair under another relation, and a
    repeated triple.  Returns (src, dst, erel) on the device and the brute-force typed / untyped lists per query."""
    rng = np.random.default_rng(seed)
    triples = []
    for i, (h, r) in enumerate(zip(nodes.tolist(), rel.tolist())):
        if i % 5 == 4:
            continue                                                     # a query with no known edge of its own
        for t in rng.integers(0, N, 1 + i % 4).tolist():
            triples.append((h, r, t))
            if i % 3 == 0:
                triples.append((h, (r + 1) % R, (t + 1) % N))             # a partner under ANOTHER relation
        if i % 6 == 0:
            triples.append(triples[-1])
    typed = [sorted({t for s, r, t in triples if s == h and r == q}) for h, q in zip(nodes.tolist(), rel.tolist())]
    untyped = [sorted({t for s, _, t in triples if s == h}) for h in nodes.tolist()]
    cols = [torch.tensor([t[k] for t in triples], dtype=torch.int64, device=DEV) for k in (0, 2, 1)]
    return (cols[0], cols[1], cols[2]), typed, untyped


def csr(lists):
    ptr = np.zeros(len(lists) + 1, dtype=np.int64)
    ptr[1:] = np.cumsum([len(l) for l in lists])
    idx = np.concatenate([np.asarray(l, dtype=np.int64) for l in lists])
    return torch.from_numpy(ptr).to(DEV), torch.from_numpy(idx).to(DEV)


def decoder(d, text_dim=16, scale=None, seed=0):
    torch.manual_seed(seed)
    dec = RelationDecoder(text_dim=text_dim, hidden_dim=d).to(DEV).eval()
    if scale is not None:                                               # a fresh decoder deviates by ~1e-4: make it visible
        for p in dec.generator.log_scales.values():
            p.data.fill_(math.log(scale))
    rel_embs = torch.randn(R, text_dim, device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed + 1))
    return dec, rel_embs


# ---- 1. the transform against float64 -------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", (20, 64, 128, 160, 256))       # 160: the kernel's fourth width (64 / 128 / 192 / 256 columns)
def test_transform_matches_float64(d):
    x = layernorm_rows(N, d, seed=d)
    W, b = weights(d, seed=10 + d)
    ix, rel = queries(seed=20 + d)
    group = _native.group_edges(rel, R)
    for transpose in (False, True):
        for bias in (b, None):
            for add_x in (True, False):
                got = _native.relation_rows(x, rel, W, bias, ix=ix, add_x=add_x, transpose=transpose, group=group)
                value_check(f"d={d} transpose={transpose} bias={bias is not None} add_x={add_x}", got,
                            restate(x, ix, rel, W, bias, add_x, transpose))
        got = _native.relation_rows(x, rel, W, b, ix=None, transpose=transpose)        # ix = NULL: rows 0 .. B-1, grouped inside
        value_check(f"d={d} transpose={transpose} ix=None", got, restate(x, None, rel, W, b, True, transpose))


# ---- 2. exact data --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", (20, 160, 256))
def test_integer_data_is_exact(d):
    """Every partial sum is an integer below 2^12: fp32 is exact in any order, so the result must EQUAL the int64 one."""
    rng = np.random.default_rng(d)
    x = torch.from_numpy(rng.integers(-4, 5, (N, d)))
    W = torch.from_numpy(rng.integers(-2, 3, (R, d, d)))
    b = torch.from_numpy(rng.integers(-4, 5, (R, d)))
    ix, rel = queries(seed=30 + d)
    for transpose in (False, True):
        Wr = W[rel.cpu()]
        xr = x[ix.cpu()]
        want = xr + (xr.unsqueeze(2) * (Wr.transpose(1, 2) if transpose else Wr)).sum(1) + b[rel.cpu()]
        got = _native.relation_rows(x.float().to(DEV), rel, W.float().to(DEV), b.float().to(DEV), ix=ix, transpose=transpose)
        assert torch.equal(got.cpu().to(torch.int64), want) and torch.equal(got.cpu(), want.float()), f"transpose={transpose}"


# ---- 3. independence and reproducibility ----------------------------------------------------------------------------------
@pytest.mark.parametrize("d", (20, 128))
def test_rows_are_independent_of_the_batch_and_reproducible(d):
    x = layernorm_rows(N, d, seed=d + 1)
    W, b = weights(d, seed=40 + d)
    ix, rel = queries(seed=50 + d)
    for transpose in (False, True):
        full = _native.relation_rows(x, rel, W, b, ix=ix, transpose=transpose)
        assert torch.equal(full, _native.relation_rows(x, rel, W, b, ix=ix, transpose=transpose))      # two launches
        rev = _native.relation_rows(x, rel.flip(0), W, b, ix=ix.flip(0), transpose=transpose)
        assert torch.equal(rev.flip(0), full)                                                          # the batch reversed
        in2 = torch.nonzero(rel == 2).flatten().tolist()
        for i in sorted(set(list(range(0, B, 13)) + in2[:2] + in2[-3:] + torch.nonzero(rel == 1).flatten().tolist())):
            alone = _native.relation_rows(x, rel[i:i + 1], W, b, ix=ix[i:i + 1], transpose=transpose)
            assert torch.equal(alone[0], full[i]), f"query {i} (relation {int(rel[i])}) differs when it runs alone"


# ---- 4. bad ids in the raw call ---------------------------------------------------------------------------------------------
def test_out_of_range_ids_give_nan_for_their_row_only():
    d = 64
    x = layernorm_rows(N, d, seed=3)
    W, b = weights(d, seed=4)
    ix, rel = queries(seed=5)
    clean = _native.relation_rows(x, rel, W, b, ix=ix)
    bad_ix, bad_rel = ix.clone(), rel.clone()
    bad_ix[11], bad_ix[12] = N, -1
    bad_rel[40], bad_rel[41] = R, -3
    got = _native.relation_rows(x, bad_rel, W, b, ix=bad_ix)
    torch.cuda.synchronize()
    bad = [11, 12, 40, 41]
    assert bool(torch.isnan(got[bad]).all())
    keep = torch.ones(B, dtype=torch.bool, device=DEV)
    keep[bad] = False
    assert torch.equal(got[keep], clean[keep])


def test_the_call_is_capturable_into_a_hip_graph():
    """Nothing allocates, reads back or synchronises: with the grouping, the workspace and the output given, the call is
    captured and the replay reads the inputs as they are then."""
    d = 64
    x = layernorm_rows(N, d, seed=15)
    W, b = weights(d, seed=16)
    ix, rel = queries(seed=17)
    group = _native.group_edges(rel, R)
    ws = torch.empty(_native.relation_rows_workspace_bytes(B, R), dtype=torch.uint8, device=DEV)
    out = torch.empty(B, d, device=DEV)
    call = lambda: _native.relation_rows(x, rel, W, b, ix=ix, group=group, workspace=ws, out=out)     # noqa: E731
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        call()                                                          # warm-up off the capture (the kernel's LDS limit)
    torch.cuda.current_stream(DEV).wait_stream(side)
    want = out.clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    out.zero_()
    graph.replay()
    assert torch.equal(out, want)
    x.mul_(2.0)                                                         # read at replay time
    graph.replay()
    assert torch.equal(out, _native.relation_rows(x, rel, W, b, ix=ix))


# ---- 5. a generator that emits zeros: the typed calls ARE the untyped ones ------------------------------------------------
def test_zero_generator_reproduces_the_untyped_calls_bit_for_bit():
    d = 64
    model = HyperGNN(text_dim=32, node_feat_dim=16, hidden_dim=16).to(DEV)
    dec, rel_embs = decoder(d)
    for head in dec.generator.generators.values():
        head[-1].weight.data.zero_()                                   # (its bias is zero from the start)
    embs = layernorm_rows(N, d, seed=6)
    nodes, rel = queries(seed=7)
    target = torch.from_numpy(np.random.default_rng(8).integers(0, N, B)).to(DEV)
    known, _, _ = typed_known(nodes, rel, seed=9)
    with torch.no_grad():
        for direction in ("tail", "head"):
            Q = dec(embs, nodes, rel, rel_embs, direction=direction)
            assert torch.equal(Q, embs[nodes]), direction
        kn = (known[0], known[1])
        g0, e0 = model.rank_candidates(embs, nodes, target, known=kn)
        g1, e1 = model.rank_candidates(embs, nodes, target, known=kn, query_rows=Q)
        assert torch.equal(g0, g1) and torch.equal(e0, e1)
        s0, i0 = model.topk_candidates(embs, nodes, 10, known=kn)
        s1, i1 = model.topk_candidates(embs, nodes, 10, known=kn, query_rows=Q)
        assert torch.equal(s0, s1) and torch.equal(i0, i1)
        l0 = model.softmax_loss(embs, nodes, target, scale=d ** -0.5, known=kn)
        l1 = model.softmax_loss(embs, nodes, target, scale=d ** -0.5, known=kn, query_rows=Q)
        assert torch.equal(l0, l1)
        assert torch.equal(dec.score(embs, nodes, rel, target, rel_embs), model.score_edges(embs, nodes, target))


# ---- 6. composition -------------------------------------------------------------------------------------------------------
def test_typed_methods_are_the_raw_sweeps_on_the_decoder_rows_and_typed_lists():
    d = 20
    model = HyperGNN(text_dim=32, node_feat_dim=16, hidden_dim=16).to(DEV)
    dec, rel_embs = decoder(d, scale=3.0)
    embs = layernorm_rows(N, d, seed=11)
    nodes, rel = queries(seed=12)
    target = torch.from_numpy(np.random.default_rng(13).integers(0, N, B)).to(DEV)
    known, typed, untyped = typed_known(nodes, rel, seed=14)
    assert typed != untyped
    ptr, idx = csr(typed)
    scale = d ** -0.5
    with torch.no_grad():
        Q = dec(embs, nodes, rel, rel_embs)
        heads = dec.generator(rel_embs)
        value_check("decoder rows", Q, restate(embs, nodes, rel, heads["W_msg"], heads["bias"]))
        value_check("decoder rows, head direction", dec(embs, nodes, rel, rel_embs, direction="head"),
                    restate(embs, nodes, rel, heads["W_self"], heads["bias"]))
        assert float((Q - embs[nodes]).abs().max()) > 1e-2                # the relation matters
        value_check("score", dec.score(embs, nodes, rel, target, rel_embs), (Q.double() * embs[target].double()).sum(-1))
        g, e = model.rank_candidates(embs, nodes, target, query_rows=Q, known=known, query_rel=rel)
        g_raw, e_raw = _native.score_rank(Q, embs, target, filt_ptr=ptr, filt_idx=idx)
        assert torch.equal(g, g_raw) and torch.equal(e, e_raw) and bool((g >= 0).all())
        s, i = model.topk_candidates(embs, nodes, 10, query_rows=Q, known=known, query_rel=rel)
        s_raw, i_raw = _native.score_topk(Q, embs, 10, filt_ptr=ptr, filt_idx=idx)
        assert torch.equal(s, s_raw) and torch.equal(i, i_raw)
        for q, row in enumerate(i.tolist()):
            assert not set(row) & set(typed[q]), f"query {q}: a listed partner among its top-k"
        loss = model.softmax_loss(embs, nodes, target, scale=scale, query_rows=Q, known=known, query_rel=rel)
        loss_raw, _ = _native.score_softmax_fwd(Q, embs, target, filt_ptr=ptr, filt_idx=idx, scale=scale)
        assert torch.equal(loss, loss_raw)
        # all relations equal: the typed known is the two-member known
        one, kn = torch.full_like(rel, 3), (known[0], known[1])
        kn1 = (known[0], known[1], torch.full_like(known[2], 3))
        for a, b_ in zip(model.rank_candidates(embs, nodes, target, query_rows=Q, known=kn1, query_rel=one),
                         model.rank_candidates(embs, nodes, target, query_rows=Q, known=kn)):
            assert torch.equal(a, b_)
        assert torch.equal(model.softmax_loss(embs, nodes, target, scale=scale, query_rows=Q, known=kn1, query_rel=one),
                           model.softmax_loss(embs, nodes, target, scale=scale, query_rows=Q, known=kn))


# ---- 7. gradients ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", (20, 128))
def test_relation_rows_gradients_match_float64(d):
    x = layernorm_rows(N, d, seed=d + 2)
    W, b = weights(d, seed=60 + d)
    ix, rel = queries(seed=70 + d)
    G = torch.randn(B, d, device=DEV, generator=torch.Generator(device=DEV).manual_seed(d))

    def run():
        leaves = [t.clone().requires_grad_(True) for t in (x, W, b)]
        (RelationRowsFn.apply(leaves[0], ix, rel, leaves[1], leaves[2]) * G).sum().backward()
        return [t.grad for t in leaves]

    got = run()
    ref = [t.double().requires_grad_(True) for t in (x, W, b)]
    (restate(ref[0], ix, rel, ref[1], ref[2]) * G.double()).sum().backward()
    for name, g, r in zip(("x", "A", "b"), got, ref):
        grad_check(f"{name} (d={d})", g, r.grad)
    assert bool((got[1][0] == 0).all()) and bool((got[2][0] == 0).all())           # the relation without a query
    for g, g2 in zip(got, run()):
        assert torch.equal(g, g2)                                                   # two backward runs: equal bits
    # ix = None: the rows in order; rows past the B queries get zero
    xl = x.clone().requires_grad_(True)
    (RelationRowsFn.apply(xl, None, rel, W, b) * G).sum().backward()
    r0 = x.double().requires_grad_(True)
    (restate(r0, None, rel, W, b) * G.double()).sum().backward()
    grad_check(f"x, ix=None (d={d})", xl.grad, r0.grad)


@pytest.mark.parametrize("d", (20, 128))
def test_typed_softmax_loss_and_score_gradients_match_float64(d):
    model = HyperGNN(text_dim=32, node_feat_dim=16, hidden_dim=16).to(DEV)
    embs = layernorm_rows(N, d, seed=d + 3)
    W, b = weights(d, seed=80 + d)
    nodes, rel = queries(seed=90 + d)
    target = torch.from_numpy(np.random.default_rng(d).integers(0, N, B)).to(DEV)
    target[10:20] = target[0]
    known, typed, _ = typed_known(nodes, rel, seed=91 + d)
    scale = d ** -0.5
    gl = torch.rand(B, device=DEV, generator=torch.Generator(device=DEV).manual_seed(d)) + 0.5
    Q0 = _native.relation_rows(embs, rel, W, b, ix=nodes)

    def run():
        e, Q = embs.clone().requires_grad_(True), Q0.clone().requires_grad_(True)
        loss = model.softmax_loss(e, nodes, target, scale=scale, query_rows=Q, known=known, query_rel=rel)
        (loss * gl).sum().backward()
        return loss.detach(), Q.grad, e.grad

    loss, dQ, dE = run()
    e64, Q64 = embs.double().requires_grad_(True), Q0.double().requires_grad_(True)
    S = scale * (Q64 @ e64.T)
    mask = torch.zeros(B, N, dtype=torch.bool, device=DEV)
    for i, l in enumerate(typed):
        if l:
            mask[i, torch.tensor(l, device=DEV)] = True
    ar = torch.arange(B, device=DEV)
    mask[ar, target] = False
    want = S.masked_fill(mask, -np.inf).logsumexp(1) - S[ar, target]
    (want * gl.double()).sum().backward()
    value_check(f"typed loss (d={d})", loss, want)
    grad_check(f"Q (d={d})", dQ, Q64.grad)
    grad_check(f"embs (d={d})", dE, e64.grad)
    loss2, dQ2, dE2 = run()
    assert torch.equal(loss, loss2) and torch.equal(dQ, dQ2) and torch.equal(dE, dE2)
    # only query_rows requires grad: still recorded
    Q = Q0.clone().requires_grad_(True)
    model.softmax_loss(embs, nodes, target, scale=scale, query_rows=Q, known=known, query_rel=rel).sum().backward()
    assert Q.grad is not None and bool(torch.isfinite(Q.grad).all())

    # the pair score: s_i = Q_i . embs[tail_i]
    def score():
        e, Q = embs.clone().requires_grad_(True), Q0.clone().requires_grad_(True)
        (ScoreRowsFn.apply(Q, e, target) * gl).sum().backward()
        return Q.grad, e.grad

    sQ, sE = score()
    e64, Q64 = embs.double().requires_grad_(True), Q0.double().requires_grad_(True)
    ((Q64 * e64[target]).sum(-1) * gl.double()).sum().backward()
    grad_check(f"score: Q (d={d})", sQ, Q64.grad)
    grad_check(f"score: embs (d={d})", sE, e64.grad)
    for a, b_ in zip((sQ, sE), score()):
        assert torch.equal(a, b_)

    # dec.score end to end: the gradient with respect to embs through ScoreRowsFn and RelationRowsFn
    dec, rel_embs = decoder(d, scale=3.0)
    e = embs.clone().requires_grad_(True)
    (dec.score(e, nodes, rel, target, rel_embs) * gl).sum().backward()
    with torch.no_grad():
        heads = dec.generator(rel_embs)
    e64 = embs.double().requires_grad_(True)
    ((restate(e64, nodes, rel, heads["W_msg"], heads["bias"]) * e64[target]).sum(-1) * gl.double()).sum().backward()
    grad_check(f"dec.score: embs (d={d})", e.grad, e64.grad)
    used = [p.grad for n, p in dec.named_parameters() if ".W_msg." in n or ".bias." in n]
    assert used and all(g is not None and bool(torch.isfinite(g).all()) for g in used)
    assert any(bool((g != 0).any()) for g in used)


# ---- 8. end to end --------------------------------------------------------------------------------------------------------
def test_training_a_typed_query_with_an_unseen_relation_end_to_end():
    kg = ToyKnowledgeGraph(feat_dim=16)
    x, ei = kg.node_features.to(DEV), kg.edge_index.to(DEV)
    rel_texts = kg.relation_types + ["is colleague of"]                  # the last one labels no edge of the graph
    edge_rel = torch.tensor([rel_texts.index(t) for t in kg.edge_texts], device=DEV)
    unseen = len(rel_texts) - 1
    head = torch.cat([ei[0], torch.tensor([1], device=DEV)])             # ... and (Bob, is colleague of, Carol)
    tail = torch.cat([ei[1], torch.tensor([2], device=DEV)])
    rel = torch.cat([edge_rel, torch.tensor([unseen], device=DEV)])
    hidden = 16
    torch.manual_seed(0)
    model = HyperGNN(text_dim=32, node_feat_dim=16, hidden_dim=hidden).to(DEV)
    dec = RelationDecoder(text_dim=32, hidden_dim=hidden).to(DEV)

    def step(direction):
        embs = model(x, ei, kg.edge_texts)
        rel_embs = model.text_encoder(rel_texts, embs.device)
        if direction == "tail":
            Q = dec(embs, head, rel, rel_embs, direction="tail")
            return model.softmax_loss(embs, head, tail, query_rows=Q, scale=hidden ** -0.5, known=(ei[0], ei[1], edge_rel),
                                      query_rel=rel).mean()
        Q = dec(embs, tail, rel, rel_embs, direction="head")
        return model.softmax_loss(embs, tail, head, query_rows=Q, scale=hidden ** -0.5, known=(ei[1], ei[0], edge_rel),
                                  query_rel=rel).mean()

    def usable(g):
        return g is not None and bool(torch.isfinite(g).all()) and bool((g != 0).any())

    for direction, used, unused in (("tail", "W_msg", "W_self"), ("head", "W_self", "W_msg")):
        model.zero_grad(set_to_none=True)
        dec.zero_grad(set_to_none=True)
        step(direction).backward()
        for n, p in model.named_parameters():
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), f"{direction}: {n} has no finite gradient"
        for n, p in model.text_encoder.named_parameters():
            assert usable(p.grad), f"{direction}: text encoder {n}"
        for n, p in dec.generator.named_parameters():
            if f".{used}." in n or ".bias." in n or n in (f"log_scales.{used}", "log_scales.bias"):
                assert p.grad is not None and bool(torch.isfinite(p.grad).all()), f"{direction}: {n}"
            if f".{unused}." in n or n == f"log_scales.{unused}":
                assert p.grad is None or not bool((p.grad != 0).any()), f"{direction}: {n} belongs to the other direction"
        assert usable(dec.generator.generators[used][-1].weight.grad), direction
        assert usable(dec.generator.generators["bias"][-1].weight.grad), direction

    model.zero_grad(set_to_none=True)
    dec.zero_grad(set_to_none=True)
    opt = torch.optim.Adam(list(model.parameters()) + list(dec.parameters()), lr=1e-3)
    losses = []
    for it in range(21):
        opt.zero_grad()
        loss = step("tail")
        losses.append(loss.item())
        if it == 20:
            break
        loss.backward()
        opt.step()
    print("typed softmax loss over 20 Adam steps:", " ".join(f"{l:.4f}" for l in losses[::4]))
    assert np.isfinite(losses).all() and losses[20] < losses[0], losses
