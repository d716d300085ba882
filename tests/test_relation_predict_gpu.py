"""Relation prediction on the GPU, (head, ?, tail): ghf_relation_scores and its two backward calls (csrc/relation_predict.hip),
autograd.RelationScoresFn and RelationDecoder.score_relations / rank_relations / topk_relations / relation_loss, against a
float64 restatement through the einsum that the kernel never materialises:

    S[i, u] = (a_i + a_i @ op(W[u]) + bias[u]) . b_i,    a = x[ia], b = x[ib]

Tolerances are the project's own: values under tests/_util.assert_close's defaults (rtol 1e-4, atol 1e-5, relative L2
1e-5), gradients under the standing gradient rule (rtol 2e-4, atol 1e-4 * max|want|, relative L2 < 5e-5), restated below as
in tests/test_relation_gpu.py.  Inputs: x = 0.5 layer_norm(randn), W = (0.5 / sqrt(d)) randn, bias = 0.1 randn — a score is a
sum of d products of O(1) rows, and with these scales two fp32 summation orders stay within 0.17 of the pointwise bound
against float64 at every size below, so a failure here is the kernel's, not fp32's.

Shapes: N = 5003 rows, B = 150 pairs (two full 64-row tiles and a ragged one of 22; three slabs of the weight gradient),
U in {1, 7, 37} relations (37 is a multiple of no chunk).  The ids hold repeated heads, a pair with head = tail, and node
N - 1."""

import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _util import assert_close
from graph_hypernetwork_forge_amd import HyperGNN, RelationDecoder, ToyKnowledgeGraph, _native, link_prediction_metrics
from graph_hypernetwork_forge_amd.autograd import RelationScoresFn

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
N, B = 5003, 150
US = (1, 7, 37)


def grad_check(name, got, want, rtol=2e-4, l2=5e-5):
    gw, gg = want.detach().cpu().numpy().astype(np.float64), got.detach().cpu().numpy().astype(np.float64)
    assert gg.shape == gw.shape, f"d{name}: shape {gg.shape} vs {gw.shape}"
    assert np.isfinite(gg).all(), f"d{name}: non-finite values"
    scale = float(np.abs(gw).max())
    rel_l2 = np.linalg.norm(gg - gw) / max(np.linalg.norm(gw), 1e-30)
    print(f"d{name}: max abs err {np.abs(gg - gw).max():.3e} at scale {scale:.3e} (err / atol "
          f"{np.abs(gg - gw).max() / (1e-4 * max(scale, 1e-30)):.3e}), relative L2 {rel_l2:.3e}")
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
def pairs(seed, n=B):
    """(ia, ib) int64 [n] on the device: heads repeat, pair 9 has head = tail, pair 7 names node N - 1 (as a head) and pair 8
    (as a tail).  The first B pairs do not depend on n."""
    rng = np.random.default_rng(seed)
    ia, ib = rng.integers(0, N, B).astype(np.int64), rng.integers(0, N, B).astype(np.int64)
    if n > B:
        ia, ib = np.concatenate([ia, rng.integers(0, N, n - B)]), np.concatenate([ib, rng.integers(0, N, n - B)])
    ia[B // 2:B // 2 + 5] = ia[:5]
    ia[140:145] = ia[0]
    ib[B // 2 + 1] = ib[1]                                   # a repeated pair as well
    ia[7], ib[8] = N - 1, N - 1
    ib[9] = ia[9]
    return torch.from_numpy(ia).to(DEV), torch.from_numpy(ib).to(DEV)


def rows(n, d, seed):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    return 0.5 * F.layer_norm(torch.randn(n, d, device=DEV, generator=gen), (d,))


def weights(U, d, seed):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    return (0.5 / math.sqrt(d)) * torch.randn(U, d, d, device=DEV, generator=gen), 0.1 * torch.randn(U, d, device=DEV, generator=gen)


def restate(x, ia, ib, W, b, add_x=True, transpose=False, dtype=torch.float64):
    """The einsum formulation with its [B, U, d] intermediate, in `dtype`."""
    a, bb, Wd = x[ia].to(dtype), x[ib].to(dtype), W.to(dtype)
    q = torch.einsum("bi,uji->buj" if transpose else "bi,uij->buj", a, Wd)
    if add_x:
        q = q + a.unsqueeze(1)
    if b is not None:
        q = q + b.to(dtype).unsqueeze(0)
    return torch.einsum("buj,bj->bu", q, bb)


def decoder(d, U, text_dim=16, scale=None, seed=0):
    torch.manual_seed(seed)
    dec = RelationDecoder(text_dim=text_dim, hidden_dim=d).to(DEV).eval()
    if scale is not None:                                               # a fresh decoder deviates by ~1e-4: make it visible
        for p in dec.generator.log_scales.values():
            p.data.fill_(math.log(scale))
    rel_embs = torch.randn(U, text_dim, device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed + 1))
    return dec, rel_embs


def known_triples(head, tail, rel, U, seed):
    """Known triples around the pairs: the target itself, the same directed pair under other relations, a repeated triple and
    reverse edges.  Returns (src, dst, erel) on the device and the brute-force lists per pair, without / with the target."""
    rng = np.random.default_rng(seed)
    triples = []
    for i, (h, t, r) in enumerate(zip(head.tolist(), tail.tolist(), rel.tolist())):
        if i % 5 == 4:
            continue                                                     # a pair nothing is known about
        triples.append((h, r, t))
        for u in rng.integers(0, U, i % 4).tolist():
            triples.append((h, u, t))
        if i % 3 == 0:
            triples.append((t, (r + 1) % U, h))                          # the reverse edge under another relation
        if i % 6 == 0:
            triples.append(triples[-1])
    lists = [sorted({u for s, u, t_ in triples if s == h and t_ == t and u != r})
             for h, t, r in zip(head.tolist(), tail.tolist(), rel.tolist())]
    lists_all = [sorted({u for s, u, t_ in triples if s == h and t_ == t}) for h, t in zip(head.tolist(), tail.tolist())]
    cols = [torch.tensor([t[k] for t in triples], dtype=torch.int64, device=DEV) for k in (0, 2, 1)]
    return (cols[0], cols[1], cols[2]), lists, lists_all


def csr(lists):
    ptr = np.zeros(len(lists) + 1, dtype=np.int64)
    ptr[1:] = np.cumsum([len(l) for l in lists])
    idx = np.concatenate([np.asarray(l, dtype=np.int64) for l in lists])
    return torch.from_numpy(ptr).to(DEV), torch.from_numpy(idx).to(DEV)


# ---- 1. the table against float64 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", (20, 64, 128, 160, 256))       # 160: the kernel's third width (64 / 128 / 192 / 256 columns)
def test_scores_match_float64(d):
    x = rows(N, d, seed=d)
    ia, ib = pairs(seed=20 + d)
    for U in US:
        W, b = weights(U, d, seed=10 + d + U)
        for transpose in (False, True):
            for bias in (b, None):
                for add_x in (True, False):
                    got = _native.relation_scores(x, ia, ib, W, bias, add_x=add_x, transpose=transpose)
                    assert got.shape == (B, U) and got.dtype == torch.float32
                    value_check(f"d={d} U={U} transpose={transpose} bias={bias is not None} add_x={add_x}", got,
                                restate(x, ia, ib, W, bias, add_x, transpose))


# ---- 2. exact data ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", (20, 160, 256))
def test_integer_data_is_exact(d):
    """x in -2..2, W and b in -1..1: |q| <= 2 + 2 d + 1 and |S| <= 2 d (2 d + 3) < 2^19, every partial sum an integer below
    2^24: fp32 is exact in any order, so the table must EQUAL the int64 one."""
    rng = np.random.default_rng(d)
    U = 37
    x = torch.from_numpy(rng.integers(-2, 3, (N, d)))
    W = torch.from_numpy(rng.integers(-1, 2, (U, d, d)))
    b = torch.from_numpy(rng.integers(-1, 2, (U, d)))
    ia, ib = pairs(seed=30 + d)
    for transpose in (False, True):
        want = restate(x.to(DEV), ia, ib, W.to(DEV), b.to(DEV), True, transpose).to(torch.int64)   # float64 holds these integers exactly
        got = _native.relation_scores(x.float().to(DEV), ia, ib, W.float().to(DEV), b.float().to(DEV), transpose=transpose)
        assert torch.equal(got.to(torch.int64), want) and torch.equal(got, want.float()), f"transpose={transpose}"


# ---- 3. independence and reproducibility -----------------------------------------------------------------------------------
@pytest.mark.parametrize("d", (20, 128))
def test_entries_are_independent_of_the_batch_and_of_the_other_relations(d):
    U = 37
    x = rows(N, d, seed=d + 1)
    W, b = weights(U, d, seed=40 + d)
    ia, ib = pairs(seed=50 + d)
    perm = torch.from_numpy(np.random.default_rng(d).permutation(B)).to(DEV)
    for transpose in (False, True):
        full = _native.relation_scores(x, ia, ib, W, b, transpose=transpose)
        assert torch.equal(full, _native.relation_scores(x, ia, ib, W, b, transpose=transpose))          # two launches
        shuffled = _native.relation_scores(x, ia[perm], ib[perm], W, b, transpose=transpose)
        assert torch.equal(shuffled, full[perm])                                                        # a permuted batch
        for i in (0, 7, 9, 63, 64, 127, 128, 149):
            alone = _native.relation_scores(x, ia[i:i + 1], ib[i:i + 1], W, b, transpose=transpose)      # B = 1
            assert torch.equal(alone[0], full[i]), f"pair {i} differs when it runs alone"
        for u in (0, 1, 18, 19, 31, 32, 36):
            col = _native.relation_scores(x, ia, ib, W[u:u + 1], b[u:u + 1], transpose=transpose)        # W[u] alone
            assert torch.equal(col[:, 0], full[:, u]), f"relation {u} differs when it is the only one"
        first = _native.relation_scores(x, ia, ib, W[:7], b[:7], transpose=transpose)
        assert torch.equal(first, full[:, :7])


@pytest.mark.parametrize("n", (6422, 33046))
def test_large_batches_sweep_runs_of_relations(n):
    """With three tiles every workgroup takes ONE relation.  101 tiles: runs of 4 relations forward, a tile's relations split
    five ways (partials) in the row gradients; 517 tiles: runs of 19 forward, one workgroup sweeps all 37 backward; the weight
    gradient goes from 3 slabs of 64 queries to 14 slabs of thousands.  Same bits forward, same bounds backward."""
    d, U = 20, 37
    x = rows(N, d, seed=5)
    W, b = weights(U, d, seed=6)
    ia, ib = pairs(seed=7, n=n)
    G = torch.randn(n, U, device=DEV, generator=torch.Generator(device=DEV).manual_seed(n))

    def run():
        leaves = [t.clone().requires_grad_(True) for t in (x, W, b)]
        S = RelationScoresFn.apply(leaves[0], ia, ib, leaves[1], leaves[2])
        (S * G).sum().backward()
        return S.detach(), [t.grad for t in leaves]

    S, got = run()
    assert torch.equal(S[:B], _native.relation_scores(x, ia[:B], ib[:B], W, b))          # the runs change no bit
    assert torch.equal(S, _native.relation_scores(x, ia, ib, W.transpose(1, 2).contiguous(), b, transpose=True))
    ref = [t.double().requires_grad_(True) for t in (x, W, b)]
    want = restate(ref[0], ia, ib, ref[1], ref[2])
    (want * G.double()).sum().backward()
    value_check(f"S (B={n})", S, want)
    for name, g, r in zip(("embs", "A", "b"), got, ref):
        grad_check(f"{name} (B={n})", g, r.grad)
    for g, g2 in zip(got, run()[1]):
        assert torch.equal(g, g2)


# ---- 4. against the existing kernels ---------------------------------------------------------------------------------------
def test_table_agrees_with_relation_rows_and_the_decoder():
    d, U = 64, 7
    x = rows(N, d, seed=3)
    W, b = weights(U, d, seed=4)
    ia, ib = pairs(seed=5)
    S = _native.relation_scores(x, ia, ib, W, b)
    for u in range(U):
        Q = _native.relation_rows(x, torch.full((B,), u, dtype=torch.int64, device=DEV), W, b, ix=ia)
        value_check(f"column {u} vs relation_rows . b", S[:, u], _native.score_pairs_fwd(Q, x, None, ib).double())
    dec, rel_embs = decoder(d, U, scale=3.0)
    rel = torch.from_numpy(np.random.default_rng(6).integers(0, U, B)).to(DEV)
    ar = torch.arange(B, device=DEV)
    with torch.no_grad():
        St = dec.score_relations(x, ia, ib, rel_embs)
        assert float((St - St[:, :1]).abs().max()) > 1e-2                         # the relation matters
        value_check("S[i, rel_i] vs dec.score", St[ar, rel], dec.score(x, ia, rel, ib, rel_embs).double())
        Sh = dec.score_relations(x, ia, ib, rel_embs, direction="head")
        assert not torch.equal(Sh, St)
        for u in range(U):
            Qh = dec(x, ib, torch.full((B,), u, dtype=torch.int64, device=DEV), rel_embs, "head")
            value_check(f"head direction, column {u}", Sh[:, u], (Qh.double() * x[ia].double()).sum(-1))
        # negative ids wrap, int32 ids are accepted
        assert torch.equal(dec.score_relations(x, (ia - N).int(), ib.int(), rel_embs), St)
        # a generator that emits zeros: every relation scores as the dot product, so all columns are the same bits
        for head in dec.generator.generators.values():
            head[-1].weight.data.zero_()                                           # (its bias is zero from the start)
        S0 = dec.score_relations(x, ia, ib, rel_embs)
        assert torch.equal(S0, S0[:, :1].expand(-1, U))
        value_check("zero generator vs the dot product", S0[:, 0], (x[ia].double() * x[ib].double()).sum(-1))


# ---- 5. bad ids in the raw calls --------------------------------------------------------------------------------------------
def test_out_of_range_ids_give_nan_for_their_row_only():
    """The kernels test every id against its range before any address is formed from it (rp_sweep_kernel: rowa / rowb;
    rp_wgrad_kernel: ids): this checks the documented outcome, not whether such an id faults."""
    d, U = 64, 7
    x = rows(N, d, seed=13)
    W, b = weights(U, d, seed=14)
    ia, ib = pairs(seed=15)
    clean = _native.relation_scores(x, ia, ib, W, b)
    bad_a, bad_b = ia.clone(), ib.clone()
    bad_a[11], bad_a[12] = N, -1
    bad_b[70], bad_b[149] = N + 5, -(1 << 40)
    got = _native.relation_scores(x, bad_a, bad_b, W, b)
    torch.cuda.synchronize()
    bad = [11, 12, 70, 149]
    assert bool(torch.isnan(got[bad]).all())
    keep = torch.ones(B, dtype=torch.bool, device=DEV)
    keep[bad] = False
    assert torch.equal(got[keep], clean[keep])
    G = torch.randn(B, U, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    r_clean, r_bad = _native.relation_scores_bwd_rows(x, ia, G, W, b), _native.relation_scores_bwd_rows(x, bad_a, G, W, b)
    assert bool(torch.isnan(r_bad[[11, 12]]).all())
    keep_a = torch.ones(B, dtype=torch.bool, device=DEV)
    keep_a[[11, 12]] = False
    assert torch.equal(r_bad[keep_a], r_clean[keep_a])
    G0 = G.clone()
    G0[bad] = 0                                                                    # a bad pair adds nothing: as if its G were 0
    for g, w in zip(_native.relation_scores_bwd_weights(x, bad_a, bad_b, G), _native.relation_scores_bwd_weights(x, ia, ib, G0)):
        assert bool(torch.isfinite(g).all()) and torch.equal(g, w)


# ---- 6. capture -----------------------------------------------------------------------------------------------------------
def test_the_forward_call_is_capturable_into_a_hip_graph():
    d, U = 64, 37
    x = rows(N, d, seed=16)
    W, b = weights(U, d, seed=17)
    ia, ib = pairs(seed=18)
    out = torch.empty(B, U, device=DEV)
    call = lambda: _native.relation_scores(x, ia, ib, W, b, out=out)     # noqa: E731
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
    assert torch.equal(out, _native.relation_scores(x, ia, ib, W, b))


# ---- 7. gradients ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", (20, 128))
def test_gradients_match_float64_autograd_through_the_einsum(d):
    x = rows(N, d, seed=d + 2)
    for U in (7, 37):
        W, b = weights(U, d, seed=60 + d + U)
        G = torch.randn(B, U, device=DEV, generator=torch.Generator(device=DEV).manual_seed(d + U))
        for direction, (ia, ib) in (("tail", pairs(seed=70 + d)), ("head", pairs(seed=70 + d)[::-1])):
            def run():
                leaves = [t.clone().requires_grad_(True) for t in (x, W, b)]
                S = RelationScoresFn.apply(leaves[0], ia, ib, leaves[1], leaves[2])
                (S * G).sum().backward()
                return S.detach(), [t.grad for t in leaves]

            S, got = run()
            ref = [t.double().requires_grad_(True) for t in (x, W, b)]
            want = restate(ref[0], ia, ib, ref[1], ref[2])
            (want * G.double()).sum().backward()
            value_check(f"S (d={d} U={U} {direction})", S, want)
            for name, g, r in zip(("embs", "A", "b"), got, ref):
                grad_check(f"{name} (d={d} U={U} {direction})", g, r.grad)
            S2, got2 = run()
            assert torch.equal(S, S2)
            for g, g2 in zip(got, got2):
                assert torch.equal(g, g2)                                           # two backward runs: equal bits
    # only some inputs need a gradient
    ia, ib = pairs(seed=1)
    W, b = weights(7, d, seed=2)
    Wl = W.clone().requires_grad_(True)
    RelationScoresFn.apply(x, ia, ib, Wl, b).sum().backward()
    xl = x.clone().requires_grad_(True)
    RelationScoresFn.apply(xl, ia, ib, W, None).sum().backward()
    assert Wl.grad is not None and xl.grad is not None
    r = x.double().requires_grad_(True)
    restate(r, ia, ib, W, None).sum().backward()
    grad_check(f"embs, no bias (d={d})", xl.grad, r.grad)


# ---- 8. the methods -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("direction", ("tail", "head"))
def test_methods_are_the_helpers_on_the_table_and_the_brute_force_lists(direction):
    d, U = 20, 37
    dec, rel_embs = decoder(d, U, scale=3.0)
    embs = rows(N, d, seed=11)
    head, tail = pairs(seed=12)
    rel = torch.from_numpy(np.random.default_rng(13).integers(0, U, B)).to(DEV)
    known, lists, lists_all = known_triples(head, tail, rel, U, seed=14)
    assert any(lists) and lists != lists_all
    ptr, idx = csr(lists)
    ptr_a, idx_a = csr(lists_all)
    scale = d ** -0.5
    with torch.no_grad():
        S = dec.score_relations(embs, head, tail, rel_embs, direction=direction)
        heads = dec.generator(rel_embs)
    A = heads["W_msg" if direction == "tail" else "W_self"]
    ia, ib = (head, tail) if direction == "tail" else (tail, head)
    value_check(f"score_relations ({direction})", S, restate(embs, ia, ib, A, heads["bias"]))
    g, e = dec.rank_relations(embs, head, tail, rel, rel_embs, known=known, direction=direction)
    g_h, e_h = RelationDecoder._ranks_from_scores(S, rel, ptr, idx)
    assert g.dtype == torch.int64 and torch.equal(g, g_h) and torch.equal(e, e_h)
    g_c, e_c = RelationDecoder._ranks_from_scores(S.cpu(), rel.cpu(), ptr.cpu(), idx.cpu())        # the helpers run anywhere
    assert torch.equal(g.cpu(), g_c) and torch.equal(e.cpu(), e_c)
    g_u, _ = dec.rank_relations(embs, head, tail, rel, rel_embs, direction=direction)
    assert bool((g_u >= g).all()) and bool((g_u > g).any())                                         # the filter removes competitors
    m = link_prediction_metrics(g, e)
    assert 0.0 < m["mrr"] <= 1.0 and m["mean_rank"] >= 1.0
    s, i = dec.topk_relations(embs, head, tail, 10, rel_embs, known=known, direction=direction)
    s_h, i_h = RelationDecoder._topk_from_scores(S, 10, ptr_a, idx_a)
    assert torch.equal(s, s_h) and torch.equal(i, i_h) and s.shape == (B, 10)
    for q, row in enumerate(i.tolist()):
        assert not set(row) & set(lists_all[q]), f"pair {q}: a known relation among its top-k"
    assert bool((s[:, :-1] >= s[:, 1:]).all())
    s64, i64 = dec.topk_relations(embs, head, tail, 64, rel_embs, direction=direction)               # k > U: padding
    assert bool((i64[:, U:] == -1).all()) and bool(torch.isinf(s64[:, U:]).all()) and bool((i64[:, :U] >= 0).all())

    # the loss and its gradients against the float64 masked cross-entropy
    e32 = embs.clone().requires_grad_(True)
    dec.zero_grad(set_to_none=True)
    loss = dec.relation_loss(e32, head, tail, rel, rel_embs, scale=scale, known=known, direction=direction)
    gl = torch.rand(B, device=DEV, generator=torch.Generator(device=DEV).manual_seed(3)) + 0.5
    (loss * gl).sum().backward()
    e64, A64, b64 = embs.double().requires_grad_(True), A.double().requires_grad_(True), heads["bias"].double().requires_grad_(True)
    logits = scale * restate(e64, ia, ib, A64, b64)
    mask = RelationDecoder._list_mask(S, ptr, idx)
    want = F.cross_entropy(logits.masked_fill(mask, -np.inf), rel, reduction="none")
    (want * gl.double()).sum().backward()
    value_check(f"relation_loss ({direction})", loss, want)
    grad_check(f"relation_loss: embs ({direction})", e32.grad, e64.grad)
    assert torch.equal(loss.detach(), RelationDecoder._loss_from_scores(S, rel, ptr, idx, scale))
    used, unused = ("W_msg", "W_self") if direction == "tail" else ("W_self", "W_msg")
    for n, p in dec.generator.named_parameters():
        if f".{used}." in n or ".bias." in n:
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n
        if f".{unused}." in n:
            assert p.grad is None or not bool((p.grad != 0).any()), f"{n} belongs to the other direction"
    assert bool((dec.generator.generators[used][-1].weight.grad != 0).any())
    assert bool((dec.generator.generators["bias"][-1].weight.grad != 0).any())


def test_d_beyond_256_raises_with_the_library_message():
    dec, rel_embs = decoder(260, 3)
    embs = rows(64, 260, seed=1)
    ids = torch.arange(8, device=DEV)
    with pytest.raises(RuntimeError, match="exceeds 256"):
        dec.score_relations(embs, ids, ids + 1, rel_embs)


# ---- 9. end to end --------------------------------------------------------------------------------------------------------
def test_training_relation_prediction_with_an_unseen_text_end_to_end():
    kg = ToyKnowledgeGraph(feat_dim=16)
    x, ei = kg.node_features.to(DEV), kg.edge_index.to(DEV)
    rel_texts = kg.relation_types + ["is colleague of"]                  # the last one labels no edge of the graph
    edge_rel = torch.tensor([rel_texts.index(t) for t in kg.edge_texts], device=DEV)
    hidden = 16
    torch.manual_seed(0)
    model = HyperGNN(text_dim=32, node_feat_dim=16, hidden_dim=hidden).to(DEV)
    dec = RelationDecoder(text_dim=32, hidden_dim=hidden).to(DEV)
    known = (ei[0], ei[1], edge_rel)

    def step():
        embs = model(x, ei, kg.edge_texts)
        rel_embs = model.text_encoder(rel_texts, embs.device)
        return dec.relation_loss(embs, ei[0], ei[1], edge_rel, rel_embs, scale=hidden ** -0.5, known=known).mean()

    def usable(g):
        return g is not None and bool(torch.isfinite(g).all()) and bool((g != 0).any())

    step().backward()
    for n, p in model.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), f"{n} has no finite gradient"
    assert any(usable(p.grad) for n, p in model.named_parameters() if "text_encoder" not in n)
    for n, p in model.text_encoder.named_parameters():
        assert usable(p.grad), f"text encoder {n}"
    assert usable(dec.generator.generators["W_msg"][-1].weight.grad) and usable(dec.generator.generators["bias"][-1].weight.grad)

    model.zero_grad(set_to_none=True)
    dec.zero_grad(set_to_none=True)
    opt = torch.optim.Adam(list(model.parameters()) + list(dec.parameters()), lr=1e-3)
    losses = []
    for it in range(21):
        opt.zero_grad()
        loss = step()
        losses.append(loss.item())
        if it == 20:
            break
        loss.backward()
        opt.step()
    print("relation loss over 20 Adam steps:", " ".join(f"{l:.4f}" for l in losses[::4]))
    assert np.isfinite(losses).all() and losses[20] < losses[0], losses
    with torch.no_grad():
        embs = model(x, ei, kg.edge_texts)
        rel_embs = model.text_encoder(rel_texts, embs.device)
        g, e = dec.rank_relations(embs, ei[0], ei[1], edge_rel, rel_embs, known=known)
        s, i = dec.topk_relations(embs, ei[0], ei[1], 3, rel_embs)
    assert 0.0 < link_prediction_metrics(g, e)["mrr"] <= 1.0
    assert i.shape == (ei.size(1), 3) and bool((i >= 0).all()) and bool((i < len(rel_texts)).all())
