"""Pairwise ranking losses on per-query negative sets (include/ghf_pairwise.h; HyperGNN.pairwise_loss): the contract restated
in float64 torch on the CPU, autograd-able, a loop over the K positions (a position is a term, whatever id it holds).

    J_i  = { j : neg[i, j] != -1, neg[i, j] not in list_i, neg[i, j] != target[i] }          (tests/_negatives_ref.py)
    z_ij = scale q_i . c[n_ij] (+ bias[n_ij])  ("dot")   or   -scale D(q_i, c[n_ij])  ("l1", "l2", "complex": _distance_ref.dist)
    u_ij = z_ij - z_it + margin
    hinge: phi(u) = u where u > 0, else 0 (gradient 0 at the kink)        logistic: phi(u) = softplus(u)
    loss_i = (normalize ? 1 / |J_i| : 1) sum_{J_i} phi(u_ij), 0 where J_i is empty;   active_i = #{ j in J_i : u_ij > 0 }

The distances carry the stated zero conventions as their gradient (_Dist), not autograd's NaN at a zero root.  Also here: the
problems the GPU parity test runs (`problem`, SHAPES, SEEDS — the seeds picked on the CPU so that no pair of any problem lies
in the near-tie band, tests/test_pairwise_host.py holds them to it) and the documented order of the sum behind the target's
coefficient (`documented_row_sum`).  Nothing here needs a GPU."""

from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch

from _distance_ref import dist
from _negatives_ref import _softplus, live_positions

SCORES = ("dot", "l1", "l2", "complex")
KINDS = ("hinge", "logistic")


class _Dist(torch.autograd.Function):
    """D(x, y) of _distance_ref.dist with its stated gradient: g for x, -g for y, 0 where a denominator is 0."""

    @staticmethod
    def forward(ctx, x, y, metric):
        D, g = dist(metric, x, y)
        ctx.save_for_backward(g)
        return D

    @staticmethod
    def backward(ctx, gD):
        (g,) = ctx.saved_tensors
        t = gD.unsqueeze(-1) * g
        return t, -t, None


def _pair_score(score: str, x, y):
    return (x * y).sum(-1) if score == "dot" else -_Dist.apply(x, y, score)


def scores(score: str, q, c, target, neg, bias=None, scale: float = 1.0):
    """(z [B, K], z_t [B]) float64, position by position; q [B, d], c [N, d] (and bias [N]) float64, possibly leaves."""
    neg, target = neg.cpu().to(torch.int64), target.cpu().to(torch.int64)
    cols = []
    for j in range(neg.size(1)):
        ids = neg[:, j].clamp(min=0)
        z = scale * _pair_score(score, q, c[ids])
        cols.append(z if bias is None else z + bias[ids])
    zt = scale * _pair_score(score, q, c[target])
    return torch.stack(cols, 1), (zt if bias is None else zt + bias[target])


def loss(kind: str, score: str, q, c, target, neg, lists: Optional[Sequence] = None, bias=None, scale: float = 1.0,
         margin: float = 1.0, normalize: bool = True, grad: Optional[torch.Tensor] = None):
    """A dict of float64 CPU tensors: loss [B], count [B], active [B], u [B, K], live [B, K], zt [B]; with `grad` [B] also coef
    [B, K + 1] (the gradients with respect to the scores s, the target's last), dq [B, d] (per query), dc [N, d] and db [N]
    (zeros without a bias) by autograd of this very formulation."""
    assert kind in KINDS and score in SCORES
    q64 = q.detach().cpu().double().requires_grad_(grad is not None)
    c64 = c.detach().cpu().double().requires_grad_(grad is not None)
    b64 = None if bias is None else bias.detach().cpu().double().requires_grad_(grad is not None)
    z, zt = scores(score, q64, c64, target, neg, b64, scale)
    live = live_positions(neg, target, lists)
    u = z - zt.unsqueeze(1) + margin
    zero = torch.zeros_like(u)
    phi = torch.where(u > 0, u, zero) if kind == "hinge" else _softplus(u)
    n = live.sum(1)
    inv = torch.where(n > 0, 1.0 / n.clamp(min=1).double(), torch.zeros(len(n), dtype=torch.float64)) if normalize else \
        torch.ones(len(n), dtype=torch.float64)
    l = torch.where(live, phi, zero).sum(1) * inv
    out = dict(loss=l.detach(), count=n, active=((u > 0) & live).sum(1), u=u.detach(), live=live, zt=zt.detach())
    if grad is None:
        return out
    g = grad.detach().cpu().double()
    (l * g).sum().backward()
    dphi = (u > 0).double() if kind == "hinge" else torch.sigmoid(u)
    G = torch.where(live, (g * scale * inv).unsqueeze(1) * dphi.detach(), zero.detach())
    out.update(coef=torch.cat([G, -G.sum(1, keepdim=True)], 1), dq=q64.grad if q64.grad is not None else torch.zeros_like(q64),
               dc=c64.grad if c64.grad is not None else torch.zeros_like(c64),
               db=torch.zeros(c64.size(0), dtype=torch.float64) if b64 is None or b64.grad is None else b64.grad)
    return out


def embs_grad(out: dict, query: torch.Tensor) -> torch.Tensor:
    """d embs [N, d] of a call whose query rows are embs[query]: dc plus dq folded into the rows `query` names."""
    return out["dc"].clone().index_add_(0, query.cpu().to(torch.int64), out["dq"])


def kink_clear(score: str, q, c, target, neg, lists=None, bias=None, scale: float = 1.0, margin: float = 1.0):
    """(clear [B], zt [B]) float64: per query the smallest |u_ij| over all of J_i (inf where J_i is empty) — how far its
    nearest pair lies from the hinge's kink, which is also the line `active` counts across — and the target's z."""
    r = loss("hinge", score, q, c, target, neg, lists, bias, scale, margin)
    big = torch.full_like(r["u"], float("inf"))
    return torch.where(r["live"], r["u"].abs(), big).min(1).values, r["zt"]


def band(zt: torch.Tensor, margin: float) -> torch.Tensor:
    """The project's near-tie band (tests/test_distance_gpu.py) around the kink: 1e-4 (1 + |z_it| + |margin|)."""
    return 1e-4 * (1 + zt.abs() + abs(margin))


# ---- the problems of the GPU parity test ------------------------------------------------------------------------------------
# (d, K, B, N): every d of {1, 3, 20, 64, 128, 200, 256}, every K of {1, 7, 8, 9, 63, 64, 65, 256, 257, 1000} (256 | 257: the
# split of a query over four waves), B of {1, 5, 129}, N of {300, 5000}
SHAPES = [(1, 1, 1, 300), (1, 65, 5, 300), (3, 7, 5, 300), (3, 257, 5, 5000), (20, 8, 5, 300), (20, 63, 5, 5000), (20, 64, 5, 300),
          (20, 9, 129, 300), (20, 256, 5, 300), (20, 1000, 1, 300), (64, 9, 129, 300), (64, 63, 5, 300), (64, 65, 5, 5000),
          (64, 257, 5, 300), (128, 1, 1, 300), (128, 7, 129, 5000), (128, 8, 5, 300), (128, 65, 5, 300), (128, 256, 5, 300),
          (128, 257, 5, 300), (128, 1000, 5, 5000), (200, 9, 5, 300), (200, 65, 5, 300), (256, 7, 5, 300), (256, 8, 129, 300),
          (256, 257, 5, 5000), (256, 1000, 1, 300)]
VARIANTS = ("dot", "dot+bias", "l1", "l2", "complex")          # a problem per shape and variant; complex: even d only
MARGIN = 1.0


def variant_score(variant: str) -> str:
    return "dot" if variant.startswith("dot") else variant


def parity_scale(score: str, d: int) -> float:
    """Scores of order 1 whatever d: dot products of rows of norm ~ sqrt(d), distances that grow as d, sqrt(d), d / 2."""
    return {"dot": d ** -0.5, "l1": 1.0 / d, "l2": d ** -0.5, "complex": 2.0 / d}[score]


def problem(d: int, K: int, B: int, N: int, seed: int):
    """CPU tensors and lists: embs [N, d] fp32 (rows of mixed length, so that distances spread), query, target [B], neg [B, K]
    with padding, a repeat, the target and a listed id among the entries, the known edges (src, dst) and the per-query lists
    they make, a bias [N] and the loss's gradient [B]."""
    rng = np.random.default_rng(seed)
    embs = (rng.standard_normal((N, d)) * rng.uniform(0.3, 2.0, (N, 1))).astype(np.float32)
    query, target = rng.integers(0, N, B), rng.integers(0, N, B)
    neg = rng.integers(0, N, (B, K))
    neg[rng.random((B, K)) < 0.15] = -1
    E = 3 * B
    src, dst = query[rng.integers(0, B, E)], rng.integers(0, N, E)
    lists = [np.unique(dst[src == query[i]]) for i in range(B)]
    for i in range(B):
        if K >= 3:
            neg[i, K // 2] = neg[i, 0]                                      # a repeat
        if K >= 4 and i % 2 == 0:
            neg[i, K - 1] = target[i]                                       # the target among its own negatives
        if K >= 2 and len(lists[i]):
            neg[i, 1] = lists[i][0]                                         # a known partner
    t = torch.from_numpy
    return dict(embs=t(embs), query=t(query), target=t(target), neg=t(neg), known=(t(src), t(dst)), lists=lists,
                bias=t(rng.standard_normal(N).astype(np.float32)), grad=t(rng.standard_normal(B).astype(np.float32)))


# the seed of every (shape, variant): the first of base, base + 1, ... whose float64 reference keeps every pair outside the band
# (tools are not needed to re-derive them: tests/test_pairwise_host.py::test_no_parity_problem_has_a_pair_in_the_band checks
# each, and `pick_seed` below is the search)
SEEDS = {s: (1, 1, 1, 1, 1) for s in SHAPES}
SEEDS.update({(20, 63, 5, 5000): (1, 1, 1, 1, 2), (20, 256, 5, 300): (1, 2, 1, 1, 1), (64, 257, 5, 300): (1, 1, 2, 1, 1), (200, 65, 5, 300): (1, 2, 1, 1, 1), (256, 257, 5, 5000): (1, 2, 1, 1, 1)})


def pick_seed(shape, variant, base=0, tries=4000):
    d, K, B, N = shape
    score = variant_score(variant)
    for seed in range(base, base + tries):
        p = problem(d, K, B, N, seed)
        q = p["embs"][p["query"]]
        clear, zt = kink_clear(score, q, p["embs"], p["target"], p["neg"], p["lists"], p["bias"] if variant == "dot+bias" else None,
                               parity_scale(score, d), MARGIN)
        if bool((clear >= band(zt, MARGIN)).all()):
            return seed
    raise RuntimeError(f"no seed for {shape} {variant}")


def parity_cases():
    """[(shape, variant, seed)] of the GPU parity test."""
    return [(s, v, SEEDS[s][VARIANTS.index(v)]) for s in SHAPES for v in VARIANTS if v != "complex" or s[0] % 2 == 0]


# ---- the documented order of the sum behind coef[i, K] ----------------------------------------------------------------------
def documented_row_sum(row: np.ndarray, d: int, vector_path: bool) -> np.float32:
    """sum_j row[j] in fp32 in the order include/ghf_pairwise.h states for K = len(row): a group of L lanes adds its positions
    (every 64 / L-th, in steps of 8 x 64 / L dealt round-robin to four waves when K > 256) ascending, the groups merge by a
    butterfly, the waves' sums are added in wave order."""
    row = np.asarray(row, dtype=np.float32)
    K = len(row)
    L = 64 if not vector_path else (8 if d <= 32 else 16 if d <= 64 else 32 if d <= 128 else 64)
    G, W = 64 // L, (4 if K > 256 else 1)
    step = 8 * G
    waves = []
    for w in range(W):
        part = np.zeros(G, dtype=np.float32)
        for base in range(w * step, K, W * step):
            for u in range(8):
                for g in range(G):
                    j = base + u * G + g
                    if j < K:
                        part[g] = np.float32(part[g] + row[j])
        m = 1
        while m < G:                                                        # every group ends with the same bits
            part = np.array([np.float32(part[g] + part[g ^ m]) for g in range(G)], dtype=np.float32)
            m *= 2
        waves.append(part[0])
    total = waves[0]
    for w in range(1, W):
        total = np.float32(total + waves[w])
    return total
