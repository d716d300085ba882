"""Distance scores against every node or a candidate subset (include/ghf_distance_sweep.h; HyperGNN.rank_by_distance /
topk_by_distance): the contract restated in float64 numpy on the CPU, from its formulas, one query at a time so that nothing
of size [B, N, d] is built.

    s(i, j) = -D(row_i, c[j]),  D as tests/_distance_ref.dist states it
    rank:   greater[i] = #{ j allowed : s(i, j) > t_i },  equal[i] likewise with ==,  t_i = s(i, target[i])
    top-k:  the k allowed j of largest s, ties towards the lower id, (-inf, -1) behind the last
    allowed = the candidates (every node without a subset) minus the query's list, and for the rank minus the target

and the rounding bound of one fp32 distance, eps = (d + 8) 2^-24 D: one rounding per difference, at most d - 1 per sum in any
order, at most 4 for a square, product and root, the root's 1 ulp.  l1_chain32 is the stated L1 chain in numpy float32, every
operation a single IEEE rounding.  Nothing here needs a GPU."""

from __future__ import annotations

import numpy as np
import torch

from _distance_ref import dist

U = 2.0 ** -24


def distances(metric: str, rows, c) -> np.ndarray:
    """D [B, N] float64 of fp32 rows [B, d] against c [N, d], a query at a time."""
    rows, c = torch.as_tensor(rows).detach().cpu(), torch.as_tensor(c).detach().cpu()
    out = np.empty((rows.size(0), c.size(0)), dtype=np.float64)
    for i in range(rows.size(0)):
        out[i] = dist(metric, rows[i].unsqueeze(0), c)[0].numpy()
    return out


def eps(D: np.ndarray, d: int) -> np.ndarray:
    return (d + 8) * U * D


def allowed(N: int, lists, i: int, target=None, cand=None) -> np.ndarray:
    m = np.ones(N, dtype=bool)
    if cand is not None:
        m[:] = False
        m[np.asarray(cand, dtype=np.int64)] = True
    if lists is not None and len(lists[i]):
        m[np.asarray(lists[i], dtype=np.int64)] = False
    if target is not None:
        m[target[i]] = False
    return m


def rank(D: np.ndarray, target, lists=None, cand=None):
    """(greater, equal) int64 [B] of the distances D [B, N]."""
    B, N = D.shape
    g, e = np.zeros(B, dtype=np.int64), np.zeros(B, dtype=np.int64)
    for i in range(B):
        m = allowed(N, lists, i, target, cand)
        t = -D[i, target[i]]
        g[i], e[i] = np.count_nonzero(-D[i][m] > t), np.count_nonzero(-D[i][m] == t)
    return g, e


def topk(D: np.ndarray, k: int, lists=None, cand=None):
    """(scores [B, k] float64 = -D, ids [B, k] int64)."""
    B, N = D.shape
    sc, ids = np.full((B, k), -np.inf), np.full((B, k), -1, dtype=np.int64)
    for i in range(B):
        c = np.nonzero(allowed(N, lists, i, None, cand))[0]
        order = c[np.lexsort((c, D[i, c]))][:k]
        sc[i, :len(order)], ids[i, :len(order)] = -D[i, order], order
    return sc, ids


def l1_chain32(rows: np.ndarray, c: np.ndarray) -> np.ndarray:
    """The stated L1 chain in float32: acc = acc + |q_k - c_k|, k ascending from 0; [B, N] float32."""
    rows, c = np.ascontiguousarray(rows, dtype=np.float32), np.ascontiguousarray(c, dtype=np.float32)
    acc = np.zeros((rows.shape[0], c.shape[0]), dtype=np.float32)
    for k in range(rows.shape[1]):
        delta = rows[:, k, None] - c[None, :, k]                     # one fp32 subtraction
        acc = acc + np.abs(delta)                                    # one fp32 addition
        assert delta.dtype == np.float32 and acc.dtype == np.float32
    return acc


def exact_rows(N: int, d: int, seed: int, metric: str) -> np.ndarray:
    """test_rank_gpu.exact_rows — multiples of 2^-6 in [-4, 4], the last 500 rows copies of the first 500 — and for "complex"
    one member of every (re, im) pair zeroed in all rows, so that a pair's difference lies on an axis and its modulus is the
    root of a perfect square."""
    g = np.random.default_rng(seed).standard_normal((N, d))
    c = np.clip(np.round(64 * g) / 64, -4, 4).astype(np.float32)
    if metric == "complex":
        axis = np.random.default_rng(seed + 1).integers(0, 2, d // 2)
        c[:, 2 * np.arange(d // 2) + axis] = 0.0
    c[-500:] = c[:500]
    return c
