"""A float64 numpy restatement of ``candidate_bias=`` for the four all-node operations and the three
gradients, on the float32 rows and the float32 bias, with and without a candidate subset (tests/_candidates_ref.py states the
sub-table rule this builds on).

``bias`` is [N], one entry per NODE, also when P is given.  With s(i, j) = q_i . c_j:

  rank, top-k     s_b(i, j) = s(i, j) + bias[j]; the target's score the same way from its own row and entry, a candidate or not
  softmax, bce    z_ij = scale s(i, j) + bias[j] (the bias is not scaled) wherever the unbiased rule has scale s(i, j)
  gradients       G_ij = grad_i scale (p_ij - [j = target_i])  /  grad_i scale (sigma(z_ij) - y_ij), dq = G c, dc = G^T q as
                  before, and db[j] = sum_i G_ij / scale; dc and db are [N], zero outside P
  -inf            a candidate whose entry is -inf (and that is no query's target) is gone: in neither rank count, never among
                  the top k, a zero term of the softmax with zero gradients

Everything is dense and takes numpy arrays: qrows [B, d], c [N, d], bias [N] float32, target [B] int, lists a sequence of B id
sequences (or None), P any sequence of node ids or None for every node."""

import numpy as np

from _candidates_ref import _listed, candidate_set


def _set(P, N):
    return np.arange(N, dtype=np.int64) if P is None else candidate_set(P, N)


def _scores(qrows, c, P):
    return qrows.astype(np.float64) @ c[P].astype(np.float64).T


def rank(qrows, c, bias, target, lists, P=None):
    """(greater, equal) int64 [B] over j in P minus list_i minus {target_i}, on the biased scores"""
    P = _set(P, c.shape[0])
    b = bias.astype(np.float64)
    target = np.asarray(target, dtype=np.int64)
    S = _scores(qrows, c, P) + b[P][None, :]
    t = np.einsum("ik,ik->i", qrows.astype(np.float64), c[target].astype(np.float64)) + b[target]
    out = _listed(lists, P, qrows.shape[0]) | (P[None, :] == target[:, None])
    return ((S > t[:, None]) & ~out).sum(1).astype(np.int64), ((S == t[:, None]) & ~out).sum(1).astype(np.int64)


def topk(qrows, c, bias, lists, P, k):
    """(scores [B, k] descending, ids [B, k] node ids): the k best biased scores of P minus list_i, ties to the lower id,
    (-inf, -1) pads; a candidate at -inf is never returned"""
    P = _set(P, c.shape[0])
    B = qrows.shape[0]
    S = _scores(qrows, c, P) + bias.astype(np.float64)[P][None, :]
    out = _listed(lists, P, B) | np.isneginf(S)
    scores = np.full((B, k), -np.inf)
    ids = np.full((B, k), -1, dtype=np.int64)
    for i in range(B):
        keep = np.nonzero(~out[i])[0]
        order = keep[np.lexsort((P[keep], -S[i, keep]))][:k]
        scores[i, :len(order)] = S[i, order]
        ids[i, :len(order)] = P[order]
    return scores, ids


def softmax(qrows, c, bias, target, lists, P, scale, grad=None):
    """(loss, lse[, dq, dc, db]) with J_i = (P minus list_i) plus {target_i} and z = scale s + bias.  A target outside P: NaN
    for that query, which takes no part in the gradients.  dc is [N, d], db [N]."""
    N = c.shape[0]
    P = _set(P, N)
    target = np.asarray(target, dtype=np.int64)
    B = qrows.shape[0]
    S = scale * _scores(qrows, c, P) + bias.astype(np.float64)[P][None, :]
    is_t = P[None, :] == target[:, None]
    ok = is_t.any(1)
    mask = _listed(lists, P, B) & ~is_t
    Z = np.where(mask, -np.inf, S)
    m = Z.max(1)
    with np.errstate(invalid="ignore"):
        lse = m + np.log(np.exp(Z - m[:, None]).sum(1))
    t = np.where(is_t, S, 0.0).sum(1)
    lse = np.where(ok, lse, np.nan)
    loss = lse - t
    if grad is None:
        return loss, lse
    with np.errstate(invalid="ignore"):
        p = np.exp(Z - lse[:, None])
    D = np.asarray(grad, dtype=np.float64)[:, None] * (p - is_t)             # d loss / d z, weighted
    D[~ok] = 0.0
    dq = scale * (D @ c[P].astype(np.float64))
    dc = np.zeros((N, c.shape[1]))
    dc[P] = scale * (D.T @ qrows.astype(np.float64))
    db = np.zeros(N)
    db[P] = D.sum(0)
    return loss, lse, dq, dc, db


def bce(qrows, c, bias, lists, P, scale, smoothing, grad=None):
    """(loss[, dq, dc, db]): the SUM over j in P of bce_with_logits(z_ij, y_ij), z = scale s + bias (finite), y_ij =
    (1 - smoothing) [P_j listed] + smoothing / C.  dc is [N, d], db [N]."""
    N = c.shape[0]
    P = _set(P, N)
    B, C = qrows.shape[0], len(P)
    Z = scale * _scores(qrows, c, P) + bias.astype(np.float64)[P][None, :]
    Y = (1.0 - smoothing) * _listed(lists, P, B) + smoothing / C
    loss = (np.maximum(Z, 0) + np.log1p(np.exp(-np.abs(Z))) - Y * Z).sum(1)
    if grad is None:
        return loss
    e = np.exp(-np.abs(Z))
    sig = np.where(Z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
    D = np.asarray(grad, dtype=np.float64)[:, None] * (sig - Y)
    dq = scale * (D @ c[P].astype(np.float64))
    dc = np.zeros((N, c.shape[1]))
    dc[P] = scale * (D.T @ qrows.astype(np.float64))
    db = np.zeros(N)
    db[P] = D.sum(0)
    return loss, dq, dc, db


def exact_bias(N, seed):
    """multiples of 1/64 in [-32, 32], the last entries copies of the first (as test_candidates_gpu.exact_rows copies rows: the
    copies keep their ties), every seventh entry zero"""
    g = np.random.default_rng(seed).standard_normal(N)
    b = np.clip(np.round(512 * g) / 64, -32, 32).astype(np.float32)
    k = min(500, N // 3)
    if k:
        b[-k:] = b[:k]
    b[::7] = 0.0
    return b
