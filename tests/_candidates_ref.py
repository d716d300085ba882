"""A float64 numpy restatement of the sub-table rule of ``candidates=`` for the four all-node operations
and both gradients, on the float32 rows (as the ``reference()`` helpers of test_softmax_gpu / test_bce_gpu work).

With P the set of candidate node ids, a call gives what the all-node call gives on the table ``c[sorted(P)]``, except that
every id that goes in (target, lists) or comes out (top-k ids) is a row id of ``c``, list entries outside P take no part,
and gradients land in ``c``'s own rows (rows outside P: exactly zero).

Everything here is dense and takes numpy arrays: qrows [B, d] and c [N, d] float32, target [B] int, lists a sequence of B
id sequences (or None), P any sequence of node ids."""

import numpy as np


def candidate_set(P, N):
    """sorted distinct ids of P, negative ids wrapped"""
    P = np.asarray(P, dtype=np.int64)
    return np.unique(np.where(P < 0, P + N, P))


def softmax_set(P, target, N):
    """the set HyperGNN.softmax_loss sweeps: the candidates and the batch's targets"""
    return np.unique(np.concatenate([candidate_set(P, N), np.asarray(target, dtype=np.int64)]))


def _scores(qrows, c, P):
    return qrows.astype(np.float64) @ c[P].astype(np.float64).T


def _listed(lists, P, B):
    """[B, C] bool: candidate P[j] is on query i's list"""
    m = np.zeros((B, len(P)), dtype=bool)
    if lists is not None:
        for i, l in enumerate(lists):
            if len(l):
                m[i] = np.isin(P, np.asarray(l, dtype=np.int64))
    return m


def rank(qrows, c, target, lists, P):
    """(greater, equal) int64 [B] over j in P minus list_i minus {target_i}; the target is any row of c"""
    P = candidate_set(P, c.shape[0])
    target = np.asarray(target, dtype=np.int64)
    B = qrows.shape[0]
    S = _scores(qrows, c, P)
    t = np.einsum("ik,ik->i", qrows.astype(np.float64), c[target].astype(np.float64))
    out = _listed(lists, P, B) | (P[None, :] == target[:, None])
    return ((S > t[:, None]) & ~out).sum(1).astype(np.int64), ((S == t[:, None]) & ~out).sum(1).astype(np.int64)


def topk(qrows, c, lists, P, k):
    """(scores [B, k] descending, ids [B, k] node ids): the k best of P minus list_i, ties to the lower id, (-inf, -1) pads"""
    P = candidate_set(P, c.shape[0])
    B = qrows.shape[0]
    S = _scores(qrows, c, P)
    out = _listed(lists, P, B)
    scores = np.full((B, k), -np.inf)
    ids = np.full((B, k), -1, dtype=np.int64)
    for i in range(B):
        keep = np.nonzero(~out[i])[0]
        order = keep[np.lexsort((P[keep], -S[i, keep]))][:k]
        scores[i, :len(order)] = S[i, order]
        ids[i, :len(order)] = P[order]
    return scores, ids


def softmax(qrows, c, target, lists, P, scale, grad=None):
    """(loss, lse[, dq, dc]) with J_i = (P minus list_i) plus {target_i}.  A target outside P: NaN for that query, which then
    takes no part in the gradients (the C ABI's rule; HyperGNN.softmax_loss sweeps softmax_set).  dc is [N, d]."""
    N = c.shape[0]
    P = candidate_set(P, N)
    target = np.asarray(target, dtype=np.int64)
    B = qrows.shape[0]
    S = scale * _scores(qrows, c, P)
    is_t = P[None, :] == target[:, None]
    ok = is_t.any(1)
    mask = _listed(lists, P, B) & ~is_t
    Z = np.where(mask, -np.inf, S)
    m = Z.max(1)
    lse = m + np.log(np.exp(Z - m[:, None]).sum(1))
    # the target's logit is the matrix's own entry (one per row: P holds no id twice), so that at C = 1 the loss is exactly 0
    # and not the difference of two roundings of the same dot product
    t = np.where(is_t, S, 0.0).sum(1)
    lse = np.where(ok, lse, np.nan)
    loss = lse - t
    if grad is None:
        return loss, lse
    with np.errstate(invalid="ignore"):
        p = np.exp(Z - lse[:, None])
    G = np.asarray(grad, dtype=np.float64)[:, None] * scale * (p - is_t)
    G[~ok] = 0.0
    dq = G @ c[P].astype(np.float64)
    dc = np.zeros((N, c.shape[1]))
    dc[P] = G.T @ qrows.astype(np.float64)
    return loss, lse, dq, dc


def bce(qrows, c, lists, P, scale, smoothing, grad=None):
    """(loss[, dq, dc]): the SUM over j in P of bce_with_logits(z_ij, y_ij), y_ij = (1 - smoothing) [P_j listed] +
    smoothing / C; listed ids outside P take no part.  dc is [N, d]."""
    N = c.shape[0]
    P = candidate_set(P, N)
    B, C = qrows.shape[0], len(P)
    Z = scale * _scores(qrows, c, P)
    Y = (1.0 - smoothing) * _listed(lists, P, B) + smoothing / C
    loss = (np.maximum(Z, 0) + np.log1p(np.exp(-np.abs(Z))) - Y * Z).sum(1)
    if grad is None:
        return loss
    sig = np.where(Z >= 0, 1.0 / (1.0 + np.exp(-np.abs(Z))), np.exp(-np.abs(Z)) / (1.0 + np.exp(-np.abs(Z))))
    G = np.asarray(grad, dtype=np.float64)[:, None] * scale * (sig - Y)
    dq = G @ c[P].astype(np.float64)
    dc = np.zeros((N, c.shape[1]))
    dc[P] = G.T @ qrows.astype(np.float64)
    return loss, dq, dc


def renumber(lists, target, P, N):
    """What a caller of the all-node entry points has to do by hand to run them on the copy c[P]: lists cut down to P and
    renumbered to positions, targets as positions (-1: not in P)."""
    P = candidate_set(P, N)
    pos = np.full(N, -1, dtype=np.int64)
    pos[P] = np.arange(len(P))
    new_lists = None
    if lists is not None:
        new_lists = []
        for l in lists:
            l = pos[np.asarray(l, dtype=np.int64)] if len(l) else np.zeros(0, dtype=np.int64)
            new_lists.append(l[l >= 0])
    new_target = None if target is None else pos[np.asarray(target, dtype=np.int64)]
    return new_lists, new_target
