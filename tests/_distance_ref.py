"""Distance scores for per-query negative sets (include/ghf_distance.h; HyperGNN.rank_candidates / softmax_loss /
negative_sampling_loss with negatives= and distance=): the contract restated in float64 torch on the CPU, from its formulas.
No autograd: the gradients of the three distances are written out, with their zero conventions as `where`, and the detached
weights of the negative-sampling loss are stated, not inherited.  A loop over the K positions; a position is a term, whatever
id it holds (tests/_negatives_ref.py, whose J_i this builds on).

    delta = q_i - c[v]
    "l1"       D = sum_k |delta_k|                        g_k = sign(delta_k), 0 at delta_k = 0
    "l2"       D = sqrt(sum_k delta_k^2)                  g_k = delta_k / D, all 0 where D = 0
    "complex"  D = sum_p sqrt(delta_2p^2 + delta_2p+1^2)  g_k = delta_k / rho_p, both 0 where rho_p = 0
    s = -D,  z = scale s

Nothing here needs a GPU."""

from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from _negatives_ref import _softplus, live_positions

METRICS = ("l1", "l2", "complex")


def dist(metric: str, x: torch.Tensor, y: torch.Tensor):
    """(D [...], g [..., d]) float64 for rows x, y [..., d]: the distance and its gradient with respect to x."""
    delta = x.double() - y.double()
    zero, one = torch.zeros_like(delta), torch.ones_like(delta)
    if metric == "l1":
        return delta.abs().sum(-1), torch.where(delta > 0, one, torch.where(delta < 0, -one, zero))
    if metric == "l2":
        D = torch.sqrt((delta * delta).sum(-1))
        den = torch.where(D > 0, D, torch.ones_like(D)).unsqueeze(-1)
        return D, torch.where(D.unsqueeze(-1) > 0, delta / den, zero)
    if metric == "complex":
        assert delta.size(-1) % 2 == 0, "complex: d must be even"
        pairs = delta.reshape(*delta.shape[:-1], -1, 2)
        rho = torch.sqrt((pairs * pairs).sum(-1))
        den = torch.where(rho > 0, rho, torch.ones_like(rho)).unsqueeze(-1)
        g = torch.where(rho.unsqueeze(-1) > 0, pairs / den, torch.zeros_like(pairs))
        return rho.sum(-1), g.reshape(delta.shape)
    raise ValueError(metric)


def distances(metric, q, c, target, neg):
    """(D [B, K], D_t [B]) float64, position by position (whatever row 0 gives at a padding position: it is never live)."""
    q64, c64 = q.detach().cpu().double(), c.detach().cpu().double()
    neg, target = neg.cpu().to(torch.int64), target.cpu().to(torch.int64)
    B, K = neg.shape
    D = torch.zeros(B, K, dtype=torch.float64)
    for j in range(K):
        D[:, j] = dist(metric, q64, c64[neg[:, j].clamp(min=0)])[0]
    return D, dist(metric, q64, c64[target])[0]


def rank(metric, q, c, target, neg, lists=None):
    """(greater, equal) int64 [B]: the positions of J_i whose score -D is above / equal to the target's."""
    D, Dt = distances(metric, q, c, target, neg)
    live = live_positions(neg, target, lists)
    return ((-D > -Dt.unsqueeze(1)) & live).sum(1), ((D == Dt.unsqueeze(1)) & live).sum(1)


def loss(mode: str, metric: str, q, c, target, neg, lists=None, scale: float = 1.0, margin: float = 0.0, alpha: float = 0.0,
         grad: Optional[torch.Tensor] = None):
    """mode "softmax" or "negsamp".  A dict of float64 CPU tensors: loss [B], aux [B] (lse or lw), and with `grad` [B] also
    coef [B, K + 1] (gradients with respect to s, the target's last), dq [B, d] (per query) and dc [N, d]."""
    D, Dt = distances(metric, q, c, target, neg)
    z, zt = -scale * D, -scale * Dt
    live = live_positions(neg, target, lists)
    B, K = z.shape
    ninf = torch.full_like(z, -np.inf)
    if mode == "softmax":
        aux = torch.logsumexp(torch.cat([zt.unsqueeze(1), torch.where(live, z, ninf)], 1), 1)
        out = {"loss": aux - zt, "aux": aux}
    else:
        aux = torch.logsumexp(torch.where(live, alpha * z, ninf), 1)                 # -inf where J_i is empty
        w = torch.where(live, torch.exp(alpha * z - torch.where(torch.isinf(aux), torch.zeros_like(aux), aux).unsqueeze(1)),
                        torch.zeros_like(z))
        out = {"loss": _softplus(-(zt + margin)) + (w * _softplus(z + margin)).sum(1), "aux": aux}
    if grad is None:
        return out
    gs = grad.detach().cpu().double() * scale
    if mode == "softmax":
        G = torch.where(live, gs.unsqueeze(1) * torch.exp(z - aux.unsqueeze(1)), torch.zeros_like(z))
        Gt = gs * (torch.exp(zt - aux) - 1.0)
    else:
        G = gs.unsqueeze(1) * w * torch.sigmoid(z + margin)
        Gt = -gs * torch.sigmoid(-(zt + margin))
    q64, c64 = q.detach().cpu().double(), c.detach().cpu().double()
    neg, target = neg.cpu().to(torch.int64), target.cpu().to(torch.int64)
    # s = -D: ds / dq = -g, ds / dc = +g
    dq = torch.zeros_like(q64)
    dc = torch.zeros_like(c64)
    for j in range(K):                                     # a term per POSITION: a repeated id gets one per occurrence
        ids = neg[:, j].clamp(min=0)
        term = G[:, j].unsqueeze(1) * dist(metric, q64, c64[ids])[1]
        term = torch.where(live[:, j].unsqueeze(1), term, torch.zeros_like(term))
        dq -= term
        dc.index_add_(0, ids, term)
    term = Gt.unsqueeze(1) * dist(metric, q64, c64[target])[1]
    dq -= term
    dc.index_add_(0, target, term)
    out.update(coef=torch.cat([G, Gt.unsqueeze(1)], 1), dq=dq, dc=dc)
    return out


def embs_grad(out: dict, query: torch.Tensor) -> torch.Tensor:
    """d embs [N, d] of a call whose query rows are embs[query]: dc plus dq folded into the rows `query` names."""
    return out["dc"].clone().index_add_(0, query.cpu().to(torch.int64), out["dq"])


def near_ties(metric, q, c, target, neg, lists=None):
    """(clear [B, K] bool, slack [B]): where float64 separates a position's score from the target's by more than
    1e-4 (1 + |t|), and per query the number of live positions where it does not — the cap of what a rank test may excuse."""
    D, Dt = distances(metric, q, c, target, neg)
    live = live_positions(neg, target, lists)
    clear = (D - Dt.unsqueeze(1)).abs() > 1e-4 * (1 + Dt.abs().unsqueeze(1))
    return clear, (~clear & live).sum(1)
