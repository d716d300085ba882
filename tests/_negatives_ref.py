"""Per-query negative sets (include/ghf_negatives.h; HyperGNN.rank_candidates / softmax_loss / negative_sampling_loss with
negatives=): the contract restated in float64 torch on the CPU, from its formulas — no autograd (the detached weights of the
negative-sampling loss are stated, not inherited), a loop over the K positions, multiset semantics: a position is a term,
whatever id it holds.

    J_i = { j : neg[i, j] != -1, neg[i, j] not in list_i, neg[i, j] != target[i] }
    z_ij = scale q_i . c[neg[i, j]] (+ bias[neg[i, j]]),   z_it likewise from the target's row

Nothing here needs a GPU."""

from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch


def live_positions(neg: torch.Tensor, target: torch.Tensor, lists: Optional[Sequence]) -> torch.Tensor:
    """bool [B, K]: the positions in J_i."""
    neg, target = neg.cpu().to(torch.int64), target.cpu().to(torch.int64)
    live = (neg != -1) & (neg != target.unsqueeze(1))
    if lists is not None:
        for i, l in enumerate(lists):
            if len(l):
                live[i] &= ~torch.from_numpy(np.isin(neg[i].numpy(), np.asarray(l, dtype=np.int64)))
    return live


def scores(q: torch.Tensor, c: torch.Tensor, target: torch.Tensor, neg: torch.Tensor, bias: Optional[torch.Tensor] = None,
           scale: float = 1.0):
    """(z [B, K], z_t [B]) float64: scale q_i . c[row] + bias[row], position by position (0 at a padding position)."""
    q64, c64 = q.detach().cpu().double(), c.detach().cpu().double()
    b64 = None if bias is None else bias.detach().cpu().double()
    neg, target = neg.cpu().to(torch.int64), target.cpu().to(torch.int64)
    B, K = neg.shape
    z = torch.zeros(B, K, dtype=torch.float64)
    for j in range(K):
        ids = neg[:, j].clamp(min=0)
        z[:, j] = scale * (q64 * c64[ids]).sum(1) + (0.0 if b64 is None else b64[ids])
    zt = scale * (q64 * c64[target]).sum(1) + (0.0 if b64 is None else b64[target])
    return z, zt


def rank(q, c, target, neg, lists=None, bias=None):
    """(greater, equal) int64 [B]: scale 1, the bias one add."""
    z, zt = scores(q, c, target, neg, bias)
    live = live_positions(neg, target, lists)
    return ((z > zt.unsqueeze(1)) & live).sum(1), ((z == zt.unsqueeze(1)) & live).sum(1)


def _softplus(x):
    return torch.clamp(x, min=0) + torch.log1p(torch.exp(-x.abs()))


def loss(mode: str, q, c, target, neg, lists=None, bias=None, scale: float = 1.0, margin: float = 0.0, alpha: float = 0.0,
         grad: Optional[torch.Tensor] = None):
    """mode "softmax" or "negsamp".  A dict of float64 CPU tensors: loss [B], aux [B] (lse or lw), and with `grad` [B] also
    coef [B, K + 1], dq [B, d] (per query), dc [N, d] (the gradient of c by its own role: negative or target), db [N]."""
    z, zt = scores(q, c, target, neg, bias, scale)
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
    g = grad.detach().cpu().double() * scale
    if mode == "softmax":
        G = torch.where(live, g.unsqueeze(1) * torch.exp(z - aux.unsqueeze(1)), torch.zeros_like(z))
        Gt = g * (torch.exp(zt - aux) - 1.0)
    else:
        G = g.unsqueeze(1) * w * torch.sigmoid(z + margin)
        Gt = -g * torch.sigmoid(-(zt + margin))
    q64, c64 = q.detach().cpu().double(), c.detach().cpu().double()
    neg, target = neg.cpu().to(torch.int64), target.cpu().to(torch.int64)
    dq = Gt.unsqueeze(1) * c64[target]
    dc = torch.zeros_like(c64)
    db = torch.zeros(c64.size(0), dtype=torch.float64)
    for j in range(K):                                     # a term per POSITION: a repeated id gets one per occurrence
        ids = neg[:, j].clamp(min=0)
        dq += G[:, j].unsqueeze(1) * c64[ids]
        dc.index_add_(0, ids, G[:, j].unsqueeze(1) * q64)
        db.index_add_(0, ids, G[:, j] / scale)
    dc.index_add_(0, target, Gt.unsqueeze(1) * q64)
    db.index_add_(0, target, Gt / scale)
    out.update(coef=torch.cat([G, Gt.unsqueeze(1)], 1), dq=dq, dc=dc, db=db)
    return out


def embs_grad(out: dict, query: torch.Tensor) -> torch.Tensor:
    """d embs [N, d] of a call whose query rows are embs[query]: dc plus dq folded into the rows `query` names."""
    return out["dc"].clone().index_add_(0, query.cpu().to(torch.int64), out["dq"])
