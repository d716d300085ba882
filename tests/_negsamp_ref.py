"""The float64 restatement of the negative-sampling loss with self-adversarial weighting (include/ghf.h:
ghf_score_negsamp_fwd / _bwd), written out from its formulas: no autograd, so that the weights being constants is stated, not
inherited.  tests/test_negsamp_host.py checks it against an independently written PyKEEN-style autograd formulation."""

import numpy as np
import torch


def softplus64(x):
    return torch.logaddexp(x, torch.zeros_like(x))


def negsamp_reference(qrows, c, target, lists=None, scale=1.0, margin=0.0, alpha=0.0, grad=None, ic=None, bias=None):
    """float64 (loss [B], lw [B], dq [B, d], dc [M, d], db [M]) for gathered query rows `qrows` [B, d], the table `c` [N, d],
    node-id targets and per-query lists of node ids; `ic` (node ids, any order-preserving tensor) is the candidate set P, M its
    size (M = N without).  z = scale q . c[j] + bias[j]; J_i = P minus list_i minus target_i; the weights are constants in the
    backward.  A query whose target is not in P (or is outside [0, N)) has loss = lw = NaN and zero gradients; an empty J_i gives
    lw = -inf and the positive term alone.  Without `grad` the three gradients are None."""
    dev = c.device
    B, N = qrows.size(0), c.size(0)
    q = qrows.detach().double()
    P = torch.arange(N, device=dev) if ic is None else torch.as_tensor(ic, device=dev).long()
    cp = c.detach().double()[P]
    z = scale * (q @ cp.T)
    if bias is not None:
        z = z + bias.detach().double()[P][None, :]
    target = torch.as_tensor(target, device=dev).long()
    is_t = P[None, :] == target[:, None]                                 # [B, M]
    valid = is_t.any(1)
    neg = ~is_t
    if lists is not None:
        for i, l in enumerate(lists):
            if len(l):
                neg[i] &= ~torch.isin(P, torch.as_tensor(np.asarray(l, dtype=np.int64), device=dev))
    az = (alpha * z).masked_fill(~neg, -np.inf)
    lw = torch.logsumexp(az, 1)                                          # -inf where J is empty
    some = torch.isfinite(lw)
    w = torch.where(neg & some[:, None], torch.exp(az - torch.where(some, lw, torch.zeros_like(lw))[:, None]), torch.zeros_like(z))
    zt = (z * is_t).sum(1)
    loss = softplus64(-(zt + margin)) + (w * softplus64(z + margin)).sum(1)
    nan = torch.full_like(loss, float("nan"))
    loss, lw = torch.where(valid, loss, nan), torch.where(valid, lw, nan)
    if grad is None:
        return loss, lw, None, None, None
    gs = (grad.detach().double() * scale)[:, None]
    G = gs * w * torch.sigmoid(z + margin)                               # the negatives; 0 at listed candidates and at the target
    G = torch.where(is_t, -gs * torch.sigmoid(-(zt + margin))[:, None], G)
    G = torch.where(valid[:, None], G, torch.zeros_like(G))
    return loss, lw, G @ cp, G.T @ q, G.sum(0) / scale
