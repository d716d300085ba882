"""The softmax and the negative-sampling loss under a distance against every node or a shared candidate set
(include/ghf_distance_loss.h; HyperGNN.softmax_loss_by_distance / negative_sampling_loss_by_distance), restated in float64 on
the CPU.  The restatement is thin: the set P every query is scored against — all N nodes, or the candidates with the batch's
targets added, ascending — is repeated per query as its negatives, and tests/_distance_ref.loss does the rest: J_i (the listed
ids and the target leave), "the target exactly once", the detached weights, and the gradients written out.

Nothing here needs a GPU."""

from __future__ import annotations

from typing import Optional

import numpy as np
import torch

import _distance_ref as R


def candidate_set(N: int, target, cand=None) -> np.ndarray:
    """P, ascending node ids: every node, or `cand` (ids in any order) with the targets added."""
    if cand is None:
        return np.arange(N, dtype=np.int64)
    t = target.cpu().numpy() if isinstance(target, torch.Tensor) else np.asarray(target)
    c = cand.cpu().numpy() if isinstance(cand, torch.Tensor) else np.asarray(cand)
    return np.unique(np.concatenate([c.astype(np.int64), t.astype(np.int64)]))


def loss(mode: str, metric: str, rows, c, target, lists=None, cand=None, scale: float = 1.0, margin: float = 0.0,
         alpha: float = 0.0, grad: Optional[torch.Tensor] = None, add_targets: bool = True):
    """_distance_ref.loss's dict (loss, aux[, coef, dq [B, d], dc [N, d]]) for queries `rows` [B, d] against P.  `add_targets`
    False: P is `cand` as given (the C ABI adds nothing; a target outside P is then the caller's to exclude)."""
    N, B = c.size(0), rows.size(0)
    P = candidate_set(N, target, cand) if add_targets or cand is None else np.unique(np.asarray(cand, dtype=np.int64))
    neg = torch.from_numpy(P).unsqueeze(0).expand(B, len(P)).contiguous()
    return R.loss(mode, metric, rows, c, target, neg, lists, scale=scale, margin=margin, alpha=alpha, grad=grad)


embs_grad = R.embs_grad
