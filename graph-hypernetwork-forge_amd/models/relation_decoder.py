"""RelationDecoder — relation-typed link-prediction scores, the hypernetwork way.

No counterpart in the reference, whose ``score_triple`` (models/hypergnn.py:304-318) is a relation-blind dot product.
Here the relation's scoring matrix is GENERATED from the relation's text, as the layers' weights are, so a relation never
seen in training scores with no retraining.  For a relation with text embedding ``z_r`` let ``(A_r, A'_r, b_r)`` be the
heads ``("W_msg", "W_self", "bias")`` of one ``WeightGenerator``; with ``x = embs``:

    direction="tail", (h, r, ?):   Q_i = x[h_i] + x[h_i] @ A_{r_i}  + b_{r_i},     s(i, j) = Q_i . x[j]
    direction="head", (?, r, t):   Q_i = x[t_i] + x[t_i] @ A'_{r_i} + b_{r_i}      (the reciprocal relation has its own matrix)

The residual makes a fresh decoder (``init_scale = 0.01``) score almost exactly as the dot product: a model trained
relation-blind keeps its behaviour and learns the relation-specific deviation from there.  ``Q`` is what the sweeps of
``HyperGNN.rank_candidates / topk_candidates / softmax_loss`` take as ``query_rows``.  The rows are built by one kernel
(``ghf_relation_rows``, csrc/relation.hip) that indexes ``A[r]`` in place: the ``[B, d, d]`` operand of
``torch.bmm(embs[h].unsqueeze(1), A[rel])`` does not exist, forward or backward.
"""

from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn

from .. import _native
from .hypergnn import HyperGNN
from .weight_generator import WeightGenerator

DIRECTIONS = {"tail": 0, "head": 1}       # the generator head that holds the direction's matrix (W_msg / W_self)


class RelationDecoder(nn.Module):
    """``dec(embs, nodes, rel, rel_embs, direction)`` -> the transformed query rows ``[B, d]``; ``dec.score`` -> pair scores.

    A module of its own on purpose: ``HyperGNN``'s constructor, parameter draws, ``state_dict`` keys and
    ``num_parameters()`` do not change.  The generator is sized as ``HyperGNN`` sizes its layers' generators."""

    def __init__(self, text_dim: int, hidden_dim: int, gen_hidden_dim: Optional[int] = None, num_hidden: int = 2,
                 dropout: float = 0.0, init_scale: float = 0.01) -> None:
        super().__init__()
        self.text_dim, self.hidden_dim = text_dim, hidden_dim
        self.generator = WeightGenerator(text_dim, hidden_dim, hidden_dim, hidden_dim=gen_hidden_dim or max(64, 2 * text_dim),
                                         num_hidden=num_hidden, dropout=dropout, init_scale=init_scale)

    def forward(self, embs: torch.Tensor, nodes: torch.Tensor, rel: torch.Tensor, rel_embs: torch.Tensor,
                direction: str = "tail") -> torch.Tensor:
        """``nodes`` int ids ``[B]`` into ``embs`` (the heads for "tail", the tails for "head"; negative ids wrap), ``rel``
        int ids ``[B]`` into ``rel_embs [U, text_dim]`` (``model.text_encoder(rel_texts, device)``: any texts, seen in the
        graph or not).  fp32 ``[B, d]``.  Recorded for autograd when grad mode is on and anything upstream requires grad; in
        training mode with ``dropout > 0`` the generator draws its masks."""
        if direction not in DIRECTIONS:
            raise ValueError(f"direction must be 'tail' or 'head', got {direction!r}")
        for name, t in (("embs", embs), ("rel_embs", rel_embs)):
            if not isinstance(t, torch.Tensor) or not t.is_cuda:
                raise RuntimeError(f"RelationDecoder computes on an MI355X HIP device only ({name} is on "
                                   f"{getattr(t, 'device', type(t))}); this package has no CPU or eager-PyTorch fallback")
        if embs.dim() != 2 or embs.size(1) != self.hidden_dim:
            raise ValueError(f"embs must be [N, {self.hidden_dim}], got {tuple(embs.shape)}")
        if rel_embs.dim() != 2 or rel_embs.size(1) != self.text_dim or rel_embs.size(0) == 0:
            raise ValueError(f"rel_embs must be [U, {self.text_dim}], got {tuple(rel_embs.shape)}")
        ix = HyperGNN._rank_ids(nodes, embs.size(0), embs, "nodes")
        r = HyperGNN._rank_ids(rel, rel_embs.size(0), embs, "rel")
        if ix.numel() != r.numel() or ix.numel() == 0:
            raise ValueError(f"{ix.numel()} nodes and {r.numel()} relation ids")
        heads = self.generator(rel_embs)                     # records WeightGeneratorFn when gradients are wanted
        A, b = heads[("W_msg", "W_self")[DIRECTIONS[direction]]], heads["bias"]
        if torch.is_grad_enabled() and (embs.requires_grad or A.requires_grad or b.requires_grad):
            from ..autograd import RelationRowsFn
            return RelationRowsFn.apply(embs, ix, r, A, b)
        return _native.relation_rows(embs.detach().float(), r, A.detach(), b.detach(), ix=ix, add_x=True)

    def score(self, embs: torch.Tensor, head: torch.Tensor, rel: torch.Tensor, tail: torch.Tensor,
              rel_embs: torch.Tensor) -> torch.Tensor:
        """``s_i = Q_i . embs[tail_i]`` with ``Q = self(embs, head, rel, rel_embs, "tail")``: the score of the triples
        ``(head_i, rel_i, tail_i)``, fp32 ``[B]``.  Gradients (to the decoder, the text encoder and ``embs``) are
        bit-reproducible: per-node sums in a fixed order, no atomics."""
        Q = self(embs, head, rel, rel_embs, direction="tail")
        t = HyperGNN._rank_ids(tail, embs.size(0), embs, "tail")
        if t.numel() != Q.size(0):
            raise ValueError(f"{Q.size(0)} heads and {t.numel()} tails")
        if torch.is_grad_enabled() and (Q.requires_grad or embs.requires_grad):
            from ..autograd import ScoreRowsFn
            return ScoreRowsFn.apply(Q, embs, t)
        return _native.score_pairs_fwd(Q, embs.detach().float(), None, t)

    def num_parameters(self) -> int:
        return sum(p.numel() for p in self.parameters() if p.requires_grad)
