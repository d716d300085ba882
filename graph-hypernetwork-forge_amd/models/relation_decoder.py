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

Relation prediction, (h, ?, t) — which relation holds between two given nodes: ``score_relations`` gives
``S[i, u] = (x[h_i] + x[h_i] @ A_u + b_u) . x[t_i]`` for EVERY relation text u in one sweep (``ghf_relation_scores``,
csrc/relation_predict.hip) that writes only the ``[B, U]`` table; ``rank_relations``, ``topk_relations`` and ``relation_loss``
are tensor operations over that small table, with the other relations known for a directed pair filtered out.
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
        self._check_inputs(embs, rel_embs, direction)
        ix = HyperGNN._rank_ids(nodes, embs.size(0), embs, "nodes")
        r = HyperGNN._rank_ids(rel, rel_embs.size(0), embs, "rel")
        if ix.numel() != r.numel() or ix.numel() == 0:
            raise ValueError(f"{ix.numel()} nodes and {r.numel()} relation ids")
        self._device_only(embs, rel_embs, "forward")
        return self._generated(embs, rel_embs, direction, "RelationRowsFn", (ix, r),
                               lambda x, A, b: _native.relation_rows(x, r, A, b, ix=ix, add_x=True))

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

    # -- the checks and the generated (A, b) that every method shares -----------------------------------------------------------
    def _check_inputs(self, embs, rel_embs, direction):
        """What every method tests first, cheapest first: the direction and the two shapes."""
        if direction not in DIRECTIONS:
            raise ValueError(f"direction must be 'tail' or 'head', got {direction!r}")
        if not isinstance(embs, torch.Tensor) or embs.dim() != 2 or embs.size(1) != self.hidden_dim:
            raise ValueError(f"embs must be [N, {self.hidden_dim}], got {getattr(embs, 'shape', type(embs))}")
        if not isinstance(rel_embs, torch.Tensor) or rel_embs.dim() != 2 or rel_embs.size(1) != self.text_dim or rel_embs.size(0) == 0:
            raise ValueError(f"rel_embs must be [U, {self.text_dim}], got {getattr(rel_embs, 'shape', type(rel_embs))}")

    @staticmethod
    def _device_only(embs, rel_embs, what):
        for name, t in (("embs", embs), ("rel_embs", rel_embs)):
            if not t.is_cuda:
                raise RuntimeError(f"RelationDecoder.{what} computes on an MI355X HIP device only ({name} is on {t.device}); "
                                   "this package has no CPU or eager-PyTorch fallback")

    @staticmethod
    def _check_known(known):
        if known is not None and len(known) != 3:
            raise ValueError(f"known must be (src, dst, rel), got {len(known)} members")

    def _generated(self, embs, rel_embs, direction, recorded, ids, raw):
        """The direction's ``(A, b)`` from the generator, then the autograd function named ``recorded`` when gradients are
        wanted and the ``raw`` call otherwise."""
        heads = self.generator(rel_embs)                     # records WeightGeneratorFn when gradients are wanted
        A, b = heads[("W_msg", "W_self")[DIRECTIONS[direction]]], heads["bias"]
        if torch.is_grad_enabled() and (embs.requires_grad or A.requires_grad or b.requires_grad):
            from .. import autograd
            return getattr(autograd, recorded).apply(embs, *ids, A, b)
        return raw(embs.detach().float(), A.detach(), b.detach())

    # -- relation prediction: which relation holds between two given nodes, (head, ?, tail) (csrc/relation_predict.hip) --------
    def _pair_ids(self, embs, head, tail, rel_embs, direction, what, *rel, known=None):
        """The checks every relation-prediction method shares, the device last; ``(head, tail, rel)`` int64 on embs' device
        (``rel``: the target texts of the methods that take them, else None)."""
        self._check_inputs(embs, rel_embs, direction)
        h = HyperGNN._rank_ids(head, embs.size(0), embs, "head")
        t = HyperGNN._rank_ids(tail, embs.size(0), embs, "tail")
        if h.numel() != t.numel() or h.numel() == 0:
            raise ValueError(f"{what}: {h.numel()} heads and {t.numel()} tails")
        r = None
        if rel:
            r, U = HyperGNN._rel_ids(rel[0], h.numel(), embs, "rel"), rel_embs.size(0)
            if r.numel() and int(r.max()) >= U:
                raise IndexError(f"rel holds ids outside [0, {U}): the rows of rel_embs")
        self._check_known(known)
        self._device_only(embs, rel_embs, what)
        return h, t, r

    def _score_table(self, embs, h, t, rel_embs, direction):
        ia, ib = (h, t) if direction == "tail" else (t, h)
        return self._generated(embs, rel_embs, direction, "RelationScoresFn", (ia, ib),
                               lambda x, A, b: _native.relation_scores(x, ia, ib, A, b, add_x=True))

    def score_relations(self, embs: torch.Tensor, head: torch.Tensor, tail: torch.Tensor, rel_embs: torch.Tensor,
                        direction: str = "tail") -> torch.Tensor:
        """``S[i, u]`` = the score of the triple ``(head_i, text u, tail_i)`` for EVERY row ``u`` of ``rel_embs [U, text_dim]``
        (any texts, seen in the graph or not), fp32 ``[B, U]``.  ``direction="tail"``: ``(x[h] + x[h] @ A_u + b_u) . x[t]``, the
        score ``dec.score`` gives; ``"head"``: the reciprocal matrix with the roles swapped, ``(x[t] + x[t] @ A'_u + b_u) . x[h]``.
        One sweep (``ghf_relation_scores``): every (64-pair tile, relation) multiplies on the fp32 matrix cores and ends in a
        dot product; the ``[B, U, d]`` operand of ``einsum("bi,uij->buj", x[h], A)`` does not exist, forward or backward.
        Recorded for autograd (decoder, text encoder and, through ``embs``, the model); gradients are bit-reproducible."""
        h, t, _ = self._pair_ids(embs, head, tail, rel_embs, direction, "score_relations")
        return self._score_table(embs, h, t, rel_embs, direction)

    @staticmethod
    def _relation_filter_lists(embs: torch.Tensor, head: torch.Tensor, tail: torch.Tensor, rel: Optional[torch.Tensor], known,
                               num_relations: Optional[int] = None):
        """Per-pair filter lists (CSR ``ptr [B + 1]``, ``idx``; every list ascending, repeats gone), or ``(None, None)``:
        pair i's list is every relation id ``r != rel_i`` (every ``r`` when ``rel`` is None) with a known triple
        ``(head_i, r, tail_i)`` in ``known = (src, dst, rel)``.  Directed: a ``tail -> head`` edge does not count.  Node ids
        wrap, relation ids do not; ids ``>= num_relations`` are dropped.  Sorted keys and ``searchsorted``, on embs' device
        (CPU tensors work)."""
        if known is None:
            return None, None
        RelationDecoder._check_known(known)
        N = embs.size(0)
        h = HyperGNN._rank_ids(head, N, embs, "head")
        t = HyperGNN._rank_ids(tail, N, embs, "tail")
        B = h.numel()
        if t.numel() != B:
            raise ValueError(f"{B} heads and {t.numel()} tails")
        src = HyperGNN._rank_ids(known[0], N, embs, "known[0]")
        dst = HyperGNN._rank_ids(known[1], N, embs, "known[1]")
        if src.numel() != dst.numel():
            raise ValueError(f"known: {src.numel()} sources and {dst.numel()} destinations")
        krel = HyperGNN._rel_ids(known[2], src.numel(), embs, "known[2]")
        qrel = None if rel is None else HyperGNN._rel_ids(rel, B, embs, "rel")
        if src.numel() == 0 or B == 0:
            return None, None
        R = 1 + int(krel.max())
        if N * N * R >= 1 << 63:
            raise ValueError(f"known: {N} nodes x {R} relations do not fit the 64-bit (src, dst, rel) keys")
        key = torch.unique((src * N + dst) * R + krel)            # sorted by (src, dst, rel), repeats gone
        kp = torch.div(key, R, rounding_mode="floor")
        qk = h * N + t
        lo = torch.searchsorted(kp, qk)
        lens = torch.searchsorted(kp, qk, right=True) - lo
        nnz = int(lens.sum())
        if nnz == 0:
            return None, None
        start = torch.cumsum(lens, 0) - lens
        seg = torch.repeat_interleave(torch.arange(B, device=embs.device), lens, output_size=nnz)
        pos = torch.arange(nnz, device=embs.device) + (lo - start)[seg]
        r = key[pos] - kp[pos] * R
        keep = torch.ones_like(r, dtype=torch.bool)
        if qrel is not None:
            keep &= r != qrel[seg]
        if num_relations is not None:
            keep &= r < num_relations
        seg, r = seg[keep], r[keep]
        if r.numel() == 0:
            return None, None
        ptr = torch.zeros(B + 1, dtype=torch.int64, device=embs.device)
        torch.cumsum(torch.bincount(seg, minlength=B), 0, out=ptr[1:])
        return ptr, r.contiguous()

    @staticmethod
    def _list_mask(S: torch.Tensor, ptr: Optional[torch.Tensor], idx: Optional[torch.Tensor]) -> torch.Tensor:
        """bool ``[B, U]``: entry (i, u) is set when u is in pair i's list."""
        B, U = S.shape
        mask = torch.zeros(B, U, dtype=torch.bool, device=S.device)
        if ptr is not None and idx is not None and idx.numel():
            lens = ptr[1:] - ptr[:-1]
            seg = torch.repeat_interleave(torch.arange(B, device=S.device), lens.to(S.device), output_size=idx.numel())
            mask[seg, idx.to(S.device)] = True
        return mask

    @classmethod
    def _ranks_from_scores(cls, S: torch.Tensor, rel: torch.Tensor, ptr: Optional[torch.Tensor] = None,
                           idx: Optional[torch.Tensor] = None):
        """``(greater, equal)`` int64 ``[B]``: how many relations score above / exactly as ``rel[i]`` in row i of ``S [B, U]``,
        the target itself and the pair's listed relations left out.  Any device."""
        ar = torch.arange(S.size(0), device=S.device)
        out = cls._list_mask(S, ptr, idx)
        out[ar, rel] = True
        st = S[ar, rel].unsqueeze(1)
        return ((S > st) & ~out).sum(1), ((S == st) & ~out).sum(1)

    @classmethod
    def _topk_from_scores(cls, S: torch.Tensor, k: int, ptr: Optional[torch.Tensor] = None, idx: Optional[torch.Tensor] = None):
        """``(scores [B, k], ids [B, k] int64)``: the k best relations of every row outside its list, best first, ties to the
        lower id (a stable descending sort), ``(-inf, -1)`` where fewer than k remain.  Any device."""
        B, U = S.shape
        out = cls._list_mask(S, ptr, idx)
        order = torch.sort(S.masked_fill(out, float("-inf")), dim=1, descending=True, stable=True).indices
        listed = out.gather(1, order)
        order = order.gather(1, torch.sort(listed.to(torch.int8), dim=1, stable=True).indices)   # the listed ones last, in place
        left = (U - out.sum(1)).unsqueeze(1)
        scores = torch.full((B, k), float("-inf"), dtype=S.dtype, device=S.device)
        ids = torch.full((B, k), -1, dtype=torch.int64, device=S.device)
        m = min(k, U)
        live = torch.arange(m, device=S.device).unsqueeze(0) < left
        scores[:, :m] = torch.where(live, S.gather(1, order[:, :m]), scores[:, :m])
        ids[:, :m] = torch.where(live, order[:, :m], ids[:, :m])
        return scores, ids

    @classmethod
    def _loss_from_scores(cls, S: torch.Tensor, rel: torch.Tensor, ptr: Optional[torch.Tensor] = None,
                          idx: Optional[torch.Tensor] = None, scale: float = 1.0) -> torch.Tensor:
        """``[B]``: ``logsumexp_u(scale S[i, u]) - scale S[i, rel_i]`` over the relations outside pair i's list; the target
        always stays in the sum.  Differentiable in ``S``; any device."""
        ar = torch.arange(S.size(0), device=S.device)
        out = cls._list_mask(S, ptr, idx)
        out[ar, rel] = False
        z = (scale * S).masked_fill(out, float("-inf"))
        return torch.logsumexp(z, dim=1) - z[ar, rel]

    def rank_relations(self, embs: torch.Tensor, head: torch.Tensor, tail: torch.Tensor, rel: torch.Tensor,
                       rel_embs: torch.Tensor, *, known=None, direction: str = "tail"):
        """Where the text ``rel[i]`` ranks among ALL rows of ``rel_embs`` as the relation of ``(head_i, ?, tail_i)``:
        ``(greater, equal)`` int64 ``[B]`` for ``link_prediction_metrics``.  ``known=(src, dst, rel)`` names true triples: every
        other relation known to hold for the same directed pair is left out (the filtered setting).  No autograd graph."""
        h, t, r = self._pair_ids(embs, head, tail, rel_embs, direction, "rank_relations", rel, known=known)
        with torch.no_grad():
            S = self._score_table(embs, h, t, rel_embs, direction)
            ptr, idx = self._relation_filter_lists(embs, h, t, r, known, rel_embs.size(0))
            return self._ranks_from_scores(S, r, ptr, idx)

    def topk_relations(self, embs: torch.Tensor, head: torch.Tensor, tail: torch.Tensor, k: int, rel_embs: torch.Tensor, *,
                       known=None, direction: str = "tail"):
        """``(scores [B, k] fp32, ids [B, k] int64)``: the k best relation texts for every pair, best first, ties to the lower
        id, ``(-inf, -1)`` padding; ``1 <= k <= 128``.  ``known=(src, dst, rel)``: relations already known for the directed pair
        are left out, so what remains are the NEW relations the decoder proposes.  No autograd graph."""
        k = int(k)
        if not 1 <= k <= 128:
            raise ValueError(f"topk_relations: k = {k} outside 1..128")
        h, t, _ = self._pair_ids(embs, head, tail, rel_embs, direction, "topk_relations", known=known)
        with torch.no_grad():
            S = self._score_table(embs, h, t, rel_embs, direction)
            ptr, idx = self._relation_filter_lists(embs, h, t, None, known, rel_embs.size(0))
            return self._topk_from_scores(S, k, ptr, idx)

    def relation_loss(self, embs: torch.Tensor, head: torch.Tensor, tail: torch.Tensor, rel: torch.Tensor,
                      rel_embs: torch.Tensor, scale: float = 1.0, *, known=None, direction: str = "tail") -> torch.Tensor:
        """``[B]``: ``lse_u(scale S[i, u]) - scale S[i, rel_i]``, the softmax cross-entropy of the true relation against every
        relation text; the other relations known for the pair (``known``) are left out of the sum, the target never is.
        Recorded for autograd: one ``backward()`` reaches the decoder, the text encoder and the model."""
        scale = float(scale)
        if not (0.0 < scale < float("inf")):
            raise ValueError(f"relation_loss: scale must be finite and positive, got {scale}")
        h, t, r = self._pair_ids(embs, head, tail, rel_embs, direction, "relation_loss", rel, known=known)
        S = self._score_table(embs, h, t, rel_embs, direction)
        with torch.no_grad():
            ptr, idx = self._relation_filter_lists(embs, h, t, r, known, rel_embs.size(0))
        return self._loss_from_scores(S, r, ptr, idx, scale)

    def num_parameters(self) -> int:
        return sum(p.numel() for p in self.parameters() if p.requires_grad)
