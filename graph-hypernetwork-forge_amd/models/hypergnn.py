"""HyperGNN — host mirror of the reference model, computing on MI355X.

Same constructor, attributes, ``state_dict`` keys, ``forward(node_features,
edge_index, edge_texts)`` signature and ``ValueError`` behaviour as
``graph_hypernetwork_forge/models/hypergnn.py:88-322`` of the reference.  The
forward is a sequence of C-ABI calls into ``libghf_hip.so``:

    plan (cached)            ghf_plan_build            replaces hypergnn.py:264-268 + edge order
    weights per relation     ghf_weightgen_fwd_batched replaces :278 (weight_generator.py:137-141), all layers up front
    h0 = relu(x W_in^T + b)  ghf_input_proj_fwd        replaces :261
    per layer:
      messages+mean+self+tail ghf_message_layer_fwd    replaces :281-296

The per-edge weight gather of the reference (:281-283, O(E d^2) memory) does
not exist here: kernels index W[r] in place.
"""

from __future__ import annotations

import operator
from typing import Dict, List, Optional, Sequence, Tuple


import numpy as np
import torch
import torch.nn as nn

from .. import _native
from ..plan import GraphPlan, PlanCache, build_plan, build_rs, empty_plan, exact_plan, plan_config, relation_ids
from ..plan import CSR_CONFIG
from ..plan import check_pool
from .weight_generator import WeightGenerator, check_dropout, draw_mask, require_inference, wants_grad


class TextEncoder(nn.Module):
    """Relation string -> ``[text_dim]``: mean of character embeddings, Linear, Tanh.

    Mirrors reference hypergnn.py:39-81 (ids = min(ord(c), 127), '' -> [0]).
    ``forward`` encodes all strings with one ``ghf_text_encode_fwd`` launch; the
    padded id matrix of a list of strings is built once and kept on the device
    (keyed on the tuple of strings), so a warm forward has no host work here.
    """

    ASCII_VOCAB = 128

    def __init__(self, text_dim: int, char_emb_dim: int = 32) -> None:
        super().__init__()
        self.text_dim = text_dim
        self.char_emb = nn.Embedding(self.ASCII_VOCAB, char_emb_dim)
        self.proj = nn.Sequential(nn.Linear(char_emb_dim, text_dim), nn.Tanh())
        self._tokens: Dict[Tuple, Tuple[torch.Tensor, torch.Tensor]] = {}      # padded id matrices, on the device

    def _codes(self, text: str) -> List[int]:
        codes = [min(ord(c), self.ASCII_VOCAB - 1) for c in text]
        return codes or [0]

    def _tokenize(self, text: str, device: torch.device) -> torch.Tensor:
        return torch.tensor(self._codes(text), dtype=torch.long, device=device)

    def _token_matrix(self, texts: Sequence[str], device: torch.device):
        key = (tuple(texts), str(device))
        hit = self._tokens.get(key)
        if hit is None:
            codes = [self._codes(t) for t in texts]
            lens = np.fromiter((len(c) for c in codes), dtype=np.int32, count=len(codes))
            ids = np.zeros((len(codes), int(lens.max())), dtype=np.int32)
            for i, c in enumerate(codes):
                ids[i, :len(c)] = c
            hit = (torch.from_numpy(ids).to(device), torch.from_numpy(lens).to(device))
            if len(self._tokens) >= 8:
                self._tokens.pop(next(iter(self._tokens)))
            self._tokens[key] = hit
        return hit

    def encode_one(self, text: str, device: torch.device) -> torch.Tensor:
        """One string -> ``[text_dim]`` (reference hypergnn.py:73-77)."""
        return self.forward([text], device)[0]

    def forward(self, texts: Sequence[str], device: torch.device) -> torch.Tensor:
        grad = wants_grad(self, self.char_emb.weight)
        ids, lens = self._token_matrix(texts, torch.device(device))
        lin = self.proj[0]
        if grad:
            from ..autograd import TextEncoderFn
            return TextEncoderFn.apply(self.char_emb.weight, lin.weight, lin.bias, ids, lens)
        return _native.text_encode_fwd(ids, lens, self.char_emb.weight.detach(), lin.weight.detach(), lin.bias.detach())


class GraphedForward:
    """The warm inference forward of one (model, graph plan, feature shape) captured into a HIP graph.

    A forward is ~6 + 4 L kernel launches; on small graphs (BASELINE configs 1 and 2) their host cost exceeds the
    device time.  Replaying the captured graph costs one launch.  Parameters are read at replay time (in-place updates
    are seen); the plan, the feature shape and the relation strings are frozen.  ``replay(node_features)`` copies new
    features into the captured input buffer; the returned tensor is overwritten by the next replay."""

    def __init__(self, model: "HyperGNN", node_features: torch.Tensor, plan: GraphPlan) -> None:
        self.input = node_features.detach().float().clone()
        dev = self.input.device
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side), torch.no_grad():            # warm-up off the capture: lazy scratch, LDS limits
            for _ in range(2):
                model.forward_planned(self.input, plan)
        torch.cuda.current_stream(dev).wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph), torch.no_grad():
            self.output = model.forward_planned(self.input, plan)
        # The captured launches hold raw device pointers into the plan's arrays (and its scratch), the relation strings'
        # token matrices and the parameters; the plan cache and the token cache are small LRUs, so this object keeps its
        # own references — evicting the plan elsewhere must not free memory a replay still reads.
        self._keep = (model, plan, plan.rs, plan._partial, None if plan.rs is None else (plan.rs._Y, plan.rs._P),
                      model.text_encoder._token_matrix(plan.unique_texts, dev))

    def replay(self, node_features: Optional[torch.Tensor] = None) -> torch.Tensor:
        if node_features is not None:
            if node_features.shape != self.input.shape:
                raise ValueError(f"captured for features {tuple(self.input.shape)}, got {tuple(node_features.shape)}")
            self.input.copy_(node_features)
        model, plan = self._keep[0], self._keep[1]
        guard = model._guarded(plan)
        if guard:
            flag = _native.range_flag(self.input.device)
            flag.zero_()
        self.graph.replay()
        if guard and int(flag.item()):                      # (one 4-byte read per replay; GHF_RANGE_GUARD=0 skips it)
            with torch.no_grad():
                self.output.copy_(model._forward_exact(self.input, plan, int(flag.item())))
        return self.output

    __call__ = replay


class HyperGNN(nn.Module):
    """Hypernetwork-conditioned GNN (reference hypergnn.py:88-154), forward on HIP kernels."""

    SIDE_STREAM_MIN_EDGES = 4_000_000     # below this a forward is too short for cross-stream overlap to pay

    def __init__(self, text_dim: int, node_feat_dim: int, hidden_dim: int, num_layers: int = 2,
                 dropout: float = 0.0, char_emb_dim: int = 32) -> None:
        super().__init__()
        if num_layers < 1:                                            # reference :123-124
            raise ValueError("num_layers must be at least 1")
        check_dropout(dropout)
        self.text_dim, self.node_feat_dim, self.hidden_dim = text_dim, node_feat_dim, hidden_dim
        self.num_layers, self.dropout = num_layers, dropout
        self.text_encoder = TextEncoder(text_dim=text_dim, char_emb_dim=char_emb_dim)
        self.input_proj = nn.Linear(node_feat_dim, hidden_dim)
        self.weight_generators = nn.ModuleList([
            WeightGenerator(text_dim=text_dim, d_in=hidden_dim, d_out=hidden_dim,
                            hidden_dim=max(64, text_dim * 2), num_hidden=2, dropout=dropout)
            for _ in range(num_layers)])
        self.layer_norms = nn.ModuleList([nn.LayerNorm(hidden_dim) for _ in range(num_layers)])
        self._plans = PlanCache()
        self._wg_stream = None
        self.last_range_flags = 0        # what the range guard saw in the last forward (include/ghf.h: ghf_set_range_flag)
        self.last_subgraph = None        # the last forward_nodes call's subgraph: m (rows within j hops), edges, plan geometry

    # -- plan ------------------------------------------------------------------------------
    def plan_for(self, edge_index: torch.Tensor, edge_texts: Sequence[str], num_nodes: int,
                 device: torch.device, training: bool = False) -> GraphPlan:
        """Cached graph plan for these inputs (cold: O(E) host work + one device sort).  Inference plans of graphs with
        many relations are CSR plans for the relation-stationary layer (_native.prefer_rs); plans that will record
        gradients keep the destination-block geometry the backward kernels run on."""
        return self._plan_lookup(edge_index, edge_texts, num_nodes, device, training)[0]

    def _plan_lookup(self, edge_index: torch.Tensor, edge_texts: Sequence[str], num_nodes: int, device: torch.device,
                     training: bool = False, defer_check: bool = False):
        """(plan, check, settle): the cached plan, or a fresh one (settle: None, or — with `defer_check` — a callable the caller
        runs after its launches are enqueued: it waits for the new cache entry's checksums, taken on the cache's threads
        meanwhile).  A hit on a relation list too long for the key's fingerprint to
        cover whole (plan.FULL_FINGERPRINT_MAX) is confirmed against the snapshot of the list taken when the plan was built
        (plan.same_relations: ~4 ms at 10 M entries) — here, before returning, or, with `defer_check`, by the caller:
        `check` is then a callable () -> bool to run once the forward is enqueued (the host is idle while the GPU works);
        False means the list was edited in place, the result must be dropped and the lookup repeated (it will miss)."""
        key = PlanCache.key(edge_index, edge_texts, num_nodes, self.hidden_dim, device) + (bool(training),)
        plan = self._plans.get(key)
        if plan is not None:
            check = self._plans.verifier(key, edge_texts)
            if check is None:
                return plan, None, None
            if defer_check:
                return plan, check, None
            if check():
                return plan, None, None
        unique, ids, objects = relation_ids(edge_texts, want_objects=True)
        wide = not training and _native.prefer_rs(self.hidden_dim, len(unique))
        plan = build_plan(edge_index, torch.from_numpy(ids), unique, num_nodes, self.hidden_dim, device, force_generic=wide)
        # (defer_check: the caller collects the entry's checksums — taken on the cache's threads beside its launches)
        taking = self._plans.put(key, plan, edge_index, edge_texts, objects=objects, background=defer_check)
        return plan, None, (None if taking is None else taking.result)

    def graphed(self, node_features: torch.Tensor, edge_index: torch.Tensor, edge_texts: List[str]) -> GraphedForward:
        """Capture ``forward`` for these inputs into a HIP graph (inference only); see GraphedForward."""
        self._check_inputs(node_features, edge_index, edge_texts, "edge_texts")
        if not node_features.is_cuda:
            raise RuntimeError("HyperGNN computes on an MI355X HIP device only; there is no CPU path to capture")
        plan = self.plan_for(edge_index, edge_texts, node_features.size(0), node_features.device)
        return GraphedForward(self, node_features, plan)

    def _check_inputs(self, node_features: torch.Tensor, edge_index: torch.Tensor, per_edge, name: str) -> None:
        """Every entry point's input checks (reference :252-256): `per_edge` — the strings, or a 1-D tensor of relation ids —
        holds one entry per edge, and the features are [N, node_feat_dim]."""
        ids = isinstance(per_edge, torch.Tensor)
        n = per_edge.numel() if ids else len(per_edge)
        if (ids and per_edge.dim() != 1) or edge_index.size(1) != n:
            raise ValueError(f"edge_index has {edge_index.size(1)} edges but {name} has {n} entries")
        if node_features.dim() != 2 or node_features.size(1) != self.node_feat_dim:
            raise ValueError(f"node_features must be [N, {self.node_feat_dim}], got {tuple(node_features.shape)}")

    def clear_plan_cache(self) -> None:
        self._plans.clear()

    def forward_ids(self, node_features: torch.Tensor, edge_index: torch.Tensor, edge_rel_ids: torch.Tensor,
                    relation_texts: Sequence[str]) -> torch.Tensor:
        """``forward`` for callers that already hold relation ids: ``edge_texts[e] == relation_texts[edge_rel_ids[e]]``.

        The reference's call form hands over one Python string per edge; mapping those to ids is pure host work
        (1.5 s at 10 M edges, reference hypergnn.py:264-268).  This overload skips it: the ids
        may live on the device, nothing O(E) runs on the host, and the plan is cached on the two tensors' identity."""
        self._check_inputs(node_features, edge_index, edge_rel_ids, "edge_rel_ids")
        grad = wants_grad(self, node_features) or self._dropping()
        plan = self._ids_plan(edge_index, edge_rel_ids, relation_texts, node_features, grad)
        if grad:
            return self._forward_recorded(node_features, plan, edge_index)
        return self.forward_planned(node_features, plan)

    def _ids_plan(self, edge_index: torch.Tensor, edge_rel_ids: torch.Tensor, relation_texts: Sequence[str],
                  node_features: torch.Tensor, grad: bool) -> GraphPlan:
        """forward_ids' cached plan, keyed on the two tensors' identity."""
        device, N = node_features.device, node_features.size(0)
        texts = list(relation_texts)
        key = ("ids", edge_index.data_ptr(), tuple(edge_index.shape), edge_index._version, str(edge_index.device),
               edge_rel_ids.data_ptr(), edge_rel_ids._version, str(edge_rel_ids.device), tuple(texts), N, self.hidden_dim,
               str(device), bool(grad))
        plan = self._plans.get(key)
        if plan is None:
            wide = not grad and _native.prefer_rs(self.hidden_dim, len(texts))
            plan = build_plan(edge_index, edge_rel_ids, texts, N, self.hidden_dim, device, force_generic=wide)   # ids out of range: IndexError
            self._plans.put(key, plan, edge_index, (edge_rel_ids, texts))
        return plan

    # -- forward (reference :236-298) -----------------------------------------------------
    def forward(self, node_features: torch.Tensor, edge_index: torch.Tensor, edge_texts: List[str]) -> torch.Tensor:
        self._check_inputs(node_features, edge_index, edge_texts, "edge_texts")
        grad = wants_grad(self, node_features) or self._dropping()
        device = node_features.device
        # The reference maps the strings to ids on every call (:264-268).  Here a cached plan is used at once and, when the
        # list is too long for the cache key to cover, checked entry by entry on the host WHILE the GPU runs the forward; a
        # list edited in place fails the check: fresh plan, forward again.
        plan, check, settle = self._plan_lookup(edge_index, edge_texts, node_features.size(0), device, training=grad,
                                                defer_check=not grad)
        if grad:
            return self._forward_recorded(node_features, plan, edge_index)
        # (the check runs on the plan cache's threads, outside the GIL, beside this thread's launches and its wait for the
        # range-guard word; its result is collected before the output is handed back)
        pending = None if check is None else check_pool().submit(check)
        out = self.forward_planned(node_features, plan)
        if settle is not None:
            settle()
        if pending is not None and not pending.result():
            plan = self._plan_lookup(edge_index, edge_texts, node_features.size(0), device, training=False)[0]
            out = self.forward_planned(node_features, plan)
        return out

    # -- node batches: the rows of a few nodes from their k-hop subgraph (include/ghf.h: ghf_subgraph_*) ---------------
    def forward_nodes(self, node_features: torch.Tensor, edge_index: torch.Tensor, edge_texts: List[str],
                      nodes: torch.Tensor, fanout=None, seed: Optional[int] = None, exclude=None) -> torch.Tensor:
        """``forward(node_features, edge_index, edge_texts)[nodes]`` computed on the nodes' ``num_layers``-hop
        in-neighbourhood only: an L-layer row depends on the rows within L hops upstream of it (reference hypergnn.py:190-230,
        288-296), so the result is exact, not sampled.  `nodes`: a 1-D int32 / int64 tensor (device or CPU), duplicates and
        negative ids (as torch indexing) allowed.  Gradients reach the parameters and `node_features`; dropout masks in
        training mode are drawn over the subgraph's rows (random as in ``forward``, not the full forward's draws).

        `fanout` (None: the exact call above) samples the neighbourhood as GraphSAGE / NeighborLoader do: an int, or
        ``num_layers`` ints, each >= 1 or -1 (no cap); hop j keeps at most ``fanout[j]`` in-edges, drawn uniformly without
        replacement, of every node first reached at hop j — ``fanout[0]`` caps the seeds' own in-edges, which the last layer
        consumes.  The layer aggregates by mean, so each sampled aggregate is an unbiased estimate.  `seed` (an int in
        [0, 2**63); None: drawn from torch's default CPU generator, so ``torch.manual_seed`` reproduces a run) fixes the
        draw, which is a pure function of (plan, nodes, fanout, seed) (include/ghf.h).  The plan's geometry depends on the
        hidden size and on whether gradients are recorded, so one seed may pick different edges in ``train()`` and
        ``eval()``.  ``last_subgraph`` records `fanout` (a tuple) and the seed used.

        `exclude` (None: nothing) leaves edges out of the subgraph — the batch's own edges when the rows are scored for link
        prediction, which would otherwise show the model the answer: ``(src, dst)`` drops every edge src[i] -> dst[i] whatever
        its relation, ``(src, dst, rel)`` with one relation text per entry only those labelled rel[i].  1-D int32 / int64 id
        tensors of equal length, negative ids as torch indexing; direction matters (list the reverses to drop them too);
        entries that match no edge — a text that labels no edge among them — do nothing.  The result is
        ``forward`` on the graph without those edges, rows `nodes` (include/ghf.h: ghf_subgraph_*_excl); with `fanout`
        excluded edges are no candidates.  The plan of the full graph stays cached.  ``last_subgraph["exclude"]`` records
        (entries, typed), or None."""
        self._check_inputs(node_features, edge_index, edge_texts, "edge_texts")
        sample = self._sample_args(fanout, seed)
        excl = self._exclude_args(exclude, node_features, texts=True)
        seeds = self._seed_ids(nodes, node_features)
        grad = wants_grad(self, node_features) or self._dropping()
        plan = self._plan_lookup(edge_index, edge_texts, node_features.size(0), node_features.device, training=grad)[0]
        return self._forward_nodes(node_features, plan, seeds, grad, edge_index, sample, self._exclude_keys(excl, plan))

    def forward_nodes_ids(self, node_features: torch.Tensor, edge_index: torch.Tensor, edge_rel_ids: torch.Tensor,
                          relation_texts: Sequence[str], nodes: torch.Tensor, fanout=None,
                          seed: Optional[int] = None, exclude=None) -> torch.Tensor:
        """``forward_nodes`` for callers that already hold relation ids (see ``forward_ids``); the typed `exclude` is
        ``(src, dst, rel)`` with `rel` a 1-D int tensor of ids into `relation_texts` (negative: ValueError, beyond the list:
        IndexError)."""
        self._check_inputs(node_features, edge_index, edge_rel_ids, "edge_rel_ids")
        sample = self._sample_args(fanout, seed)
        excl = self._exclude_args(exclude, node_features, num_relations=len(relation_texts))
        seeds = self._seed_ids(nodes, node_features)
        grad = wants_grad(self, node_features) or self._dropping()
        plan = self._ids_plan(edge_index, edge_rel_ids, relation_texts, node_features, grad)
        return self._forward_nodes(node_features, plan, seeds, grad, edge_index, sample, self._exclude_keys(excl, plan))

    @classmethod
    def _exclude_args(cls, exclude, node_features: torch.Tensor, texts: bool = False, num_relations: int = 0):
        """forward_nodes' `exclude` checked without a GPU: None, or (src, dst, rel or None) — the node ids through _rank_ids
        (on the features' device), `rel` the relation texts (texts=True: a list of strings, mapped to ids once the plan is
        known) or a checked int64 tensor of ids below `num_relations`."""
        if exclude is None:
            return None
        if isinstance(exclude, (torch.Tensor, str, bytes)) or not hasattr(exclude, "__len__") or len(exclude) not in (2, 3):
            n = len(exclude) if hasattr(exclude, "__len__") and not isinstance(exclude, (torch.Tensor, str, bytes)) else None
            raise ValueError("exclude must be (src, dst) or (src, dst, rel)" +
                             (f", got {n} members" if n is not None else f", got {type(exclude).__name__}"))
        N = node_features.size(0)
        src = cls._rank_ids(exclude[0], N, node_features, "exclude[0]")
        dst = cls._rank_ids(exclude[1], N, node_features, "exclude[1]")
        if src.numel() != dst.numel():
            raise ValueError(f"exclude: {src.numel()} sources and {dst.numel()} destinations")
        if len(exclude) == 2:
            return src, dst, None
        rel = exclude[2]
        if texts:
            if isinstance(rel, (str, bytes, torch.Tensor)) or not hasattr(rel, "__len__"):
                raise TypeError(f"exclude[2] must be a sequence of relation texts, one per entry, got {type(rel).__name__}")
            if len(rel) != src.numel():
                raise ValueError(f"exclude[2] holds {len(rel)} relation texts, expected {src.numel()}")
            rel = list(rel)
            if not all(isinstance(t, str) for t in rel):
                raise TypeError("exclude[2] must hold relation texts (strings); forward_nodes_ids takes relation ids")
            return src, dst, rel
        rel = cls._rel_ids(rel, src.numel(), node_features, "exclude[2]")
        if rel.numel() and int(rel.max()) >= num_relations:
            raise IndexError(f"exclude[2] holds relation ids outside [0, {num_relations})")
        return src, dst, rel

    @staticmethod
    def _exclude_keys(excl, plan: GraphPlan):
        """The checked `exclude` as (sorted int64 keys on the device, typed, entries): include/ghf.h's encoding, src << 32 | dst
        or src << 32 | (dst * R + rel) in the plan's relation ids; built and sorted on the device.  Texts that label no edge
        of the plan match nothing: their entries are dropped here."""
        if excl is None:
            return None
        src, dst, rel = excl
        entries, typed = src.numel(), rel is not None
        if typed:
            if isinstance(rel, list):
                ids = {t: i for i, t in enumerate(plan.unique_texts)}
                rel = torch.tensor([ids.get(t, -1) for t in rel], dtype=torch.int64).to(src.device)
                known = rel >= 0
                src, dst, rel = src[known], dst[known], rel[known]
            dst = dst * plan.R + rel
        return torch.sort((src << 32) | dst).values, typed, entries

    @staticmethod
    def _without_excluded(plan: GraphPlan, edge_index: torch.Tensor, keys: torch.Tensor, typed: bool):
        """The caller's edges and relation ids without the excluded ones, in the caller's order (on the plan's device)."""
        ei = edge_index.to(device=keys.device, dtype=torch.int64)
        low = ei[1] * plan.R + plan.rel_ids if typed else ei[1]
        mine = (ei[0] << 32) | low
        at = torch.searchsorted(keys, mine).clamp_(max=keys.numel() - 1)
        stay = keys[at] != mine
        return ei[:, stay].contiguous(), plan.rel_ids[stay].contiguous()

    def _sample_args(self, fanout, seed):
        """forward_nodes' `fanout` / `seed` checked on the host: None (the exact call), or (fanout tuple of num_layers ints,
        seed) — a seed of None drawn from torch's default CPU generator."""
        def integer(v, what):
            if isinstance(v, bool) or not hasattr(v, "__index__") or isinstance(v, torch.Tensor):
                raise TypeError(f"{what} must be an integer, got {type(v).__name__}")
            return operator.index(v)

        if fanout is None:
            if seed is not None:
                raise ValueError("seed given without fanout: the exact forward_nodes draws nothing")
            return None
        if isinstance(fanout, (str, bytes)) or (not hasattr(fanout, "__index__") and not hasattr(fanout, "__iter__")):
            raise TypeError(f"fanout must be an int or a sequence of {self.num_layers} ints, got {type(fanout).__name__}")
        if hasattr(fanout, "__iter__") and not isinstance(fanout, torch.Tensor):
            fan = tuple(integer(f, "fanout entries") for f in fanout)
            if len(fan) != self.num_layers:
                raise ValueError(f"fanout has {len(fan)} entries, the model has {self.num_layers} layers")
        else:
            fan = (integer(fanout, "fanout"),) * self.num_layers
        if any(f == 0 or f < -1 or f >= 1 << 31 for f in fan):
            raise ValueError(f"fanout entries must be >= 1, or -1 for no cap: got {fan}")
        if seed is None:
            seed = int(torch.randint(0, (1 << 63) - 1, (1,), dtype=torch.int64).item())
        else:
            seed = integer(seed, "seed")
            if not 0 <= seed < 1 << 63:
                raise ValueError(f"seed must be in [0, 2**63), got {seed}")
        return fan, seed

    @classmethod
    def _seed_ids(cls, nodes: torch.Tensor, node_features: torch.Tensor) -> torch.Tensor:
        """`nodes` through _rank_ids, for features that must already be on the device (forward_nodes has no CPU path)."""
        ids = cls._rank_ids(nodes, node_features.size(0), node_features, "nodes")
        if not node_features.is_cuda:
            raise RuntimeError("HyperGNN computes on an MI355X HIP device only; node_features is on the CPU and there is "
                               "no CPU path")
        return ids

    def _forward_nodes(self, x: torch.Tensor, plan: GraphPlan, seeds: torch.Tensor, grad: bool,
                       edge_index: torch.Tensor, sample=None, exclude=None) -> torch.Tensor:
        """The rows `seeds` (int64, in range) of the forward on `plan`'s graph, from the seeds' k-hop subgraph: its nodes
        ordered by (hop distance, id), so that the rows within j hops are a prefix; inference layer l (0-based) then computes
        the first m_{k-1-l} rows only (the last layer: the seeds).  The sub-plan is built per call and not cached.
        `sample` = (fanout, seed): the sampled subgraph instead (_native.subgraph_sample), which keeps the prefix property.
        `exclude` = (keys, typed, entries) of _exclude_keys: the extraction leaves those edges out, and everything after it
        follows from the edges it emits."""
        k, d, device = self.num_layers, self.hidden_dim, x.device
        if seeds.numel() == 0:
            return x.new_zeros((0, d), dtype=torch.float32)
        excl = None if exclude is None or exclude[0].numel() == 0 else exclude[:2]    # (an empty list: today's calls)
        if sample is None:
            sub, drawn = _native.subgraph(plan, seeds, k, exclude=excl), {}
        else:
            sub, drawn = _native.subgraph_sample(plan, seeds, *sample, exclude=excl), dict(fanout=sample[0], seed=sample[1])
        drawn["exclude"] = None if exclude is None else (exclude[2], exclude[1])
        m, n = sub["m"], sub["m"][k]
        xs = x.index_select(0, sub["node_list"])                     # differentiable: gradients reach node_features
        rows = sub["new_id"].index_select(0, seeds)
        config = CSR_CONFIG if plan.block_nodes == 1 else None        # (the full plan's kernel family: wide rows stay wide)
        if sub["edge_index"].size(1) == 0:
            if grad:                                                  # (no edge to train through: the full recorded forward)
                self.last_subgraph = dict(m=m, edges=0, block_nodes=plan.block_nodes, wlayout=plan.wlayout, **drawn)
                if excl is not None:
                    # ... on the graph without the excluded edges, or they would be back: a plan of the reduced edge arrays,
                    # built for this call (build_plan refuses a graph with no edge left, as forward does)
                    ei, rel = self._without_excluded(plan, edge_index, *excl)
                    reduced = build_plan(ei, rel, plan.unique_texts, plan.N, d, device)
                    return self._forward_recorded(x, reduced, ei).index_select(0, seeds)
                return self._forward_recorded(x, plan, edge_index).index_select(0, seeds)
            sub_plan = empty_plan(n, plan.unique_texts, config or plan_config(d, 0, n), device)
        else:
            sub_plan = build_plan(sub["edge_index"], sub["rel"], plan.unique_texts, n, d, device, force_generic=config is not None)
        self.last_subgraph = dict(m=m, edges=sub_plan.E, block_nodes=sub_plan.block_nodes, wlayout=sub_plan.wlayout, **drawn)
        if grad:
            out = self._forward_recorded(xs, sub_plan, sub["edge_index"])
        else:
            out = self.forward_planned(xs, sub_plan, rows_per_layer=[m[k - 1 - l] for l in range(k)])
        return out.index_select(0, rows)

    # -- range guard of the two-fp16-piece kernels (include/ghf.h: ghf_set_range_flag) ---------------------------
    def _guarded(self, plan: GraphPlan) -> bool:
        pieces = plan.wlayout in _native.SPLIT_LAYOUTS or (plan.block_nodes == 1 and _native.rs_supported(self.hidden_dim)
                                                          and not _native.rs_exact(plan))
        return pieces and _native.range_guard_enabled()

    def _forward_exact(self, x: torch.Tensor, plan: GraphPlan, flags: int) -> torch.Tensor:
        """The forward again on the exact fp32 kernels: some row of h (flags & 1) or some relation's generated weights
        (flags & 2) spans more dynamic range than two fp16 pieces hold (the reference computes in plain fp32,
        hypergnn.py:202,228)."""
        self.last_range_flags = flags
        return self.forward_planned(x, exact_plan(plan, self.hidden_dim), guard=False)

    def _dropping(self) -> bool:
        """Training mode with dropout > 0 (reference :293-294): the forward then takes the recorded path — the layer's tail
        alone with a mask operand — whether or not gradients are wanted."""
        return self.training and self.dropout > 0.0

    def _draw_mask(self, shape, device) -> torch.Tensor:
        """A dropout mask scaled by 1/(1-p), drawn with torch's generator as F.dropout does in the reference."""
        return draw_mask(shape, device, self.dropout)

    def _forward_recorded(self, node_features: torch.Tensor, plan: GraphPlan, edge_index: torch.Tensor, exact: bool = False) -> torch.Tensor:
        """The forward when gradients are required (reference: plain autograd, demo.py:79-101): the same kernels inside
        ``autograd`` Functions whose backward is C-ABI calls too.  The reversed-graph plan and the relation grouping the
        backward needs are built once per plan.  When the range guard fires, the forward is recorded again on the plan for the
        exact fp32 kernels (exact=True; the first recording is dropped) — as the inference forward reruns, and as the
        reference's plain fp32 autograd needs no such thing (hypergnn.py:202,228)."""
        from ..autograd import InputProjFn, MessageLayerFn, build_train_plan
        device = node_features.device
        if plan.train is None:
            if exact:                      # (the exact plan was built from the first plan's sorted edges: take the triple from it)
                src, dst, rel = plan.edge_arrays()
                plan.train = build_train_plan(torch.stack([src, dst]), rel, plan, self.hidden_dim, device, exact=True)
            else:
                plan.train = build_train_plan(edge_index, plan.rel_ids, plan, self.hidden_dim, device)
        guard = not exact and self._guarded(plan)
        if guard:
            flag = _native.range_flag(device)
            flag.zero_()
        text_embs = self.text_encoder(plan.unique_texts, device)
        # Large graphs, no dropout: the generators on a side stream — autograd runs a Function's backward
        # on the stream of its forward, so the generators' backward (a few dozen small latency-bound kernels per layer) then
        # runs beside the message layers' gradient kernels instead of between them (C3: backward 35.2 -> 34.1 ms).  In the
        # forward the caller's stream waits for them at once: side by side with the input projection both got slower (forward
        # 13.45 -> 13.8 ms).  (With dropout the masks are drawn in the reference's order on one stream.)
        side = plan.E >= self.SIDE_STREAM_MIN_EDGES and not self._dropping()
        generated = []
        if side:
            main = torch.cuda.current_stream(device)
            if self._wg_stream is None or self._wg_stream.device != device:
                self._wg_stream = torch.cuda.Stream(device=device)
            st = self._wg_stream                           # one stream, one hand-over each way (a hop costs ~40 us)
            st.wait_stream(main)
            with torch.cuda.stream(st):
                for gen in self.weight_generators:
                    generated.append(gen.generate_with_grad(text_embs))
            main.wait_stream(st)
            for ws in generated:
                for t in ws:
                    t.record_stream(main)
        h = InputProjFn.apply(node_features, self.input_proj.weight, self.input_proj.bias, plan.train)
        for l, (gen, norm) in enumerate(zip(self.weight_generators, self.layer_norms)):
            if side:
                W_msg, W_self, bias = generated[l]
            else:
                W_msg, W_self, bias = gen.generate_with_grad(text_embs)
            drop = self._draw_mask(tuple(h.shape), device) if self._dropping() else None
            h = MessageLayerFn.apply(h, W_msg, W_self, bias, norm.weight, norm.bias, norm.eps, plan.train, drop)
        if guard:
            bits = int(flag.item())
            self.last_range_flags = bits
            if bits:
                # (dropout: the masks of the second recording are fresh draws — one more forward's worth of the generator)
                return self._forward_recorded(node_features, exact_plan(plan, self.hidden_dim), edge_index, exact=True)
        return h

    def generate_batched(self, text_embs: torch.Tensor, layout: int):
        """Every layer's (W_msg | Wfrag, W_self | None, bias) from ONE launch sequence (ghf_weightgen_fwd_batched: the layers'
        generators have identical shapes) — three kernels for all layers on the caller's stream: ~0.11 ms whatever the
        number of layers, where layer-by-layer generation cost that per layer (between the message launches of a small
        graph: BASELINE config 2).  A model deeper than one call takes (_native.WG_BATCH_MAX generators) gets one launch
        sequence per group of consecutive layers."""
        gens, g0, out = list(self.weight_generators), self.weight_generators[0], []
        for i in range(0, len(gens), _native.WG_BATCH_MAX):
            group = gens[i:i + _native.WG_BATCH_MAX]
            out += _native.weightgen_fwd_batched(text_embs, [g._head_params() for g in group],
                                                 [g._log_scale_vector() for g in group], g0.text_dim, g0.hidden_dim,
                                                 g0.num_hidden, g0.d_in, g0.d_out, layout)
        return out

    def forward_planned(self, node_features: torch.Tensor, plan: GraphPlan,
                        exchange=None, guard: bool = True, rows_per_layer: Optional[Sequence[int]] = None) -> torch.Tensor:
        """Forward with an explicit plan.  `exchange(h)` (multi-GPU) runs after every layer to
        make all rows of h visible on this rank; the plan's row range says which rows it computes.
        Range guard: the kernels that cut rows / weights into two fp16 pieces flag inputs whose dynamic range those do not
        hold; the forward then ends with one 4-byte read of that flag (the only host sync of a warm forward;
        GHF_RANGE_GUARD=0 removes it) and, if it is set, runs again on the exact fp32 kernels (over every row).
        rows_per_layer[l]: layer l needs correct outputs on its first rows_per_layer[l] rows only (forward_nodes: a prefix
        that shrinks layer by layer, the rows of layer l + 1 among them)."""
        require_inference(self, node_features, what=".forward_planned")
        if self._dropping():
            raise NotImplementedError("HyperGNN.forward_planned: dropout in training mode runs through forward() / forward_ids() "
                                      "(the recorded path); call .eval() for inference")
        device = node_features.device
        x = node_features if node_features.dtype == torch.float32 else node_features.float()
        guard = guard and exchange is None and self._guarded(plan) and not torch.cuda.is_current_stream_capturing()
        reader = None
        if guard:
            flag = _native.range_flag(device)
            flag.zero_()
            reader = _native.RangeFlagRead(flag)
        out = self._forward_planned(x, plan, exchange, before_last=reader.arm if reader is not None else None,
                                    rows_per_layer=rows_per_layer)
        if guard:
            bits = reader.value()
            self.last_range_flags = bits
            if bits:
                return self._forward_exact(x, plan, bits)
        return out

    def _forward_planned(self, x: torch.Tensor, plan: GraphPlan, exchange=None, before_last=None,
                         rows_per_layer: Optional[Sequence[int]] = None) -> torch.Tensor:
        """before_last(): called right before the last layer is enqueued (nothing after that point raises a range-guard
        bit on the block kernels: _native.RangeFlagRead); the wide-row path cuts rows inside its last layer and is not
        given an early point.  rows_per_layer: see forward_planned (the wide-row path runs every row of every layer)."""
        device = x.device
        if plan.block_nodes == 1 and _native.rs_supported(self.hidden_dim):
            return self._forward_wide(x, plan, exchange)
        text_embs = self.text_encoder(plan.unique_texts, device)     # [U, text_dim]
        # the 16-bit-piece kernels gather rows already cut into pieces: the input projection emits them for the first
        # layer, every layer's tail for the next
        split = plan.wlayout in _native.SPLIT_LAYOUTS
        hs = _native.alloc_split(x.size(0), self.hidden_dim, plan.wlayout, device) if split else None
        hs_next = torch.empty_like(hs) if split else None
        # All layers' generators first, on this stream: beside the input projection, which saturates HBM, the same small
        # latency-bound kernels took several times as long and the first message launch waited for them.
        weights = self.generate_batched(text_embs, plan.wlayout)
        h = _native.input_proj_fwd(x, self.input_proj.weight.detach(), self.input_proj.bias.detach(), h_split=hs,
                                   split_layout=plan.wlayout if split else 0)
        h_next = torch.empty_like(h)
        if rows_per_layer is not None:
            # A shrunk layer computes whole destination blocks: rows past its prefix gather rows the layer before left
            # unwritten.  Their results are never read by a row that matters, but they must stay finite (the range guard
            # inspects every row a layer writes): the buffers that have no value yet start as zeros.
            h_next.zero_()
            if split:
                hs_next.zero_()
        lo, hi = plan.row_lo, (plan.row_hi or plan.N)
        last = len(self.weight_generators) - 1
        for l, norm in enumerate(self.layer_norms):
            W, W_self, bias = weights[l]
            if l == last and before_last is not None:
                before_last()
            fused = split and exchange is None and l < last
            if rows_per_layer is not None:                # whole blocks (the block kernels' row ranges end on one or at N)
                lo, hi = 0, min(plan.N, -(-rows_per_layer[l] // plan.block_nodes) * plan.block_nodes)
            _native.message_layer_fwd(h, plan, W, W_self, bias, plan.wlayout, norm.weight.detach(),
                                      norm.bias.detach(), norm.eps, h_next, row0=lo, rows=hi - lo,
                                      h_split=hs, h_split_out=hs_next if fused else None)
            if exchange is not None:
                exchange(h_next)
                if split and l < last:
                    _native.split_rows(h_next, plan.wlayout, out=hs_next)
            h, h_next = h_next, h
            hs, hs_next = hs_next, hs
        return h

    def _forward_wide(self, x: torch.Tensor, plan: GraphPlan, exchange=None) -> torch.Tensor:
        """Wide rows (d % 128 == 0, d >= 256: BASELINE config 5): the relation-stationary layer of csrc/message_rs.hip —
        per-edge results in relation order with the weights read once per 128 edges, then destination sums + tail."""
        device = x.device
        if plan.rs is None:
            plan.rs = build_rs(plan)
        rs = plan.rs
        text_embs = self.text_encoder(plan.unique_texts, device)
        lo, hi = plan.row_lo, (plan.row_hi or plan.N)
        # rows travel between the layers already cut into fp16 pieces (written by the input projection / pass 2's tail)
        # when one process computes every row; the fp32 MFMA variant gathers h itself
        exact = _native.rs_exact(plan)
        pieces = exchange is None and lo == 0 and hi == plan.N and not exact
        hs = _native.alloc_split(plan.N, self.hidden_dim, _native.WLAYOUT_SPLIT2H, device) if pieces else None
        hs_next = torch.empty_like(hs) if pieces else None
        h = _native.input_proj_fwd(x, self.input_proj.weight.detach(), self.input_proj.bias.detach(), h_split=hs,
                                   split_layout=_native.WLAYOUT_SPLIT2H if pieces else 0)
        h_next = torch.empty_like(h)
        Y = rs.scratch(plan.E, self.hidden_dim, device)
        last = len(self.layer_norms) - 1
        all_w = self.generate_batched(text_embs, _native.WLAYOUT_NATURAL)
        for l, norm in enumerate(self.layer_norms):
            W_msg, W_self, bias = all_w[l]
            if plan.E > 0:
                _native.edge_transform_fwd(h, rs, W_msg, W_self, bias, Y, h_split=hs, exact=exact)
            _native.segment_tail_fwd(Y, rs, h, norm.weight.detach(), norm.bias.detach(), norm.eps, h_next, row0=lo, rows=hi - lo,
                                     h_split_out=hs_next if pieces and l < last else None, exact=exact)
            if exchange is not None:
                exchange(h_next)
            h, h_next = h_next, h
            hs, hs_next = hs_next, hs
        return h

    # -- reference-internal seam kept for API parity (reference :160-230) ---------------------
    def _message_passing(self, h: torch.Tensor, edge_index: torch.Tensor, rel_weights: Dict[str, torch.Tensor]) -> torch.Tensor:
        """agg + self_out for per-EDGE weights ``W_msg [E,d,d]``, ``W_self [E,d,d]``, ``bias [E,d]``.

        Every edge is treated as its own relation on the generic kernel (no residual/norm);
        needs N*E < 2^32, which per-edge [E,d,d] inputs never approach."""
        require_inference(self, h, what="._message_passing")
        N, E = h.size(0), edge_index.size(1)
        rel = torch.arange(E, dtype=torch.int64, device=h.device)
        plan = build_plan(edge_index, rel, [""] * E, N, h.size(1), h.device, force_generic=True)
        out = torch.empty_like(h)
        return _native.message_layer_fwd(h, plan, rel_weights["W_msg"].contiguous(), rel_weights["W_self"].contiguous(),
                                         rel_weights["bias"].contiguous(), _native.WLAYOUT_NATURAL, None, None, 0.0,
                                         out, flags=_native.GHF_FLAG_NO_TAIL)

    # -- convenience (reference :304-322) ---------------------------------------------------
    def score_triple(self, head_emb: torch.Tensor, tail_emb: torch.Tensor) -> torch.Tensor:
        """Dot-product score of (head, tail) embeddings, ``[d]`` or ``[B, d]`` (reference :304-318)."""
        for t in (head_emb, tail_emb):
            if not t.is_cuda:
                raise RuntimeError(f"score_triple computes on an MI355X HIP device only (input is on {t.device})")
        if head_emb.shape != tail_emb.shape or head_emb.dim() not in (1, 2):
            raise ValueError(f"score_triple: shapes {tuple(head_emb.shape)} and {tuple(tail_emb.shape)}")
        single = head_emb.dim() == 1
        a = (head_emb.unsqueeze(0) if single else head_emb).float()
        b = (tail_emb.unsqueeze(0) if single else tail_emb).float()
        if torch.is_grad_enabled() and (a.requires_grad or b.requires_grad):
            from ..autograd import ScorePairsFn
            s = ScorePairsFn.apply(a, b)
        else:
            s = _native.score_pairs_fwd(a, b)
        return s[0] if single else s

    def score_edges(self, embs: torch.Tensor, src: torch.Tensor, dst: torch.Tensor) -> torch.Tensor:
        """``score_triple(embs[src], embs[dst])`` (the reference's call form, demo.py:90-94) without materialising the
        two gathered ``[E, d]`` matrices — nor, when gradients are recorded, their index backward: the gradient is one
        gather pass over the pairs grouped by node (``autograd.ScoreEdgesFn``), reproducible."""
        if not embs.is_cuda:
            raise RuntimeError(f"score_edges computes on an MI355X HIP device only (input is on {embs.device})")
        if torch.is_grad_enabled() and embs.requires_grad:
            from ..autograd import ScoreEdgesFn
            return ScoreEdgesFn.apply(embs, src, dst)
        return _native.score_pairs_fwd(embs, embs, src.to(torch.int64), dst.to(torch.int64))

    # -- link prediction against every node (csrc/rank.hip; no counterpart in the reference, whose demo stops at the loss) --
    @staticmethod
    def _rank_ids(ids: torch.Tensor, rows: int, embs: torch.Tensor, name: str, bounds=None) -> torch.Tensor:
        """1-D node ids checked as indexing checks them (IndexError), negative ids wrapped: int64 on embs' device.  `bounds`:
        the ids' (smallest, largest), where the caller has read them already."""
        if not isinstance(ids, torch.Tensor) or ids.dim() != 1:
            raise ValueError(f"{name} must be a 1-D tensor of node ids, got {getattr(ids, 'shape', type(ids))}")
        if ids.dtype not in (torch.int32, torch.int64):
            raise TypeError(f"{name} must be int32 or int64, got {ids.dtype}")
        if ids.numel():
            lo, hi = bounds if bounds is not None else (int(v) for v in torch.aminmax(ids))
            if lo < -rows or hi >= rows:
                raise IndexError(f"{name} holds ids outside [-{rows}, {rows}) (range {lo}..{hi})")
        ids = ids.to(device=embs.device, dtype=torch.int64)
        return torch.where(ids < 0, ids + rows, ids)

    @staticmethod
    def _candidate_ids(candidates, embs: torch.Tensor) -> torch.Tensor:
        """``candidates=`` of the four all-node operations in the form the kernels take: node ids, strictly ascending, int64 on
        embs' device.  Given as a 1-D int32 / int64 tensor (any order, on any device; repeats collapse, negative ids wrap as
        in indexing, an id out of range is an IndexError) or as a bool mask of length N.  An empty set is a ValueError."""
        N = embs.size(0)
        if not isinstance(candidates, torch.Tensor) or candidates.dim() != 1:
            raise ValueError(f"candidates must be a 1-D tensor of node ids or a bool mask of length N = {N}, got "
                             f"{getattr(candidates, 'shape', type(candidates))}")
        if candidates.dtype == torch.bool:
            if candidates.numel() != N:
                raise ValueError(f"a candidates mask must have length N = {N}, got {candidates.numel()}")
            ids = torch.nonzero(candidates.to(embs.device)).flatten()
        elif candidates.dtype in (torch.int32, torch.int64):
            if candidates.numel():
                lo, hi = (int(v) for v in torch.aminmax(candidates))
                if lo < -N or hi >= N:
                    raise IndexError(f"candidates holds ids outside [-{N}, {N}) (range {lo}..{hi})")
            ids = candidates.to(device=embs.device, dtype=torch.int64)
            ids = torch.unique(torch.where(ids < 0, ids + N, ids))          # sorted ascending, repeats gone
        else:
            raise TypeError(f"candidates must be int32, int64 or bool, got {candidates.dtype}")
        if ids.numel() == 0:
            raise ValueError("candidates is empty")
        return ids.contiguous()

    @staticmethod
    def _negative_ids(negatives, B: int, embs: torch.Tensor, bounds=None) -> torch.Tensor:
        """``negatives=`` of ``rank_candidates``, ``softmax_loss`` and ``negative_sampling_loss`` in the form the kernels take:
        int64 ``[B, K]``, ``K >= 1``, contiguous, on embs' device; row ``i`` is query ``i``'s own set.  An entry is a node id in
        ``[0, N)`` or exactly ``-1``, "no entry" (padding for ragged sets).  Negative ids do NOT wrap here, unlike everywhere
        else in this class, because ``-1`` is the padding: an id outside ``{-1} | [0, N)`` is an IndexError (one ``aminmax``, as
        ``_candidate_ids``; `bounds` = its result where the caller has it).  Nothing is sorted or de-duplicated: a row is a
        multiset in the given order."""
        N = embs.size(0)
        if not isinstance(negatives, torch.Tensor) or negatives.dim() != 2 or negatives.size(0) != B or negatives.size(1) < 1:
            raise ValueError(f"negatives must be a 2-D tensor [B = {B}, K >= 1] of node ids (-1 = no entry), got "
                             f"{getattr(negatives, 'shape', type(negatives))}")
        if negatives.dtype not in (torch.int32, torch.int64):
            raise TypeError(f"negatives must be int32 or int64, got {negatives.dtype}")
        lo, hi = bounds if bounds is not None else ((int(v) for v in torch.aminmax(negatives)) if negatives.numel() else (0, 0))
        if lo < -1 or hi >= N:
            raise IndexError(f"negatives holds ids outside [0, {N}) other than the padding -1 (range {lo}..{hi}; negative ids do "
                             "not wrap here)")
        return negatives.to(device=embs.device, dtype=torch.int64).contiguous()

    @classmethod
    def _negatives_arg(cls, negatives, candidates, query, target, embs: torch.Tensor):
        """``negatives=`` with the queries and targets it belongs to, checked without a device and ahead of every device
        check: None without the keyword, else ``(negatives, query, target)`` in the kernels' form.  Not together with
        ``candidates``; ``query`` and ``target`` go through ``_rank_ids`` exactly as without the keyword (the same forms
        accepted, the same errors), ``negatives`` through ``_negative_ids``.  Each of the three checks needs the smallest and
        largest id, and reading a device value costs a synchronisation — three of them were 0.14 ms of a 0.33 ms call at
        B = 1,024 x K = 1,000 — so where the three tensors share a device the six values are read at once."""
        if negatives is None:
            return None
        if candidates is not None:
            raise ValueError("pass either negatives= (a set per query) or candidates= (one set for all queries), not both")
        N, bounds = embs.size(0), (None, None, None)
        ids = (query, target, negatives)
        if (all(isinstance(x, torch.Tensor) and x.dtype in (torch.int32, torch.int64) and x.numel() for x in ids)
                and query.device == target.device == negatives.device):
            v = torch.stack([m.to(torch.int64) for x in ids for m in torch.aminmax(x)]).tolist()
            bounds = ((v[0], v[1]), (v[2], v[3]), (v[4], v[5]))
        q = cls._rank_ids(query, N, embs, "query", bounds[0])
        t = cls._rank_ids(target, N, embs, "target", bounds[1])
        if q.numel() != t.numel():
            raise ValueError(f"{q.numel()} queries and {t.numel()} targets")
        return cls._negative_ids(negatives, q.numel(), embs, bounds[2]), q, t

    @staticmethod
    def _distance_arg(distance, negatives, candidates, candidate_bias, embs: torch.Tensor) -> Optional[int]:
        """``distance=`` of ``rank_candidates``, ``softmax_loss`` and ``negative_sampling_loss``: None without the keyword, else
        the metric of the ``ghf_dist_*`` calls (``include/ghf_distance.h``).  Only metadata is looked at, ahead of every device
        check.  The keyword goes with ``negatives=`` alone: the all-node and shared-set sweeps are matrix-core tiles and score
        by dot product, and no distance call takes a per-candidate bias."""
        if distance is None:
            return None
        metric = _native.DIST_METRICS.get(distance) if isinstance(distance, str) else None
        if metric is None:
            raise ValueError(f"distance must be one of {sorted(_native.DIST_METRICS)} or None, got {distance!r}")
        if negatives is None or candidates is not None or candidate_bias is not None:
            raise ValueError("distance= needs negatives= (a set per query) and goes with neither candidates= nor candidate_bias=: "
                             "the all-node and shared-set sweeps of this method score by dot product; rank_by_distance / "
                             "topk_by_distance rank against every node, or a candidates= subset, under a distance")
        if metric == _native.DIST_COMPLEX and embs.size(1) % 2:
            raise ValueError(f'distance="complex" reads a row as interleaved re / im pairs and needs an even d, got {embs.size(1)}')
        return metric

    @staticmethod
    def _candidate_bias(candidate_bias, embs: torch.Tensor) -> Optional[torch.Tensor]:
        """``candidate_bias=`` of the four all-node operations: a 1-D fp32 tensor with one entry per NODE (length ``N``, also
        with ``candidates=``) on ``embs``' device, made contiguous.  Only metadata is looked at — no device work, no
        synchronisation; what the values may be (``-inf`` removes a node, NaN is outside the contract) is the kernels' rule."""
        if candidate_bias is None:
            return None
        N = embs.size(0)
        b = candidate_bias
        if (not isinstance(b, torch.Tensor) or b.dim() != 1 or b.numel() != N or b.dtype != torch.float32
                or b.device != embs.device):
            got = f"{tuple(b.shape)} {b.dtype} on {b.device}" if isinstance(b, torch.Tensor) else type(b).__name__
            raise ValueError(f"candidate_bias must be a float32 tensor of shape [N] = [{N}] on {embs.device}, got {got}")
        return b.contiguous()

    @staticmethod
    def _softmax_candidates(cand: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        """The candidate set of ``softmax_loss(candidates=)``: the given ids (``_candidate_ids``' form) and every target of the
        batch, ascending.  A query's own target has to be in its sum; the other queries' targets come in with it, as in-batch
        negatives."""
        return torch.unique(torch.cat([cand, target]))

    @staticmethod
    def _rel_ids(ids: torch.Tensor, n: int, embs: torch.Tensor, name: str) -> torch.Tensor:
        """1-D relation ids, one per entry: int64 on embs' device.  The id space is the caller's (``plan.rel_ids``, the ids
        passed to ``forward_ids``); relation ids do not wrap: a negative one is a ValueError."""
        if not isinstance(ids, torch.Tensor) or ids.dim() != 1:
            raise ValueError(f"{name} must be a 1-D tensor of relation ids, got {getattr(ids, 'shape', type(ids))}")
        if ids.dtype not in (torch.int32, torch.int64):
            raise TypeError(f"{name} must be int32 or int64, got {ids.dtype}")
        if ids.numel() != n:
            raise ValueError(f"{name} holds {ids.numel()} relation ids, expected {n}")
        if ids.numel() and int(ids.min()) < 0:
            raise ValueError(f"{name} holds a negative relation id (relation ids do not wrap)")
        return ids.to(device=embs.device, dtype=torch.int64)

    @staticmethod
    def _query_rows(embs: torch.Tensor, query: torch.Tensor, query_rows: Optional[torch.Tensor], what: str) -> None:
        """``query_rows`` ([B, d] fp32, one row per query, on embs' device) stands in for the gathered rows ``embs[query]``."""
        if query_rows is None:
            return
        B = query.numel() if isinstance(query, torch.Tensor) else -1
        if not isinstance(query_rows, torch.Tensor) or query_rows.dim() != 2 or tuple(query_rows.shape) != (B, embs.size(1)):
            raise ValueError(f"{what}: query_rows must be [B = {B}, d = {embs.size(1)}], one row per query, got "
                             f"{getattr(query_rows, 'shape', type(query_rows))}")
        if query_rows.dtype != torch.float32:
            raise TypeError(f"{what}: query_rows must be float32, got {query_rows.dtype}")
        if not query_rows.is_cuda or query_rows.device != embs.device:
            raise RuntimeError(f"{what} computes on an MI355X HIP device only (query_rows is on {query_rows.device}, embs on "
                               f"{embs.device})")

    @staticmethod
    def _known_form(known, filt_ptr, filt_idx, query_rel) -> bool:
        """Which of known / CSR lists / query_rel go together (no tensor is read); whether ``known`` is the typed form."""
        if known is not None and (filt_ptr is not None or filt_idx is not None):
            raise ValueError("pass either known=(src, dst) or filt_ptr / filt_idx, not both")
        typed = known is not None and len(known) == 3
        if query_rel is not None and not typed:
            raise ValueError("query_rel needs the typed known=(src, dst, rel)")
        if typed and query_rel is None:
            raise ValueError("known=(src, dst, rel) needs query_rel: the relation of every query")
        return typed

    @classmethod
    def _filter_lists(cls, embs: torch.Tensor, query: torch.Tensor, known, filt_ptr, filt_idx, query_rel=None):
        """Each query's filter list in the form the kernels take (CSR, every list sorted ascending), built on the device.
        `known` = (src, dst) names true edges: query[i]'s list is every dst of an edge whose src is query[i] (pass the
        edges in both directions for an undirected reading).  `known` = (src, dst, rel) with `query_rel` [B] is the typed
        form: query[i]'s list is every dst of an edge with src == query[i] AND rel == query_rel[i] (for (?, r, t) queries
        pass known=(dst, src, rel))."""
        N, B = embs.size(0), query.numel()
        typed = cls._known_form(known, filt_ptr, filt_idx, query_rel)
        if known is not None:
            if len(known) not in (2, 3):
                raise ValueError(f"known must be (src, dst) or (src, dst, rel), got {len(known)} members")
            src, dst = known[0], known[1]
            src = cls._rank_ids(src, N, embs, "known[0]")
            dst = cls._rank_ids(dst, N, embs, "known[1]")
            if src.numel() != dst.numel():
                raise ValueError(f"known: {src.numel()} sources and {dst.numel()} destinations")
            qkey = query
            if typed:
                rel = cls._rel_ids(known[2], src.numel(), embs, "known[2]")
                qrel = cls._rel_ids(query_rel, B, embs, "query_rel")
                R = 1 + max(int(rel.max()) if rel.numel() else 0, int(qrel.max()) if B else 0)
                if (N * R + R) * N >= 1 << 63:
                    raise ValueError(f"known: {N} nodes x {R} relations do not fit the 64-bit (src, rel, dst) keys")
                src, qkey = src * R + rel, query * R + qrel
            key = torch.unique(src * N + dst)                       # sorted by (src[, rel], dst), repeats gone
            ks = torch.div(key, N, rounding_mode="floor")
            lo = torch.searchsorted(ks, qkey)
            lens = torch.searchsorted(ks, qkey, right=True) - lo
            ptr = torch.zeros(B + 1, dtype=torch.int64, device=embs.device)
            torch.cumsum(lens, 0, out=ptr[1:])
            nnz = int(ptr[-1])
            if nnz == 0:
                return None, None
            pos = torch.arange(nnz, device=embs.device) + torch.repeat_interleave(lo - ptr[:-1], lens, output_size=nnz)
            return ptr, (key[pos] - ks[pos] * N).contiguous()
        if filt_ptr is None and filt_idx is None:
            return None, None
        if filt_ptr is None or filt_idx is None:
            raise ValueError("filt_ptr and filt_idx come together")
        if filt_ptr.dim() != 1 or filt_ptr.numel() != B + 1 or filt_ptr.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"filt_ptr must hold B + 1 = {B + 1} integer offsets, got {tuple(filt_ptr.shape)} {filt_ptr.dtype}")
        idx = cls._rank_ids(filt_idx, N, embs, "filt_idx")
        ptr = filt_ptr.to(device=embs.device, dtype=torch.int64).contiguous()
        lens = ptr[1:] - ptr[:-1]
        nnz = idx.numel()
        if int(ptr[0]) != 0 or int(ptr[-1]) != nnz or (nnz and int(lens.min()) < 0):
            raise ValueError(f"filt_ptr must rise from 0 to filt_idx.numel() = {nnz}")
        if nnz == 0:
            return None, None
        seg = torch.repeat_interleave(torch.arange(B, device=embs.device), lens, output_size=nnz)
        key = torch.sort(seg * N + idx).values                      # every list ascending, the lists in place
        return ptr, (key - seg * N).contiguous()

    def rank_candidates(self, embs: torch.Tensor, query: torch.Tensor, target: torch.Tensor, *, known=None,
                        filt_ptr: Optional[torch.Tensor] = None, filt_idx: Optional[torch.Tensor] = None,
                        query_rows: Optional[torch.Tensor] = None, query_rel: Optional[torch.Tensor] = None,
                        candidates: Optional[torch.Tensor] = None, candidate_bias: Optional[torch.Tensor] = None,
                        negatives: Optional[torch.Tensor] = None, distance: Optional[str] = None):
        """Where ``target[i]`` ranks among ALL nodes as a partner of ``query[i]`` under the dot-product score
        (``score_triple``): ``(greater, equal)``, int64 ``[B]`` — the nodes scoring above / exactly as the target, the target
        itself and the query's known partners (the "filtered" setting) left out.  ``known=(src, dst)`` names true edges
        (the query's list = every ``dst`` whose ``src`` is the query); or pass CSR lists as ``filt_ptr`` / ``filt_idx``.
        Feed the counts to ``link_prediction_metrics``.  One tiled ``q . c^T`` on the fp32 matrix cores with the comparison
        in its epilogue (``ghf_score_rank``): the ``[B, N]`` scores are never stored.  The counts carry no autograd graph
        (``embs`` is read as data).

        Relation-typed queries ``(head, relation, ?)``: ``query_rows`` (``[B, d]`` fp32, ``RelationDecoder``'s output) replaces
        the gathered rows ``embs[query]`` as the sweep's query matrix; ``query`` still names the node each row stands for and
        is used only to build the filter lists.  ``known=(src, dst, rel)`` with ``query_rel`` (``[B]`` relation ids, in the
        caller's id space, e.g. ``plan.rel_ids``) lists for query ``i`` every ``dst`` of a known edge with ``src == query[i]``
        and ``rel == query_rel[i]``.  For ``(?, relation, tail)`` queries (``direction="head"``) pass ``known=(dst, src, rel)``.
        With both ``None`` the call is the untyped one.

        ``candidates`` (node ids in any order, or a bool mask of length N) restricts the count to those nodes: the rank of
        the true partner among sampled negatives, or among the nodes of one type (``ghf_score_rank_sub``).  The result is
        that of the call on the table ``embs[sorted(candidates)]``, except that ``target`` and the lists stay node ids of
        ``embs``: the target may be any node, a candidate or not (its score comes from its own row), and listed nodes that
        are no candidates take no part.  The candidate rows are read in place; no ``[C, d]`` copy is made.

        ``candidate_bias`` (fp32 ``[N]``, one entry per node, also with ``candidates``): every score becomes
        ``embs[query[i]] . embs[j] + candidate_bias[j]`` — one fp32 add behind the dot product — and the target's score is
        formed the same way from its own entry (``ghf_score_rank_b``): a trained entity bias, a popularity prior, a type
        penalty.  ``-inf`` on a node that is no query's target takes it out of both counts.  A bias of zeros returns the
        counts of the call without the keyword.

        ``negatives`` (int32 / int64 ``[B, K]``, not together with ``candidates``): query ``i`` is ranked against ITS OWN set,
        row ``i`` — the protocol of OGB ``wikikg2`` / ``biokg`` / ``citation2``, whose test triples come with their 500 /
        1,000 negatives.  An entry is a node id in ``[0, N)`` or exactly ``-1`` for "no entry" (padding for ragged sets);
        negative ids do NOT wrap here, an id outside ``{-1} | [0, N)`` is an IndexError.  A row is a multiset in the given
        order: an id that occurs three times counts three times, nothing is sorted or de-duplicated.  Positions that hold
        the target or one of the query's ``known`` partners take no part.  A gather-and-dot kernel, one wave per query
        (``ghf_neg_rank``, ``include/ghf_negatives.h``): each candidate row is read once, the query row once per query.  The
        scores are fp32 dot products in an order that depends on ``d`` alone; they agree with the all-node sweep's to
        rounding.  ``query_rows``, typed ``known`` and ``candidate_bias`` work as above.

        ``distance`` (``"l1"``, ``"l2"`` or ``"complex"``; with ``negatives`` only, and not with ``candidate_bias``): the score
        becomes ``-D(row_i, embs[j])``, the distance of TransE (``"l1"`` / ``"l2"`` of ``row_i - embs[j]``) or of RotatE
        (``"complex"``: the sum of the moduli of the ``d / 2`` interleaved re / im pairs, ``d`` even), so a candidate ranks
        above the target when it lies CLOSER to the query's row (``ghf_dist_rank``, ``include/ghf_distance.h``).  The
        translated or rotated query rows are the caller's, through ``query_rows``.  The all-node and shared-set sweeps score by
        dot product: without ``negatives`` the keyword is a ``ValueError``."""
        if embs.dim() != 2:
            raise ValueError(f"embs must be [N, d], got {tuple(embs.shape)}")
        metric = self._distance_arg(distance, negatives, candidates, candidate_bias, embs)
        bias = self._candidate_bias(candidate_bias, embs)
        pre = self._negatives_arg(negatives, candidates, query, target, embs)
        cand = None if candidates is None else self._candidate_ids(candidates, embs)
        if not embs.is_cuda:
            raise RuntimeError(f"rank_candidates computes on an MI355X HIP device only (input is on {embs.device})")
        self._query_rows(embs, query, query_rows, "rank_candidates")
        e = embs.detach().float()
        if pre is not None:
            neg, q, t = pre
        else:
            neg = None
            q = self._rank_ids(query, e.size(0), e, "query")
            t = self._rank_ids(target, e.size(0), e, "target")
            if q.numel() != t.numel():
                raise ValueError(f"{q.numel()} queries and {t.numel()} targets")
        ptr, idx = self._filter_lists(e, q, known, filt_ptr, filt_idx, query_rel)
        if metric is not None:
            if query_rows is not None:
                return _native.score_dist_rank(metric, query_rows.detach(), e, t, neg, filt_ptr=ptr, filt_idx=idx)
            return _native.score_dist_rank(metric, e, e, t, neg, iq=q, filt_ptr=ptr, filt_idx=idx)
        if neg is not None:
            if query_rows is not None:
                return _native.score_neg_rank(query_rows.detach(), e, t, neg, filt_ptr=ptr, filt_idx=idx, bias=bias)
            return _native.score_neg_rank(e, e, t, neg, iq=q, filt_ptr=ptr, filt_idx=idx, bias=bias)
        if query_rows is not None:
            return _native.score_rank(query_rows.detach(), e, t, filt_ptr=ptr, filt_idx=idx, ic=cand, bias=bias)
        return _native.score_rank(e, e, t, iq=q, filt_ptr=ptr, filt_idx=idx, ic=cand, bias=bias)

    def topk_candidates(self, embs: torch.Tensor, query: torch.Tensor, k: int, *, known=None,
                        filt_ptr: Optional[torch.Tensor] = None, filt_idx: Optional[torch.Tensor] = None,
                        query_rows: Optional[torch.Tensor] = None, query_rel: Optional[torch.Tensor] = None,
                        candidates: Optional[torch.Tensor] = None, candidate_bias: Optional[torch.Tensor] = None):
        """The ``k`` (1..128) best partners of every ``query[i]`` among ALL nodes outside its filter list (``known`` /
        ``filt_ptr, filt_idx`` as in ``rank_candidates``): ``(scores [B, k]`` fp32 descending, ``ids [B, k]`` int64``)``, ties
        towards the lower id, ``(-inf, -1)`` where fewer than k candidates remain.  The query node itself is a candidate
        unless listed.  No autograd graph.  ``query_rows`` / ``known=(src, dst, rel)`` with ``query_rel``: relation-typed
        queries, as in ``rank_candidates``.  ``candidates`` (ids or a bool mask, as in ``rank_candidates``): the k best among
        those nodes only, e.g. the cities for ``(person, born in, ?)``; the ids returned are node ids of ``embs``, ties still go
        to the lower node id, and ``(-inf, -1)`` fills up where fewer than k candidates remain outside the list.
        ``candidate_bias`` (fp32 ``[N]``, as in ``rank_candidates``): nodes are ordered by, and ``scores`` holds,
        ``embs[query[i]] . embs[j] + candidate_bias[j]`` (``ghf_score_topk_b``); a node whose entry is ``-inf`` is never
        returned — "never propose this node" without a filter list per query."""
        if embs.dim() != 2:
            raise ValueError(f"embs must be [N, d], got {tuple(embs.shape)}")
        bias = self._candidate_bias(candidate_bias, embs)
        cand = None if candidates is None else self._candidate_ids(candidates, embs)
        if not embs.is_cuda:
            raise RuntimeError(f"topk_candidates computes on an MI355X HIP device only (input is on {embs.device})")
        self._query_rows(embs, query, query_rows, "topk_candidates")
        if not 1 <= int(k) <= 128:
            raise ValueError(f"k = {k} outside 1..128")
        e = embs.detach().float()
        q = self._rank_ids(query, e.size(0), e, "query")
        ptr, idx = self._filter_lists(e, q, known, filt_ptr, filt_idx, query_rel)
        if query_rows is not None:
            return _native.score_topk(query_rows.detach(), e, int(k), filt_ptr=ptr, filt_idx=idx, ic=cand, bias=bias)
        return _native.score_topk(e, e, int(k), iq=q, filt_ptr=ptr, filt_idx=idx, ic=cand, bias=bias)

    # -- distance scores against every node (csrc/distance_sweep.hip): TransE / RotatE evaluation --------------------------
    @staticmethod
    def _sweep_metric(distance, embs: torch.Tensor) -> int:
        """``distance`` of ``rank_by_distance`` / ``topk_by_distance``: the metric of the ``ghf_dist_sweep_*`` calls.  Only
        metadata is looked at, ahead of every device check."""
        if embs.dim() != 2:
            raise ValueError(f"embs must be [N, d], got {tuple(embs.shape)}")
        metric = _native.DIST_METRICS.get(distance) if isinstance(distance, str) else None
        if metric is None:
            raise ValueError(f"distance must be one of {sorted(_native.DIST_METRICS)}, got {distance!r}")
        if metric == _native.DIST_COMPLEX and embs.size(1) % 2:
            raise ValueError(f'distance="complex" reads a row as interleaved re / im pairs and needs an even d, got {embs.size(1)}')
        return metric

    def rank_by_distance(self, embs: torch.Tensor, query: torch.Tensor, target: torch.Tensor, distance: str, *, known=None,
                         filt_ptr: Optional[torch.Tensor] = None, filt_idx: Optional[torch.Tensor] = None,
                         query_rows: Optional[torch.Tensor] = None, query_rel: Optional[torch.Tensor] = None,
                         candidates: Optional[torch.Tensor] = None):
        """``rank_candidates`` under a DISTANCE: where ``target[i]`` ranks among ALL nodes (or ``candidates``) when a node scores
        ``-D(row_i, embs[j])`` — the filtered rank TransE and RotatE are reported by (FB15k-237, WN18RR).  ``distance`` is
        ``"l1"``, ``"l2"`` (TransE) or ``"complex"`` (RotatE: the sum of the moduli of the ``d / 2`` interleaved re / im pairs,
        ``d`` even).  ``(greater, equal)``, int64 ``[B]``: the nodes CLOSER to the query's row than / exactly as far as the
        target, the target itself and the query's known partners left out; feed them to ``link_prediction_metrics``.

        The translated or rotated query rows are the caller's, through ``query_rows`` (``[B, d]`` fp32: ``embs[h] + r`` or
        ``embs[h] o r``); without it row ``i`` is ``embs[query[i]]``.  ``known`` / ``filt_ptr, filt_idx`` / ``query_rel`` /
        ``candidates`` are ``rank_candidates``' keywords with the same meaning.  There is no ``candidate_bias`` and no
        ``negatives`` here (``rank_candidates(negatives=, distance=)`` ranks against a set per query).

        A register-tiled VALU sweep (``ghf_dist_sweep_rank``, ``include/ghf_distance_sweep.h``): every candidate row is read
        once per 64 queries and the ``[B, N]`` distances are never stored.  A pair's distance is one fixed fp32 chain, so two
        nodes at the same distance tie exactly and the same call gives the same counts whatever the batch.  No autograd graph
        (``embs`` is read as data)."""
        metric = self._sweep_metric(distance, embs)
        self._known_form(known, filt_ptr, filt_idx, query_rel)
        cand = None if candidates is None else self._candidate_ids(candidates, embs)
        q = self._rank_ids(query, embs.size(0), embs, "query")
        t = self._rank_ids(target, embs.size(0), embs, "target")
        if q.numel() != t.numel():
            raise ValueError(f"{q.numel()} queries and {t.numel()} targets")
        if not embs.is_cuda:
            raise RuntimeError(f"rank_by_distance computes on an MI355X HIP device only (input is on {embs.device})")
        self._query_rows(embs, query, query_rows, "rank_by_distance")
        e = embs.detach().float()
        ptr, idx = self._filter_lists(e, q, known, filt_ptr, filt_idx, query_rel)
        if query_rows is not None:
            return _native.score_dist_sweep_rank(metric, query_rows.detach(), e, t, filt_ptr=ptr, filt_idx=idx, ic=cand)
        return _native.score_dist_sweep_rank(metric, e, e, t, iq=q, filt_ptr=ptr, filt_idx=idx, ic=cand)

    def topk_by_distance(self, embs: torch.Tensor, query: torch.Tensor, k: int, distance: str, *, known=None,
                         filt_ptr: Optional[torch.Tensor] = None, filt_idx: Optional[torch.Tensor] = None,
                         query_rows: Optional[torch.Tensor] = None, query_rel: Optional[torch.Tensor] = None,
                         candidates: Optional[torch.Tensor] = None):
        """``topk_candidates`` under a DISTANCE: the ``k`` (1..128) NEAREST nodes of every query's row among all nodes (or
        ``candidates``) outside its filter list.  ``(scores [B, k]`` fp32 ``= -D`` descending, i.e. nearest first, ``ids [B, k]``
        int64``)``, ties towards the lower id, ``(-inf, -1)`` where fewer than k candidates remain.  ``distance`` and every
        keyword as in ``rank_by_distance``; the query's own node is a candidate (at distance 0 without ``query_rows``) unless
        listed.  ``ghf_dist_sweep_topk``; no autograd graph."""
        metric = self._sweep_metric(distance, embs)
        if not 1 <= int(k) <= 128:
            raise ValueError(f"k = {k} outside 1..128")
        self._known_form(known, filt_ptr, filt_idx, query_rel)
        cand = None if candidates is None else self._candidate_ids(candidates, embs)
        q = self._rank_ids(query, embs.size(0), embs, "query")
        if not embs.is_cuda:
            raise RuntimeError(f"topk_by_distance computes on an MI355X HIP device only (input is on {embs.device})")
        self._query_rows(embs, query, query_rows, "topk_by_distance")
        e = embs.detach().float()
        ptr, idx = self._filter_lists(e, q, known, filt_ptr, filt_idx, query_rel)
        if query_rows is not None:
            return _native.score_dist_sweep_topk(metric, query_rows.detach(), e, int(k), filt_ptr=ptr, filt_idx=idx, ic=cand)
        return _native.score_dist_sweep_topk(metric, e, e, int(k), iq=q, filt_ptr=ptr, filt_idx=idx, ic=cand)

    def _by_distance_loss(self, what: str, mode: int, embs, query, target, distance, scale, margin, alpha, known, filt_ptr,
                          filt_idx, query_rows, query_rel, candidates) -> torch.Tensor:
        """``softmax_loss_by_distance`` / ``negative_sampling_loss_by_distance``: every check on metadata ahead of the device
        check, then the recorded call (``autograd.DistanceSweepLossFn``) or the forward alone."""
        metric = self._sweep_metric(distance, embs)
        self._known_form(known, filt_ptr, filt_idx, query_rel)
        scale, margin, alpha = float(scale), float(margin), float(alpha)
        if not (0.0 < scale < float("inf")):
            raise ValueError(f"scale must be finite and positive, got {scale}")
        if not (float("-inf") < margin < float("inf")):
            raise ValueError(f"margin must be finite, got {margin}")
        if not (0.0 <= alpha < float("inf")):
            raise ValueError(f"adversarial_temperature must be finite and not negative, got {alpha}")
        cand = None if candidates is None else self._candidate_ids(candidates, embs)
        q = self._rank_ids(query, embs.size(0), embs, "query")
        t = self._rank_ids(target, embs.size(0), embs, "target")
        if q.numel() != t.numel():
            raise ValueError(f"{q.numel()} queries and {t.numel()} targets")
        self._query_rows(embs, query, query_rows, what)
        if not embs.is_cuda:
            raise RuntimeError(f"{what} computes on an MI355X HIP device only (input is on {embs.device})")
        ptr, idx = self._filter_lists(embs, q, known, filt_ptr, filt_idx, query_rel)
        if cand is not None:
            cand = self._softmax_candidates(cand, t)
        grad = embs.requires_grad or (query_rows is not None and query_rows.requires_grad)
        if torch.is_grad_enabled() and grad:
            from ..autograd import DistanceSweepLossFn
            if query_rows is not None:
                return DistanceSweepLossFn.apply(embs, query_rows, None, t, ptr, idx, metric, mode, scale, margin, alpha, cand)
            return DistanceSweepLossFn.apply(embs, None, q, t, ptr, idx, metric, mode, scale, margin, alpha, cand)
        e = embs.detach().float()
        qm, iq = (e, q) if query_rows is None else (query_rows.detach(), None)
        if mode == _native.NEG_SOFTMAX:
            return _native.score_dist_loss_softmax_fwd(metric, qm, e, t, iq=iq, filt_ptr=ptr, filt_idx=idx, scale=scale, ic=cand)[0]
        return _native.score_dist_loss_negsamp_fwd(metric, qm, e, t, iq=iq, filt_ptr=ptr, filt_idx=idx, scale=scale, margin=margin,
                                                   adversarial_temperature=alpha, ic=cand)[0]

    def softmax_loss_by_distance(self, embs: torch.Tensor, query: torch.Tensor, target: torch.Tensor, distance: str, *,
                                 scale: float = 1.0, known=None, filt_ptr: Optional[torch.Tensor] = None,
                                 filt_idx: Optional[torch.Tensor] = None, query_rows: Optional[torch.Tensor] = None,
                                 query_rel: Optional[torch.Tensor] = None,
                                 candidates: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``softmax_loss`` under a DISTANCE, fp32 ``[B]``: the 1-vs-all cross-entropy of the true tail against every node (or
        one ``candidates`` set shared by the batch) when a node scores ``-D(row_i, embs[j])``: ``loss[i] = logsumexp_j z[i, j]
        - z[i, target[i]]`` with ``z = -scale * D`` over the candidates outside query ``i``'s list; the target always stays in
        the sum.  ``distance`` is ``"l1"``, ``"l2"`` (TransE) or ``"complex"`` (RotatE, ``d`` even), as in ``rank_by_distance``,
        whose ``query_rows`` / ``known`` / ``filt_ptr, filt_idx`` / ``query_rel`` / ``candidates`` keywords mean the same here.
        With ``candidates`` the batch's targets are added to the set, as in ``softmax_loss``.  There is no ``negatives`` (a set
        per query is ``softmax_loss(negatives=, distance=)``) and no ``candidate_bias``.

        The tile sweep of ``rank_by_distance`` with an online softmax in its epilogue (``ghf_dist_loss_softmax_fwd``,
        ``include/ghf_distance_loss.h``): a candidate row is read once per 64 queries, and neither the ``[B, C]`` distances nor
        the ``[B, C, d]`` differences exist, forward or backward.  Recorded for autograd when grad mode is on and ``embs`` or
        ``query_rows`` requires grad (``autograd.DistanceSweepLossFn``, ``ghf_dist_loss_bwd``): the gradient follows the
        distance (``sign(delta)``, ``delta / D``, ``delta / |pair|``, each 0 where its denominator is 0); rows of ``embs`` that
        are neither candidate, target nor query get exactly zero.  Bit-reproducible, and a query's loss does not depend on its
        batch."""
        return self._by_distance_loss("softmax_loss_by_distance", _native.NEG_SOFTMAX, embs, query, target, distance, scale, 0.0, 0.0,
                                      known, filt_ptr, filt_idx, query_rows, query_rel, candidates)

    def negative_sampling_loss_by_distance(self, embs: torch.Tensor, query: torch.Tensor, target: torch.Tensor, distance: str, *,
                                           scale: float = 1.0, margin: float = 0.0, adversarial_temperature: float = 0.0,
                                           known=None, filt_ptr: Optional[torch.Tensor] = None,
                                           filt_idx: Optional[torch.Tensor] = None, query_rows: Optional[torch.Tensor] = None,
                                           query_rel: Optional[torch.Tensor] = None,
                                           candidates: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``negative_sampling_loss`` under a DISTANCE on one negative set shared by the batch (DGL-KE, the OGB ``wikikg2`` /
        ``biokg`` baselines), fp32 ``[B]``.  With ``z[i, j] = -scale * D(row_i, embs[j])`` and ``J_i`` = every node (every
        candidate) except query ``i``'s known partners and its target::

            w[i, j] = softmax over J_i of (adversarial_temperature * z[i, j])          # a constant: detached
            loss[i] = softplus(-(z[i, target[i]] + margin)) + sum_{j in J_i} w[i, j] * softplus(z[i, j] + margin)

        At ``scale=1, margin=gamma`` the positive term is ``-log sigmoid(gamma - D_target)``: TransE's and RotatE's published
        loss.  ``adversarial_temperature=0`` is the uniform mean; a query without negatives has the positive term alone.
        ``distance`` and every other keyword as in ``softmax_loss_by_distance``; ``ghf_dist_loss_negsamp_fwd`` /
        ``ghf_dist_loss_bwd``, recorded and reproducible the same way."""
        return self._by_distance_loss("negative_sampling_loss_by_distance", _native.NEG_NEGSAMP, embs, query, target, distance, scale,
                                      margin, adversarial_temperature, known, filt_ptr, filt_idx, query_rows, query_rel, candidates)

    def pairwise_loss_by_distance(self, embs: torch.Tensor, query: torch.Tensor, target: torch.Tensor, distance: str, *,
                                  loss: str = "hinge", margin: float = 1.0, scale: float = 1.0, normalize: bool = True, known=None,
                                  filt_ptr: Optional[torch.Tensor] = None, filt_idx: Optional[torch.Tensor] = None,
                                  query_rows: Optional[torch.Tensor] = None, query_rel: Optional[torch.Tensor] = None,
                                  candidates: Optional[torch.Tensor] = None, return_active: bool = False):
        """``pairwise_loss`` under a DISTANCE against every node, or one ``candidates`` set shared by the batch (the way DGL-KE
        and the OGB ``wikikg2`` / ``biokg`` baselines draw negatives), fp32 ``[B]``.  With ``z[i, j] = -scale * D(row_i,
        embs[j])`` and ``J_i`` = every node (every candidate) except query ``i``'s known partners and its target::

            u[i, j] = z[i, j] - z[i, target[i]] + margin
            loss[i] = mean over J_i of max(u, 0)          # loss="hinge": TransE's published max(0, gamma + D_pos - D_neg)
            loss[i] = mean over J_i of softplus(u)        # loss="logistic": the soft margin ranking loss

        ``normalize=False`` gives the sum instead of the mean; a query whose ``J_i`` is empty has loss exactly 0.  TransE with
        one shared negative set::

            rows = embs[head] + rel_vec[rel]
            loss = model.pairwise_loss_by_distance(embs, head, tail, "l1", margin=gamma, query_rows=rows, candidates=neg).mean()

        ``distance`` is ``"l1"``, ``"l2"`` or ``"complex"`` (RotatE, ``d`` even) and ``query_rows`` / ``known`` / ``filt_ptr,
        filt_idx`` / ``query_rel`` / ``candidates`` mean what they mean in ``softmax_loss_by_distance``; with ``candidates`` the
        batch's targets are added to the set.  ``return_active=True`` returns ``(loss, active)``, ``active`` int32 ``[B]`` the
        number of violated pairs ``u > 0``; at ``margin=0, scale=1`` it is ``rank_by_distance``'s ``greater``.  There is no
        ``negatives`` (a set per query is ``pairwise_loss(negatives=, distance=)``) and no ``candidate_bias``.

        The tile sweep of ``rank_by_distance`` with a pairwise epilogue (``ghf_dist_pair_fwd``,
        ``include/ghf_pairwise_sweep.h``): a candidate row is read once per 64 queries, and neither the ``[B, C]`` distances,
        ids or coefficients nor the ``[B, C, d]`` differences exist, forward or backward.  Recorded for autograd when grad mode
        is on and ``embs`` or ``query_rows`` requires grad (``autograd.DistancePairSweepLossFn``, ``ghf_dist_pair_bwd``); rows
        of ``embs`` that are neither candidate, target nor query get exactly zero.  Bit-reproducible, and a query's loss does
        not depend on its batch.  ``scale`` finite and ``> 0``, ``margin`` finite (``ValueError`` otherwise)."""
        what = "pairwise_loss_by_distance"
        metric = self._sweep_metric(distance, embs)
        kind = _native.PAIR_KINDS.get(loss) if isinstance(loss, str) else None
        if kind is None:
            raise ValueError(f"loss must be one of {sorted(_native.PAIR_KINDS)}, got {loss!r}")
        self._known_form(known, filt_ptr, filt_idx, query_rel)
        scale, margin = float(scale), float(margin)
        if not (0.0 < scale < float("inf")):
            raise ValueError(f"scale must be finite and positive, got {scale}")
        if not (float("-inf") < margin < float("inf")):
            raise ValueError(f"margin must be finite, got {margin}")
        if not isinstance(normalize, bool) or not isinstance(return_active, bool):
            raise TypeError(f"normalize and return_active must be bools, got {normalize!r} and {return_active!r}")
        cand = None if candidates is None else self._candidate_ids(candidates, embs)
        q = self._rank_ids(query, embs.size(0), embs, "query")
        t = self._rank_ids(target, embs.size(0), embs, "target")
        if q.numel() != t.numel():
            raise ValueError(f"{q.numel()} queries and {t.numel()} targets")
        self._query_rows(embs, query, query_rows, what)
        if not embs.is_cuda:
            raise RuntimeError(f"{what} computes on an MI355X HIP device only (input is on {embs.device})")
        ptr, idx = self._filter_lists(embs, q, known, filt_ptr, filt_idx, query_rel)
        if cand is not None:
            cand = self._softmax_candidates(cand, t)
        grad = embs.requires_grad or (query_rows is not None and query_rows.requires_grad)
        if torch.is_grad_enabled() and grad:
            from ..autograd import DistancePairSweepLossFn
            rows, iq = (None, q) if query_rows is None else (query_rows, None)
            out, active = DistancePairSweepLossFn.apply(embs, rows, iq, t, ptr, idx, metric, kind, scale, margin, normalize, cand)
        else:
            e = embs.detach().float()
            qm, iq = (e, q) if query_rows is None else (query_rows.detach(), None)
            out, _, _, active = _native.score_dist_pair_sweep_fwd(metric, kind, qm, e, t, iq=iq, filt_ptr=ptr, filt_idx=idx, scale=scale,
                                                                  margin=margin, normalize=normalize, ic=cand)
        return (out, active) if return_active else out

    def pairwise_loss_by_dot(self, embs: torch.Tensor, query: torch.Tensor, target: torch.Tensor, *, loss: str = "hinge",
                             margin: float = 1.0, scale: float = 1.0, normalize: bool = True, known=None,
                             filt_ptr: Optional[torch.Tensor] = None, filt_idx: Optional[torch.Tensor] = None,
                             query_rows: Optional[torch.Tensor] = None, query_rel: Optional[torch.Tensor] = None,
                             candidates: Optional[torch.Tensor] = None, candidate_bias: Optional[torch.Tensor] = None,
                             return_active: bool = False):
        """``pairwise_loss`` by DOT PRODUCT — this model's own score — against every node, or one ``candidates`` set shared by
        the batch (sampled or in-batch negatives, the way LightGCN, NGCF and PinSage train), fp32 ``[B]``.  With ``z[i, j] =
        scale * row_i . embs[j]`` (``fma(scale, ., candidate_bias[j])`` with a bias), ``row_i = embs[query[i]]`` or
        ``query_rows[i]``, and ``J_i`` = every node (every candidate) except query ``i``'s known partners and its target::

            u[i, j] = z[i, j] - z[i, target[i]] + margin
            loss[i] = mean over J_i of max(u, 0)          # loss="hinge": the max-margin ranking loss (PinSage, GraphSAGE)
            loss[i] = mean over J_i of softplus(u)        # loss="logistic": BPR at margin=0 (LightGCN, NGCF)

        ``normalize=False`` gives the sum instead of the mean; a query whose ``J_i`` is empty has loss exactly 0.  BPR with one
        shared negative set, on ``RelationDecoder`` rows::

            rows = decoder(embs, head, rel, rel_embs)
            loss = model.pairwise_loss_by_dot(embs, head, tail, loss="logistic", margin=0.0, query_rows=rows,
                                              candidates=neg).mean()

        ``query_rows`` / ``known`` / ``filt_ptr, filt_idx`` / ``query_rel`` / ``candidates`` / ``candidate_bias`` mean what
        they mean in ``negative_sampling_loss``; with ``candidates`` the batch's targets are added to the set, so another
        query's target is an in-batch negative unless that query's ``known`` lists it.  ``return_active=True`` returns ``(loss,
        active)``, ``active`` int32 ``[B]`` the number of violated pairs ``u > 0``; at ``margin=0, scale=1`` without a bias it
        is ``rank_candidates``' ``greater``.  There is no ``negatives`` here: a set per query is ``pairwise_loss(negatives=)``,
        which gathers every row once per query; this call reads a candidate row once per 128 queries.

        The matrix-core sweep of ``rank_candidates`` with a pairwise epilogue (``ghf_score_pair_fwd``,
        ``include/ghf_pairwise_dot_sweep.h``): neither the ``[B, C]`` scores, ids or coefficients nor the ``[C, d]`` gather
        exist, forward or backward.  Recorded for autograd when grad mode is on and ``embs``, ``query_rows`` or
        ``candidate_bias`` requires grad (``autograd.DotPairSweepLossFn``, ``ghf_score_pair_bwd``); rows of ``embs`` that are
        neither candidate, target nor query get exactly zero, and so do the bias entries of nodes outside the set.
        Bit-reproducible, a query's loss does not depend on its batch, and a bias of zeros gives the bits of the call without
        the keyword.  ``scale`` finite and ``> 0``, ``margin`` finite (``ValueError`` otherwise)."""
        what = "pairwise_loss_by_dot"
        if embs.dim() != 2:
            raise ValueError(f"embs must be [N, d], got {tuple(embs.shape)}")
        kind = _native.PAIR_KINDS.get(loss) if isinstance(loss, str) else None
        if kind is None:
            raise ValueError(f"loss must be one of {sorted(_native.PAIR_KINDS)}, got {loss!r}")
        self._known_form(known, filt_ptr, filt_idx, query_rel)
        scale, margin = float(scale), float(margin)
        if not (0.0 < scale < float("inf")):
            raise ValueError(f"scale must be finite and positive, got {scale}")
        if not (float("-inf") < margin < float("inf")):
            raise ValueError(f"margin must be finite, got {margin}")
        if not isinstance(normalize, bool) or not isinstance(return_active, bool):
            raise TypeError(f"normalize and return_active must be bools, got {normalize!r} and {return_active!r}")
        bias = self._candidate_bias(candidate_bias, embs)
        bias_grad = bias is not None and bias.requires_grad
        cand = None if candidates is None else self._candidate_ids(candidates, embs)
        q = self._rank_ids(query, embs.size(0), embs, "query")
        t = self._rank_ids(target, embs.size(0), embs, "target")
        if q.numel() != t.numel():
            raise ValueError(f"{q.numel()} queries and {t.numel()} targets")
        self._query_rows(embs, query, query_rows, what)
        if not embs.is_cuda:
            raise RuntimeError(f"{what} computes on an MI355X HIP device only (input is on {embs.device})")
        ptr, idx = self._filter_lists(embs, q, known, filt_ptr, filt_idx, query_rel)
        if cand is not None:
            cand = self._softmax_candidates(cand, t)
        grad = embs.requires_grad or (query_rows is not None and query_rows.requires_grad) or bias_grad
        if torch.is_grad_enabled() and grad:
            from ..autograd import DotPairSweepLossFn
            rows, iq = (None, q) if query_rows is None else (query_rows, None)
            out, active = DotPairSweepLossFn.apply(embs, rows, iq, t, ptr, idx, kind, scale, margin, normalize, cand, bias)
        else:
            e = embs.detach().float()
            qm, iq = (e, q) if query_rows is None else (query_rows.detach(), None)
            out, _, _, active = _native.score_pair_sweep_fwd(kind, qm, e, t, iq=iq, filt_ptr=ptr, filt_idx=idx, scale=scale,
                                                             margin=margin, normalize=normalize, ic=cand,
                                                             bias=None if bias is None else bias.detach())
        return (out, active) if return_active else out

    def softmax_loss(self, embs: torch.Tensor, query: torch.Tensor, target: torch.Tensor, *, scale: float = 1.0, known=None,
                     filt_ptr: Optional[torch.Tensor] = None, filt_idx: Optional[torch.Tensor] = None,
                     query_rows: Optional[torch.Tensor] = None, query_rel: Optional[torch.Tensor] = None,
                     candidates: Optional[torch.Tensor] = None, candidate_bias: Optional[torch.Tensor] = None,
                     negatives: Optional[torch.Tensor] = None, distance: Optional[str] = None) -> torch.Tensor:
        """The 1-vs-all softmax cross-entropy that ``rank_candidates``' filtered metrics measure, fp32 ``[B]``:
        ``loss[i] = logsumexp_j(scale * embs[query[i]] . embs[j]) - scale * embs[query[i]] . embs[target[i]]`` over ALL nodes
        ``j`` except ``query[i]``'s known partners (``known`` / ``filt_ptr, filt_idx`` as in ``rank_candidates``; the target
        itself always stays in the sum).  ``F.cross_entropy(scale * embs[query] @ embs.T, target)`` without the ``[B, N]``
        logits, forward or backward: one sweep on the fp32 matrix cores with an online softmax in its epilogue
        (``ghf_score_softmax_fwd``), and a backward that recomputes the scores from the saved log-sum (``ghf_score_softmax_bwd``,
        ``autograd.SoftmaxLossFn``).  Bit-reproducible.  Recorded for autograd when grad mode is on and ``embs`` requires grad.
        ``query_rows`` / ``known=(src, dst, rel)`` with ``query_rel``: relation-typed queries, as in ``rank_candidates``; the
        loss is then recorded when ``embs`` or ``query_rows`` requires grad (``autograd.SoftmaxLossFn`` with the rows: the per-query
        gradient is ``query_rows``' own, the per-candidate one ``embs``').

        ``candidates`` (ids in any order or a bool mask, as in ``rank_candidates``) turns the loss into the 1-vs-C one of
        sampled-negative training: the sum runs over the candidates instead of all nodes, at ``C / N`` of the cost
        (``ghf_score_softmax_fwd_sub`` / ``_bwd_sub``).  The batch's targets are ADDED to the set before the call, so every
        query's own target is in its sum — and every other query's target is an in-batch negative for it, unless that query's
        ``known`` lists it.  Everything else is the sub-table rule: ``target`` and the lists stay node ids, listed nodes
        outside the set take no part, the candidate rows are read in place (no ``[C, d]`` copy, forward or backward), and
        the gradient lands in ``embs``' own rows: rows that are neither candidates, targets nor queries get exactly zero.
        Still bit-reproducible.

        ``candidate_bias`` (fp32 ``[N]``, one entry per node, also with ``candidates``): the logits become
        ``fma(scale, embs[query[i]] . embs[j], candidate_bias[j])`` — the bias is not multiplied by ``scale`` — in the
        log-sum and in the target's term (``ghf_score_softmax_fwd_b`` / ``_bwd_b``).  With negatives drawn with probability
        ``p[j]``, ``candidate_bias=-torch.log(p)`` is the log-Q correction that makes the sampled loss an estimate of the full
        one.  ``-inf`` on a node that is no query's target adds nothing to any sum and leaves its gradients exactly zero.  When
        the bias requires grad it receives ``[N]``: ``sum_i grad[i] (p_ij - [j = target_i])``, exactly zero for nodes outside
        the candidate set; the loss is recorded for autograd also when only the bias requires grad.  A bias of zeros gives the
        bits of the call without the keyword.

        ``negatives`` (int32 / int64 ``[B, K]``, not together with ``candidates``; ids in ``[0, N)`` or exactly ``-1`` for "no
        entry"; negative ids do NOT wrap here; a multiset in the given order, as in ``rank_candidates``): the sampled softmax
        with a set PER QUERY, ``F.cross_entropy`` over ``[z_target | z_negatives]``: ``loss[i] = log(exp(z_it) + sum_j
        exp(z_ij)) - z_it`` over the positions ``j`` of row ``i`` that hold neither ``-1``, the target nor a known partner.  The
        target enters exactly once and always; a query without negatives has loss exactly 0.  Nothing is added to the sets.
        One wave per query gathers its rows (``ghf_neg_softmax_fwd`` / ``ghf_neg_bwd``, ``autograd.PerQueryLossFn``); the
        gradient of ``embs`` sums, per node, over every position that names it — a repeated id gets a term per occurrence —
        and rows that are no one's negative, target or query get exactly zero.  Bit-reproducible, and a query's loss does
        not depend on the batch it is in.  ``query_rows``, typed ``known`` and ``candidate_bias`` work as above.

        ``distance`` (``"l1"``, ``"l2"`` or ``"complex"``, as in ``rank_candidates``; with ``negatives`` only, and not with
        ``candidate_bias``): the logits become ``z = -scale * D(row_i, embs[j])`` (``ghf_dist_softmax_fwd`` / ``ghf_dist_bwd`` /
        ``ghf_dist_rows_grad``, ``autograd.PerQueryLossFn``).  The gradient of ``embs`` and of ``query_rows`` follows the
        distance: ``sign(delta)`` under ``"l1"``, ``delta / D`` under ``"l2"``, ``delta / |pair|`` under ``"complex"``, each
        exactly 0 where its denominator is 0 (a candidate equal to the query's row).  Still bit-reproducible, no ``[B, K, d]``
        tensor, forward or backward."""
        if embs.dim() != 2:
            raise ValueError(f"embs must be [N, d], got {tuple(embs.shape)}")
        metric = self._distance_arg(distance, negatives, candidates, candidate_bias, embs)
        bias = self._candidate_bias(candidate_bias, embs)
        bias_grad = bias is not None and bias.requires_grad
        pre = self._negatives_arg(negatives, candidates, query, target, embs)
        cand = None if candidates is None else self._candidate_ids(candidates, embs)
        self._query_rows(embs, query, query_rows, "softmax_loss")
        scale = float(scale)
        if not (0.0 < scale < float("inf")):
            raise ValueError(f"scale must be finite and positive, got {scale}")
        if pre is not None:
            neg, q, t = pre
        else:
            neg = None
            q = self._rank_ids(query, embs.size(0), embs, "query")
            t = self._rank_ids(target, embs.size(0), embs, "target")
            if q.numel() != t.numel():
                raise ValueError(f"{q.numel()} queries and {t.numel()} targets")
        if not embs.is_cuda:
            raise RuntimeError(f"softmax_loss computes on an MI355X HIP device only (input is on {embs.device})")
        ptr, idx = self._filter_lists(embs, q, known, filt_ptr, filt_idx, query_rel)
        if neg is not None:                              # with distance= there are always negatives (_distance_arg)
            return self._per_query_loss("softmax", _native.PAIR_DOT if metric is None else metric, embs, q, t, ptr, idx, neg, scale,
                                        0.0, 0.0, True, query_rows, bias)
        if cand is not None:
            cand = self._softmax_candidates(cand, t)
        if query_rows is not None:
            if torch.is_grad_enabled() and (embs.requires_grad or query_rows.requires_grad or bias_grad):
                from ..autograd import SoftmaxLossFn
                return SoftmaxLossFn.apply(embs, query_rows, None, t, ptr, idx, scale, cand, bias)
            return _native.score_softmax_fwd(query_rows.detach(), embs.detach().float(), t, filt_ptr=ptr, filt_idx=idx,
                                             scale=scale, ic=cand, bias=bias)[0]
        if torch.is_grad_enabled() and (embs.requires_grad or bias_grad):
            from ..autograd import SoftmaxLossFn
            return SoftmaxLossFn.apply(embs, None, q, t, ptr, idx, scale, cand, bias)
        e = embs.detach().float()
        return _native.score_softmax_fwd(e, e, t, iq=q, filt_ptr=ptr, filt_idx=idx, scale=scale, ic=cand, bias=bias)[0]

    def negative_sampling_loss(self, embs: torch.Tensor, query: torch.Tensor, target: torch.Tensor, *, scale: float = 1.0,
                               margin: float = 0.0, adversarial_temperature: float = 0.0, known=None,
                               filt_ptr: Optional[torch.Tensor] = None, filt_idx: Optional[torch.Tensor] = None,
                               query_rows: Optional[torch.Tensor] = None, query_rel: Optional[torch.Tensor] = None,
                               candidates: Optional[torch.Tensor] = None,
                               candidate_bias: Optional[torch.Tensor] = None,
                               negatives: Optional[torch.Tensor] = None, distance: Optional[str] = None) -> torch.Tensor:
        """The negative-sampling loss with self-adversarial weighting (RotatE; PyKEEN's ``NSSALoss``; the DGL-KE and OGB
        ``wikikg2`` / ``biokg`` baselines) on one shared set of negatives, fp32 ``[B]``.  With ``z[i, j] = scale * embs[query[i]]
        . embs[j]`` and the negatives ``J_i`` = every node (every candidate) except ``query[i]``'s known partners (``known`` /
        ``filt_ptr, filt_idx`` as in ``rank_candidates``) and except ``target[i]`` itself::

            w[i, j] = softmax over J_i of (adversarial_temperature * z[i, j])          # a constant: detached
            loss[i] = softplus(-(z[i, target[i]] + margin)) + sum_{j in J_i} w[i, j] * softplus(z[i, j] + margin)

        i.e. ``-logsigmoid(margin + pos) - sum_j w_j logsigmoid(-(margin + neg_j))``.  ``adversarial_temperature=0`` is the
        uniform mean over the negatives (TransE / word2vec negative sampling).  The value per query is the positive term plus
        the weighted negative term: PyKEEN's ``/ 2`` and the batch mean are the caller's.  A query without negatives has the
        positive term alone.  Neither the ``[B, C]`` logits, the weights nor the ``[C, d]`` gather exist, forward or backward:
        one sweep on the fp32 matrix cores with an online softmax-weighted sum in its epilogue (``ghf_score_negsamp_fwd``), and
        a backward that recomputes the weights from the saved log-sum (``ghf_score_negsamp_bwd``,
        ``autograd.NegSamplingLossFn``), the weights taken as constants as those libraries do.  Bit-reproducible.  ``margin``
        finite, ``adversarial_temperature`` finite and ``>= 0``, ``scale`` finite and ``> 0`` (``ValueError`` otherwise).

        Recording, ``query_rows`` / ``known=(src, dst, rel)`` with ``query_rel``, ``candidates`` and ``candidate_bias`` follow
        ``softmax_loss``: with ``candidates`` the batch's targets are added to the set, so another query's target is an
        in-batch negative unless that query's ``known`` lists it; rows of ``embs`` that are neither candidates, targets nor
        queries get exactly zero gradient; the logits become ``fma(scale, ., candidate_bias[j])`` with a finite bias, which
        receives its ``[N]`` gradient when it requires grad; a bias of zeros gives the bits of the call without the keyword.

        ``negatives`` (int32 / int64 ``[B, K]``, not together with ``candidates``; ids in ``[0, N)`` or exactly ``-1`` for "no
        entry"; negative ids do NOT wrap here; a multiset in the given order, as in ``rank_candidates``): ``K`` negatives PER
        QUERY, as RotatE's training loop and PyKEEN's default sampler draw them.  ``J_i`` is then the set of positions of row
        ``i`` that hold neither ``-1``, the target nor a known partner, and the formulas above run over it, the weights
        detached; a query whose ``J_i`` is empty has the positive term alone.  Nothing is added to the sets.  One wave per
        query (``ghf_neg_negsamp_fwd`` / ``ghf_neg_bwd``, ``autograd.PerQueryLossFn``); gradients, reproducibility and the
        other keywords as for ``softmax_loss(negatives=)``.

        ``distance`` (``"l1"``, ``"l2"`` or ``"complex"``, as in ``softmax_loss``; with ``negatives`` only, and not with
        ``candidate_bias``): ``z = -scale * D(row_i, embs[j])``.  At ``scale=1`` the positive term is ``-log sigmoid(margin -
        D_target)`` and a negative's ``-log sigmoid(D_j - margin)``: the margin is the distance budget gamma of TransE's and
        RotatE's published losses (``ghf_dist_negsamp_fwd``, ``autograd.PerQueryLossFn``)."""
        if embs.dim() != 2:
            raise ValueError(f"embs must be [N, d], got {tuple(embs.shape)}")
        metric = self._distance_arg(distance, negatives, candidates, candidate_bias, embs)
        bias = self._candidate_bias(candidate_bias, embs)
        bias_grad = bias is not None and bias.requires_grad
        pre = self._negatives_arg(negatives, candidates, query, target, embs)
        cand = None if candidates is None else self._candidate_ids(candidates, embs)
        self._query_rows(embs, query, query_rows, "negative_sampling_loss")
        scale, margin, alpha = float(scale), float(margin), float(adversarial_temperature)
        if not (0.0 < scale < float("inf")):
            raise ValueError(f"scale must be finite and positive, got {scale}")
        if not (float("-inf") < margin < float("inf")):
            raise ValueError(f"margin must be finite, got {margin}")
        if not (0.0 <= alpha < float("inf")):
            raise ValueError(f"adversarial_temperature must be finite and not negative, got {alpha}")
        if pre is not None:
            neg, q, t = pre
        else:
            neg = None
            q = self._rank_ids(query, embs.size(0), embs, "query")
            t = self._rank_ids(target, embs.size(0), embs, "target")
            if q.numel() != t.numel():
                raise ValueError(f"{q.numel()} queries and {t.numel()} targets")
        if not embs.is_cuda:
            raise RuntimeError(f"negative_sampling_loss computes on an MI355X HIP device only (input is on {embs.device})")
        ptr, idx = self._filter_lists(embs, q, known, filt_ptr, filt_idx, query_rel)
        if neg is not None:                              # with distance= there are always negatives (_distance_arg)
            return self._per_query_loss("negsamp", _native.PAIR_DOT if metric is None else metric, embs, q, t, ptr, idx, neg, scale,
                                        margin, alpha, True, query_rows, bias)
        if cand is not None:
            cand = self._softmax_candidates(cand, t)
        if query_rows is not None:
            if torch.is_grad_enabled() and (embs.requires_grad or query_rows.requires_grad or bias_grad):
                from ..autograd import NegSamplingLossFn
                return NegSamplingLossFn.apply(embs, query_rows, None, t, ptr, idx, scale, margin, alpha, cand, bias)
            return _native.score_negsamp_fwd(query_rows.detach(), embs.detach().float(), t, filt_ptr=ptr, filt_idx=idx, scale=scale,
                                             margin=margin, adversarial_temperature=alpha, ic=cand, bias=bias)[0]
        if torch.is_grad_enabled() and (embs.requires_grad or bias_grad):
            from ..autograd import NegSamplingLossFn
            return NegSamplingLossFn.apply(embs, None, q, t, ptr, idx, scale, margin, alpha, cand, bias)
        e = embs.detach().float()
        return _native.score_negsamp_fwd(e, e, t, iq=q, filt_ptr=ptr, filt_idx=idx, scale=scale, margin=margin,
                                         adversarial_temperature=alpha, ic=cand, bias=bias)[0]

    def pairwise_loss(self, embs: torch.Tensor, query: torch.Tensor, target: torch.Tensor, *, negatives: torch.Tensor,
                      loss: str = "hinge", margin: float = 1.0, scale: float = 1.0, normalize: bool = True,
                      distance: Optional[str] = None, known=None, filt_ptr: Optional[torch.Tensor] = None,
                      filt_idx: Optional[torch.Tensor] = None, query_rows: Optional[torch.Tensor] = None,
                      query_rel: Optional[torch.Tensor] = None, candidate_bias: Optional[torch.Tensor] = None,
                      return_active: bool = False):
        """The pairwise ranking losses on per-query negatives, fp32 ``[B]``: every term couples one negative of query ``i`` to
        that query's positive.  With ``z[i, j] = scale * embs[query[i]] . embs[negatives[i, j]]`` (``+ candidate_bias[.]``), or
        ``z = -scale * D(row_i, embs[.])`` under ``distance`` (``"l1"``, ``"l2"``, ``"complex"``, as in ``softmax_loss``), and
        ``J_i`` the positions of row ``i`` that hold neither ``-1``, the target nor a known partner (``known`` / ``filt_ptr,
        filt_idx`` as in ``rank_candidates``)::

            u[i, j] = z[i, j] - z[i, target[i]] + margin
            loss[i] = mean over J_i of max(u, 0)          # loss="hinge": margin ranking (TransE; PinSage / GraphSAGE max-margin)
            loss[i] = mean over J_i of softplus(u)        # loss="logistic": BPR at margin=0 (LightGCN, NGCF); soft margin ranking

        ``normalize=False`` gives the sum instead of the mean; a query whose ``J_i`` is empty has loss exactly 0.  The
        published TransE loss is::

            rows = embs[head] + rel_vec[rel]
            loss = model.pairwise_loss(embs, head, tail, negatives=neg, query_rows=rows, distance="l1", margin=gamma).mean()

        ``negatives`` (int32 / int64 ``[B, K]``, required; ids in ``[0, N)`` or exactly ``-1`` for "no entry"; negative ids do
        NOT wrap; a multiset in the given order).  ``return_active=True`` returns ``(loss, active)``, ``active`` int32 ``[B]``
        the number of violated pairs ``u > 0`` — what one logs while training; at ``margin=0`` it is ``rank_candidates``'
        ``greater``.  Neither the ``[B, K]`` scores nor the ``[B, K, d]`` gather exist, forward or backward: one wave per query
        (``ghf_pair_fwd`` / ``ghf_pair_bwd``, ``include/ghf_pairwise.h``, ``autograd.PerQueryLossFn``).  Gradients reach
        ``embs``, ``query_rows`` and (dot product only) ``candidate_bias``; rows of ``embs`` that are no one's negative, target
        or query get exactly zero; bit-reproducible.  ``scale`` finite and ``> 0``, ``margin`` finite (``ValueError``
        otherwise); ``candidate_bias`` together with ``distance`` is a ``ValueError``."""
        if embs.dim() != 2:
            raise ValueError(f"embs must be [N, d], got {tuple(embs.shape)}")
        kind = _native.PAIR_KINDS.get(loss) if isinstance(loss, str) else None
        if kind is None:
            raise ValueError(f"loss must be one of {sorted(_native.PAIR_KINDS)}, got {loss!r}")
        if negatives is None:
            raise ValueError("pairwise_loss needs negatives= (a set per query): its terms are (positive, negative) pairs")
        if distance is not None and candidate_bias is not None:
            raise ValueError("candidate_bias= does not go with distance=: no distance call takes a per-candidate bias")
        metric = self._distance_arg(distance, negatives, None, None, embs)
        metric = _native.PAIR_DOT if metric is None else metric
        bias = self._candidate_bias(candidate_bias, embs)
        neg, q, t = self._negatives_arg(negatives, None, query, target, embs)
        self._query_rows(embs, query, query_rows, "pairwise_loss")
        scale, margin = float(scale), float(margin)
        if not (0.0 < scale < float("inf")):
            raise ValueError(f"scale must be finite and positive, got {scale}")
        if not (float("-inf") < margin < float("inf")):
            raise ValueError(f"margin must be finite, got {margin}")
        if not isinstance(normalize, bool) or not isinstance(return_active, bool):
            raise TypeError(f"normalize and return_active must be bools, got {normalize!r} and {return_active!r}")
        if not embs.is_cuda:
            raise RuntimeError(f"pairwise_loss computes on an MI355X HIP device only (input is on {embs.device})")
        ptr, idx = self._filter_lists(embs, q, known, filt_ptr, filt_idx, query_rel)
        out, active = self._per_query_loss(loss, metric, embs, q, t, ptr, idx, neg, scale, margin, 0.0, normalize, query_rows, bias)
        return (out, active) if return_active else out

    @staticmethod
    def _per_query_loss(loss: str, metric: int, embs, q, t, ptr, idx, neg, scale: float, margin: float, alpha: float, normalize: bool,
                        query_rows, bias):
        """``softmax_loss`` / ``negative_sampling_loss`` with ``negatives=`` (``loss`` "softmax" / "negsamp") and
        ``pairwise_loss`` ("hinge" / "logistic") once every argument is checked, under the dot product (``metric``
        ``_native.PAIR_DOT``) or a distance: recorded (``autograd.PerQueryLossFn``) under the rules of the calls without the
        keyword, else the forward alone.  Returns the loss, for the pairwise losses ``(loss, active)``."""
        from ..autograd import PerQueryLossFn, per_query_forward
        grad = embs.requires_grad or (bias is not None and bias.requires_grad) or (query_rows is not None and query_rows.requires_grad)
        if torch.is_grad_enabled() and grad:
            rows, iq = (None, q) if query_rows is None else (query_rows, None)
            return PerQueryLossFn.apply(embs, rows, iq, t, ptr, idx, neg, metric, loss, scale, margin, alpha, normalize, bias)
        e = embs.detach().float()
        qm, iq = (e, q) if query_rows is None else (query_rows.detach(), None)
        out, _, active = per_query_forward(loss, metric, qm, e, t, neg, iq, ptr, idx, scale, margin, alpha, normalize, bias)
        return out if active is None else (out, active)

    def bce_loss(self, embs: torch.Tensor, query: torch.Tensor, *, known=None, pos_ptr: Optional[torch.Tensor] = None,
                 pos_idx: Optional[torch.Tensor] = None, scale: float = 1.0, smoothing: float = 0.0, normalize: bool = True,
                 query_rows: Optional[torch.Tensor] = None, query_rel: Optional[torch.Tensor] = None,
                 candidates: Optional[torch.Tensor] = None, candidate_bias: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The multi-label 1-vs-all loss of ConvE / TuckER / CompGCN, fp32 ``[B]``: every ``query[i]`` is scored against ALL
        nodes, all of its known partners are positives at once, and the loss is binary cross-entropy with label smoothing,
        ``F.binary_cross_entropy_with_logits(scale * embs[query] @ embs.T, y, reduction="none").mean(1)`` with
        ``y[i, j] = (1 - smoothing) * [j is a partner of query i] + smoothing / N`` — without the ``[B, N]`` logits or labels,
        forward or backward (``ghf_score_bce_fwd`` / ``ghf_score_bce_bwd``, ``autograd.BceLossFn``).  One row per DISTINCT query,
        however many partners it has.  The partners come as ``known`` (``(src, dst)``, or ``(src, dst, rel)`` with ``query_rel``)
        or as CSR lists ``pos_ptr`` / ``pos_idx``, exactly as the filter lists of ``rank_candidates`` — here they are the label
        set, not a mask; a repeated id counts once.  ``normalize=False`` returns the sum over the candidates instead of their
        mean.  ``0 <= smoothing < 1``.  Bit-reproducible.  Recorded for autograd when grad mode is on and ``embs`` requires grad.
        ``query_rows``: relation-typed queries, as in ``softmax_loss``; the loss is then recorded when ``embs`` or ``query_rows``
        requires grad (``autograd.BceLossFn`` with the rows).

        ``candidates`` (ids in any order or a bool mask, as in ``rank_candidates``): the loss over those ``C`` nodes alone
        (``ghf_score_bce_fwd_sub`` / ``_bwd_sub``): the positives are the partners that are candidates, the labels
        ``(1 - smoothing) * [partner] + smoothing / C``, and ``normalize=True`` divides by ``C``.  A partner outside the set
        takes no part, as a label or as a logit — so when sampling negatives, INCLUDE the batch's positives in ``candidates``
        (nothing is added here: unlike ``softmax_loss`` there is no single target to add).  The candidate rows are read in
        place; rows of ``embs`` that are neither candidates nor queries get exactly zero gradient.

        ``candidate_bias`` (fp32 ``[N]``, finite, one entry per node, also with ``candidates``): the per-entity bias ``b_t`` of
        those models' ``f(h, r) . e_t + b_t`` — the logits are ``fma(scale, embs[query[i]] . embs[j], candidate_bias[j])``
        (``ghf_score_bce_fwd_b`` / ``_bwd_b``).  Pass an ``nn.Parameter``: when it requires grad it receives ``[N]``,
        ``sum_i grad[i] (sigmoid(z_ij) - y_ij)`` (already divided by the candidate count under ``normalize=True``), exactly zero
        for nodes outside ``candidates``; the loss is recorded also when only the bias requires grad.  A bias of zeros gives the
        bits of the call without the keyword."""
        if embs.dim() != 2:
            raise ValueError(f"embs must be [N, d], got {tuple(embs.shape)}")
        bias = self._candidate_bias(candidate_bias, embs)
        bias_grad = bias is not None and bias.requires_grad
        cand = None if candidates is None else self._candidate_ids(candidates, embs)
        self._query_rows(embs, query, query_rows, "bce_loss")
        scale, smoothing = float(scale), float(smoothing)
        if not (0.0 < scale < float("inf")):
            raise ValueError(f"scale must be finite and positive, got {scale}")
        if not (0.0 <= smoothing < 1.0):
            raise ValueError(f"smoothing must be in [0, 1), got {smoothing}")
        q = self._rank_ids(query, embs.size(0), embs, "query")
        self._known_form(known, pos_ptr, pos_idx, query_rel)
        if not embs.is_cuda:
            raise RuntimeError(f"bce_loss computes on an MI355X HIP device only (input is on {embs.device})")
        ptr, idx = self._filter_lists(embs, q, known, pos_ptr, pos_idx, query_rel)
        if query_rows is not None:
            if torch.is_grad_enabled() and (embs.requires_grad or query_rows.requires_grad or bias_grad):
                from ..autograd import BceLossFn
                loss = BceLossFn.apply(embs, query_rows, None, ptr, idx, scale, smoothing, cand, bias)
            else:
                loss = _native.score_bce_fwd(query_rows.detach(), embs.detach().float(), pos_ptr=ptr, pos_idx=idx, scale=scale,
                                             smoothing=smoothing, ic=cand, bias=bias)
        elif torch.is_grad_enabled() and (embs.requires_grad or bias_grad):
            from ..autograd import BceLossFn
            loss = BceLossFn.apply(embs, None, q, ptr, idx, scale, smoothing, cand, bias)
        else:
            e = embs.detach().float()
            loss = _native.score_bce_fwd(e, e, iq=q, pos_ptr=ptr, pos_idx=idx, scale=scale, smoothing=smoothing, ic=cand,
                                         bias=bias)
        return loss * (1.0 / (embs.size(0) if cand is None else cand.numel())) if normalize else loss

    def num_parameters(self) -> int:
        return sum(p.numel() for p in self.parameters() if p.requires_grad)


def link_prediction_metrics(greater: torch.Tensor, equal: torch.Tensor, ks: Sequence[int] = (1, 3, 10)) -> Dict[str, float]:
    """Filtered link-prediction metrics from ``HyperGNN.rank_candidates``' counts, with the realistic rank
    ``1 + greater + equal / 2`` (a tie counts half): ``{"mrr", "mean_rank", "hits@k" for k in ks}``.  Queries whose counts
    are negative (an id was out of range in a raw call) are an error."""
    if greater.shape != equal.shape or greater.dim() != 1 or greater.numel() == 0:
        raise ValueError(f"need two non-empty [B] count tensors, got {tuple(greater.shape)} and {tuple(equal.shape)}")
    if bool((greater < 0).any()) or bool((equal < 0).any()):
        raise ValueError("negative counts: a query had an id out of range")
    rank = 1.0 + greater.to(torch.float64) + 0.5 * equal.to(torch.float64)
    out = {"mrr": float((1.0 / rank).mean()), "mean_rank": float(rank.mean())}
    for k in ks:
        out[f"hits@{int(k)}"] = float((rank <= int(k)).to(torch.float64).mean())
    return out
