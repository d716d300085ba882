"""Multi-GPU forward: one process per GPU (`torch.distributed`, backend "nccl" = RCCL over xGMI).

Two partitions of the path, behind one interface (`ShardedHyperGNN`):

* ``mode="dst"`` (default) — shards by DESTINATION node: a rank owns every in-edge of its rows, so the per-destination sums
  never cross ranks and the fused tail stays local.  The one exchange per layer makes the new rows visible everywhere: an
  all-gather of rows (half the bytes of the reduction an edge-range split needs).  What travels is what the next layer's
  kernel gathers — for the d = 128 kernel the rows already cut into their two fp16 pieces plus the row scales (written by
  the fused tail; the same volume as fp32), so no rank re-splits the full h; fp32 rows travel once, after the last layer.
  Ownership is block-cyclic so that the exchange overlaps the compute: the rows are cut into C x G slots (BN-aligned), slot
  c*G + g belongs to rank g, and a layer runs as
      for c in chunks:  message kernel on my slot of chunk c (compute stream);  exchange of chunk c (comm stream)
  so chunk c travels while chunk c + 1 computes.  Slots hold equal numbers of rows (``balance="rows"``) or about equal
  numbers of in-edges (``balance="edges"``: power-law graphs, BASELINE config 5).
  The exchange is either ``all_gather_into_tensor`` per chunk (RCCL picks ring or direct) or ``exchange="pairs"``: every
  rank sends its slot straight to each peer (batched send/recv) — xGMI is a full mesh of point-to-point links, and a
  pairwise exchange uses all seven of a GPU's links at once where a ring is bound by one.  ``exchange="sparse"`` sends
  only what the receiver reads: a rank gathers the SOURCE rows of its in-edges, so at plan time every rank tells each peer
  which of that peer's rows it needs (per chunk), and a layer's exchange is gather-pack -> pairwise send/recv -> scatter
  of exactly those rows (a uniform random shard of C3 at 8 ranks reads 71 % of the rows; graphs with locality far
  fewer).  The last layer's rows travel whole: every rank returns the full [N, d].
* ``mode="edges"`` — BASELINE.json's north-star split (config 4): every rank takes a contiguous range of the EDGE list
  (balanced by construction), computes raw partial sums for all rows (GHF_FLAG_RAW_SUM), the partial sums are reduced
  (reduce-scatter; all-reduce where the backend has no reduce-scatter), each rank divides by the global in-degree and runs
  the tail (ghf_tail_fwd) on its rows, and the new rows are all-gathered.  Twice the exchange volume of ``dst`` and
  chunks of 1/G the rows per weight fetch; kept for A/B (bench.py --dist-mode).

Weight generation (0.5 GFLOP) and the input projection (33 GFLOP) are recomputed on every rank instead of exchanged.
The compute steps come from an `ops` object so that the sharding / exchange logic runs on CPU with gloo
(tests/test_dist_gloo.py injects the oracle there); the product default, NativeOps, calls the HIP library and nothing else.
Collective errors propagate: a failed RCCL call raises on the rank that saw it and the job exits non-zero.
"""

from __future__ import annotations

import os
import time
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import torch
import torch.distributed as dist

from . import _native
from .plan import CSR_CONFIG, GraphPlan, PlanCache, block_kernel_max_nodes, build_plan, build_rs, plan_config, relation_ids


@dataclass
class ShardSpec:
    N: int
    world: int
    rank: int
    block_nodes: int
    chunks: int                 # C
    bounds: List[int]           # C*G + 1 row boundaries (multiples of block_nodes); slot c*G + g = [bounds[s], bounds[s+1])
    uniform: bool = True        # every slot holds S rows (then the chunk all-gather is in place)

    @property
    def S(self) -> int:
        return self.bounds[1] - self.bounds[0]

    @property
    def padded_rows(self) -> int:
        return max(self.bounds[-1], self.N)

    def slot(self, c: int, g: Optional[int] = None) -> Tuple[int, int]:
        """Row range [lo, hi) (clipped to N) that rank g owns in chunk c."""
        g = self.rank if g is None else g
        s = c * self.world + g
        return min(self.N, self.bounds[s]), min(self.N, self.bounds[s + 1])

    def chunk_rows(self, c: int) -> Tuple[int, int]:
        """Row range of chunk c (all ranks' slots, padded): what one all-gather fills."""
        return self.bounds[c * self.world], self.bounds[(c + 1) * self.world]

    def owned(self) -> List[Tuple[int, int]]:
        return [r for r in (self.slot(c) for c in range(self.chunks)) if r[1] > r[0]]

    def owner_arg(self, device=None):
        """What plan.build_plan needs to keep this rank's in-edges."""
        if self.uniform:
            return dict(owner=(self.S, self.world, self.rank))
        return dict(owner_bounds=(torch.tensor(self.bounds, dtype=torch.int64), self.world, self.rank))


def shard_spec(N: int, block_nodes: int, world: int, rank: int, chunks: int = 1,
               block_edges: Optional[Sequence[int]] = None) -> ShardSpec:
    """Block-cyclic slots of equal row count, or — with `block_edges[b]` = in-edges of destination block b — of about equal
    in-edge count (every slot still a whole number of blocks; a slot may be empty)."""
    nb = -(-N // block_nodes)
    chunks = max(1, min(chunks, -(-nb // world)))          # no more chunks than blocks per rank
    nslots = world * chunks
    if block_edges is None:
        S = -(-nb // nslots) * block_nodes
        return ShardSpec(N=N, world=world, rank=rank, block_nodes=block_nodes, chunks=chunks,
                         bounds=[s * S for s in range(nslots + 1)])
    import numpy as np
    be = np.asarray(block_edges, dtype=np.float64)
    assert be.shape[0] == nb, "one in-edge count per destination block"
    # a block's cost: its edges plus a constant per block (an empty block still runs its tail)
    cost = be + max(1.0, be.sum() / max(nb, 1) * 0.05)
    cum = np.concatenate([[0.0], np.cumsum(cost)])
    total = cum[-1]
    # chunks of equal cost; inside chunk c rank g takes blocks until its running total reaches its share of everything up
    # to and including this chunk — a rank that a hub block pushed over its share gets less (or nothing) in later chunks
    ccut = [int(np.searchsorted(cum, total * c / chunks, side="left")) for c in range(chunks + 1)]
    ccut[0], ccut[-1] = 0, nb
    cuts, have = [0], np.zeros(world)
    for c in range(chunks):
        lo, hi = max(ccut[c], cuts[-1]), max(ccut[c + 1], cuts[-1])
        b = lo
        for g in range(world):
            target = cum[hi] / world                          # rank g's share of all blocks up to the end of this chunk
            e = b
            if g == world - 1:
                e = hi
            else:
                while e < hi and have[g] + (cum[e + 1] - cum[b]) <= target + 0.5 * cost[e]:
                    e += 1
            have[g] += cum[e] - cum[b]
            cuts.append(e)
            b = e
    return ShardSpec(N=N, world=world, rank=rank, block_nodes=block_nodes, chunks=chunks,
                     bounds=[c * block_nodes for c in cuts], uniform=False)


class NativeOps:
    """The product compute steps: C-ABI calls only."""

    def message_config(self, d: int, E: int, N: Optional[int] = None, exact: bool = False):
        if exact:                                                   # the range guard's fallback (plan.build_plan(exact=True))
            cfg = _native.exact_config(d)
            return CSR_CONFIG if N is not None and cfg[0] > 1 and N > block_kernel_max_nodes(d, cfg[1]) else cfg
        return plan_config(d, E, N)

    def build_plan(self, edge_index, rel_ids, unique, N, d, device, exact: bool = False, **shard) -> GraphPlan:
        if exact:
            plan = build_plan(edge_index, rel_ids, unique, N, d, device, exact=True, **shard)
            plan.force_exact = True                      # (wide rows: pass 1 on fp32 MFMAs — carried by the plan)
            return plan
        return build_plan(edge_index, rel_ids, unique, N, d, device,
                          force_generic=_native.prefer_rs(d, len(unique)) and "edge_range" not in shard, **shard)

    def plan_sources(self, plan) -> torch.Tensor:
        """Source node of every edge this rank's plan holds (what its kernels gather from h)."""
        return plan.edge_arrays()[0]

    def text_embs(self, model, unique: Sequence[str], device) -> torch.Tensor:
        return model.text_encoder(unique, device)

    def input_proj(self, model, x: torch.Tensor, out: torch.Tensor, h_split, plan) -> None:
        """h0 for ALL rows on every rank (with the split form the first layer gathers, when the kernel wants one):
        0.7 ms of replicated compute at C3 instead of an exchange of N rows, which costs more on every fabric size
        (one xGMI link moves 258 MB in 3.4 ms at 2 GPUs; seven move 451 MB in >= 0.84 ms at 8)."""
        _native.input_proj_fwd(x, model.input_proj.weight.detach(), model.input_proj.bias.detach(), out=out,
                               h_split=h_split, split_layout=plan.wlayout if h_split is not None else 0)

    def all_weights(self, model, text_embs, plan):
        """[weights of layer l]: every layer's generation, batched, on this stream (HyperGNN.generate_batched)."""
        return model.generate_batched(text_embs, plan.wlayout)

    def split_rows(self, plan, h):
        """What the message kernel gathers: h itself, or its rows cut into 16-bit pieces."""
        return _native.split_rows(h, plan.wlayout) if plan.wlayout in _native.SPLIT_LAYOUTS else None

    # -- exchanging the split form (SPLIT2H: N rows of 4d bytes, then N float scales) ---------------------
    def exchanges_split(self, plan) -> bool:
        return plan.wlayout == _native.WLAYOUT_SPLIT2H

    def alloc_split(self, plan, N: int, d: int, device) -> torch.Tensor:
        return _native.alloc_split(N, d, plan.wlayout, device)

    def split_parts(self, plan, hs: torch.Tensor, N: int, d: int) -> List[torch.Tensor]:
        """The row-indexed regions of a split buffer as [N, bytes] views: what the exchange moves."""
        b = hs.view(torch.uint8)
        return [b[: N * 4 * d].view(N, 4 * d), b[N * 4 * d: N * 4 * d + 4 * N].view(N, 4)]

    def pack_rows(self, tables: List[torch.Tensor], idx: torch.Tensor) -> torch.Tensor:
        """The sparse exchange's message: rows `idx` of every table of `tables` (the split form's rows and scales, or fp32
        rows), one contiguous [n, bytes] buffer — ghf_rows_pack (csrc/exchange.hip)."""
        return _native.rows_pack([t.view(torch.uint8).view(t.size(0), -1) for t in tables], idx)

    def unpack_rows(self, tables: List[torch.Tensor], idx: torch.Tensor, packed: torch.Tensor) -> None:
        _native.rows_unpack([t.view(torch.uint8).view(t.size(0), -1) for t in tables], idx, packed)

    def layer_begin(self, model, l: int, weights, h, plan) -> None:
        """Once per layer, before its chunks.  Wide rows (csrc/message_rs.hip): pass 1 over all of this rank's edges —
        it runs in relation order, not by destination chunk; the chunks then only do pass 2 on their rows."""
        if plan.block_nodes == 1 and _native.rs_supported(h.size(1)) and plan.E > 0:
            if plan.rs is None:
                plan.rs = build_rs(plan)
            W_msg, W_self, bias = weights
            _native.edge_transform_fwd(h, plan.rs, W_msg, W_self, bias, plan.rs.scratch(plan.E, h.size(1), h.device), exact=plan.force_exact)

    def layer_rows(self, model, l: int, weights, h, h_split, plan, h_out, lo: int, hi: int, h_split_out=None) -> None:
        norm = model.layer_norms[l]
        W, W_self, bias = weights
        if plan.block_nodes == 1 and _native.rs_supported(h.size(1)):
            if plan.rs is None:
                plan.rs = build_rs(plan)
            _native.segment_tail_fwd(plan.rs.scratch(plan.E, h.size(1), h.device), plan.rs, h, norm.weight.detach(),
                                     norm.bias.detach(), norm.eps, h_out, row0=lo, rows=hi - lo, exact=plan.force_exact)
            return
        _native.message_layer_fwd(h, plan, W, W_self, bias, plan.wlayout, norm.weight.detach(), norm.bias.detach(),
                                  norm.eps, h_out, row0=lo, rows=hi - lo, h_split=h_split, h_split_out=h_split_out)

    # -- edge-range shards ------------------------------------------------------------------------------------
    def layer_raw(self, model, l: int, weights, h, h_split, plan, partial) -> None:
        """partial[v] = sum over THIS rank's edges into v of (h_u W_msg[r] + bias[r] + h_v W_self[r]) — no division, no tail."""
        W, W_self, bias = weights
        if plan.E == 0:
            partial.zero_()
            return
        _native.message_layer_fwd(h, plan, W, W_self, bias, plan.wlayout, None, None, 0.0, partial, h_split=h_split,
                                  flags=_native.GHF_FLAG_RAW_SUM)

    def scale_rows(self, sums: torch.Tensor, inv: torch.Tensor) -> torch.Tensor:
        return _native.rowscale(sums, inv)

    def tail_rows(self, model, l: int, agg, h, h_out, lo: int, hi: int) -> None:
        norm = model.layer_norms[l]
        _native.tail_fwd(agg, h, norm.weight.detach(), norm.bias.detach(), norm.eps, h_out, row0=lo, rows=hi - lo)

    # -- training (ShardedHyperGNN._forward_train) ---------------------------------------------------------
    def train_inputs(self, model, x: torch.Tensor, plan, device):
        """(h0 [N, d], [(W_msg, W_self, bias, gamma, beta) per layer]) recorded by autograd, on every rank alike: the text
        encoder, the generators and the input projection of the single-GPU training forward (their Functions unchanged)."""
        from .autograd import InputProjFn
        te = model.text_encoder(plan.unique_texts, device)
        layers = [(*gen.generate_with_grad(te), norm.weight, norm.bias)
                  for gen, norm in zip(model.weight_generators, model.layer_norms)]
        return InputProjFn.apply(x, model.input_proj.weight, model.input_proj.bias, None), layers

    def train_layer_begin(self, model, l: int, nat, h: torch.Tensor, plan) -> dict:
        """Once per layer, every row of h in place: the weights packed for the plan's kernel, the split rows it gathers, and
        (two-piece plans) the rows' scales the weight gradients read."""
        from .autograd import _layer_weights
        W_msg, W_self, bias, gamma, beta = (t.detach() for t in nat)
        W, W2 = _layer_weights(plan, W_msg, W_self, transpose=False)
        st = dict(weights=(W, W2, bias.contiguous()), gamma=gamma, beta=beta, split=self.split_rows(plan, h), h_scales=None)
        if st["split"] is not None and plan.wlayout == _native.WLAYOUT_SPLIT2H and _native.side_output_supported(plan, h.size(1)):
            st["h_scales"] = _native.split_row_scales(st["split"], h.size(0), h.size(1)).clone()
        self.layer_begin(model, l, st["weights"], h, plan)
        return st

    def layer_rows_train(self, model, l: int, st: dict, h, plan, h_out, agg, lo: int, hi: int) -> None:
        """The recorded layer forward on my rows [lo, hi) (MessageLayerFn.forward): h_out and the aggregate before the tail
        (`agg`, for ghf_tail_bwd) — one launch with the side output, else GHF_FLAG_NO_TAIL + ghf_tail_fwd."""
        W, W2, bias = st["weights"]
        eps = model.layer_norms[l].eps
        d = h.size(1)
        if _native.side_output_supported(plan, d):
            _native.message_layer_fwd(h, plan, W, W2, bias, plan.wlayout, st["gamma"], st["beta"], eps, h_out, row0=lo,
                                      rows=hi - lo, h_split=st["split"], agg_out=agg)
            return
        if plan.block_nodes == 1 and _native.rs_supported(d):
            if plan.E > 0:                              # (pass 1 ran in train_layer_begin; without edges agg stays zero)
                _native.segment_tail_fwd(plan.rs.scratch(plan.E, d, h.device), plan.rs, None, None, None, 0.0, agg, row0=lo,
                                         rows=hi - lo, flags=_native.GHF_FLAG_NO_TAIL, exact=plan.force_exact)
        elif plan.E > 0:
            _native.message_layer_fwd(h, plan, W, W2, bias, plan.wlayout, None, None, 0.0, agg, row0=lo, rows=hi - lo,
                                      flags=_native.GHF_FLAG_NO_TAIL, h_split=st["split"])
        _native.tail_fwd(agg, h, st["gamma"], st["beta"], eps, h_out, row0=lo, rows=hi - lo)

    def layer_backward(self, model, l: int, nat, st: dict, h, agg, plan, g, need_dh: bool = True):
        """(dh, dW_msg, dW_self, db, dgamma, dbeta) of my shard: `g` is zero outside my rows; the weight gradients are sums over
        my edges; dh = dpre + the self term on my rows + the message term on the SOURCE rows of my edges (any rank's rows).
        The shard's TrainPlan (the owner plan, and its edges reversed) is built once per plan."""
        from .autograd import build_train_plan, layer_backward
        W_msg, W_self, bias, gamma, beta = nat
        eps = model.layer_norms[l].eps
        if plan.E == 0:                                 # no in-edges on this rank: the tail alone
            dpre, _, _, dgamma, dbeta = _native.tail_bwd(g, agg, h, gamma.detach(), eps, plan.indeg)
            R, d = W_msg.shape[0], h.size(1)
            z = torch.zeros(R, d, d, dtype=torch.float32, device=h.device)
            return dpre, z, torch.zeros_like(z), torch.zeros(R, d, dtype=torch.float32, device=h.device), dgamma, dbeta
        if plan.train is None:
            src, dst, rel = plan.edge_arrays()
            plan.train = build_train_plan(torch.stack([src, dst]), rel, plan, h.size(1), h.device, exact=plan.force_exact)
        return layer_backward(g, h, agg, W_msg, W_self, gamma, eps, plan.train, h_scales=st["h_scales"], need_dh=need_dh,
                              shard=True)

    def accumulate_rows(self, rows: torch.Tensor, idx: Optional[torch.Tensor], packed: torch.Tensor) -> None:
        """rows[idx[i]] += packed[i] (idx None: rows[i]) — ghf_rows_accumulate (csrc/exchange.hip)."""
        _native.rows_accumulate(rows, idx, packed)


class ShardedHyperGNN:
    """Runs ``HyperGNN.forward`` across the ranks of a process group; every rank returns the full [N, d].

    mode: "dst" | "edges"; exchange: "allgather" | "pairs" | "sparse" (dst mode); balance: "rows" | "edges" (dst mode; "edges"
    implies a pairwise exchange, whose messages may differ in size).  Defaults from GHF_DIST_MODE / GHF_DIST_EXCHANGE /
    GHF_DIST_BALANCE / GHF_DIST_CHUNKS.

    Training: when the model is in training mode, grad mode is on and some parameter or `node_features` requires grad, the
    output carries a grad_fn (mode="dst", every exchange and balance; mode="edges" and dropout > 0 raise NotImplementedError).
    Convention: the backward reads, on each rank, only the rows of the output gradient that the rank owns.  So when every
    rank computes the same loss from the replicated output (score_edges / score_triple over all edges, as the reference demo
    does), every rank ends with the single-process gradient; when each rank's loss reads only its own rows, with the
    gradient of the sum of the ranks' losses.  Either way the gradients are complete and bitwise identical on every rank, and
    an optimizer step keeps the replicas in sync without DDP.  Otherwise the forward is the inference path, under no_grad."""

    def __init__(self, model, group: Optional[dist.ProcessGroup] = None, ops=None, chunks: Optional[int] = None,
                 mode: Optional[str] = None, exchange: Optional[str] = None, balance: Optional[str] = None) -> None:
        self.model = model
        self.group = group
        self.ops = ops or NativeOps()
        self.world = dist.get_world_size(group)
        self.rank = dist.get_rank(group)
        self.chunks = int(os.environ.get("GHF_DIST_CHUNKS", "4")) if chunks is None else chunks
        self.mode = mode or os.environ.get("GHF_DIST_MODE", "dst")
        self.balance = balance or os.environ.get("GHF_DIST_BALANCE", "rows")
        self.exchange = exchange or os.environ.get("GHF_DIST_EXCHANGE", "allgather")
        if self.mode not in ("dst", "edges") or self.balance not in ("rows", "edges") or self.exchange not in ("allgather", "pairs", "sparse"):
            raise ValueError(f"ShardedHyperGNN: mode={self.mode!r} balance={self.balance!r} exchange={self.exchange!r}")
        if self.balance == "edges" and self.exchange == "allgather":
            self.exchange = "pairs"
        self.backend = dist.get_backend(group)
        # what the backend offers is decided once, here — not by catching errors around a collective, which would hide real
        # RCCL failures and let one rank leave a collective the others are still in
        self._fused_gather = self.backend != "gloo"                      # all_gather_into_tensor / reduce_scatter_tensor
        self.profile = "full"                                            # "compute" / "exchange": bench.py's breakdown passes
        self.stats: Dict[str, float] = {}
        self._plans: Dict[Tuple, Tuple] = {}                             # key -> (plan, spec, 1/in-degree, inputs kept alive)
        self._plan = None
        self._spec: Optional[ShardSpec] = None
        self._inv = None
        self.last_range_flags = 0                                        # what the range guard saw in the last forward (OR over ranks)
        self._full_rows = False
        self._sparse: Optional[dict] = None
        self._comm_stream = None
        self._compute_streams: List = []

    # -- exchange ---------------------------------------------------------------------------------------
    def _gather_chunk(self, buf: torch.Tensor, spec: ShardSpec, c: int) -> None:
        """Make every rank's slot of chunk c of a row-indexed buffer visible on every rank."""
        if self.profile == "compute":
            return
        if self.exchange in ("pairs", "sparse") or not spec.uniform:
            return self._gather_pairs(buf, spec, c)
        lo, hi = spec.chunk_rows(c)
        if hi > buf.size(0):                                   # a buffer of exactly N rows: the chunk that reaches past N
            stage = torch.empty((hi - lo,) + tuple(buf.shape[1:]), dtype=buf.dtype, device=buf.device)
            a, b = spec.slot(c)
            if b > a:
                stage[a - lo: b - lo].copy_(buf[a:b])
            sub = ShardSpec(N=hi - lo, world=spec.world, rank=spec.rank, block_nodes=spec.block_nodes, chunks=1,
                            bounds=[g * spec.S for g in range(spec.world + 1)])
            self._gather_chunk(stage, sub, 0)
            if buf.size(0) > lo:
                buf[lo:].copy_(stage[: buf.size(0) - lo])
            return
        whole = buf[lo:hi]
        mine = buf[lo + spec.rank * spec.S: lo + (spec.rank + 1) * spec.S]
        self.stats["bytes_recv"] = self.stats.get("bytes_recv", 0.0) + (whole.numel() - mine.numel()) * whole.element_size()
        if self._fused_gather:
            dist.all_gather_into_tensor(whole, mine, group=self.group)
        elif buf.is_cuda:
            # gloo moves host memory only: bounce (this is how the multi-rank GPU test runs two ranks on one card)
            parts = [torch.empty(mine.shape, dtype=mine.dtype) for _ in range(self.world)]
            dist.all_gather(parts, mine.cpu(), group=self.group)
            whole.copy_(torch.cat(parts), non_blocking=False)
        else:
            parts = [buf[lo + g * spec.S: lo + (g + 1) * spec.S] for g in range(self.world)]
            dist.all_gather(parts, mine.clone(), group=self.group)

    def _gather_bufs(self, bufs: List[torch.Tensor], spec: ShardSpec, c: int) -> None:
        if self.profile == "compute":
            return
        if self.exchange == "sparse" and not self._full_rows:
            return self._gather_sparse(bufs, spec, c)
        for b in bufs:
            self._gather_chunk(b, spec, c)

    def _peers(self) -> List[int]:
        return [p for p in range(self.world) if p != self.rank]

    @staticmethod
    def _slot_rows(buf: torch.Tensor, spec: ShardSpec, c: int, g: int) -> torch.Tensor:
        """The rows of rank g's slot of chunk c in a row-indexed buffer (a view; clipped to the buffer's rows)."""
        lo, hi = spec.slot(c, g)
        return buf[min(lo, buf.size(0)): min(hi, buf.size(0))]

    def _peer_exchange(self, sends: Dict[int, torch.Tensor], into: Dict[int, torch.Tensor], stat: Optional[str]) -> None:
        """One batch of pairwise messages: sends[p] goes to peer p, peer p's message lands in into[p] (a view of the caller's
        buffer is fine: RCCL then receives in place); empty tensors do not travel.  Peers in ascending rank order, the send
        before the receive for each.  gloo moves host memory only, so device tensors bounce through host copies (this is
        how the multi-rank GPU tests run several ranks on one card).  The received bytes are added to self.stats[stat]
        ("bytes_recv" / "bytes_recv_bwd"; None: plan-time traffic, not counted)."""
        bounce = self.backend == "gloo"
        ops, keep, staged = [], [], []
        for p in sorted(set(sends) | set(into)):
            if p in sends and sends[p].numel():
                t = sends[p].cpu() if bounce and sends[p].is_cuda else sends[p].contiguous()
                keep.append(t)                                    # alive until the wait
                ops.append(dist.P2POp(dist.isend, t, p, group=self.group))
            if p in into and into[p].numel():
                dst = into[p]
                t = torch.empty(dst.shape, dtype=dst.dtype) if bounce and dst.is_cuda else dst
                if t is not dst:
                    staged.append((dst, t))
                ops.append(dist.P2POp(dist.irecv, t, p, group=self.group))
                if stat is not None:
                    self.stats[stat] = self.stats.get(stat, 0.0) + dst.numel() * dst.element_size()
        if ops:
            for req in dist.batch_isend_irecv(ops):
                req.wait()
        for dst, t in staged:
            dst.copy_(t)

    def _gather_pairs(self, buf: torch.Tensor, spec: ShardSpec, c: int) -> None:
        """Pairwise exchange of chunk c: my slot to every peer, every peer's slot from it, received in place.
        Only real rows travel (slots are clipped to N), and slots may differ in size."""
        mine = self._slot_rows(buf, spec, c, self.rank)
        self._peer_exchange({p: mine for p in self._peers()}, {p: self._slot_rows(buf, spec, c, p) for p in self._peers()},
                            "bytes_recv")

    # the sparse exchanges' messages: rows `idx` of every table ([N, bytes] uint8 views), side by side — ops.pack_rows /
    # ops.unpack_rows (csrc/exchange.hip) where the ops object has them and the tables are on the GPU, else torch indexing
    # (the CPU rehearsal); the layout is the same
    def _pack_rows(self, tables: List[torch.Tensor], idx: torch.Tensor) -> torch.Tensor:
        if hasattr(self.ops, "pack_rows") and tables[0].is_cuda:
            return self.ops.pack_rows(tables, idx)
        return torch.cat([t.index_select(0, idx) for t in tables], dim=1)

    def _unpack_rows(self, tables: List[torch.Tensor], idx: torch.Tensor, packed: torch.Tensor) -> None:
        if hasattr(self.ops, "unpack_rows") and tables[0].is_cuda:
            return self.ops.unpack_rows(tables, idx, packed)
        for t, part in zip(tables, torch.split(packed, [t.size(1) for t in tables], dim=1)):
            t.index_copy_(0, idx, part)

    def _gather_sparse(self, bufs: List[torch.Tensor], spec: ShardSpec, c: int) -> None:
        """Chunk c, needed rows only: to every peer the rows of my slot it asked for at plan time, from every peer the rows of
        its slot that my edges read, scattered to their places — ONE message per peer for all of `bufs` (the split form's
        rows and their scales travel together).  Rows nobody on this rank reads stay stale."""
        send_idx, recv_idx = self._sparse["send"][c], self._sparse["recv"][c]
        tables = [b.view(torch.uint8).view(b.size(0), -1) for b in bufs]
        row_bytes = sum(t.size(1) for t in tables)
        sends = {p: self._pack_rows(tables, send_idx[p]) for p in self._peers() if send_idx[p].numel()}
        into = {p: torch.empty(recv_idx[p].numel(), row_bytes, dtype=torch.uint8, device=tables[0].device)
                for p in self._peers() if recv_idx[p].numel()}
        self._peer_exchange(sends, into, "bytes_recv")
        for p, packed in into.items():
            self._unpack_rows(tables, recv_idx[p], packed)

    def _plan_sparse(self, plan: GraphPlan, spec: ShardSpec, device) -> dict:
        """Who needs which rows: recv[c][p] = the rows of rank p's slot of chunk c that this rank's edges read (sorted row ids,
        on the device), send[c][q] = the rows of MY slot of chunk c that rank q reads.  One exchange of index lists per
        plan (counts by all_gather, lists pairwise)."""
        G, C, me = self.world, spec.chunks, self.rank
        if plan.E > 0:
            need = torch.unique(self.ops.plan_sources(plan)).to(device)
            slot = torch.bucketize(need, torch.tensor(spec.bounds[1:], dtype=torch.int64, device=device), right=True)
        else:
            need = slot = torch.zeros(0, dtype=torch.int64, device=device)
        recv = [[need[(slot == c * G + p)].contiguous() if p != me else need[:0] for p in range(G)] for c in range(C)]
        # (the counts are a host tensor over gloo, which moves host memory only)
        cnt = torch.tensor([[recv[c][p].numel() for p in range(G)] for c in range(C)], dtype=torch.int64,
                           device="cpu" if self.backend == "gloo" else device)
        allc = [torch.zeros_like(cnt) for _ in range(G)]
        dist.all_gather(allc, cnt, group=self.group)                    # allc[q][c][p]: rows q needs from p in chunk c
        allc = [t.cpu() for t in allc]
        asked = {p: torch.empty(int(allc[p][:, me].sum()), dtype=torch.int64, device=device) for p in self._peers()}
        self._peer_exchange({p: torch.cat([recv[c][p] for c in range(C)]) for p in self._peers()}, asked, None)
        send = [[need[:0]] * G for _ in range(C)]
        for p, t in asked.items():
            for c, part in enumerate(torch.split(t, [int(allc[p][c, me]) for c in range(C)])):
                send[c][p] = part
        owned = sum(hi - lo for lo, hi in spec.owned())
        return {"send": send, "recv": recv, "rows_needed": int(allc[me].sum()), "rows_other": int(spec.N - owned)}

    def _run_chunked(self, bufs, spec: ShardSpec, compute_rows, full_rows: bool = False) -> None:
        """compute_rows(lo, hi) fills my rows of a chunk in every buffer of `bufs`; the chunk's exchange overlaps the next
        chunk's compute."""
        bufs = [bufs] if isinstance(bufs, torch.Tensor) else list(bufs)
        buf = bufs[0]
        self._full_rows = full_rows                            # (sparse exchange: this step's rows travel whole)
        on_gpu = buf.is_cuda
        skip_compute = self.profile == "exchange"
        if on_gpu:
            # The chunks of one step are independent, so their kernels go to alternating streams: a rank's chunk is a
            # fraction of a chip-filling launch (145 workgroups at 8 GPUs x 4 chunks), and in one stream every launch
            # would wait for the previous one's last workgroup (tools/dist_rank_cost.py, one rank of 8 at C3: 3.5 -> 2.7 ms per forward).
            if self._comm_stream is None:
                self._comm_stream = torch.cuda.Stream(device=buf.device)
                self._compute_streams = [torch.cuda.Stream(device=buf.device) for _ in range(2)]
            main = torch.cuda.current_stream(buf.device)
            self._comm_stream.wait_stream(main)               # the previous users of `buf` are ordered before the gathers
            lanes = self._compute_streams if spec.chunks > 1 else [main]
            for s in lanes:
                if s is not main:
                    s.wait_stream(main)
        for c in range(spec.chunks):
            lo, hi = spec.slot(c)
            if on_gpu:
                lane = lanes[c % len(lanes)]
                try:                                          # (set_stream, not the context manager: that one costs two
                    torch.cuda.set_stream(lane)               #  slow current_stream() lookups per use)
                    if hi > lo and not skip_compute:
                        compute_rows(lo, hi)
                    ready = torch.cuda.Event()
                    ready.record(lane)
                    torch.cuda.set_stream(self._comm_stream)
                    self._comm_stream.wait_event(ready)
                    self._gather_bufs(bufs, spec, c)
                finally:
                    torch.cuda.set_stream(main)
            else:
                if hi > lo and not skip_compute:
                    compute_rows(lo, hi)
                self._gather_bufs(bufs, spec, c)
        if on_gpu:
            for s in lanes:
                if s is not main:
                    main.wait_stream(s)
            main.wait_stream(self._comm_stream)                # every row of `buf` is in place for the next layer

    # -- plan -------------------------------------------------------------------------------------------
    def plan_for(self, edge_index: torch.Tensor, edge_texts: Sequence[str], N: int, device, exact: bool = False) -> GraphPlan:
        """This rank's plan (and, in self._spec / self._inv, its shard geometry).  exact: the same shards planned for the exact
        fp32 kernels — what every rank reruns on when the range guard fired on any of them."""
        key = PlanCache.key(edge_index, edge_texts, N, self.model.hidden_dim, device,
                            extra=(self.world, self.rank, self.chunks, self.mode, self.balance, bool(exact)))
        hit = None if os.environ.get("GHF_PLAN_CACHE") == "0" else self._plans.get(key)
        if hit is None:
            d = self.model.hidden_dim
            unique, ids = relation_ids(edge_texts)
            E = edge_index.size(1)
            bn = self.ops.message_config(d, E, N, **({"exact": True} if exact else {}))[0]
            kw = {"exact": True} if exact else {}
            inv = None
            if self.mode == "edges":
                # contiguous ranges of the edge list; the rows are split evenly for the reduce-scatter / all-gather
                spec = shard_spec(N, 1, self.world, self.rank, 1)
                lo, hi = E * self.rank // self.world, E * (self.rank + 1) // self.world
                plan = self.ops.build_plan(edge_index, torch.from_numpy(ids), unique, N, d, device, edge_range=(lo, hi), **kw)
                deg = torch.bincount(edge_index[1].to(device), minlength=N).clamp_(min=1)
                inv = (1.0 / deg.to(torch.float32)).contiguous()
            else:
                block_edges = None
                if self.balance == "edges":
                    nb = -(-N // bn)
                    block_edges = torch.bincount(torch.div(edge_index[1], bn, rounding_mode="floor"), minlength=nb).cpu().tolist()
                spec = shard_spec(N, bn, self.world, self.rank, self.chunks, block_edges)
                plan = self.ops.build_plan(edge_index, torch.from_numpy(ids), unique, N, d, device, **spec.owner_arg(), **kw)
            sparse = None
            if self.mode == "dst" and self.world > 1 and (self.exchange == "sparse" or os.environ.get("GHF_DIST_ROW_STATS") == "1"):
                sparse = self._plan_sparse(plan, spec, device)
            hit = (plan, spec, inv, (edge_index, edge_texts), sparse)
            while len(self._plans) >= 4:
                self._plans.pop(next(iter(self._plans)))
            self._plans[key] = hit
        self._plan, self._spec, self._inv, self._sparse = hit[0], hit[1], hit[2], hit[4]
        return self._plan

    # -- forward ----------------------------------------------------------------------------------------
    def forward(self, node_features: torch.Tensor, edge_index: torch.Tensor, edge_texts: List[str]) -> torch.Tensor:
        """The full [N, d] output on every rank.  Recorded for a backward (`_forward_train`) only in training mode, with grad
        mode on and some parameter or `node_features` requiring grad; otherwise the inference forward, under no_grad."""
        if self._wants_training(node_features):
            return self._forward_train(node_features, edge_index, edge_texts)
        return self._forward_infer(node_features, edge_index, edge_texts)

    def _wants_training(self, node_features: torch.Tensor) -> bool:
        m = self.model
        return (bool(getattr(m, "training", False)) and torch.is_grad_enabled()
                and (node_features.requires_grad or any(p.requires_grad for p in m.parameters())))

    @torch.no_grad()
    def _forward_infer(self, node_features: torch.Tensor, edge_index: torch.Tensor, edge_texts: List[str]) -> torch.Tensor:
        if edge_index.size(1) != len(edge_texts):
            raise ValueError(f"edge_index has {edge_index.size(1)} edges but edge_texts has {len(edge_texts)} entries")
        N, device = node_features.size(0), node_features.device
        plan = self.plan_for(edge_index, edge_texts, N, device)
        guard = isinstance(self.ops, NativeOps) and self.model._guarded(plan) and self.profile == "full"
        if guard:
            flag = _native.range_flag(device)
            flag.zero_()
        out = self._forward_on(node_features, plan)
        self.last_range_flags = 0
        if guard:
            word = self._reduce_guard(flag)                    # every rank must take the same decision
            self.last_range_flags = word
            if word:
                # Some row of h or some relation's weights spans more dynamic range than two fp16 pieces hold (include/ghf.h:
                # ghf_set_range_flag).  The single-GPU forward reruns on the exact fp32 kernels (HyperGNN._forward_exact), and
                # so does this one — on every rank, since the reduced word is the same everywhere: the same shards planned for
                # the exact kernels (reference: plain fp32 bmm, hypergnn.py:202,228).
                out = self._forward_on(node_features, self.plan_for(edge_index, edge_texts, N, device, exact=True))
        return out

    def _forward_on(self, node_features: torch.Tensor, plan: GraphPlan) -> torch.Tensor:
        model, spec = self.model, self._spec
        N, device, d = node_features.size(0), node_features.device, model.hidden_dim
        self.stats = {"bytes_recv": 0.0}
        # fresh buffers per call (the result is a view of one of them); pad rows are exchanged but never read
        h = torch.empty(spec.padded_rows, d, dtype=torch.float32, device=device)
        h_next = torch.empty_like(h)
        text_embs = self.ops.text_embs(model, plan.unique_texts, device)
        if self.mode == "edges":
            return self._forward_edges(node_features, plan, spec, text_embs, h, h_next)
        if self.ops.exchanges_split(plan):
            return self._forward_split(node_features, plan, spec, text_embs, h, h_next)
        return self._forward_rows(node_features, plan, spec, text_embs, h, h_next)

    def _all_weights(self, text_embs, plan) -> List:
        """ops.all_weights' list.  The ops object is an injection seam: one written against the earlier interface returns
        (list, events) — generated on the caller's stream, the events None — and keeps working: its list is taken."""
        w = self.ops.all_weights(self.model, text_embs, plan)
        return w[0] if isinstance(w, tuple) else w

    def _forward_rows(self, node_features, plan, spec, text_embs, h, h_next) -> torch.Tensor:
        model, N = self.model, node_features.size(0)
        all_w = self._all_weights(text_embs, plan)
        self.ops.input_proj(model, node_features, h[:N], None, plan)
        for l in range(model.num_layers):
            weights = all_w[l]
            src, dst = h, h_next
            self.ops.layer_begin(model, l, weights, src[:N], plan)
            src_split = self.ops.split_rows(plan, src[:N])          # all rows are in place after the previous exchange
            self._run_chunked(dst, spec, lambda lo, hi: self.ops.layer_rows(model, l, weights, src[:N], src_split, plan,
                                                                            dst[:N], lo, hi),
                              full_rows=l == model.num_layers - 1)
            h, h_next = h_next, h
        return h[:N]

    def _forward_split(self, node_features, plan, spec, text_embs, h, h_next) -> torch.Tensor:
        """Layers whose kernel gathers pre-split rows: a rank keeps fp32 h for its own rows only (the residual input of
        the next layer) and the ranks exchange the split rows their fused tails wrote; fp32 rows travel once, at the end."""
        model, ops = self.model, self.ops
        N, d, device = node_features.size(0), model.hidden_dim, node_features.device
        hs, hs_next = ops.alloc_split(plan, N, d, device), ops.alloc_split(plan, N, d, device)
        ops.input_proj(model, node_features, h[:N], hs, plan)
        all_w = self._all_weights(text_embs, plan)
        last = model.num_layers - 1
        for l in range(model.num_layers):
            weights = all_w[l]
            src, dst, src_split = h, h_next, hs
            out_split = None if l == last else hs_next
            self._run_chunked(dst if l == last else ops.split_parts(plan, hs_next, N, d), spec,
                              lambda lo, hi: ops.layer_rows(model, l, weights, src[:N], src_split, plan, dst[:N], lo, hi,
                                                            h_split_out=out_split), full_rows=l == last)
            h, h_next = h_next, h
            hs, hs_next = hs_next, hs
        return h[:N]

    def _forward_edges(self, node_features, plan, spec, text_embs, h, h_next) -> torch.Tensor:
        """Edge-range shards (BASELINE config 4 as written): per layer raw partial sums over my edges -> reduction across
        ranks -> my rows: mean, tail -> all-gather of the new rows."""
        model, ops = self.model, self.ops
        N, d, device = node_features.size(0), model.hidden_dim, node_features.device
        G, S = self.world, spec.S
        all_w = self._all_weights(text_embs, plan)
        ops.input_proj(model, node_features, h[:N], None, plan)
        partial = torch.empty(spec.padded_rows, d, dtype=torch.float32, device=device)
        if spec.padded_rows > N:
            partial[N:].zero_()
        lo, hi = spec.slot(0)
        for l in range(model.num_layers):
            weights = all_w[l]
            src_split = ops.split_rows(plan, h[:N])
            if self.profile != "exchange":
                ops.layer_raw(model, l, weights, h[:N], src_split, plan, partial[:N])
            agg = h_next                                             # (scratch until the tail overwrites my rows of it)
            if self.profile != "compute":
                self.stats["bytes_recv"] += (G - 1) * S * d * 4
                if self._fused_gather:
                    dist.reduce_scatter_tensor(agg[self.rank * S:(self.rank + 1) * S], partial, group=self.group)
                else:
                    red = partial.cpu() if partial.is_cuda else partial
                    dist.all_reduce(red, group=self.group)           # backends without reduce-scatter (gloo rehearsals)
                    agg[self.rank * S:(self.rank + 1) * S].copy_(red[self.rank * S:(self.rank + 1) * S])
            if hi > lo and self.profile != "exchange":
                agg[lo:hi] = ops.scale_rows(agg[lo:hi], self._inv[lo:hi])
                ops.tail_rows(model, l, agg[:N], h[:N], partial[:N], lo, hi)       # (partial: free after the reduction)
                h_next[lo:hi].copy_(partial[lo:hi])
            self._gather_chunk(h_next, spec, 0)
            h, h_next = h_next, h
        return h[:N]

    # -- training across GPUs ---------------------------------------------------------------------------
    def _forward_train(self, node_features: torch.Tensor, edge_index: torch.Tensor, edge_texts: List[str]) -> torch.Tensor:
        """The recorded forward ("Training across GPUs").  Upstream of the layers everything is replicated and
        recorded by the single-GPU Functions (text encoder, generators, input projection); the layers are one Function,
        ShardedLayersFn, whose forward runs the fp32 row exchange every layer and whose backward runs the exchange's adjoint
        and all-reduces the weight gradients — its gradients leave complete and identical on every rank."""
        if edge_index.size(1) != len(edge_texts):
            raise ValueError(f"edge_index has {edge_index.size(1)} edges but edge_texts has {len(edge_texts)} entries")
        model = self.model
        if self.mode != "dst":
            raise NotImplementedError(f"ShardedHyperGNN: training runs on destination shards (mode='dst'); mode={self.mode!r} "
                                      "is inference only (its backward would be an all-gather of G and a reduce-scatter of dh)")
        if getattr(model, "dropout", 0.0) > 0.0 or any(g.dropout > 0.0 for g in getattr(model, "weight_generators", [])):
            raise NotImplementedError("ShardedHyperGNN: no training with dropout > 0 (every rank would have to draw the same "
                                      "masks); set dropout=0 or call .eval()")
        N, device = node_features.size(0), node_features.device
        plan = self.plan_for(edge_index, edge_texts, N, device)
        guard = isinstance(self.ops, NativeOps) and model._guarded(plan) and self.profile == "full"
        if guard:
            flag = _native.range_flag(device)
            flag.zero_()
        h0, layers = self.ops.train_inputs(model, node_features, plan, device)
        flat = [t for lw in layers for t in lw]
        out = ShardedLayersFn.apply(self, plan, h0, *flat)
        self.last_range_flags = 0
        if guard:
            word = self._reduce_guard(flag)
            self.last_range_flags = word
            if word:
                # as the inference forward: every rank reruns the layers on the same shards planned for the exact kernels
                # (the reduced word is the same everywhere); the first recording is dropped
                out = ShardedLayersFn.apply(self, self.plan_for(edge_index, edge_texts, N, device, exact=True), h0, *flat)
        return out

    def _reduce_guard(self, flag: torch.Tensor) -> int:
        """The range-guard bits OR-ed over the ranks: one small collective, MAX per bit (a MAX of the words would turn
        {1, 2} into 2)."""
        word = flag.cpu() if self.backend == "gloo" else flag
        bits = torch.stack([(word >> i) & 1 for i in range(3)]).flatten()
        dist.all_reduce(bits, op=dist.ReduceOp.MAX, group=self.group)
        return sum(int(b) << i for i, b in enumerate(bits.tolist()))

    def _layers_fwd(self, plan, h0: torch.Tensor, layers) -> Tuple[torch.Tensor, List]:
        """Every layer on my rows, then the exchange of its fp32 rows (chunked, as _forward_rows — also where inference would
        exchange split rows: the weight gradients need fp32 h of every source row).  Saves per layer the input rows h, the
        aggregate of my rows (zero elsewhere: ghf_tail_bwd reads every row) and the kernels' per-layer state."""
        model, ops, spec = self.model, self.ops, self._spec
        N, d, device = h0.size(0), h0.size(1), h0.device
        self.stats = {"bytes_recv": 0.0}
        h, saved = h0.contiguous(), []
        for l, nat in enumerate(layers):
            st = ops.train_layer_begin(model, l, nat, h, plan)
            agg = torch.zeros(N, d, dtype=h.dtype, device=device)
            # rows the sparse exchange does not send stay zero, not stale: the backward's tail reads them (times a zero g)
            h_out = torch.zeros(spec.padded_rows, d, dtype=h.dtype, device=device)
            self._run_chunked(h_out, spec, lambda lo, hi: ops.layer_rows_train(model, l, st, h, plan, h_out[:N], agg, lo, hi),
                              full_rows=l == len(layers) - 1)
            saved.append((h, agg, st))
            h = h_out[:N]
        return (h if spec.padded_rows == N else h.clone()), saved

    def _layers_bwd(self, ctx, grad_out: torch.Tensor, layers, need_dh0: bool):
        """Per layer, in reverse: my shard's backward on my rows of the gradient, the adjoint exchange of dh (the rows of
        other ranks' nodes to their owners, summed there), the all-reduce of the weight gradients; at the end dh0 of my
        rows all-gathered.  Returns (dh0 [N, d] or None, [(dW_msg, dW_self, db, dgamma, dbeta) per layer])."""
        model, ops, spec, plan = self.model, self.ops, ctx.spec, ctx.plan
        N = grad_out.size(0)
        self.stats["bytes_recv_bwd"] = 0.0
        g = self._own_rows(grad_out.contiguous(), spec)
        grads: List = [None] * len(layers)
        dh = None
        for l in range(len(layers) - 1, -1, -1):
            h, agg, st = ctx.saved[l]
            need_dh = l > 0 or need_dh0
            dh, dWm, dWs, db, dgamma, dbeta = ops.layer_backward(model, l, layers[l], st, h, agg, plan, g, need_dh)
            grads[l] = self._all_reduce_grads([dWm, dWs, db, dgamma, dbeta])
            if need_dh:
                self._reduce_rows(dh, spec, ctx.sparse)
                if l > 0:
                    g = self._own_rows(dh, spec)
        if not need_dh0:
            return None, grads
        full = torch.empty(spec.padded_rows, dh.size(1), dtype=dh.dtype, device=dh.device)
        full[:N].copy_(dh)
        self._full_rows = True
        for c in range(spec.chunks):
            self._gather_bufs([full], spec, c)
        return full[:N], grads

    @staticmethod
    def _own_rows(t: torch.Tensor, spec: ShardSpec) -> torch.Tensor:
        """t on my rows, zero elsewhere."""
        out = torch.zeros_like(t)
        for lo, hi in spec.owned():
            out[lo:hi] = t[lo:hi]
        return out

    def _all_reduce_grads(self, ts: List[torch.Tensor]) -> List[torch.Tensor]:
        """The sum over the ranks of a layer's weight gradients (every rank's are partial sums over its edges / rows): one
        all-reduce of the concatenation, whose result is the same on every rank."""
        flat = torch.cat([t.reshape(-1) for t in ts])
        if self.world > 1:
            if flat.is_cuda and self.backend == "gloo":
                host = flat.cpu()
                dist.all_reduce(host, group=self.group)
                flat.copy_(host)
            else:
                dist.all_reduce(flat, group=self.group)
        return [p.view(t.shape) for p, t in zip(torch.split(flat, [t.numel() for t in ts]), ts)]

    def _reduce_rows(self, dh: torch.Tensor, spec: ShardSpec, sparse: Optional[dict]) -> None:
        """The adjoint of the forward's exchange, in place on dh [N, d]: the rows of peer p's slots go to p, which adds them
        to its own; afterwards my rows of dh are complete (other rows: undefined)."""
        if self.world == 1:
            return
        for c in range(spec.chunks):
            if self.exchange == "sparse" and sparse is not None:
                self._reduce_sparse(dh, sparse, c)
            elif self.exchange == "pairs" or self.exchange == "sparse" or not spec.uniform:
                self._reduce_pairs(dh, spec, c)
            else:
                self._reduce_chunk(dh, spec, c)

    def _reduce_chunk(self, dh: torch.Tensor, spec: ShardSpec, c: int) -> None:
        """Adjoint of the chunk all-gather: a reduce-scatter of the chunk (gloo has none: all-reduce, then my slot)."""
        N, d = dh.shape
        lo, hi = spec.chunk_rows(c)
        a, b = spec.slot(c)
        if hi <= N:
            stage = dh[lo:hi]
        else:                                                  # the chunk that reaches past N: padded with zero rows
            stage = torch.zeros(hi - lo, d, dtype=dh.dtype, device=dh.device)
            if N > lo:
                stage[: N - lo].copy_(dh[lo:N])
        self.stats["bytes_recv_bwd"] += (self.world - 1) * spec.S * d * dh.element_size()
        if self._fused_gather:
            mine = torch.empty(spec.S, d, dtype=dh.dtype, device=dh.device)
            dist.reduce_scatter_tensor(mine, stage.contiguous(), group=self.group)
            if b > a:
                dh[a:b].copy_(mine[: b - a])
            return
        red = stage.cpu() if stage.is_cuda else stage.clone()
        dist.all_reduce(red, group=self.group)
        if b > a:
            dh[a:b].copy_(red[a - lo: b - lo])

    def _reduce_pairs(self, dh: torch.Tensor, spec: ShardSpec, c: int) -> None:
        """Adjoint of _gather_pairs: to every peer my rows of its slot of chunk c, from every peer its rows of my slot, added
        to mine in rank order (so the bits do not depend on arrival order)."""
        mine = self._slot_rows(dh, spec, c, self.rank)
        into = {p: torch.empty_like(mine) for p in self._peers()}
        self._peer_exchange({p: self._slot_rows(dh, spec, c, p) for p in self._peers()}, into, "bytes_recv_bwd")
        if mine.size(0):
            for p in sorted(into):
                self.ops.accumulate_rows(mine, None, into[p])

    def _reduce_sparse(self, dh: torch.Tensor, sparse: dict, c: int) -> None:
        """Adjoint of _gather_sparse: to peer p the rows of its slot that my edges read (recv[c][p] — my only nonzero rows
        outside my slots), from peer q its rows of my slot that q read (send[c][q]), added at their places in rank order."""
        send_idx, recv_idx = sparse["send"][c], sparse["recv"][c]
        d, table = dh.size(1), [dh.view(torch.uint8).view(dh.size(0), -1)]
        sends = {p: self._pack_rows(table, recv_idx[p]).view(dh.dtype).view(-1, d) for p in self._peers() if recv_idx[p].numel()}
        into = {p: torch.empty(send_idx[p].numel(), d, dtype=dh.dtype, device=dh.device) for p in self._peers() if send_idx[p].numel()}
        self._peer_exchange(sends, into, "bytes_recv_bwd")
        for p in sorted(into):
            self.ops.accumulate_rows(dh, send_idx[p], into[p])

    __call__ = forward


class ShardedLayersFn(torch.autograd.Function):
    """Every message layer of a ShardedHyperGNN, recorded: inputs h0 [N, d] (replicated) and per layer (W_msg, W_self, bias,
    gamma, beta) (replicated, natural layout); output the full [N, d] on every rank.  The backward reads only this rank's
    rows of its incoming gradient and returns gradients that are complete and bitwise identical on every rank."""

    @staticmethod
    def forward(ctx, runner: "ShardedHyperGNN", plan, h0: torch.Tensor, *flat: torch.Tensor):
        layers = [tuple(flat[i:i + 5]) for i in range(0, len(flat), 5)]
        out, saved = runner._layers_fwd(plan, h0, layers)
        ctx.runner, ctx.plan, ctx.spec, ctx.sparse, ctx.saved = runner, plan, runner._spec, runner._sparse, saved
        ctx.save_for_backward(*flat)
        return out

    @staticmethod
    def backward(ctx, grad_out: torch.Tensor):
        flat = ctx.saved_tensors
        layers = [tuple(flat[i:i + 5]) for i in range(0, len(flat), 5)]
        dh0, grads = ctx.runner._layers_bwd(ctx, grad_out, layers, need_dh0=ctx.needs_input_grad[2])
        out = []
        for lw, gl in zip(layers, grads):
            out += [gt.to(t.dtype) for gt, t in zip(gl, lw)]
        return (None, None, dh0, *out)
