"""Training through the HIP path: ``torch.autograd.Function`` wrappers whose forward AND backward are C-ABI calls.

The reference trains through plain autograd (``demo.py:79-101``, ``tests/test_hypergnn.py:183-226``,
``tests/test_weight_generator.py:86-106``).  Here autograd only records the chain; every gradient is computed by
``libghf_hip.so`` (``include/ghf.h``: "backward of the path").  With, per layer,

    out_v = (1/c_v) sum_{e=(u->v)} ( h_u Wm[r_e] + b[r_e] + h_v Ws[r_e] ),   h'_v = LayerNorm(ReLU(out_v + h_v))

and ``g' = dL/dh'``:

    (dpre, G, G_split, dgamma, dbeta) = ghf_tail_bwd(g', out, h)          G_v = dpre_v / c_v
    dWm[r] = sum_{e in r} h_u^T G_v      dWs[r] = sum_{e in r} h_v^T G_v      db[r] = sum_{e in r} G_v      (ghf_group_outer)
    dh = dpre + [sum_{e->v} G_v Ws[r]^T]_v + [sum_{e: src=u} G_{dst(e)} Wm[r]^T]_u
         (two ghf_message_layer_fwd passes with GHF_FLAG_RAW_SUM: transposed weights on the plan / on the reversed plan)

Exact fp32 contractions for the weight gradients, the message kernel for the h gradients (each of its two passes has one
zero half of the weights and says so: GHF_FLAG_ZERO_SRC / GHF_FLAG_ZERO_DST).  The training forward is the inference
launch with one more store: the kernel writes ``out`` beside ``h'`` (``agg_out``) and the split rows the next layer
gathers; kernels without that side output run GHF_FLAG_NO_TAIL plus ``ghf_tail_fwd``.

The callers either side of the layer have their own Functions here: ``WeightGeneratorFn`` (three MLP heads and the
learnable log-scales, reference weight_generator.py:120-143), ``InputProjFn`` (hypergnn.py:261), ``TextEncoderFn``
(hypergnn.py:57-81), ``ScorePairsFn`` (hypergnn.py:304-318), its fused form over index arrays ``ScoreEdgesFn`` and the 1-vs-all softmax loss
against every node ``SoftmaxLossFn`` (no counterpart in the reference).  All of
their contractions are ``A^T B`` over rows, i.e. ``ghf_group_outer`` again (``_native.matmul_tn``).
"""

from __future__ import annotations

import weakref
from dataclasses import dataclass
from typing import List, Optional, Sequence

import torch

from . import _native
from .plan import GraphPlan, build_plan, build_rs


@dataclass
class TrainPlan:
    """What a training step needs beyond the forward plan: the reversed graph's plan and the edges grouped by relation."""
    fwd: GraphPlan
    rev: GraphPlan
    src_by_rel: torch.Tensor      # [E] int64: source of the edges in relation order (ascending destination inside one)
    dst_by_rel: torch.Tensor      # [E] int64
    goff: torch.Tensor            # [R+1] int64
    slice_tab: Optional[torch.Tensor] = None   # [S, 3] int64 (relation, first edge, end edge): ghf_edge_outer's work list
    slice_off: Optional[torch.Tensor] = None   # [R+1] int64
    slice_order: Optional[torch.Tensor] = None # [S] int32: the slices in launch order (by position inside their relation)
    ident: Optional[tuple] = None               # (arange(N), slice table, slice offsets): InputProjFn's weight gradient as ghf_edge_outer
    zero_bias: Optional[torch.Tensor] = None    # [R, d] zeros: the bias operand of the two gradient passes
    carry: Optional["_SplitCarry"] = None       # split rows handed from one layer's launch to the next

SLICE_EDGES = 4096                # edges per ghf_edge_outer workgroup (a multiple of its 32-edge tile)


def build_train_plan(edge_index: torch.Tensor, rel_ids: torch.Tensor, fwd: GraphPlan, d: int, device, exact: bool = False) -> TrainPlan:
    """exact: `fwd` is a plan for the exact fp32 kernels (the range guard's fallback): the reversed graph is planned for them
    too, and wide rows run the relation-stationary layer on fp32 MFMAs in both directions (GraphPlan.force_exact)."""
    if fwd.row_lo != 0 or (fwd.row_hi or fwd.N) != fwd.N or fwd.E != edge_index.size(1):
        raise NotImplementedError("training runs on single-GPU plans (every destination row, every edge)")
    ei = edge_index.to(device=device, dtype=torch.int64)
    rel = rel_ids.to(device=device, dtype=torch.int64).contiguous()
    rev = build_plan(ei.flip(0).contiguous(), rel, fwd.unique_texts, fwd.N, d, device, exact=exact)
    fwd.force_exact = rev.force_exact = exact
    by_dst = torch.sort(ei[1], stable=True).indices          # destinations ascending inside a relation: G / h_dst rows stay
    perm, goff = _native.group_edges(rel.index_select(0, by_dst), fwd.R)   # hot in L2 while a slice is contracted
    perm = by_dst.index_select(0, perm)
    tp = TrainPlan(fwd=fwd, rev=rev, src_by_rel=ei[0].index_select(0, perm).contiguous(),
                   dst_by_rel=ei[1].index_select(0, perm).contiguous(), goff=goff, carry=_SplitCarry())
    if _native.load().ghf_edge_outer_supported(d):
        tab, soff, order = _slice_tables(goff.cpu().tolist(), fwd.R)   # (one host sync per plan)
        if tab:
            tp.slice_tab = torch.tensor(tab, dtype=torch.int64).to(device)
            tp.slice_off = torch.tensor(soff, dtype=torch.int64).to(device)
            tp.slice_order = torch.tensor(order, dtype=torch.int32).to(device)
    return tp


def _slice_tables(off, R: int):
    """ghf_edge_outer's work list for relation offsets `off` [R+1]: (slice_tab rows (relation, first edge, end edge) of at most
    SLICE_EDGES edges, slice_off [R+1], the slices in launch order) as host lists."""
    tab, soff = [], [0]
    for r in range(R):
        tab += [(r, a, min(a + SLICE_EDGES, off[r + 1])) for a in range(off[r], off[r + 1], SLICE_EDGES)]
        soff.append(len(tab))
    # Destinations ascend inside a relation, so a slice's place in its relation (as a fraction of the relation's
    # slices) says which band of destination rows it reads.  Launched band by band — every relation's slice of the
    # band together — the workgroups in flight share that band's rows of h and G (Infinity Cache) instead of each
    # relation sweeping all N rows alone.  Same bits: ghf.h, ghf_edge_outer.
    place = [((k + 0.5) / (soff[r + 1] - soff[r]), r) for r in range(R) for k in range(soff[r + 1] - soff[r])]
    return tab, soff, sorted(range(len(tab)), key=place.__getitem__)


def _ident_slices(N: int):
    """The same work list for InputProjFn's weight gradient: the "edges" v -> v of one relation, v < N."""
    step = min(SLICE_EDGES, max(256, (N // 1024 + 31) // 32 * 32))           # ~1,000 slices: all CUs also at 10^5 rows
    return [(0, a, min(a + step, N)) for a in range(0, N, step)]


def _layer_weights(plan: GraphPlan, Wm: Optional[torch.Tensor], Ws: Optional[torch.Tensor], transpose: bool):
    """(W, W_self) arguments of ghf_message_layer_fwd for natural [R,d,d] matrices (None = zeros) in the plan's layout."""
    R, d = plan.R, (Wm if Wm is not None else Ws).size(1)
    if plan.wlayout == _native.WLAYOUT_NATURAL:
        z = None

        def nat(w):
            nonlocal z
            if w is None:
                if z is None:
                    z = torch.zeros(R, d, d, dtype=torch.float32, device=(Wm if Wm is not None else Ws).device)
                return z
            return _native.transpose_batched(w) if transpose else w.contiguous()
        return nat(Wm), nat(Ws)
    if plan.wlayout not in (_native.WLAYOUT_SPLIT2H, _native.WLAYOUT_FRAG16):
        raise NotImplementedError(f"training needs the generic, the FRAG16 or the SPLIT2H message kernel (plan layout "
                                  f"{plan.wlayout}; unset GHF_KERNEL)")
    return _native.weights_pack(Wm, Ws, transpose, R, d, plan.wlayout), None


def _message(x: torch.Tensor, plan: GraphPlan, W, W_self, bias: torch.Tensor, flags: int, x_split=None, residual=None,
             zero_out: bool = False) -> torch.Tensor:
    """A message pass without tail (NO_TAIL / RAW_SUM) on the plan's kernel: the destination-block or generic kernel, or —
    CSR plans of wide rows — the relation-stationary layer.  zero_out: rows the plan's kernel does not write read zero."""
    out = torch.zeros_like(x) if zero_out else torch.empty_like(x)
    if plan.block_nodes == 1 and _native.rs_supported(x.size(1)) and plan.E > 0:
        if plan.rs is None:
            plan.rs = build_rs(plan)
        Y = plan.rs.scratch(plan.E, x.size(1), x.device)      # (plan.force_exact — the guard's fallback: pass 1 on fp32 MFMAs, forward and backward)
        _native.edge_transform_fwd(x, plan.rs, W, W_self, bias, Y, exact=plan.force_exact)
        _native.segment_tail_fwd(Y, plan.rs, None, None, None, 0.0, out, flags=flags, exact=plan.force_exact)
        return out
    if residual is not None:                 # out = (the pass) + residual, added in the kernel's tail (GHF_FLAG_ADD_H): x_split names
        _native.message_layer_fwd(residual, plan, W, W_self, bias, plan.wlayout, None, None, 0.0, out,      # the gathered rows
                                  flags=flags | _native.GHF_FLAG_ADD_H, h_split=x_split)
        return out
    _native.message_layer_fwd(x, plan, W, W_self, bias, plan.wlayout, None, None, 0.0, out, flags=flags, h_split=x_split)
    return out


def _raw_message(x: torch.Tensor, plan: GraphPlan, W, W_self, zero_bias: torch.Tensor, zero_half: int, x_split=None, residual=None,
                 zero_out: bool = False) -> torch.Tensor:
    # GHF_FLAG_ZERO_*: "this half must not be read" (include/ghf.h) — the block kernels honour it; the others are handed
    # packs whose other half really is zero (MessageLayerFn.backward) and no flag
    if not _native.side_output_supported(plan, x.size(1)):
        zero_half = 0
    return _message(x, plan, W, W_self, zero_bias, _native.GHF_FLAG_RAW_SUM | zero_half, x_split, residual, zero_out)


class _SplitCarry:
    """The split form of a layer's output rows, written by that layer's launch for the next layer's gathers (the
    inference path's h_split chain).  Valid for the very tensor object the launch returned, unmodified since — anything
    else (another tensor, an in-place edit) finds nothing and the rows are cut again."""

    def __init__(self) -> None:
        self.ref = None
        self.version = -1
        self.split = None

    def take(self, h: torch.Tensor):
        hit = self.ref is not None and self.ref() is h and h._version == self.version
        split, self.ref, self.split = (self.split if hit else None), None, None
        return split

    def put(self, h: torch.Tensor, split: torch.Tensor) -> None:
        self.ref, self.version, self.split = weakref.ref(h), h._version, split


# The weight gradients run on the main stream: on a second stream beside the two gradient passes they were no faster (round 3,
# DESIGN_HISTORY.md: the three kernels contend for the same gather path).
_WG_FUSED_BWD = 1                 # WeightGeneratorFn.backward through ghf_weightgen_bwd: 0 never, 1 small generators, 2 always
WG_FUSED_MAX = 1 << 18            # ... "small": relations x d_in x d_out (config 2: 2^17, config 3: 2^20)
_IP_EDGE_OUTER = True             # InputProjFn.backward: dW / db through ghf_edge_outer (where it applies)


class MessageLayerFn(torch.autograd.Function):
    """One HyperGNN layer (reference hypergnn.py:281-296) with per-relation weights in natural layout."""

    @staticmethod
    def forward(ctx, h, W_msg, W_self, bias, gamma, beta, eps: float, tp: TrainPlan, drop: Optional[torch.Tensor] = None):
        """drop: the layer's dropout mask scaled by 1/(1-p) ([N, d]; reference hypergnn.py:293-294: between ReLU and LayerNorm),
        None without dropout."""
        plan = tp.fwd
        h = h.contiguous()
        W, W2 = _layer_weights(plan, W_msg.detach(), W_self.detach(), transpose=False)
        out = torch.empty_like(h)
        h_scales = None
        if drop is None and _native.side_output_supported(plan, h.size(1)):   # one launch: h', the aggregate, the next layer's split rows
            agg = torch.empty_like(h)
            hs = tp.carry.take(h)
            if hs is None:
                hs = _native.split_rows(h, plan.wlayout)
            hs_out = torch.empty_like(hs)
            _native.message_layer_fwd(h, plan, W, W2, bias.detach().contiguous(), plan.wlayout, gamma.detach(), beta.detach(), eps,
                                      out, h_split=hs, h_split_out=hs_out, agg_out=agg)
            tp.carry.put(out, hs_out)
            if plan.wlayout == _native.WLAYOUT_SPLIT2H:
                # 4 bytes per row: the weight gradients read their scale for h off these (ghf_edge_outer_scaled)
                h_scales = _native.split_row_scales(hs, h.size(0), h.size(1)).clone()
        else:
            agg = _message(h, plan, W, W2, bias.detach().contiguous(), _native.GHF_FLAG_NO_TAIL)
            _native.tail_fwd(agg, h, gamma.detach(), beta.detach(), eps, out, drop=drop)
        ctx.save_for_backward(h, agg, W_msg, W_self, gamma)
        ctx.tp, ctx.eps, ctx.drop, ctx.h_scales = tp, eps, drop, h_scales
        return out

    @staticmethod
    def backward(ctx, grad_out):
        h, agg, W_msg, W_self, gamma = ctx.saved_tensors
        dh, dWm, dWs, db, dgamma, dbeta = layer_backward(grad_out, h, agg, W_msg, W_self, gamma, ctx.eps, ctx.tp, ctx.drop,
                                                         ctx.h_scales, ctx.needs_input_grad[0])
        return dh, dWm, dWs, db, dgamma, dbeta, None, None, None


def layer_backward(grad_out, h, agg, W_msg, W_self, gamma, eps: float, tp: TrainPlan, drop=None, h_scales=None,
               need_dh: bool = True, shard: bool = False):
    """(dh, dW_msg, dW_self, db, dgamma, dbeta) of one layer (MessageLayerFn.backward).  shard: `tp.fwd` is a destination shard's
    plan (dist.ShardedHyperGNN) — its kernels write the owned rows only, so the outputs of the passes on it start from zeros
    (`grad_out` is zero outside the owned rows, and so are dpre and G there)."""
    plan = tp.fwd
    g = grad_out.contiguous().float()
    # both gradient passes gather the same rows of G: two-piece plans get them cut by the same launch
    split_G = (need_dh and plan.wlayout in _native.SPLIT_LAYOUTS and tp.rev.wlayout == plan.wlayout
               and plan.block_nodes > 1)
    dpre, G, Gs, dgamma, dbeta = _native.tail_bwd(g, agg, h, gamma.detach(), eps, plan.indeg, drop=drop,
                                                  split_layout=plan.wlayout if split_G else None)
    scales = {}
    if Gs is not None and h_scales is not None and plan.wlayout == _native.WLAYOUT_SPLIT2H:
        scales = dict(h_scales=h_scales, G_scales=_native.split_row_scales(Gs, G.size(0), G.size(1)))
    if tp.slice_tab is not None:
        dW, db = _native.edge_outer(h, G, tp.src_by_rel, tp.dst_by_rel, tp.slice_tab, tp.slice_off, plan.R, exact=plan.force_exact, order=tp.slice_order, **scales)
        d = h.size(1)
        dWm, dWs = dW[:, :d], dW[:, d:]
    else:
        dWm = _native.group_outer(h, tp.src_by_rel, G, tp.dst_by_rel, tp.goff)
        dWs = _native.group_outer(h, tp.dst_by_rel, G, tp.dst_by_rel, tp.goff)
        db = _native.group_outer(None, None, G, tp.dst_by_rel, tp.goff).reshape(plan.R, -1)
    dh = None
    if need_dh:
        if tp.zero_bias is None or tp.zero_bias.shape != (plan.R, h.size(1)):      # (one fill per plan, not one per layer and step)
            tp.zero_bias = torch.zeros(plan.R, h.size(1), dtype=torch.float32, device=h.device)
        zero_b = tp.zero_bias
        if plan.wlayout == tp.rev.wlayout and plan.wlayout in _native.SPLIT_LAYOUTS:
            # one packed tensor serves both passes: each declares the half it does not read zero (ZERO_SRC / ZERO_DST)
            Wf, Wf2 = _layer_weights(plan, W_msg.detach(), W_self.detach(), transpose=True)
            Wr, Wr2 = Wf, Wf2
        else:
            Wf, Wf2 = _layer_weights(plan, None, W_self.detach(), transpose=True)       # self term: rows keyed by destination
            Wr, Wr2 = _layer_weights(tp.rev, W_msg.detach(), None, transpose=True)      # message term: scattered to the sources
        if Gs is not None and _native.side_output_supported(plan, h.size(1)) and _native.side_output_supported(tp.rev, h.size(1)):
            # the three terms are added in the two passes' tails: dpre + self term, then + message term
            t1 = _raw_message(G, plan, Wf, Wf2, zero_b, _native.GHF_FLAG_ZERO_SRC, Gs, residual=dpre, zero_out=shard)
            dh = _raw_message(G, tp.rev, Wr, Wr2, zero_b, _native.GHF_FLAG_ZERO_DST, Gs, residual=t1)
        else:
            dh = _native.add3(dpre, _raw_message(G, plan, Wf, Wf2, zero_b, _native.GHF_FLAG_ZERO_SRC, Gs, zero_out=shard),
                              _raw_message(G, tp.rev, Wr, Wr2, zero_b, _native.GHF_FLAG_ZERO_DST, Gs), out=dpre)
    return dh, dWm, dWs, db, dgamma, dbeta


class WeightGeneratorFn(torch.autograd.Function):
    """(W_msg [R,d_in,d_out], W_self [R,d_in,d_out], bias [R,d_out]) = exp(log_scale_k) * MLP_k(text_emb), k = three heads.

    Arguments after the dims: text_emb [R,T], the three log-scales ([1] each), then the flat parameter list
    [head][layer][weight, bias] exactly as ghf_weightgen_fwd takes it."""

    @staticmethod
    def forward(ctx, dims, x, ls0, ls1, ls2, *params):
        """dims = (T, Hh, nh, d_in, d_out[, hidden_drop, log_keep]): hidden_drop = the hidden layers' dropout masks scaled by
        1/(1-p) ([3, nh, R, Hh]; reference weight_generator.py:96-107) and log_keep = a 1-element device tensor log(1/(1-p))."""
        T, Hh, nh, d_in, d_out = dims[:5]
        hidden_drop, log_keep = (dims[5], dims[6]) if len(dims) > 5 else (None, None)
        x = x.contiguous().float()
        flat = [p.detach() for p in params]
        ls = torch.cat([ls0.detach().reshape(1), ls1.detach().reshape(1), ls2.detach().reshape(1)])
        # (the hidden activations the backward needs leave with the same launch)
        *outs, acts = _native.weightgen_fwd(x, flat, ls, T, Hh, nh, d_in, d_out, _native.WLAYOUT_NATURAL, hidden_drop=hidden_drop,
                                            want_acts=True)
        outs = tuple(outs)
        ctx.dims, ctx.acts, ctx.n_params, ctx.log_keep = dims[:5], acts, len(params), log_keep
        ctx.save_for_backward(x, ls, *outs, *params)
        return outs

    @staticmethod
    def backward(ctx, *grads):
        T, Hh, nh, d_in, d_out = ctx.dims
        x, ls = ctx.saved_tensors[0], ctx.saved_tensors[1]
        outs, params = ctx.saved_tensors[2:5], ctx.saved_tensors[5:]
        R, nl = x.size(0), nh + 1
        if (_WG_FUSED_BWD and (_WG_FUSED_BWD > 1 or R * d_in * d_out <= WG_FUSED_MAX) and all(g is not None for g in grads)
                and _native.weightgen_bwd_supported(T, Hh, nh)):
            # all heads, all layers: three launches (csrc/weightgen_bwd.hip) instead of ~68.  For small generators only: the
            # three kernels are chains of short latency-bound phases (0.1 ms per call at BASELINE configs 1 and 2, 0.25 ms at
            # config 3) — a win where the step is launch latencies (config 1: 4.7 -> 2.4 ms per step), a loss where the ~68
            # small launches hide on the side stream beside the gradient passes (config 3: 42.1 -> 42.9 ms).
            dparams, dls3, dx = _native.weightgen_bwd(x, [p.detach() for p in params], ctx.acts, [o.view(R, -1) for o in outs],
                                                      [g.contiguous().float().view(R, -1) for g in grads], ls, T, Hh, nh, d_in, d_out,
                                                      log_keep=ctx.log_keep, want_dx=ctx.needs_input_grad[1])
            return (None, dx, dls3[0:1], dls3[1:2], dls3[2:3], *dparams)
        dls: List[Optional[torch.Tensor]] = []
        dparams: List[Optional[torch.Tensor]] = [None] * len(params)
        dxs: List[torch.Tensor] = []
        for k in range(3):
            if grads[k] is None:
                dls.append(None)
                continue
            g = grads[k].contiguous().float().view(R, -1)
            dls.append(_native.dot(g, outs[k]))                        # out = y exp(ls): d out / d ls = out
            dy = _native.scale_exp(g, ls[k:k + 1])
            for l in range(nl - 1, -1, -1):
                W = params[(k * nl + l) * 2].detach()
                a_prev = ctx.acts[k, l - 1] if l > 0 else x
                if l < nl - 1:
                    # acts are post-dropout: a > 0 <=> kept and active; a kept unit's gradient carries the mask's 1/(1-p)
                    dy = _native.relu_mask(dy, ctx.acts[k, l])
                    if ctx.log_keep is not None:
                        dy = _native.scale_exp(dy, ctx.log_keep)
                dparams[(k * nl + l) * 2] = _native.matmul_tn(dy, a_prev)
                dparams[(k * nl + l) * 2 + 1] = _native.colsum(dy)
                if l > 0 or ctx.needs_input_grad[1]:
                    dy = _native.matmul_nn(dy, W)
            dxs.append(dy)
        dx = None
        if ctx.needs_input_grad[1] and dxs:
            dx = dxs[0] if len(dxs) == 1 else _native.add3(dxs[0], dxs[1], dxs[2] if len(dxs) > 2 else None)
        return (None, dx, *dls, *dparams)


class InputProjFn(torch.autograd.Function):
    """h0 = relu(x W^T + b) (reference hypergnn.py:261)."""

    @staticmethod
    def forward(ctx, x, W, b, tp=None):
        """tp (a TrainPlan on a two-piece layout): the rows also leave cut into pieces for the first layer's gathers, by
        the same launch, through the plan's carry."""
        x = x.contiguous().float()
        split = tp is not None and tp.fwd.wlayout in _native.SPLIT_LAYOUTS and tp.fwd.block_nodes > 1
        hs = _native.alloc_split(x.size(0), W.size(0), tp.fwd.wlayout, x.device) if split else None
        h0 = _native.input_proj_fwd(x, W.detach(), b.detach(), h_split=hs, split_layout=tp.fwd.wlayout if split else 0)
        if split:
            tp.carry.put(h0, hs)
        ctx.save_for_backward(x, W, h0)
        ctx.tp = tp
        return h0

    @staticmethod
    def backward(ctx, g):
        x, W, h0 = ctx.saved_tensors
        dz = _native.relu_mask(g.contiguous().float(), h0)
        tp, N, d = ctx.tp, x.size(0), x.size(1)
        if (_IP_EDGE_OUTER and tp is not None and W.size(0) == d and N >= 65536 and _native.load().ghf_edge_outer_supported(d)):
            # dW^T = x^T dz and db = the column sums of dz are ghf_edge_outer's sums over the "edges" v -> v of one relation
            # (its [h_src | h_dst] is [x | x]: the second read of a row is an L2 hit): the tall contraction on the matrix pipe
            # with its slices over all CUs instead of ghf_group_outer + two ghf_colsum (1.0 -> 0.3 ms at C3).  Same two-piece
            # arithmetic and one-scale-per-tensor contract as the layers' weight gradients (ghf.h); the exact chain when the
            # step fell back to the exact kernels.
            if tp.ident is None or tp.ident[0].numel() != N:
                tab = _ident_slices(N)
                tp.ident = (torch.arange(N, dtype=torch.int64, device=x.device), torch.tensor(tab, dtype=torch.int64).to(x.device),
                            torch.tensor([0, len(tab)], dtype=torch.int64).to(x.device))
            ids, tab, soff = tp.ident
            dWt, db1 = _native.edge_outer(x, dz, ids, ids, tab, soff, 1, exact=tp.fwd.force_exact)
            dW, db = dWt[0, :d].t().contiguous(), db1[0]
        else:
            dW = _native.matmul_tn(dz, x)
            db = _native.colsum(dz)
        dx = None
        if ctx.needs_input_grad[0]:
            # dz W in slabs of rows: one launch holds at most 65,535 x 16 rows of the result (a grid dimension)
            Wc, slab = W.detach().contiguous(), 16 * 65535
            if x.size(0) <= slab:
                dx = _native.matmul_nn(dz, Wc)
            else:
                dx = torch.empty(x.size(0), Wc.size(1), dtype=torch.float32, device=x.device)
                for a in range(0, x.size(0), slab):
                    dx[a:a + slab] = _native.matmul_nn(dz[a:a + slab], Wc)
        return dx, dW, db, None


class TextEncoderFn(torch.autograd.Function):
    """te = tanh(mean_l E[ids] W^T + b) for all strings at once (reference hypergnn.py:57-81)."""

    @staticmethod
    def forward(ctx, E, W, b, ids, lens):
        te = _native.text_encode_fwd(ids, lens, E.detach(), W.detach(), b.detach())
        ctx.save_for_backward(E, W, te, ids, lens)
        return te

    @staticmethod
    def backward(ctx, g):
        E, W, te, ids, lens = ctx.saved_tensors
        dE, dW, db = _native.text_encode_bwd(ids, lens, E.detach(), W.detach(), te, g.contiguous().float())
        return dE, dW, db, None, None


class ScoreEdgesFn(torch.autograd.Function):
    """s_i = embs[src_i] . embs[dst_i] without the two gathered [P, d] matrices (HyperGNN.score_edges).  Backward: the 2P
    (node, partner, pair) entries grouped by node (ghf_group_edges, stable) and summed per node in that order —
    d embs[v] = sum_{i: src_i = v} g_i embs[dst_i] + sum_{i: dst_i = v} g_i embs[src_i] — one gather pass, reproducible."""

    @staticmethod
    def forward(ctx, embs, src, dst):
        embs = embs.contiguous().float()
        src, dst = src.to(torch.int64).contiguous(), dst.to(torch.int64).contiguous()
        ctx.save_for_backward(embs, src, dst)
        return _native.score_pairs_fwd(embs, embs, src, dst)

    @staticmethod
    def backward(ctx, g):
        embs, src, dst = ctx.saved_tensors
        P, N = src.numel(), embs.size(0)
        if P == 0:                                          # no pair, nothing to group: the gradient of an empty sum
            return torch.zeros_like(embs), None, None
        keys = torch.cat([src, dst]).clamp_(0, N - 1)
        perm, off = _native.group_edges(keys, N)
        partner = torch.cat([dst, src]).index_select(0, perm)
        pair = torch.remainder(perm, P)
        return _native.segment_axpy(g.contiguous().float(), pair, embs, partner, off), None, None


def _all_node_loss_grads(ctx, embs, rows, query, dq, dc, cand=None):
    """(d embs, d rows) of a loss against every node from its backward call's dq (per query) and dc (per candidate).  With
    the query rows given (q = rows, c = embs) they are those, as they are.  Without (q = c = embs): d embs = dc + dq summed
    into the rows `query` names, grouped by node (ghf_group_edges, stable) and added per node in that order (_fold_rows), as
    ScoreEdgesFn does: reproducible.  Over a candidate subset `cand` (ascending node ids) dc is [C, d]: its rows are first
    added into a zeroed [N, d] gradient at the rows `cand` names (ghf_rows_accumulate_any — ghf_rows_accumulate for every
    row width the losses take —: the ids are distinct, one add per element, so reproducible too); every other row of it
    stays exactly zero.  Nothing of size [N, d] is made when embs needs no gradient."""
    if rows is None and not ctx.needs_input_grad[0]:        # recorded for the bias alone: embs is data
        return None, None
    if cand is not None and (rows is None or ctx.needs_input_grad[0]):
        dc = _native.rows_accumulate(torch.zeros_like(embs), cand, dc, any_width=True)
    if rows is None:
        return _native.add3(dc, _fold_rows(dq, query, embs.size(0)), out=dc), None
    return (dc if ctx.needs_input_grad[0] else None), (dq if ctx.needs_input_grad[1] else None)


def _bias_grad(ctx, pos: int, db, bias, cand):
    """The [N] gradient of a loss's per-candidate bias (input number `pos`) from its backward call's db: db itself for an
    all-node call; over a candidate subset db is [C], entry j belonging to node cand[j] — the ids are distinct, so one copy
    into a zeroed [N] places it, and every other node's entry stays exactly zero."""
    if bias is None or not ctx.needs_input_grad[pos]:
        return None
    if cand is None:
        return db
    return torch.zeros_like(bias).index_copy_(0, cand, db)


class SoftmaxLossFn(torch.autograd.Function):
    """loss_i = log sum_{j in J_i} exp(scale q_i . embs[j]) - scale q_i . embs[target_i] over ALL nodes j outside query i's
    filter list (HyperGNN.softmax_loss; include/ghf.h: ghf_score_softmax_fwd), with q_i = embs[query_i], or q_i = rows_i where
    the query rows are given (``softmax_loss(..., query_rows=Q)``): exactly one of `rows` and `query` is.  The [B, N] logits
    exist neither here nor in the backward, which recomputes them tile by tile from the saved lse (ghf_score_softmax_bwd);
    _all_node_loss_grads turns its (dq, dc) into the gradients.  `cand` (ascending node ids, HyperGNN._candidate_ids' form with
    the targets added) restricts the sum to those nodes (ghf_score_softmax_fwd_sub / _bwd_sub): dc is then one row per
    candidate and is added into embs' own rows.  `bias` (fp32 [N], one entry per node): the logits are fmaf(scale, q_i . embs[j],
    bias[j]) (ghf_score_softmax_fwd_b / _bwd_b; None runs exactly the calls above); its gradient is the backward's db
    (_bias_grad)."""

    @staticmethod
    def forward(ctx, embs, rows, query, target, ptr, idx, scale: float, cand=None, bias=None):
        assert (rows is None) != (query is None)
        embs = embs.contiguous().float()
        rows = None if rows is None else rows.contiguous().float()
        bias = None if bias is None else bias.contiguous()
        loss, lse = _native.score_softmax_fwd(embs if rows is None else rows, embs, target, iq=query, filt_ptr=ptr, filt_idx=idx,
                                              scale=scale, ic=cand, bias=bias)
        ctx.save_for_backward(embs, rows, query, target, ptr, idx, lse, cand, bias)
        ctx.scale = scale
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        embs, rows, query, target, ptr, idx, lse, cand, bias = ctx.saved_tensors
        if bias is None:
            dq, dc = _native.score_softmax_bwd(embs if rows is None else rows, embs, target, lse, g.contiguous().float(), iq=query,
                                               filt_ptr=ptr, filt_idx=idx, scale=ctx.scale, ic=cand)
            return _all_node_loss_grads(ctx, embs, rows, query, dq, dc, cand) + (None,) * 7
        dq, dc, db = _native.score_softmax_bwd(embs if rows is None else rows, embs, target, lse, g.contiguous().float(), iq=query,
                                               filt_ptr=ptr, filt_idx=idx, scale=ctx.scale, ic=cand, bias=bias,
                                               want_db=ctx.needs_input_grad[8])
        return _all_node_loss_grads(ctx, embs, rows, query, dq, dc, cand) + (None,) * 6 + (_bias_grad(ctx, 8, db, bias, cand),)


class BceLossFn(torch.autograd.Function):
    """loss_i = sum_j bce_with_logits(scale q_i . embs[j], y_ij) over ALL nodes j, y_ij = (1 - smoothing) [j in query i's list]
    + smoothing / N (HyperGNN.bce_loss; include/ghf.h: ghf_score_bce_fwd), q_i and the pair `rows` / `query` as in
    SoftmaxLossFn.  Neither the [B, N] logits nor the labels exist, here or in the backward, which recomputes the logits tile
    by tile (ghf_score_bce_bwd); _all_node_loss_grads turns its (dq, dc) into the gradients.  `cand` (ascending node ids): the
    loss over those C nodes alone, smoothing / C (ghf_score_bce_fwd_sub / _bwd_sub), dc one row per candidate.  `bias` (fp32 [N],
    finite): the learned entity bias of the 1-N models, logits fmaf(scale, q_i . embs[j], bias[j]) (ghf_score_bce_fwd_b /
    _bwd_b; None runs exactly the calls above); its gradient is the backward's db (_bias_grad)."""

    @staticmethod
    def forward(ctx, embs, rows, query, ptr, idx, scale: float, smoothing: float, cand=None, bias=None):
        assert (rows is None) != (query is None)
        embs = embs.contiguous().float()
        rows = None if rows is None else rows.contiguous().float()
        bias = None if bias is None else bias.contiguous()
        loss = _native.score_bce_fwd(embs if rows is None else rows, embs, iq=query, pos_ptr=ptr, pos_idx=idx, scale=scale,
                                     smoothing=smoothing, ic=cand, bias=bias)
        ctx.save_for_backward(embs, rows, query, ptr, idx, loss, cand, bias)
        ctx.scale, ctx.smoothing = scale, smoothing
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        embs, rows, query, ptr, idx, loss, cand, bias = ctx.saved_tensors
        if bias is None:
            dq, dc = _native.score_bce_bwd(embs if rows is None else rows, embs, loss, g.contiguous().float(), iq=query, pos_ptr=ptr,
                                           pos_idx=idx, scale=ctx.scale, smoothing=ctx.smoothing, ic=cand)
            return _all_node_loss_grads(ctx, embs, rows, query, dq, dc, cand) + (None,) * 7
        dq, dc, db = _native.score_bce_bwd(embs if rows is None else rows, embs, loss, g.contiguous().float(), iq=query, pos_ptr=ptr,
                                           pos_idx=idx, scale=ctx.scale, smoothing=ctx.smoothing, ic=cand, bias=bias,
                                           want_db=ctx.needs_input_grad[8])
        return _all_node_loss_grads(ctx, embs, rows, query, dq, dc, cand) + (None,) * 6 + (_bias_grad(ctx, 8, db, bias, cand),)


class NegSamplingLossFn(torch.autograd.Function):
    """loss_i = softplus(-(z_it + margin)) + sum_{j in J_i} w_ij softplus(z_ij + margin), z_ij = scale q_i . embs[j] (+ bias[j]),
    J_i every node (every candidate of `cand`) outside query i's filter list other than its target, w_ij = softmax_j(alpha z_ij)
    over J_i taken as a CONSTANT, as in RotatE and PyKEEN's NSSALoss (HyperGNN.negative_sampling_loss; include/ghf.h:
    ghf_score_negsamp_fwd); q_i and the pair `rows` / `query` as in SoftmaxLossFn.  Saved is lw_i = log sum_{J_i} exp(alpha
    z_ij), from which the backward recomputes the weights tile by tile (ghf_score_negsamp_bwd); _all_node_loss_grads and
    _bias_grad turn its (dq, dc, db) into the gradients exactly as for the softmax loss."""

    @staticmethod
    def forward(ctx, embs, rows, query, target, ptr, idx, scale: float, margin: float, alpha: float, cand=None, bias=None):
        assert (rows is None) != (query is None)
        embs = embs.contiguous().float()
        rows = None if rows is None else rows.contiguous().float()
        bias = None if bias is None else bias.contiguous()
        loss, lw = _native.score_negsamp_fwd(embs if rows is None else rows, embs, target, iq=query, filt_ptr=ptr, filt_idx=idx,
                                             scale=scale, margin=margin, adversarial_temperature=alpha, ic=cand, bias=bias)
        ctx.save_for_backward(embs, rows, query, target, ptr, idx, lw, cand, bias)
        ctx.scale, ctx.margin, ctx.alpha = scale, margin, alpha
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        embs, rows, query, target, ptr, idx, lw, cand, bias = ctx.saved_tensors
        res = _native.score_negsamp_bwd(embs if rows is None else rows, embs, target, lw, g.contiguous().float(), iq=query,
                                        filt_ptr=ptr, filt_idx=idx, scale=ctx.scale, margin=ctx.margin,
                                        adversarial_temperature=ctx.alpha, ic=cand, bias=bias,
                                        want_db=bias is not None and ctx.needs_input_grad[10])
        db = res[2] if bias is not None else None
        return _all_node_loss_grads(ctx, embs, rows, query, res[0], res[1], cand) + (None,) * 8 + (_bias_grad(ctx, 10, db, bias, cand),)


def per_query_forward(loss: str, metric: int, q, embs, target, neg, iq, ptr, idx, scale: float, margin: float, alpha: float,
                      normalize: bool, bias):
    """(loss, saved, active) of the forward call that `loss` ("softmax", "negsamp", "hinge", "logistic") and `metric`
    (_native.PAIR_DOT or a distance) name among the per-query family's: saved is lse, lw or the pair count, active None but
    for the pairwise losses."""
    kw = dict(iq=iq, filt_ptr=ptr, filt_idx=idx, scale=scale)
    dot = metric == _native.PAIR_DOT
    if loss in _native.PAIR_KINDS:
        return _native.score_pair_fwd(metric, _native.PAIR_KINDS[loss], q, embs, target, neg, margin=margin, normalize=normalize, bias=bias, **kw)
    if loss == "negsamp":
        kw.update(margin=margin, adversarial_temperature=alpha)
    elif loss != "softmax":
        raise ValueError(f"no per-query loss {loss!r}")
    fwd = getattr(_native, f"score_{'neg' if dot else 'dist'}_{loss}_fwd")
    return (fwd(q, embs, target, neg, bias=bias, **kw) if dot else fwd(metric, q, embs, target, neg, **kw)) + (None,)


class PerQueryLossFn(torch.autograd.Function):
    """A loss of every query against ITS OWN negatives `neg` [B, K] (node ids, -1 = no entry, a multiset in the given order;
    ``negatives=`` of HyperGNN.softmax_loss / negative_sampling_loss, and HyperGNN.pairwise_loss), q_i and the pair `rows` /
    `query` as in SoftmaxLossFn.  `loss` names it: "softmax" or "negsamp" (include/ghf_negatives.h, ghf_distance.h; returns the
    loss) or "hinge" or "logistic" (include/ghf_pairwise.h; returns (loss, active), active — the violated pairs — without a
    gradient).  `metric` names the score: _native.PAIR_DOT, the dot product, with an optional `bias`, or _native.DIST_L1 /
    DIST_L2 / DIST_COMPLEX, s = -D(q_i, embs[v]).

    Saved is what the forward's kernel left for the backward (lse, lw or the pair count) and the grouping of the B (K + 1) node
    ids [neg | target] by node (ghf_group_edges, stable; an entry that is padding stands under its query's target with
    coefficient 0), which depends on the ids alone.  The backward (ghf_neg_bwd / ghf_dist_bwd / ghf_pair_bwd) recomputes the
    logits, returns dq per query and the coefficients coef [B, K + 1] — one per position, the target's last.  Under the dot
    product d embs is the sum of coef q_i over the entries that name a node, per node in the grouping's order
    (ghf_segment_axpy, as ScoreEdgesFn does), and d bias the same sum over a column of ones, over scale; under a distance the
    gradient of a candidate row is no multiple of the query's row and d embs is ghf_dist_rows_grad over coef.  Either way dq
    is folded in through `query` when the queries are embs' own rows.  Reproducible; a row that is no one's negative, target
    or query gets exactly zero; nothing of size [N, d] is made when embs needs no gradient."""

    @staticmethod
    def forward(ctx, embs, rows, query, target, ptr, idx, neg, metric: int, loss: str, scale: float, margin: float, alpha: float,
                normalize: bool, bias=None):
        assert (rows is None) != (query is None)
        embs = embs.contiguous().float()
        rows = None if rows is None else rows.contiguous().float()
        bias = None if bias is None else bias.contiguous()
        q = embs if rows is None else rows
        out, saved, active = per_query_forward(loss, metric, q, embs, target, neg, query, ptr, idx, scale, margin, alpha, normalize, bias)
        perm = off = None
        if ctx.needs_input_grad[0] or (bias is not None and ctx.needs_input_grad[13]):
            N = embs.size(0)
            keys = torch.cat([torch.where(neg < 0, target.unsqueeze(1), neg), target.unsqueeze(1)], 1).reshape(-1).clamp_(0, N - 1)
            perm, off = _native.group_edges(keys, N)
        ctx.save_for_backward(embs, rows, query, target, ptr, idx, neg, saved, bias, perm, off)
        ctx.metric, ctx.loss, ctx.scale, ctx.margin, ctx.alpha, ctx.normalize = metric, loss, scale, margin, alpha, normalize
        if active is None:
            return out
        ctx.mark_non_differentiable(active)
        return out, active

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g, _g_active=None):
        embs, rows, query, target, ptr, idx, neg, saved, bias, perm, off = ctx.saved_tensors
        q = embs if rows is None else rows
        g = g.contiguous().float()
        kw = dict(iq=query, filt_ptr=ptr, filt_idx=idx, scale=ctx.scale, margin=ctx.margin)
        dot = ctx.metric == _native.PAIR_DOT
        if ctx.loss in _native.PAIR_KINDS:
            dq, coef = _native.score_pair_bwd(ctx.metric, _native.PAIR_KINDS[ctx.loss], q, embs, target, neg, saved, g, normalize=ctx.normalize, bias=bias, **kw)
        else:
            mode = _native.NEG_SOFTMAX if ctx.loss == "softmax" else _native.NEG_NEGSAMP
            kw.update(adversarial_temperature=ctx.alpha)
            dq, coef = (_native.score_neg_bwd(mode, q, embs, target, neg, saved, g, bias=bias, **kw) if dot else
                        _native.score_dist_bwd(ctx.metric, mode, q, embs, target, neg, saved, g, **kw))
        w = coef.reshape(-1)
        d_embs = d_rows = d_bias = None
        if ctx.needs_input_grad[0]:
            if dot:
                owner = torch.div(perm, neg.size(1) + 1, rounding_mode="floor")    # the query of every grouped entry
                if query is not None:
                    owner = query.index_select(0, owner)
                d_embs = _native.segment_axpy(w, perm, q, owner.clamp_(0, q.size(0) - 1), off)
            else:
                d_embs = _native.dist_rows_grad(ctx.metric, q, embs, coef, perm, off, iq=query)
            if rows is None:
                d_embs = _native.add3(d_embs, _fold_rows(dq, query, embs.size(0)), out=d_embs)
        if rows is not None and ctx.needs_input_grad[1]:
            d_rows = dq
        if bias is not None and ctx.needs_input_grad[13]:
            one = torch.ones(1, 1, dtype=torch.float32, device=embs.device)
            d_bias = _native.segment_axpy(w, perm, one, torch.zeros_like(perm), off).reshape(-1).mul_(1.0 / ctx.scale)
        return (d_embs, d_rows) + (None,) * 11 + (d_bias,)


class DistanceSweepLossFn(torch.autograd.Function):
    """The softmax (mode NEG_SOFTMAX) or negative-sampling (NEG_NEGSAMP) loss of a query against EVERY node, or the shared
    candidate set `cand`, with z_ij = -scale D(q_i, embs[j]) under `metric` (HyperGNN.softmax_loss_by_distance /
    negative_sampling_loss_by_distance; include/ghf_distance_loss.h).  q_i and the pair `rows` / `query` as in SoftmaxLossFn.
    Saved is the forward's lse / lw; the backward recomputes every distance (ghf_dist_loss_bwd) and returns dq per query and dc
    per candidate, which _all_node_loss_grads turns into the gradients exactly as for the dot-product losses: rows of embs that
    are neither candidate, target nor query get exactly zero."""

    @staticmethod
    def forward(ctx, embs, rows, query, target, ptr, idx, metric: int, mode: int, scale: float, margin: float, alpha: float,
                cand=None):
        assert (rows is None) != (query is None)
        embs = embs.contiguous().float()
        rows = None if rows is None else rows.contiguous().float()
        q = embs if rows is None else rows
        if mode == _native.NEG_SOFTMAX:
            loss, saved = _native.score_dist_loss_softmax_fwd(metric, q, embs, target, iq=query, filt_ptr=ptr, filt_idx=idx,
                                                              scale=scale, ic=cand)
        else:
            loss, saved = _native.score_dist_loss_negsamp_fwd(metric, q, embs, target, iq=query, filt_ptr=ptr, filt_idx=idx,
                                                              scale=scale, margin=margin, adversarial_temperature=alpha, ic=cand)
        ctx.save_for_backward(embs, rows, query, target, ptr, idx, saved, cand)
        ctx.metric, ctx.mode, ctx.scale, ctx.margin, ctx.alpha = metric, mode, scale, margin, alpha
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        embs, rows, query, target, ptr, idx, saved, cand = ctx.saved_tensors
        dq, dc = _native.score_dist_loss_bwd(ctx.metric, ctx.mode, embs if rows is None else rows, embs, target, saved,
                                             g.contiguous().float(), iq=query, filt_ptr=ptr, filt_idx=idx, scale=ctx.scale,
                                             margin=ctx.margin, adversarial_temperature=ctx.alpha, ic=cand)
        return _all_node_loss_grads(ctx, embs, rows, query, dq, dc, cand) + (None,) * 10


class DistancePairSweepLossFn(torch.autograd.Function):
    """The hinge or logistic pairwise loss (`kind` _native.PAIR_HINGE / PAIR_LOGISTIC) of a query's target against EVERY node,
    or the shared candidate set `cand`, with z_ij = -scale D(q_i, embs[j]) under `metric`
    (HyperGNN.pairwise_loss_by_distance; include/ghf_pairwise_sweep.h).  q_i and the pair `rows` / `query` as in SoftmaxLossFn.
    Returns (loss, active), active — the violated pairs — without a gradient.  Saved are the forward's dsum (the sum of phi'
    over J_i, from which the target's coefficient follows without a second sweep) and count; the backward recomputes every
    distance (ghf_dist_pair_bwd) and returns dq per query and dc per candidate, which _all_node_loss_grads turns into the
    gradients exactly as for the other losses against every node: rows of embs that are neither candidate, target nor query
    get exactly zero."""

    @staticmethod
    def forward(ctx, embs, rows, query, target, ptr, idx, metric: int, kind: int, scale: float, margin: float, normalize: bool,
                cand=None):
        assert (rows is None) != (query is None)
        embs = embs.contiguous().float()
        rows = None if rows is None else rows.contiguous().float()
        loss, dsum, count, active = _native.score_dist_pair_sweep_fwd(metric, kind, embs if rows is None else rows, embs, target,
                                                                      iq=query, filt_ptr=ptr, filt_idx=idx, scale=scale, margin=margin,
                                                                      normalize=normalize, ic=cand)
        ctx.save_for_backward(embs, rows, query, target, ptr, idx, dsum, count, cand)
        ctx.metric, ctx.kind, ctx.scale, ctx.margin, ctx.normalize = metric, kind, scale, margin, normalize
        ctx.mark_non_differentiable(active)
        return loss, active

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g, _g_active=None):
        embs, rows, query, target, ptr, idx, dsum, count, cand = ctx.saved_tensors
        dq, dc = _native.score_dist_pair_sweep_bwd(ctx.metric, ctx.kind, embs if rows is None else rows, embs, target, dsum, count,
                                                   g.contiguous().float(), iq=query, filt_ptr=ptr, filt_idx=idx, scale=ctx.scale,
                                                   margin=ctx.margin, normalize=ctx.normalize, ic=cand)
        return _all_node_loss_grads(ctx, embs, rows, query, dq, dc, cand) + (None,) * 10


class DotPairSweepLossFn(torch.autograd.Function):
    """The hinge or logistic pairwise loss (`kind` _native.PAIR_HINGE / PAIR_LOGISTIC) of a query's target against EVERY node,
    or the shared candidate set `cand`, by dot product: z_ij = scale q_i . embs[j] (+ bias[j])
    (HyperGNN.pairwise_loss_by_dot; include/ghf_pairwise_dot_sweep.h).  q_i and the pair `rows` / `query` as in SoftmaxLossFn.
    Returns (loss, active), active — the violated pairs — without a gradient.  Saved are the forward's dsum (the sum of phi'
    over J_i, from which the target's coefficient follows without a second sweep) and count; the backward recomputes every
    score on the matrix cores (ghf_score_pair_bwd) and returns dq per query, dc per candidate and db, which
    _all_node_loss_grads and _bias_grad turn into the gradients exactly as for the negative-sampling loss: rows of embs that
    are neither candidate, target nor query get exactly zero."""

    @staticmethod
    def forward(ctx, embs, rows, query, target, ptr, idx, kind: int, scale: float, margin: float, normalize: bool, cand=None,
                bias=None):
        assert (rows is None) != (query is None)
        embs = embs.contiguous().float()
        rows = None if rows is None else rows.contiguous().float()
        bias = None if bias is None else bias.contiguous()
        loss, dsum, count, active = _native.score_pair_sweep_fwd(kind, embs if rows is None else rows, embs, target, iq=query,
                                                                 filt_ptr=ptr, filt_idx=idx, scale=scale, margin=margin,
                                                                 normalize=normalize, ic=cand, bias=bias)
        ctx.save_for_backward(embs, rows, query, target, ptr, idx, dsum, count, cand, bias)
        ctx.kind, ctx.scale, ctx.margin, ctx.normalize = kind, scale, margin, normalize
        ctx.mark_non_differentiable(active)
        return loss, active

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g, _g_active=None):
        embs, rows, query, target, ptr, idx, dsum, count, cand, bias = ctx.saved_tensors
        res = _native.score_pair_sweep_bwd(ctx.kind, embs if rows is None else rows, embs, target, dsum, count, g.contiguous().float(),
                                           iq=query, filt_ptr=ptr, filt_idx=idx, scale=ctx.scale, margin=ctx.margin,
                                           normalize=ctx.normalize, ic=cand, bias=bias,
                                           want_db=bias is not None and ctx.needs_input_grad[11])
        db = res[2] if bias is not None else None
        return _all_node_loss_grads(ctx, embs, rows, query, res[0], res[1], cand) + (None,) * 9 + (_bias_grad(ctx, 11, db, bias, cand),)


class ScorePairsFn(torch.autograd.Function):
    """s_i = a_i . b_i (reference score_triple, hypergnn.py:304-318)."""

    @staticmethod
    def forward(ctx, a, b):
        a, b = a.contiguous().float(), b.contiguous().float()
        ctx.save_for_backward(a, b)
        return _native.score_pairs_fwd(a, b)

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        g = g.contiguous().float()
        return (_native.rowscale(b, g) if ctx.needs_input_grad[0] else None,
                _native.rowscale(a, g) if ctx.needs_input_grad[1] else None)


# ---- relation-typed scoring (models/relation_decoder.py; include/ghf.h: ghf_relation_rows) -----------------------------
def _fold_rows(rows: torch.Tensor, ids: torch.Tensor, n: int) -> torch.Tensor:
    """out[v] = sum_{i: ids[i] = v} rows[i], [n, d]: grouped by v (ghf_group_edges, stable) and added in that order."""
    if ids.numel() == 0:                                    # no row, nothing to group: zeros
        return torch.zeros(n, rows.size(1), dtype=torch.float32, device=rows.device)
    perm, off = _native.group_edges(ids, n)
    return _native.segment_axpy(torch.ones(ids.numel(), dtype=torch.float32, device=rows.device), perm, rows, perm, off)


class RelationRowsFn(torch.autograd.Function):
    """out_i = x[ix_i] + x[ix_i] @ A[rel_i] + b[rel_i] (ghf_relation_rows), A [R, d, d] and b [R, d] normally a
    WeightGenerator's heads.  The queries are grouped by relation once; the backward reuses the grouping:
        dx_rows_i = g_i + g_i @ A[rel_i]^T      the same call with GHF_REL_TRANSPOSE, no bias
        dx[v]     = sum_{i: ix_i = v} dx_rows_i   grouped by node, added in a fixed order (ghf_segment_axpy)
        dA[r]     = sum_{i in r} x[ix_i]^T g_i    db[r] = sum_{i in r} g_i      (ghf_group_outer over the relation groups)
    No [B, d, d] tensor, no atomics: reproducible."""

    @staticmethod
    def forward(ctx, x, ix, rel, A, b):
        x, A = x.contiguous().float(), A.contiguous().float()
        b = None if b is None else b.contiguous().float()
        group = _native.group_edges(rel, A.size(0))
        ctx.save_for_backward(x, A, rel, *group, *(() if ix is None else (ix,)))
        ctx.has_bias = b is not None
        return _native.relation_rows(x, rel, A, b, ix=ix, add_x=True, group=group)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        x, A, rel, perm, goff, *rest = ctx.saved_tensors
        ix = rest[0] if rest else None
        g = g.contiguous().float()
        B, rows = rel.numel(), x.size(0)
        dx = dA = db = None
        if ctx.needs_input_grad[0]:
            dx = _native.relation_rows(g, rel, A, None, add_x=True, transpose=True, group=(perm, goff))
            if ix is not None:
                dx = _fold_rows(dx, ix, rows)
            elif rows > B:                                   # rows beyond the B queries took no part
                dx = torch.cat([dx, torch.zeros(rows - B, dx.size(1), dtype=dx.dtype, device=dx.device)])
        if ctx.needs_input_grad[3]:
            dA = _native.group_outer(x, perm if ix is None else ix.index_select(0, perm), g, perm, goff)
        if ctx.has_bias and ctx.needs_input_grad[4]:
            db = _native.group_outer(None, None, g, perm, goff).reshape(A.size(0), -1)
        return dx, None, None, dA, db


class RelationScoresFn(torch.autograd.Function):
    """S[i, u] = (x[ia_i] + x[ia_i] @ A[u] + b[u]) . x[ib_i] (ghf_relation_scores): every relation's score for every pair,
    A [U, d, d] and b [U, d] normally a WeightGenerator's heads.  With G = dS:
        db_rows_i = sum_u G[i, u] (a_i + a_i @ A[u] + b[u])        the sweep with "add G q" as its epilogue
        da_rows_i = sum_u G[i, u] (b_i + b_i @ A[u]^T)             the same call on the b rows, transposed, no bias
        dx        = _fold_rows([da_rows; db_rows], [ia; ib])   (= fold(da_rows, ia) + fold(db_rows, ib) in one fixed order)
        dA[u]     = sum_i G[i, u] a_i^T b_i     db[u] = sum_i G[i, u] b_i      (ghf_relation_scores_bwd_weights)
    Nothing of size B x U x d or B x d x d, no atomics: reproducible."""

    @staticmethod
    def forward(ctx, x, ia, ib, A, b):
        x, A = x.contiguous().float(), A.contiguous().float()
        b = None if b is None else b.contiguous().float()
        ctx.save_for_backward(x, ia, ib, A, *(() if b is None else (b,)))
        return _native.relation_scores(x, ia, ib, A, b, add_x=True)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        x, ia, ib, A, *rest = ctx.saved_tensors
        b = rest[0] if rest else None
        g = g.contiguous().float()
        n = x.size(0)
        dx = dA = db = None
        if ctx.needs_input_grad[0]:
            da_rows = _native.relation_scores_bwd_rows(x, ib, g, A, None, add_x=True, transpose=True)
            db_rows = _native.relation_scores_bwd_rows(x, ia, g, A, b, add_x=True)
            dx = _fold_rows(torch.cat([da_rows, db_rows]), torch.cat([ia, ib]), n)   # one grouping, one pass over [n, d]
        want_b = b is not None and ctx.needs_input_grad[4]
        if ctx.needs_input_grad[3] or want_b:
            dA, db = _native.relation_scores_bwd_weights(x, ia, ib, g, want_bias=want_b)
            if not ctx.needs_input_grad[3]:
                dA = None
        return dx, None, None, dA, db


class ScoreRowsFn(torch.autograd.Function):
    """s_i = Q_i . embs[tail_i] (RelationDecoder.score).  dQ_i = g_i embs[tail_i]; d embs[v] = sum_{i: tail_i = v} g_i Q_i,
    grouped by node and summed in a fixed order as ScoreEdgesFn does."""

    @staticmethod
    def forward(ctx, Q, embs, tail):
        Q, embs = Q.contiguous().float(), embs.contiguous().float()
        ctx.save_for_backward(Q, embs, tail)
        return _native.score_pairs_fwd(Q, embs, None, tail)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        Q, embs, tail = ctx.saved_tensors
        g = g.contiguous().float()
        dQ = dE = None
        if ctx.needs_input_grad[0]:
            dQ = _native.rowscale(embs.index_select(0, tail), g)
        if ctx.needs_input_grad[1]:
            perm, off = _native.group_edges(tail, embs.size(0))
            dE = _native.segment_axpy(g, perm, Q, perm, off)
        return dQ, dE, None
