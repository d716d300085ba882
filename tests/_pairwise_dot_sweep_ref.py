"""The pairwise ranking losses by dot product against every node or a shared candidate set
(include/ghf_pairwise_dot_sweep.h; HyperGNN.pairwise_loss_by_dot), restated in float64 on the CPU.  The restatement is thin, as
tests/_pairwise_sweep_ref.py's: the set P every query is scored against — all N nodes, or the candidates with the batch's
targets added, ascending (_distance_loss_ref.candidate_set) — is repeated per query as its negatives, and
tests/_pairwise_ref.loss("dot", bias=) does the rest: J_i (the listed ids and the target leave), u, phi, the count, the violated
pairs, and the gradients (dq, dc, db) by autograd.  Added here is dsum, the sum of phi' over J_i that the forward leaves for
the backward.  The kink rule is tests/_pairwise_sweep_ref.py's (near, active_check) over _pairwise_ref.band.

Also here: the problems the parity tests run, at pinned seeds, and their references, computed once per process and shared.
Nothing here needs a GPU."""

from __future__ import annotations

import functools
from typing import Optional

import numpy as np
import torch

import _pairwise_ref as PR
import _pairwise_sweep_ref as PS
from _distance_loss_ref import candidate_set

KINDS = PR.KINDS
MARGIN = 1.0
near, active_check, embs_grad = PS.near, PS.active_check, PR.embs_grad


def loss(kind: str, rows, c, target, lists=None, cand=None, bias=None, scale: float = 1.0, margin: float = 1.0,
         normalize: bool = True, grad: Optional[torch.Tensor] = None, add_targets: bool = True):
    """_pairwise_ref.loss's dict (loss, count, active, u [B, |P|], live, zt[, coef, dq [B, d], dc [N, d], db [N]]) for queries
    `rows` [B, d] against P, and dsum [B].  `add_targets` False: P is `cand` as given (the C ABI adds nothing)."""
    N, B = c.size(0), rows.size(0)
    P = candidate_set(N, target, cand) if add_targets or cand is None else np.unique(np.asarray(cand, dtype=np.int64))
    neg = torch.from_numpy(P).unsqueeze(0).expand(B, len(P)).contiguous()
    out = PR.loss(kind, "dot", rows, c, target, neg, lists, bias, scale, margin, normalize, grad)
    dphi = (out["u"] > 0).double() if kind == "hinge" else torch.sigmoid(out["u"])
    out["dsum"] = torch.where(out["live"], dphi, torch.zeros_like(dphi)).sum(1)
    out["P"] = P
    return out


def scale_for(d: int) -> float:
    return PR.parity_scale("dot", d)


# ---- the problems of the parity tests ---------------------------------------------------------------------------------------
# (d, C, B), from the sweeps' geometry.  Forward tiles: 128 queries x 256 candidates (128 for d > 128): C of 255 | 256 | 257 and
# 127 | 128 | 129, B of 127 | 129, three tiles at C = 513.  Backward: 64 streamed rows (C and B of 63 | 64 | 65), an owner tile
# of 128 (64 for d > 128).  d = 20 and 200 are no multiple of the 32 columns of a backward step, 128 | 256 fill the two kernel
# shapes.  C = 2,600 at d = 20: eleven forward tiles in eleven slabs.  C = 8,200: softmax_bwd_geom cuts the dq pass in slabs of
# at least 64 streamed tiles = 4,096 candidates, so two slabs need 128 tiles: C > 8,128 (at C = 4,500 there is one).
SHAPES = [(20, 1, 1), (20, 63, 5), (64, 64, 127), (64, 65, 129), (128, 127, 5), (128, 128, 129), (200, 129, 127), (200, 255, 5),
          (256, 256, 129), (256, 257, 1), (20, 513, 5), (200, 513, 5), (20, 2600, 127), (64, 8200, 70)]
SHAPE_IDS = ["d%d-C%d-B%d" % s for s in SHAPES]
# Past this many candidates the near-tie band cannot stay empty: a pair of scores of order 1 lies inside it with probability
# ~ 2e-4, so a query with thousands of pairs in J_i is near the kink more often than one time in eight whatever the seed.
# There every query node lists all but ~ LIVE of the nodes: the sweeps still stream, mask and count every candidate (their
# geometry is the point of those shapes), and J_i stays of a size at which the cap can hold.
DENSE_LISTS_FROM, LIVE = 600, 300

# The seed of problem(shape, subset) where it is not parity_problem's default (11 d + C + B): the first of default + 1, ... + 60
# at which no form (by id / rows, with / without the bias) has a near query at margin 1.  A case that is absent and still has
# near queries at its default found no clear seed in 60 tries; it stays within the cap of B / 8
# (tests/test_pairwise_dot_sweep_host.py holds every case to it) and its near queries follow the kink rule.
SEEDS = {((20, 513, 5), True): 739, ((200, 513, 5), False): 2719, ((64, 64, 127), False): 909, ((64, 64, 127), True): 907,
         ((64, 65, 129), False): 901, ((64, 65, 129), True): 902, ((128, 128, 129), False): 1667, ((200, 129, 127), False): 2465,
         ((200, 129, 127), True): 2463, ((200, 255, 5), False): 2461, ((256, 257, 1), True): 3075}
# the combinations of (kind, normalize, biased) a parity problem runs in: all eight, or, at C >= DENSE_LISTS_FROM (where the
# float64 restatement walks thousands of positions per call), four that hold every value of each beside every value of another
COMBOS = [(k, n, b) for k in KINDS for n in (True, False) for b in (False, True)]
COMBOS_LARGE = [("hinge", True, False), ("hinge", False, True), ("logistic", True, True), ("logistic", False, False)]
# ... and two, with every value once, at the one shape past 4,096 candidates (two seconds per call of the restatement), which
# is there for the second slab of the backward's dq pass
COMBOS_LARGEST = [("hinge", False, True), ("logistic", True, False)]


def combos(shape):
    return COMBOS_LARGEST if shape[1] > 4096 else COMBOS_LARGE if shape[1] >= DENSE_LISTS_FROM else COMBOS


def seed_of(shape, subset: bool):
    return SEEDS.get((tuple(shape), bool(subset)))


def make_problem(d, C, B, subset, seed=None):
    """test_distance_loss_host.parity_problem with a bias [N]; at C >= DENSE_LISTS_FROM with the dense lists (per query node,
    so that known= and the CSR lists still agree; the list of query 1 still holds its target)."""
    from test_distance_loss_host import parity_problem
    i = parity_problem(d, C, B, subset, seed)
    N = i["embs"].size(0)
    rng = np.random.default_rng((11 * d + C + B if seed is None else seed) + 7919)
    i["bias"] = torch.from_numpy((0.5 * rng.standard_normal(N)).astype(np.float32))
    if C >= DENSE_LISTS_FROM:
        query = i["q"].numpy()
        node_lists = {}
        for k, v in enumerate(query):
            if int(v) not in node_lists:
                node_lists[int(v)] = np.union1d(i["lists"][k], np.sort(rng.permutation(N)[:N - LIVE])).astype(np.int64)
        i["lists"] = [node_lists[int(v)] for v in query]
        src = np.concatenate([np.full(len(l), v) for v, l in node_lists.items()]).astype(np.int64)
        dst = np.concatenate(list(node_lists.values())).astype(np.int64)
        i["known"] = (torch.from_numpy(src), torch.from_numpy(dst))
    return i


@functools.lru_cache(maxsize=None)
def problem(shape, subset: bool):
    d, C, B = shape
    return make_problem(d, C, B, subset, seed_of(shape, subset))


# the two forms every parity problem runs in: all nodes with the queries by id, a shuffled subset with given rows
FORMS = ((False, True), (True, False))                      # (subset, by_id)


def _rows(i, by_id):
    return i["embs"][i["q"]] if by_id else i["rows"]


@functools.lru_cache(maxsize=None)
def _first(shape, subset: bool, by_id: bool, biased: bool):
    """(near [B], in_band [B]) of one form: which queries are near does not depend on the kind or on normalize."""
    i = problem(shape, subset)
    out = loss("hinge", _rows(i, by_id), i["embs"], i["t"], i["lists"], i["cand"], i["bias"] if biased else None,
               scale=scale_for(shape[0]), margin=MARGIN)
    return near(out, MARGIN)


@functools.lru_cache(maxsize=None)
def reference(shape, subset: bool, kind: str, normalize: bool, by_id: bool, biased: bool):
    """The float64 reference of one parity call, with the kink rule applied: (out, grad [B] fp32 with zeros at the near
    queries under the hinge, near [B], in_band [B]).  Computed once per process; nobody writes into it."""
    i = problem(shape, subset)
    nr, inb = _first(shape, subset, by_id, biased)
    grad = i["grad"].clone()
    if kind == "hinge":                                     # the logistic kind excuses nothing: its gradient has no jump
        grad[nr] = 0.0                                      # (`active` counts across u = 0 under either kind)
    out = loss(kind, _rows(i, by_id), i["embs"], i["t"], i["lists"], i["cand"], i["bias"] if biased else None,
               scale=scale_for(shape[0]), margin=MARGIN, normalize=normalize, grad=grad)
    return out, grad, nr, inb
