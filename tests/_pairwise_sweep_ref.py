"""The pairwise ranking losses under a distance against every node or a shared candidate set
(include/ghf_pairwise_sweep.h; HyperGNN.pairwise_loss_by_distance), restated in float64 on the CPU.  The restatement is thin:
the set P every query is scored against — all N nodes, or the candidates with the batch's targets added, ascending
(_distance_loss_ref.candidate_set) — is repeated per query as its negatives, and tests/_pairwise_ref.loss does the rest: J_i
(the listed ids and the target leave), u, phi, the count, the violated pairs, and the gradients by autograd.  Added here is
dsum, the sum of phi' over J_i that the forward leaves for the backward, and the kink rule of the parity tests.

Also here: the problems the parity tests run (test_distance_loss_host.parity_problem at pinned seeds) and their references,
computed once per process and shared.  Nothing here needs a GPU."""

from __future__ import annotations

import functools
from typing import Optional

import numpy as np
import torch

import _pairwise_ref as PR
from _distance_loss_ref import candidate_set

KINDS = PR.KINDS
MARGIN = 1.0


def loss(kind: str, metric: str, rows, c, target, lists=None, cand=None, scale: float = 1.0, margin: float = 1.0,
         normalize: bool = True, grad: Optional[torch.Tensor] = None, add_targets: bool = True):
    """_pairwise_ref.loss's dict (loss, count, active, u [B, |P|], live, zt[, coef, dq [B, d], dc [N, d]]) for queries `rows`
    [B, d] against P, and dsum [B].  `add_targets` False: P is `cand` as given (the C ABI adds nothing)."""
    N, B = c.size(0), rows.size(0)
    P = candidate_set(N, target, cand) if add_targets or cand is None else np.unique(np.asarray(cand, dtype=np.int64))
    neg = torch.from_numpy(P).unsqueeze(0).expand(B, len(P)).contiguous()
    out = PR.loss(kind, metric, rows, c, target, neg, lists, None, scale, margin, normalize, grad)
    dphi = (out["u"] > 0).double() if kind == "hinge" else torch.sigmoid(out["u"])
    out["dsum"] = torch.where(out["live"], dphi, torch.zeros_like(dphi)).sum(1)
    out["P"] = P
    return out


embs_grad = PR.embs_grad


def near(out: dict, margin: float):
    """(near [B] bool, in_band [B] int64) of a reference `out`: the queries with a pair of J_i inside _pairwise_ref.band around
    the hinge's kink, and how many such pairs each has."""
    inside = out["live"] & (out["u"].abs() < PR.band(out["zt"], margin).unsqueeze(1))
    return inside.any(1), inside.sum(1)


# ---- the problems of the parity tests ---------------------------------------------------------------------------------------
# The seed of parity_problem(d, C, B, subset) per (metric, (d, C, B), subset) where it is not that function's own default: the
# first of default + 1, default + 2, ... (60 tries) at which neither form of the queries (by id, translated rows) has a near
# query at margin 1.  A case that is absent and still has near queries at its default found no clear seed in 60 tries; it
# stays within the cap of B / 8 (tests/test_pairwise_sweep_host.py holds every case to it) and its near queries follow the
# kink rule.
SEEDS = {("l1", (20, 257, 129), True): 610, ("l1", (4, 513, 5), True): 564, ("l1", (6, 63, 65), False): 201,
         ("l1", (6, 63, 65), True): 202, ("l1", (6, 64, 63), False): 199, ("l1", (6, 64, 63), True): 200,
         ("l1", (6, 65, 64), False): 196, ("l2", (20, 257, 129), True): 607, ("l2", (4, 513, 5), False): 570,
         ("l2", (4, 513, 5), True): 563, ("l2", (6, 63, 65), False): 196, ("l2", (6, 63, 65), True): 201,
         ("l2", (6, 64, 63), False): 196, ("l2", (6, 64, 63), True): 195, ("l2", (6, 65, 64), False): 201,
         ("l2", (6, 65, 64), True): 196, ("complex", (20, 257, 129), False): 607, ("complex", (20, 257, 129), True): 608,
         ("complex", (20, 2600, 129), False): 2950, ("complex", (20, 2600, 129), True): 2968, ("complex", (4, 513, 5), True): 564,
         ("complex", (6, 63, 65), False): 203, ("complex", (6, 63, 65), True): 201, ("complex", (6, 64, 63), False): 206,
         ("complex", (6, 64, 63), True): 201, ("complex", (6, 65, 64), False): 198, ("complex", (6, 65, 64), True): 198}


def seed_of(metric: str, shape, subset: bool):
    return SEEDS.get((metric, tuple(shape), bool(subset)))


@functools.lru_cache(maxsize=None)
def problem(metric: str, shape, subset: bool):
    from test_distance_loss_host import parity_problem
    d, C, B = shape
    return parity_problem(d, C, B, subset, seed_of(metric, shape, subset))


# the two forms every parity problem runs in: all nodes with the queries by id, a shuffled subset with translated rows
FORMS = ((False, True), (True, False))                      # (subset, by_id)


@functools.lru_cache(maxsize=None)
def _first(metric: str, shape, subset: bool, by_id: bool):
    """(rows, near [B], in_band [B]) of one form: which queries are near does not depend on the kind or on normalize."""
    from test_distance_gpu import scale_for
    i = problem(metric, shape, subset)
    rows = i["embs"][i["q"]] if by_id else i["rows"]
    out = loss("hinge", metric, rows, i["embs"], i["t"], i["lists"], i["cand"], scale=scale_for(metric, shape[0]), margin=MARGIN)
    return (rows,) + near(out, MARGIN)


@functools.lru_cache(maxsize=None)
def reference(metric: str, shape, subset: bool, kind: str, normalize: bool, by_id: bool):
    """The float64 reference of one parity call, with the kink rule applied: (out, grad [B] fp32 with zeros at the near
    queries under the hinge, near [B], in_band [B]).  Computed once per process; nobody writes into it."""
    from test_distance_gpu import scale_for
    i = problem(metric, shape, subset)
    rows, nr, inb = _first(metric, shape, subset, by_id)
    grad = i["grad"].clone()
    if kind == "hinge":                                     # the logistic kind excuses nothing: its gradient has no jump
        grad[nr] = 0.0                                      # (`active` counts across u = 0 under either kind)
    out = loss(kind, metric, rows, i["embs"], i["t"], i["lists"], i["cand"], scale=scale_for(metric, shape[0]), margin=MARGIN,
               normalize=normalize, grad=grad)
    return out, grad, nr, inb


def active_check(what: str, got, out: dict, nr, inb):
    """`active` exactly the reference's, but for a near query: within its number of in-band pairs."""
    got = torch.as_tensor(got).cpu().to(torch.int64)
    diff = (got - out["active"]).abs()
    assert bool((diff <= torch.where(nr, inb, torch.zeros_like(inb))).all()), f"{what}: active {got.tolist()} vs {out['active'].tolist()}"
