"""The bits of the all-node scoring family: ghf_score_rank, ghf_score_topk, ghf_score_softmax_fwd / _bwd and ghf_score_bce_fwd /
_bwd produce, case by case, exactly the bytes recorded in tests/golden/score_bits.json.

The four operations share one sweep (csrc/rank_sweep.h) and the two losses one backward kernel, so a cross-check between
them cannot see a change that hits all, and the float64-tolerance tests do not see a reordered addition or a moved launch.
This test does: the fixture holds a SHA-256 per case over the output tensors' bytes, and equality is exact.

    python tests/test_score_bits_gpu.py --record [--out PATH] [--commit ID]

records the fixture (tests/_bits.py).  Only public _native functions are called; inputs are integer hashes (tests/_bits.py).

Data: c = N hashed rows, q = 150 (hub cases: 350) hashed rows, queries i -> (37 i + 3) mod rows with query 100 repeating
query 7, targets i -> (977 i + 11) mod N, scale = 8 / sqrt(d).  Query i's list holds i mod 5 ids spread over [0, N), its
target when i mod 3 = 1, its first id twice when i mod 4 = 2 (for BCE: a duplicated positive), sorted; so the lists of
queries 0, 5, 15, ... are empty.

Cases, the smallest that reach each branch (geometry from rank_geom of csrc/rank_sweep.h with 1024 blocks wanted for rank and
256 for top-k, softmax_geom of the same file, softmax_bwd_geom of csrc/softmax.hip):
  widths d = 18 (d % 4 != 0: scalar loads), 20 (vectorised, a padded tail of k), 128 (the 256-candidate tile, full), 256 (the
  128-candidate, 256-thread instantiation).
  rank:     N = 777, B = 129: two query tiles, the second of one query; 4 candidate tiles of 256 (d = 256: 7 of 128), the last
            partial, one per slab; with and without lists; an out-of-range iq, list id and target (query 71: -1, -1).
  top-k:    the same data, k = 10 at every width, k = 1 and 128 at d = 20 and 256; N = 5 with k = 10 (five entries, then the
            (-inf, -1) fill); query 5 listing all but 3 candidates; an out-of-range iq and list id (NaN, -1).
  softmax / BCE forward: N = 777 (4 slabs of one tile; d = 256: 7); N = 33,000 at d = 20 (129 tiles, 65 slabs of 2, the last
            of 1); N = 16,500 at d = 256 (129 tiles of 128, 65 slabs); with and without lists; BCE with smoothing = 0.1; an
            out-of-range target (softmax) and list id (BCE): a NaN for query 71 alone.
  softmax / BCE backward: N = 777, B = 129 (dq: 2 owner tiles, d = 256: 3, one slab of 13 streamed tiles; dc: 7 owner tiles
            of 128, d = 256: 13 of 64, the last of 9 rows, 3 streamed query tiles); N = 8,300 (130 streamed tiles, two slabs
            of 65: the ordered sum of dq partials); hubs: B = 300, every query listing ids 130, 131, 140, 190 of N = 777, all
            inside one owner tile (128..255 at d = 64, 128..191 at d = 256): 1,200 pairs (softmax: less the few that are the
            query's target) > SB_HCAP = 1024, every id looked up; with ids 130, 190 only: 600 pairs, collected; a list id = N
            (it falls into the last owner tile's id range; the query's NaN loss keeps it out)."""

import functools
import os
import sys

import numpy as np
import pytest
import torch

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from _bits import dev, digest, hashed, load_fixture, record_main  # noqa: E402
from graph_hypernetwork_forge_amd import _native  # noqa: E402

pytestmark = pytest.mark.gpu
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "score_bits.json")
WIDTHS = (18, 20, 128, 256)
N0, B0, ROWS_Q = 777, 129, 150
HUB_B, HUB_ROWS_Q = 300, 350
BAD = 71                                                     # the query of the out-of-range cases
COVER, UNCOVERED = 5, (7, 388, 776)                          # top-k: query 5 lists every candidate but these


@functools.lru_cache(maxsize=None)
def cand(N, d):
    return dev(hashed(N, d, 11))


@functools.lru_cache(maxsize=None)
def queries(rows, d):
    return dev(hashed(rows, d, 12))


@functools.lru_cache(maxsize=None)
def grad(B):
    return dev(hashed(B, 1, 13).reshape(B))


def ids_np(B, rows_q, N):
    i = np.arange(B, dtype=np.int64)
    iq = (37 * i + 3) % rows_q
    iq[100] = iq[7]
    return iq, (977 * i + 11) % N


def lists_np(B, N, target, kind):
    """CSR lists of `kind`: lists / cover (query COVER lists all but UNCOVERED) / bad_list (query BAD's ends with N) /
    hub4, hub2 (every query lists the same ids)."""
    ptr, idx = [0], []
    for i in range(B):
        if kind in ("hub4", "hub2"):
            ids = [130, 131, 140, 190] if kind == "hub4" else [130, 190]
        else:
            ids = [(131 * i + t * (N // 5 + 1) + 17) % N for t in range(i % 5)]
            if i % 3 == 1:
                ids.append(int(target[i]))
            if i % 4 == 2 and ids:
                ids.append(ids[0])
            if kind == "cover" and i == COVER:
                ids = [j for j in range(N) if j not in UNCOVERED]
            ids.sort()
            if kind == "bad_list" and i == BAD:
                ids.append(N)
        idx += ids
        ptr.append(len(idx))
    return np.asarray(ptr, dtype=np.int64), np.asarray(idx, dtype=np.int64)


def inputs(N, d, kind, B=B0, rows_q=ROWS_Q):
    """(q, c, target, keywords iq / lists) of a case; kind: plain, bad_iq, bad_target or a kind of lists_np."""
    iq, target = ids_np(B, rows_q, N)
    kw = {}
    if kind not in ("plain", "bad_iq", "bad_target"):
        ptr, idx = lists_np(B, N, target, kind)
        kw = {"ptr": dev(ptr), "idx": dev(idx)}
    if kind == "bad_iq":
        iq[BAD] = rows_q
    if kind == "bad_target":
        target[BAD] = N
    return queries(rows_q, d), cand(N, d), dev(target), dev(iq), kw


def scale_of(d):
    return 8.0 * d ** -0.5


def case_rank(d, kind):
    q, c, target, iq, kw = inputs(N0, d, kind)
    return _native.score_rank(q, c, target, iq=iq, filt_ptr=kw.get("ptr"), filt_idx=kw.get("idx"))


def case_topk(d, k, kind, N=N0):
    q, c, _, iq, kw = inputs(N, d, kind)
    return _native.score_topk(q, c, k, iq=iq, filt_ptr=kw.get("ptr"), filt_idx=kw.get("idx"))


def case_softmax_fwd(N, d, kind):
    q, c, target, iq, kw = inputs(N, d, kind)
    return _native.score_softmax_fwd(q, c, target, iq=iq, filt_ptr=kw.get("ptr"), filt_idx=kw.get("idx"), scale=scale_of(d))


def case_bce_fwd(N, d, kind, smoothing=0.0):
    q, c, _, iq, kw = inputs(N, d, kind)
    return (_native.score_bce_fwd(q, c, iq=iq, pos_ptr=kw.get("ptr"), pos_idx=kw.get("idx"), scale=scale_of(d),
                                  smoothing=smoothing),)


def case_softmax_bwd(N, d, kind, B=B0, rows_q=ROWS_Q):
    q, c, target, iq, kw = inputs(N, d, kind, B, rows_q)
    lists = {"iq": iq, "filt_ptr": kw.get("ptr"), "filt_idx": kw.get("idx"), "scale": scale_of(d)}
    _, lse = _native.score_softmax_fwd(q, c, target, **lists)
    return _native.score_softmax_bwd(q, c, target, lse, grad(B), **lists)


def case_bce_bwd(N, d, kind, B=B0, rows_q=ROWS_Q, smoothing=0.0):
    q, c, _, iq, kw = inputs(N, d, kind, B, rows_q)
    lists = {"iq": iq, "pos_ptr": kw.get("ptr"), "pos_idx": kw.get("idx"), "scale": scale_of(d), "smoothing": smoothing}
    loss = _native.score_bce_fwd(q, c, **lists)
    return _native.score_bce_bwd(q, c, loss, grad(B), **lists)


def build_cases():
    P = functools.partial
    cases = {}
    for d in WIDTHS:
        for kind in ("lists", "plain"):
            cases[f"rank/N777/d{d}/{kind}"] = P(case_rank, d, kind)
            cases[f"softmax_fwd/N777/d{d}/{kind}"] = P(case_softmax_fwd, N0, d, kind)
            cases[f"bce_fwd/N777/d{d}/{kind}"] = P(case_bce_fwd, N0, d, kind)
        cases[f"topk/N777/d{d}/k10/lists"] = P(case_topk, d, 10, "lists")
        cases[f"softmax_bwd/N777/d{d}/lists"] = P(case_softmax_bwd, N0, d, "lists")
        cases[f"bce_bwd/N777/d{d}/lists"] = P(case_bce_bwd, N0, d, "lists")
    for kind in ("bad_iq", "bad_list", "bad_target"):
        cases[f"rank/N777/d20/{kind}"] = P(case_rank, 20, kind)
    for d in (20, 256):
        for k in (1, 128):
            cases[f"topk/N777/d{d}/k{k}/lists"] = P(case_topk, d, k, "lists")
    cases["topk/N777/d128/k10/plain"] = P(case_topk, 128, 10, "plain")
    cases["topk/N5/d20/k10/plain"] = P(case_topk, 20, 10, "plain", N=5)
    cases["topk/N777/d20/k10/cover"] = P(case_topk, 20, 10, "cover")
    cases["topk/N777/d20/k10/bad_iq"] = P(case_topk, 20, 10, "bad_iq")
    cases["topk/N777/d20/k10/bad_list"] = P(case_topk, 20, 10, "bad_list")
    for N, d in ((33_000, 20), (16_500, 256)):
        for kind in ("lists", "plain"):
            cases[f"softmax_fwd/N{N}/d{d}/{kind}"] = P(case_softmax_fwd, N, d, kind)
            cases[f"bce_fwd/N{N}/d{d}/{kind}"] = P(case_bce_fwd, N, d, kind)
    cases["softmax_fwd/N777/d20/bad_target"] = P(case_softmax_fwd, N0, 20, "bad_target")
    cases["bce_fwd/N777/d20/bad_list"] = P(case_bce_fwd, N0, 20, "bad_list")
    for d in (20, 256):
        cases[f"bce_fwd/N777/d{d}/lists/smooth"] = P(case_bce_fwd, N0, d, "lists", smoothing=0.1)
        cases[f"softmax_bwd/N8300/d{d}/lists"] = P(case_softmax_bwd, 8300, d, "lists")
        cases[f"bce_bwd/N8300/d{d}/lists"] = P(case_bce_bwd, 8300, d, "lists")
    for d in (64, 256):
        for kind in ("hub4", "hub2"):
            cases[f"softmax_bwd/N777_B300/d{d}/{kind}"] = P(case_softmax_bwd, N0, d, kind, B=HUB_B, rows_q=HUB_ROWS_Q)
            cases[f"bce_bwd/N777_B300/d{d}/{kind}"] = P(case_bce_bwd, N0, d, kind, B=HUB_B, rows_q=HUB_ROWS_Q)
    cases["softmax_bwd/N777/d20/plain"] = P(case_softmax_bwd, N0, 20, "plain")
    cases["bce_bwd/N777/d20/plain"] = P(case_bce_bwd, N0, 20, "plain")
    cases["bce_bwd/N777/d128/lists/smooth"] = P(case_bce_bwd, N0, 128, "lists", smoothing=0.1)
    cases["softmax_bwd/N777/d20/bad_list"] = P(case_softmax_bwd, N0, 20, "bad_list")
    cases["bce_bwd/N777/d20/bad_list"] = P(case_bce_bwd, N0, 20, "bad_list")
    return cases


CASES = build_cases()


@functools.lru_cache(maxsize=None)
def recorded():
    return load_fixture(FIXTURE)


def only_row(mask):
    """Whether the [B] mask holds at query BAD and nowhere else."""
    return bool(mask[BAD]) and int(mask.sum()) == 1


def check(name, out):
    """What a case's outputs must show before they are hashed: the out-of-range query's row, and no other, is marked."""
    op, bad = name.split("/")[0], name.rsplit("/", 1)[1].startswith("bad_")
    if op == "rank":
        neg = (out[0] == -1) & (out[1] == -1)
        assert only_row(neg) if bad else not bool(neg.any())
        assert bool(((out[0] >= 0) & (out[1] >= 0))[~neg].all())
    elif op == "topk":
        scores, ids = out
        nan = torch.isnan(scores).all(dim=1) & (ids == -1).all(dim=1)
        assert only_row(nan) if bad else not bool(torch.isnan(scores).any())
        if "/N5/" in name:
            assert bool((ids[:, :5] >= 0).all()) and bool((ids[:, 5:] == -1).all()) and bool(torch.isneginf(scores[:, 5:]).all())
        if name.endswith("cover"):
            assert sorted(ids[COVER, :3].tolist()) == list(UNCOVERED) and bool((ids[COVER, 3:] == -1).all())
    elif op.endswith("_fwd"):
        nan = torch.stack([torch.isnan(t) for t in out]).all(dim=0)
        assert only_row(nan) if bad else all(bool(torch.isfinite(t).all()) for t in out)
        assert all(bool(torch.isfinite(t[~nan]).all()) for t in out)
    else:
        dq, dc = out
        assert bool(torch.isfinite(dq).all()) and bool(torch.isfinite(dc).all())
        zero = (dq == 0).all(dim=1)
        assert only_row(zero) if bad else not bool(zero.any())


def test_the_fixture_names_exactly_these_cases():
    assert sorted(recorded()) == sorted(CASES)


@pytest.mark.parametrize("name", sorted(CASES))
def test_output_bytes_are_the_recorded_ones(name):
    out = CASES[name]()
    check(name, out)
    got = digest(out)
    print(f"{name}: {got}")
    assert got == recorded()[name]


if __name__ == "__main__":
    record_main(FIXTURE, CASES)
