"""The plan builder's numpy restatement (_plan_ref.py) and the crafted inputs of test_plan_gpu.py (_plan_cases.py), checked on
the host: plan_ref agrees with the cut _edge_graphs.realised states for the edge-case catalogue, its work items tile every
block, every case built for test_plan_gpu.py is what its name promises at the compute-unit counts of four cards, and a plan
never outgrows the capacities ghf_plan_max_chunks / ghf_plan_max_items hand the callers (loading the library needs no GPU)."""

import functools

import numpy as np
import pytest

import _edge_graphs as G
import _plan_cases as P
from _plan_ref import plan_ref
from graph_hypernetwork_forge_amd import _native

GEOMETRIES = {g[0]: g for g in G.geometries() if g[2] > 1}            # key -> (key, d, bn, cr, sc, npw), block plans
NO_LAST_ROUND = 10 ** 6                                               # more compute units than any case has blocks
KEYS_CUS = [(k, c) for k in GEOMETRIES for c in P.HOST_CUS]
IDS = [f"{k}-cus{c}" for k, c in KEYS_CUS]


@functools.lru_cache(maxsize=None)
def _small(key):
    """[(case, plan_ref of it)] of the cases of at most four blocks (no last round on any card); P.check proves each."""
    _, d, bn, cr, sc, npw = GEOMETRIES[key]
    out = []
    for case in P.ordinary_cases(bn, cr) + P.dropped_cases(bn, cr) + P.high_key_cases(bn):
        assert -(-case.N // bn) <= 4
        ref = P.check(case, bn, cr, sc, min(P.HOST_CUS))
        ref["seg_off"] = None                                          # (millions of groups in the high-key case: not kept)
        out.append((case, ref))
    return out


@functools.lru_cache(maxsize=None)
def _rounds(key, cus):
    _, d, bn, cr, sc, npw = GEOMETRIES[key]
    return [(case, P.check(case, bn, cr, sc, cus)) for case in P.last_round_cases(bn, cr, sc, cus) + P.value_cases(bn, cr, sc, cus)]


@pytest.mark.parametrize("key", list(GEOMETRIES))
def test_plan_ref_agrees_with_the_edge_catalogue(key):
    _, d, bn, cr, sc, npw = GEOMETRIES[key]
    for case in G.edge_cases(bn, cr, sc, npw, d):
        res = G.realised(case, bn, cr, sc, npw)
        ref = plan_ref(case.edge_index, case.rel, case.N, case.R, bn, cr, sc, NO_LAST_ROUND)
        assert ref["tail_items"] == 1 and ref["status"][0] == 0
        assert np.array_equal(ref["blk_chunk_off"], res["blk_chunk_off"]), case.name
        assert np.array_equal(ref["blk_item_off"], res["item_off"]), case.name
        assert np.array_equal(ref["chunk_tab"].reshape(-1, 2)[:, 1] & 127, res["chunk_lens"]), case.name
        assert np.array_equal(ref["chunk_tab"].reshape(-1, 2)[:, 0], [c[2] for c in res["chunks"]]), case.name
        blk, srel, loc, ssrc = res["sorted"]                           # (realised orders by block, relation and row only)
        assert np.array_equal(ref["sorted_key"].astype(np.int64), blk * (case.R * bn) + srel * bn + loc), case.name
        assert np.array_equal(ref["indeg"], res["indeg"]), case.name


@pytest.mark.parametrize("key,cus", KEYS_CUS, ids=IDS)
def test_every_case_is_what_its_name_promises(key, cus):
    """P.check asserts each case's conditions from plan_ref alone ("the last block has 63 chunks and becomes 7 items")."""
    _, d, bn, cr, sc, npw = GEOMETRIES[key]
    cases = [c for c, _ in _small(key) + _rounds(key, cus)]
    assert len({c.name for c in cases}) == len(cases) and all(c.expects for c in cases)
    assert all(c.rel.size <= 40_000 for c in cases)
    names = {c.name for c in cases}
    for n, k in ((15, 1), (16, 2), (63, 7), (64, 8), (65, 8)):        # the counts the last round's rule gives, spelt out
        (case,) = [c for c in cases if c.name == f"round_nb_c_plus_1_last_block_{n}_chunks"]
        assert ("block_items", cus, k) in case.expects or sc < n
    for stem in ("powerlaw_", "fewer_edges", "groups_around", "run_", "dropped_", "high_keys_", "round_", "values_"):
        assert any(n.startswith(stem) for n in names), stem
    if key == list(GEOMETRIES)[0]:
        for case in P.ordinary_cases(1, 0) + P.dropped_cases(1, 0) + P.high_key_cases(1):       # the CSR plan's cases
            ref = P.check(case, 1, 0, 0, cus)
            assert ref["chunk_tab"] is None and ref["item_tab"] is None and ref["seg_off"].shape == (case.N + 1,)
            assert ref["seg_off"][-1] == ref["n_valid"] == ref["indeg"].sum()


@pytest.mark.parametrize("key,cus", KEYS_CUS, ids=IDS)
def test_plan_ref_items_tile_every_block(key, cus):
    bn = GEOMETRIES[key][2]
    for case, ref in _small(key) + _rounds(key, cus):
        nb = -(-case.N // bn)
        boff, ioff = ref["blk_chunk_off"].astype(np.int64), ref["blk_item_off"].astype(np.int64)
        items = ref["item_tab"].reshape(-1, 4)
        assert boff.shape == ioff.shape == (nb + 1,) and boff[0] == ioff[0] == 0, case.name
        assert ioff[-1] == len(items) == ref["status"][1] and boff[-1] == len(ref["chunk_tab"]) // 2, case.name
        assert np.array_equal(np.diff(ioff), ref["items_per_block"]), case.name
        assert np.array_equal(items[:, 0], np.repeat(np.arange(nb), np.diff(ioff))), f"{case.name}: items are listed block after block"
        first, last = ioff[:-1], ioff[1:] - 1
        assert np.array_equal(items[first, 1], boff[:-1]) and np.array_equal(items[last, 2], boff[1:]), f"{case.name}: a block's items span its chunks"
        inner = np.ones(len(items), dtype=bool)
        inner[first] = False
        assert np.array_equal(items[inner, 1], items[np.nonzero(inner)[0] - 1, 2]), f"{case.name}: the items of a block follow one another"
        several = np.repeat(np.diff(ioff) > 1, np.diff(ioff))
        assert (items[several, 2] > items[several, 1]).all(), f"{case.name}: an empty item in a block of several"
        assert (items[~several, 3] == -1).all(), case.name
        assert np.array_equal(items[several, 3], np.arange(several.sum())) and several.sum() == ref["status"][2], f"{case.name}: slots in item order"
        tab = ref["chunk_tab"].reshape(-1, 2)
        rows = tab[:, 1] & 127
        assert np.array_equal(tab[:, 0], np.concatenate([[0], np.cumsum(rows)[:-1]])) and rows.sum() == ref["n_valid"], f"{case.name}: chunks tile the kept edges"


@pytest.mark.parametrize("key,cus", KEYS_CUS, ids=IDS)
def test_plans_stay_inside_their_capacity(key, cus):
    """status[1] items and blk_chunk_off[-1] chunks are what the builder writes into item_tab and chunk_tab, which the callers
    size by ghf_plan_max_items and ghf_plan_max_chunks."""
    _, d, bn, cr, sc, npw = GEOMETRIES[key]
    lib = _native.load()
    for case, ref in _small(key) + _rounds(key, cus):
        E = case.rel.size
        max_items = lib.ghf_plan_max_items(case.N, E, case.R, bn, cr, sc)
        max_chunks = lib.ghf_plan_max_chunks(case.N, E, case.R, bn, cr)
        assert ref["status"][1] <= max_items, f"{case.name}: {ref['status'][1]} items, room for {max_items}"
        assert ref["blk_chunk_off"][-1] <= max_chunks, f"{case.name}: {ref['blk_chunk_off'][-1]} chunks, room for {max_chunks}"
