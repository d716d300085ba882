"""Crafted inputs for the plan builder (csrc/plan.hip), built from the geometry they run at — (block_nodes, chunk_rows,
split_chunks) — and from the compute-unit count that decides the last round's split, so that a retuned kernel or another card
gets the cases of its own geometry.  `check` proves from tests/_plan_ref.py alone that a case is what its name promises.

Not collected by pytest and free of the GPU (test_plan_host.py and test_plan_gpu.py import it)."""

from __future__ import annotations

from typing import List, NamedTuple

import numpy as np

from _plan_ref import plan_ref
from graph_hypernetwork_forge_amd import synth

SEED = 9200
CSR_NOMINAL = (256, 16)          # CSR plans know no block or chunk: the sizes their ordinary graphs are built around
HOST_CUS = (64, 104, 256, 304)   # compute-unit counts the host tests build the last-round cases for


class PCase(NamedTuple):
    name: str
    N: int
    R: int
    edge_index: np.ndarray       # [2, E] int64
    rel: np.ndarray              # [E] int64
    expects: tuple               # conditions `check` asserts, (tag, *args) each


class _B:
    def __init__(self, name: str, N: int, R: int) -> None:
        self.name, self.N, self.R = name, N, R
        self.s, self.d, self.r = [], [], []

    def add(self, dst, rel, src=None) -> None:
        dst = np.atleast_1d(np.asarray(dst, dtype=np.int64))
        n = dst.size
        if src is None:
            src = synth.randint(SEED, f"{self.name}/src{len(self.s)}", n, self.N)
        self.s.append(np.broadcast_to(np.asarray(src, dtype=np.int64), (n,)))
        self.d.append(dst)
        self.r.append(np.broadcast_to(np.asarray(rel, dtype=np.int64), (n,)))

    def case(self, *expects, shuffle: bool = True) -> PCase:
        s, d, r = (np.concatenate(a) for a in (self.s, self.d, self.r))
        if shuffle:
            o = np.argsort(synth.raw_u64(SEED, self.name + "/order", s.size), kind="stable")
            s, d, r = s[o], d[o], r[o]
        return PCase(self.name, self.N, self.R, np.stack([s, d]), r.copy(), tuple(expects))


# ---- ordinary graphs (every geometry; CSR plans at CSR_NOMINAL) ---------------------------------------------------------

def ordinary_cases(bn: int, cr: int) -> List[PCase]:
    if bn == 1:
        bn, cr = CSR_NOMINAL
    out = []
    # a power-law graph whose (destination, relation) pairs repeat, every repeat from another source, the sources of a pair
    # neither ascending nor descending in the caller's order: the sorted order among equal keys shows
    N, R, E = 3 * bn + 1, 5, 4000
    ei, rel = synth.make_graph_arrays(N, E, R, seed=SEED, kind="powerlaw")
    pair = ei[1] * R + rel
    o = np.argsort(pair, kind="stable")
    first = np.concatenate([[True], pair[o][1:] != pair[o][:-1]])
    start = np.maximum.accumulate(np.where(first, np.arange(E), 0))
    nth = np.empty(E, dtype=np.int64)
    nth[o] = np.arange(E) - start                                    # an edge's place among the edges of its pair, in input order
    assert nth.max() < N and N % 7919 != 0
    src = (synth.randint(SEED, "powerlaw/base", N * R, N)[pair] + 7919 * nth) % N
    out.append(PCase("powerlaw_repeated_pairs", N, R, np.stack([src, ei[1]]), rel, (("repeats", 100), ("distinct_sources",))))

    g = _B("fewer_edges_than_groups", 2 * bn + 1, 7)
    g.add([0, bn - 1, bn, 2 * bn, 2 * bn], [6, 0, 3, 0, 5])
    out.append(g.case(("edges_below_nseg",)))

    sizes = (cr - 1, cr, cr + 1, 2 * cr)
    g = _B("groups_around_chunk_rows", 3 * bn, len(sizes) + 1)
    for i, n in enumerate(sizes):
        g.add((i % 3) * bn + (7 * i + np.arange(n)) % bn, i)
    out.append(g.case(*[("group", n) for n in sizes]))

    g = _B("run_across_tile_boundary", 2 * bn, 3)
    g.add(bn + np.concatenate([np.arange(15), np.full(2, 15), np.arange(16, 21)]), 1)      # rows 15 and 16 of the group
    out.append(g.case(("cross", 1)))
    g = _B("run_one_row_before_tile_boundary", 2 * bn, 3)
    g.add(bn + np.concatenate([np.arange(14), np.full(2, 14), np.arange(15, 21)]), 1)      # rows 14 and 15
    out.append(g.case(("cross", 0)))
    return out


# ---- dropped edges -----------------------------------------------------------------------------------------------------

def dropped_cases(bn: int, cr: int) -> List[PCase]:
    if bn == 1:
        bn, cr = CSR_NOMINAL
    N, R = 2 * bn + 1, 4
    out = []

    def valid(g, n):
        g.add(synth.randint(SEED, g.name + "/dst", n, N), synth.randint(SEED, g.name + "/rel", n, R))

    g = _B("dropped_nodes_and_relations", N, R)
    valid(g, 60)
    g.add([3, -1, 5, 6, N, -1], [0, 1, R, -1, 2, R], [N, 4, 5, 6, -1, N])
    out.append(g.case(("status", 3), ("dropped", 6)))
    g = _B("dropped_nodes_only", N, R)
    valid(g, 40)
    g.add([3, -1, N], [0, 1, 3], [N, 4, 2])
    out.append(g.case(("status", 1), ("dropped", 3)))
    g = _B("dropped_relations_only", N, R)
    valid(g, 40)
    g.add([3, 7], [R, -1], [1, 4])
    out.append(g.case(("status", 2), ("dropped", 2)))
    g = _B("dropped_outnumber_valid", N, R)
    valid(g, 5)
    g.add(np.arange(20) % N, np.where(np.arange(20) % 2, R, 0), np.where(np.arange(20) % 2, 1, N))
    out.append(g.case(("status", 3), ("dropped", 20), ("dropped_majority",)))
    g = _B("dropped_after_a_full_last_chunk", N, R)
    valid(g, 30)
    g.s, g.d, g.r = [a.copy() for a in g.s], [a.copy() for a in g.d], [a.copy() for a in g.r]
    g.r[0][(g.d[0] >= 2 * bn) & (g.r[0] == R - 1)] = 0                  # the last group of the last block: cr edges exactly
    g.add(np.full(cr, N - 1), R - 1)
    g.add([-1, 2, N], [0, R, 0], [0, 0, 0])
    out.append(g.case(("status", 3), ("dropped", 3), ("last_group", cr)))
    return out


# ---- keys at and above 2^31 --------------------------------------------------------------------------------------------

def high_key_cases(bn: int) -> List[PCase]:
    out = []
    if bn == 1:
        shapes = [(2, (1 << 31) - 1), (6, ((1 << 32) - 2) // 6)]         # N * R = 2^32 - 2: the largest key space there is
    else:
        # R = 2^23 - 1, the most a chunk_tab word carries — or, where the block is too wide for 2 * bn * R to fit the keys, the most that fits
        shapes = [(2 * bn, min((1 << 23) - 1, ((1 << 32) - 2) // (2 * bn)))]
    for N, R in shapes:
        g = _B(f"high_keys_n{N}_r{R}", N, R)
        n = 1000
        g.add(synth.randint(SEED, g.name + "/lo", n, N), synth.randint(SEED, g.name + "/lor", n, 8))            # the lowest relations
        g.add(synth.randint(SEED, g.name + "/hi", n, N), R - 1 - synth.randint(SEED, g.name + "/hir", n, 8))    # the highest
        lo_last = N - (bn if bn > 1 else 1)
        g.add(lo_last + synth.randint(SEED, g.name + "/last", n, N - lo_last), synth.randint(SEED, g.name + "/lastr", n, R))  # the last block
        g.add([0, N - 1, N - 1], [0, R - 1, R - 1], [N - 1, 0, 1])                                              # the two ends of the key range
        out.append(g.case(("key_min", 0), ("key_max", N * R - 1), ("keys_above", 1 << 31, 300)))
    return out


# ---- the last round of workgroups --------------------------------------------------------------------------------------

def _round_case(name: str, bn: int, NB: int, chunks: dict, *expects) -> PCase:
    """NB blocks; block b has chunks[b] chunks (one relation with one edge = one chunk), every other block one."""
    g = _B(name, NB * bn, max(list(chunks.values()) + [1]) + 1)
    for b in range(NB):
        k = chunks.get(b, 1)
        g.add(b * bn + (11 * np.arange(k) + b) % bn, np.arange(k))
    return g.case(("blocks", NB), *[("block_chunks", b, k) for b, k in chunks.items()], *expects)


def last_round_cases(bn: int, cr: int, sc: int, c: int) -> List[PCase]:
    """Block plans on a device of c compute units.  The item counts expected here are the header's rule worked by hand."""
    assert bn > 1 and c >= 32, "the cases need c // 8 >= 4"
    hub = lambda n: -(-n // sc) if n > sc else 1                                          # noqa: E731
    out = [_round_case("round_nb_eq_c", bn, c, {c - 1: 64}, ("tail", c, 1), ("block_items", c - 1, hub(64)))]
    for n, k in ((15, 1), (16, 2), (63, 7), (64, 8), (65, 8)):
        out.append(_round_case(f"round_nb_c_plus_1_last_block_{n}_chunks", bn, c + 1, {c: n}, ("tail", c, 8),
                               ("block_items", c, max(k, hub(n))), ("block_items", 0, 1)))
    n = sc + 1
    out.append(_round_case("round_nb_c_plus_1_last_block_sc_plus_1_chunks", bn, c + 1, {c: n}, ("tail", c, 8),
                           ("block_items", c, max(2, min(8, n // 8)))))
    n = 8 * sc + 1                                                                        # ceil(n / sc) = 9 > 8: the hub rule wins
    out.append(_round_case("round_nb_c_plus_1_last_block_is_a_hub", bn, c + 1, {c: n}, ("tail", c, 8), ("block_items", c, 9)))
    e = c // 8
    out.append(_round_case("round_remainder_c_over_8", bn, c + e, {c: 100, c + 1: 64, c + e - 1: 16, c - 1: 100},
                           ("tail", c, min(8, c // e)), ("block_items", c, max(min(8, c // e), hub(100))),
                           ("block_items", c + e - 1, 2), ("block_items", c - 1, hub(100))))
    cap = c // (e + 1)
    out.append(_round_case("round_remainder_c_over_8_plus_1", bn, c + e + 1, {c: 100, c + e: 64},
                           ("tail", c, cap), ("block_items", c, max(min(cap, 12), hub(100))), ("block_items", c + e, max(min(cap, 8), hub(64)))))
    h = c // 2
    out.append(_round_case("round_remainder_half", bn, c + h, {c: 100, c + h - 1: 15, 3: 100},
                           ("tail", c, 2), ("block_items", c, max(2, hub(100))), ("block_items", c + h - 1, 1), ("block_items", 3, hub(100))))
    out.append(_round_case("round_remainder_half_plus_1", bn, c + h + 1, {c: 100, c + h: 100},
                           ("tail", c + h + 1, 1), ("block_items", c, hub(100)), ("block_items", c + h, hub(100))))
    out.append(_round_case("round_nb_2c", bn, 2 * c, {2 * c - 1: 100, c: 100},
                           ("tail", 2 * c, 1), ("block_items", 2 * c - 1, hub(100)), ("block_items", c, hub(100))))
    out.append(_round_case("round_first_round_block_64_chunks", bn, c + 1, {0: 64, c: 64},
                           ("tail", c, 8), ("block_items", 0, hub(64)), ("block_items", c, max(8, hub(64)))))
    return out


def value_cases(bn: int, cr: int, sc: int, c: int) -> List[PCase]:
    """The two graphs a layer is run on: NB = c + 1 and NB = c + c // 8, every last-round block with 65 or more chunks of real
    edges (1 .. cr edges per chunk), relation 8 of each a group of cr + 5 edges whose two chunks lie either side of an item
    boundary.  Every second source of a group (the first one always) lies in the last round's rows, so the reversed graph's
    last-round blocks are split too; block 1 is an ordinary block with a few dozen edges."""
    assert bn > 1 and c >= 32
    out = []
    for name, NB in (("values_nb_c_plus_1", c + 1), ("values_remainder_c_over_8", c + c // 8)):
        N, R = NB * bn, 68
        g = _B(name, N, R)
        for b in range(c):
            g.add([b * bn + (5 * b) % bn], 0)
        g.add(bn + synth.randint(SEED, name + "/ord", 40, bn), synth.randint(SEED, name + "/ordr", 40, 3))
        exp = [("blocks", NB), ("tail", c, 8), ("rev_split",)]
        for b in range(c, NB):
            nrel = 64 + (b - c) % 3
            sizes = [1 + (5 * r + b) % 12 for r in range(nrel)]
            sizes[8], sizes[20], sizes[30] = cr + 5, cr, 33
            for r, n in enumerate(sizes):
                src = np.where(np.arange(n) % 2 == 0, c * bn + synth.randint(SEED, f"{name}/in{b}.{r}", n, N - c * bn),
                               synth.randint(SEED, f"{name}/out{b}.{r}", n, N))
                g.add(b * bn + synth.randint(SEED, f"{name}/dst{b}.{r}", n, bn), r, src)
            exp += [("block_chunks", b, nrel + 1), ("block_items", b, 8), ("item_boundary_inside_relation", b)]
        out.append(g.case(*exp))
    return out


# ---- the proof that a case is what it claims ---------------------------------------------------------------------------

def check(case: PCase, bn: int, cr: int, sc: int, cus: int) -> dict:
    ref = plan_ref(case.edge_index, case.rel, case.N, case.R, bn, cr, sc, cus)
    src, dst, rel, N, R = case.edge_index[0], case.edge_index[1], case.rel, case.N, case.R
    E, nv = rel.size, ref["n_valid"]
    key = ref["sorted_key"].astype(np.int64)
    if bn > 1:
        per_block = np.diff(ref["blk_chunk_off"])
        tab = ref["chunk_tab"].reshape(-1, 2)
        items = ref["item_tab"].reshape(-1, 4)
    for exp in case.expects:
        tag, a = exp[0], exp[1:]
        if tag == "repeats":
            ok = E - np.unique(dst * R + rel).size >= a[0]
        elif tag == "distinct_sources":
            ok = np.unique(np.stack([src, dst, rel]), axis=1).shape[1] == E
            pair, o = dst * R + rel, np.argsort(dst * R + rel, kind="stable")
            same = pair[o][1:] == pair[o][:-1]
            step = np.sign(np.diff(src[o]))[same]
            ok = ok and (step > 0).sum() > 50 and (step < 0).sum() > 50          # neither order of the sources is the input order
        elif tag == "edges_below_nseg":
            ok = E < ref["seg_off"].size - 1
        elif tag == "group":
            ok = bn == 1 or a[0] in np.diff(ref["seg_off"])
        elif tag == "cross":
            ok = bn == 1 or (((tab[:, 1] >> 7) & 1) == a[0]).all()
        elif tag == "status":
            ok = ref["status"][0] == a[0]
        elif tag == "dropped":
            ok = E - nv == a[0] and (key[nv:] == 0xFFFFFFFF).all() and ref["seg_off"][-1] == nv
        elif tag == "dropped_majority":
            ok = E - nv > nv
        elif tag == "last_group":
            ok = np.diff(ref["seg_off"])[-1] == a[0] or bn == 1
            ok = ok and (bn == 1 or (tab[-1, 0] + (tab[-1, 1] & 127) == nv and (tab[-1, 1] & 127) == cr))
        elif tag == "key_min":
            ok = key[0] == a[0]
        elif tag == "key_max":
            ok = key[nv - 1] == a[0] and a[0] >= 1 << 31
        elif tag == "keys_above":
            ok = (key[:nv] >= a[0]).sum() >= a[1] and (key[:nv] < a[0]).sum() >= a[1]
        elif tag == "blocks":
            ok = -(-N // bn) == a[0]
        elif tag == "block_chunks":
            ok = per_block[a[0]] == a[1]
        elif tag == "tail":
            ok = (ref["tail0"], ref["tail_items"]) == (a[0], a[1])
        elif tag == "block_items":
            ok = ref["items_per_block"][a[0]] == a[1] == ref["blk_item_off"][a[0] + 1] - ref["blk_item_off"][a[0]]
        elif tag == "item_boundary_inside_relation":
            mine = items[ref["blk_item_off"][a[0]]:ref["blk_item_off"][a[0] + 1]]
            ok = any(tab[m[2] - 1, 1] >> 8 == tab[m[2], 1] >> 8 for m in mine[:-1])
        elif tag == "rev_split":
            rev = plan_ref(case.edge_index[::-1], case.rel, N, R, bn, cr, sc, cus)
            ok = rev["tail_items"] > 1 and (rev["items_per_block"][rev["tail0"]:] > 1).any() and rev["status"][2] > 0
        else:
            raise KeyError(tag)
        assert ok, f"{case.name}: condition {exp} is not realised at bn={bn} cr={cr} sc={sc} cus={cus}"
    return ref
