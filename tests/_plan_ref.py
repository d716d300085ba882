"""The graph plan (include/ghf.h: ghf_plan_build) restated in numpy, table for table.

Not collected by pytest and free of the GPU (test_plan_host.py and test_plan_gpu.py import it).  Written from the rules the
header and csrc/plan.hip's comments state, as plain array code — an independent statement of them, not a port of the kernels:

  key        (dst // bn) * (R * bn) + rel * bn + dst % bn as uint32; an edge with a node or relation id out of range is
             dropped: key 2^32 - 1 (sorts last), source 0.
  sort       stable: equal keys keep the caller's order.
  run head   (bn > 1, kept edges only) bits 28..31 of sorted_src: with t = (position in the (block, relation) group) % 16, the
             first row of the edge's run of equal destinations inside its 16-row tile.
  seg_off    lower bounds of s * seg_div (seg_div = bn, or R for CSR plans), s = 0..nseg; seg_off[nseg] = kept edges.
  chunks     every group cut from its start into chunks of <= cr edges; cross = an equal-destination run continues over a
             16-row tile boundary inside the chunk.
  items      a block is one item, or several for one of two reasons: more than sc chunks (a hub: ceil(chunks / sc) items), or
             a place in the last, partly filled round of workgroups — with NB blocks on `cus` compute units and
             rem = NB % cus, when NB > cus and 0 < 2 * rem <= cus the blocks NB - rem .. NB - 1 are cut into
             min(8, cus // rem, chunks // 8) items where that is more than the hub rule gives.  k items cut a block's n chunks
             evenly: per = ceil(n / k), item j = chunks [j * per, min((j + 1) * per, n)).  Items of blocks with several take
             the scratch slots 0, 1, ... in item order; the only item of a block has slot -1.
"""

from __future__ import annotations

import numpy as np

KEY_INVALID = 0xFFFFFFFF
SRC_BITS = 28
SRC_MASK = (1 << SRC_BITS) - 1
TAIL_MAX_ITEMS = 8           # a last-round block becomes at most this many items ...
TAIL_MIN_CHUNKS = 8          # ... of at least this many chunks each


def _tail_split(NB: int, cus: int):
    """(first block of the last round, items each of its blocks may become): (NB, 1) when no block is cut."""
    if cus <= 0 or NB <= cus:
        return NB, 1
    rem = NB % cus
    if rem == 0 or 2 * rem > cus:
        return NB, 1
    return NB - rem, min(TAIL_MAX_ITEMS, cus // rem)


def _items_per_block(chunks_per_block: np.ndarray, sc: int, cus: int) -> np.ndarray:
    n = np.asarray(chunks_per_block, dtype=np.int64)
    NB = n.size
    k = np.where(n > sc, -(-n // sc), 1)
    tail0, tail_items = _tail_split(NB, cus)
    if tail_items > 1:
        last = np.arange(NB) >= tail0
        k = np.where(last, np.maximum(k, np.minimum(tail_items, n // TAIL_MIN_CHUNKS)), k)
    return k


def plan_ref(edge_index, rel, N: int, R: int, bn: int, cr: int, sc: int, cus: int) -> dict:
    """Every output array of ghf_plan_build for these inputs (the tables cut to the entries the build defines):
    sorted_key uint32 [E], sorted_src int32 [E], seg_off int32 [nseg + 1], indeg int32 [N], status int32 [3] and, for block
    plans, chunk_tab int32 [2 * chunks], blk_chunk_off int32 [NB + 1], item_tab int32 [4 * items], blk_item_off int32 [NB + 1]
    (None for CSR plans); plus n_valid, tail0, tail_items and items_per_block for the tests' own assertions."""
    src = np.asarray(edge_index[0], dtype=np.int64)
    dst = np.asarray(edge_index[1], dtype=np.int64)
    rel = np.asarray(rel, dtype=np.int64)
    E = rel.size
    NB = -(-N // bn)
    assert NB * bn * R < KEY_INVALID, "the key space does not fit 32 bits"
    ok_n = (src >= 0) & (src < N) & (dst >= 0) & (dst < N)
    ok_r = (rel >= 0) & (rel < R)
    ok = ok_n & ok_r
    status = np.zeros(3, dtype=np.int32)
    status[0] = (1 if (~ok_n).any() else 0) | (2 if (~ok_r).any() else 0)
    key = np.full(E, KEY_INVALID, dtype=np.uint64)
    d, r, s = dst[ok], rel[ok], src[ok]
    key[ok] = ((d // bn) * (R * bn) + r * bn + d % bn).astype(np.uint64)
    order = np.argsort(key, kind="stable")
    skey = key[order]
    ssrc = np.where(ok, src, 0)[order]
    n_valid = int(ok.sum())
    indeg = np.bincount(d, minlength=N).astype(np.int32)

    nseg, seg_div = (N, R) if bn == 1 else (NB * R, bn)
    targets = np.minimum(np.arange(nseg + 1, dtype=np.uint64) * np.uint64(seg_div), np.uint64(KEY_INVALID))
    seg_off = np.searchsorted(skey, targets, side="left").astype(np.int64)
    out = dict(sorted_key=skey.astype(np.uint32), seg_off=seg_off.astype(np.int32), indeg=indeg, status=status, n_valid=n_valid,
               chunk_tab=None, blk_chunk_off=None, item_tab=None, blk_item_off=None, tail0=NB, tail_items=1, items_per_block=None)
    if bn == 1:
        out["sorted_src"] = ssrc.astype(np.uint32).view(np.int32)
        return out

    # run heads of the kept edges
    v = skey[:n_valid]
    pos = np.arange(n_valid, dtype=np.int64)
    first = np.ones(n_valid, dtype=bool)
    first[1:] = v[1:] != v[:-1]
    run0 = np.maximum.accumulate(np.where(first, pos, 0))                 # first position of the run of equal keys
    tile0 = pos - ((pos - seg_off[(v // np.uint64(bn)).astype(np.int64)]) & 15)
    head = np.maximum(run0, tile0) - tile0
    packed = ssrc.astype(np.uint32)
    packed[:n_valid] = (packed[:n_valid] & np.uint32(SRC_MASK)) | (head.astype(np.uint32) << np.uint32(SRC_BITS))
    out["sorted_src"] = packed.view(np.int32)

    # chunk table
    size = np.diff(seg_off)
    cnt = -(-size // cr)
    per_block = cnt.reshape(NB, R).sum(axis=1)
    blk_chunk_off = np.concatenate([[0], np.cumsum(per_block)])
    tab = []
    for g in np.nonzero(size)[0].tolist():
        e0, n, r_g = int(seg_off[g]), int(size[g]), g % R
        for j in range(0, n, cr):
            rows = min(cr, n - j)
            a = e0 + j
            cross = any(skey[a + t - 1] == skey[a + t] for t in range(16, rows, 16))
            tab.append((a, (r_g << 8) | (int(cross) << 7) | rows))
    out["chunk_tab"] = np.array(tab, dtype=np.int64).reshape(-1, 2).astype(np.int32).reshape(-1)
    out["blk_chunk_off"] = blk_chunk_off.astype(np.int32)

    # work items
    k = _items_per_block(per_block, sc, cus)
    out["tail0"], out["tail_items"] = _tail_split(NB, cus)
    out["items_per_block"] = k
    items, slot = [], 0
    for b in range(NB):
        c0, n, kb = int(blk_chunk_off[b]), int(per_block[b]), int(k[b])
        per = -(-n // kb)
        for j in range(kb):
            z = c0 + min((j + 1) * per, n)
            items.append((b, min(c0 + j * per, z), z, slot + j if kb > 1 else -1))
        slot += kb if kb > 1 else 0
    out["item_tab"] = np.array(items, dtype=np.int32).reshape(-1)
    out["blk_item_off"] = np.concatenate([[0], np.cumsum(k)]).astype(np.int32)
    status[1], status[2] = len(items), slot
    return out
