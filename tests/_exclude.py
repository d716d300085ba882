"""A numpy restatement of the k-hop subgraph without given edges (include/ghf.h: ghf_subgraph_*_excl), built on _sampling.py:
the key encoding, the excluded-edge mask, and the exact and the sampled extraction with that mask.  Shared by
test_exclude_host.py and test_exclude_gpu.py; nothing here touches the library."""

import numpy as np

import _sampling as S


def keys(src, dst, rel=None, R=None):
    """ghf.h's key encoding, sorted ascending: s << 32 | t, or (typed: rel given) s << 32 | (t * R + r).  uint64."""
    s = np.asarray(src, dtype=np.uint64)
    low = np.asarray(dst, dtype=np.uint64)
    if rel is not None:
        low = low * np.uint64(R) + np.asarray(rel, dtype=np.uint64)
        assert low.size == 0 or int(low.max()) < 1 << 32
    return np.sort((s << np.uint64(32)) | low)


def excluded(src, dst, rel, R, ex_src, ex_dst, ex_rel=None):
    """The mask over the edges (src, dst, rel): in the untyped list X = {(s, t)} or the typed list X = {(s, t, r)}.  Written
    with Python sets of tuples, not with the keys: every parallel edge that matches, direction kept, no match no effect."""
    if ex_rel is None:
        X = set(zip(np.asarray(ex_src).tolist(), np.asarray(ex_dst).tolist()))
        return np.fromiter(((s, t) in X for s, t in zip(src.tolist(), dst.tolist())), dtype=bool, count=src.size)
    X = set(zip(np.asarray(ex_src).tolist(), np.asarray(ex_dst).tolist(), np.asarray(ex_rel).tolist()))
    return np.fromiter(((s, t, r) in X for s, t, r in zip(src.tolist(), dst.tolist(), rel.tolist())), dtype=bool,
                       count=src.size)


def _finish(src, dst, rel, N, k, dist, keep):
    inside = np.nonzero(dist <= k)[0]
    node_list = inside[np.lexsort((inside, dist[inside]))]
    new_id = np.full(N, -1, dtype=np.int64)
    new_id[node_list] = np.arange(node_list.size)
    m = [int((dist <= j).sum()) for j in range(k + 1)]
    return dist, node_list, new_id, m, np.stack([new_id[src[keep]], new_id[dst[keep]]]), rel[keep]


def np_subgraph_excl(src, dst, rel, N, seeds, k, dead):
    """_sampling.np_subgraph over edges in the plan's order, the edges of the mask `dead` excluded: no hop walks them and
    they are not emitted."""
    live = ~dead
    dist = np.full(N, k + 1, dtype=np.int64)
    dist[np.asarray(seeds, dtype=np.int64) % N] = 0
    for j in range(k):
        s = src[live & (dist[dst] == j)]
        dist[s[dist[s] > k]] = j + 1
    return _finish(src, dst, rel, N, k, dist, live & (dist[dst] <= k - 1))


def np_sample_keep_excl(src, dst, N, seeds, fanout, seed, dead):
    """_sampling.np_sample_keep with the mask: hop j's candidates are the in-edges of distance-j nodes that are not excluded;
    the priorities are those of the FULL plan's positions (position = index into the arrays given, excluded edges counted)."""
    k = len(fanout)
    live = ~dead
    dist = np.full(N, k + 1, dtype=np.int64)
    dist[np.asarray(seeds, dtype=np.int64) % N] = 0
    keep = np.zeros(src.size, dtype=bool)
    prio = S.priority(seed, np.arange(src.size))
    for j, f in enumerate(fanout):
        cand = np.nonzero(live & (dist[dst] == j))[0]
        sel = cand if f == -1 else S.select(dst, cand, prio, f)
        keep[sel] = True
        s = src[sel]
        dist[s[dist[s] > k]] = j + 1
    return dist, keep


def np_subgraph_sample_excl(src, dst, rel, N, seeds, fanout, seed, dead):
    dist, keep = np_sample_keep_excl(src, dst, N, seeds, fanout, seed, dead)
    return _finish(src, dst, rel, N, len(fanout), dist, keep)
