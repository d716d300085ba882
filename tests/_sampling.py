"""A numpy restatement of the sampled k-hop subgraph (include/ghf.h: ghf_subgraph_sample_*): the priority function written
out again, the plan's stable order, a per-destination smallest-f selection and the hop loop.  Shared by test_sample_host.py
and test_sample_gpu.py; nothing here touches the library."""

import numpy as np

M64 = (1 << 64) - 1


def priority(seed, position):
    """ghf.h's priority(e): splitmix64 at state seed + (position + 1) * 0x9E3779B97F4A7C15, the high 32 bits."""
    pos = np.asarray(position, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = np.uint64(seed & M64) + (pos + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(32)).astype(np.int64)


def priority_scalar(seed, position):
    """The same in Python integers (one edge): checks the array form's wrap-around arithmetic."""
    z = (seed + (position + 1) * 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return z >> 32


def plan_order(ei, rel, N, R, bn):
    """The stable order of ghf_plan_build: key = (dst / BN) R BN + rel BN + dst % BN, or dst R + rel for CSR plans."""
    dst = ei[1]
    key = dst * R + rel if bn == 1 else (dst // bn) * (R * bn) + rel * bn + dst % bn
    return np.argsort(key, kind="stable")


def select(dst, cand, prio, f):
    """Of the candidate edge positions `cand`, per destination the f with the smallest (priority, position)."""
    order = np.lexsort((cand, prio[cand], dst[cand]))
    c = cand[order]
    d = dst[c]
    rank = np.arange(c.size) - np.searchsorted(d, d, side="left")
    return np.sort(c[rank < f])


def np_sample_keep(src, dst, N, seeds, fanout, seed):
    """(dist, keep): the hop loop over edges given in the plan's order (position = index)."""
    k = len(fanout)
    dist = np.full(N, k + 1, dtype=np.int64)
    dist[np.asarray(seeds, dtype=np.int64) % N] = 0
    keep = np.zeros(src.size, dtype=bool)
    prio = priority(seed, np.arange(src.size))
    for j, f in enumerate(fanout):
        cand = np.nonzero(dist[dst] == j)[0]
        sel = cand if f == -1 else select(dst, cand, prio, f)
        keep[sel] = True
        s = src[sel]
        dist[s[dist[s] > k]] = j + 1
    return dist, keep


def np_subgraph_sample(src, dst, rel, N, seeds, fanout, seed):
    """dist, node_list, new_id, m, kept edges [2, E'] and their relations, in the order of the edges given (the plan's)."""
    k = len(fanout)
    dist, keep = np_sample_keep(src, dst, N, seeds, fanout, seed)
    inside = np.nonzero(dist <= k)[0]
    node_list = inside[np.lexsort((inside, dist[inside]))]
    new_id = np.full(N, -1, dtype=np.int64)
    new_id[node_list] = np.arange(node_list.size)
    m = [int((dist <= j).sum()) for j in range(k + 1)]
    return dist, node_list, new_id, m, np.stack([new_id[src[keep]], new_id[dst[keep]]]), rel[keep]


def np_subgraph(src, dst, rel, N, seeds, k):
    """The exact k-hop subgraph (the restatement of test_subgraph_nodes.py)."""
    dist = np.full(N, k + 1, dtype=np.int64)
    dist[np.asarray(seeds, dtype=np.int64) % N] = 0
    for j in range(k):
        s = src[dist[dst] == j]
        dist[s[dist[s] > k]] = j + 1
    inside = np.nonzero(dist <= k)[0]
    node_list = inside[np.lexsort((inside, dist[inside]))]
    new_id = np.full(N, -1, dtype=np.int64)
    new_id[node_list] = np.arange(node_list.size)
    m = [int((dist <= j).sum()) for j in range(k + 1)]
    keep = dist[dst] <= k - 1
    return dist, node_list, new_id, m, np.stack([new_id[src[keep]], new_id[dst[keep]]]), rel[keep]


def uniformity_graph(D=4096, S=32):
    """D destinations (nodes S .. S + D - 1) that share the same S sources (nodes 0 .. S - 1), one edge each: E = D * S,
    shuffled; one relation."""
    src = np.tile(np.arange(S, dtype=np.int64), D)
    dst = np.repeat(np.arange(S, S + D, dtype=np.int64), S)
    perm = np.random.default_rng(4096).permutation(src.size)
    return np.stack([src[perm], dst[perm]]), np.zeros(src.size, dtype=np.int64), S + D


UNIFORMITY_SEED = 20261017
UNIFORMITY_BOUND = (1024, 139)      # Binomial(4096, 1/4): mean 1024, five standard deviations (sqrt(768) = 27.7) = 139


def tie_graph(E=300_000, seed=7):
    """One destination (node E) with E in-edges from the distinct sources 0 .. E - 1 (position = source id), and the pairs of
    them whose priorities under `seed` collide: (lower position, higher position, the cap that falls between the two)."""
    src = np.arange(E, dtype=np.int64)
    dst = np.full(E, E, dtype=np.int64)
    prio = priority(seed, src)
    order = np.lexsort((src, prio))
    p = prio[order]
    at = np.nonzero(p[1:] == p[:-1])[0]                 # sorted ranks r, r + 1 hold equal priorities
    at = at[(np.r_[True, p[at[1:]] != p[at[:-1]]])] if at.size else at       # (the first pair of a longer run only)
    pairs = [(int(order[r]), int(order[r + 1]), int(r + 1)) for r in at]
    return src, dst, E + 1, seed, pairs
