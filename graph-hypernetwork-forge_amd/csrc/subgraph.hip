// subgraph.hip — the k-hop in-neighbourhood of a seed list, for HyperGNN.forward_nodes (no counterpart in the reference).
//
// An L-layer HyperGNN row is a function of the rows within L hops upstream of it (every layer is a mean over a row's in-edges
// plus a self term, a residual and a LayerNorm of that row: reference hypergnn.py:190-230, 288-296).  Three stages, all on
// the full graph's plan (ghf_plan_build), integer arithmetic only, no result depending on the order in which work lands:
//   hops:  dist[v] = min(hops from v to a seed along edges u -> v), k + 1 beyond k.  One edge-parallel pass per hop: an edge
//          whose destination is at distance j and whose source is unvisited sets the source to j + 1 — every writer writes
//          the same value.  A pass that discovers nothing makes the later passes return at once (a device word, no sync).
//   nodes: node_list = every node with dist <= k ordered by (dist, id), its inverse new_id and m[j] = #{dist <= j}.  Per
//          distance: flags, an exclusive scan, a scatter.  The nodes with dist <= j are the first m[j] rows.
//   edges: every edge whose destination has dist <= k - 1 (its source then has dist <= k), renumbered, in the plan's order:
//          flags, an exclusive scan, a scatter (a stable compaction).
// Edges are read from the plan's compact arrays (8 bytes each), decoded as plan.py: GraphPlan.edge_arrays does:
//   block plans (BN > 1): key = (dst / BN) * R * BN + rel * BN + dst % BN, source in bits 0..27 of sorted_src (run head above);
//   CSR plans (BN == 1):  key = dst * R + rel, sorted_src = the source.
#include "common.h"

#include <hipcub/hipcub.hpp>

namespace ghf {

struct EdgeCode {
    uint32_t R, BN, RBN;
};

__device__ __forceinline__ void sub_decode(uint32_t key, int32_t raw, const EdgeCode c, uint32_t& src, uint32_t& dst,
                                           uint32_t& rel) {
    if (c.BN == 1) {
        dst = key / c.R;
        rel = key - dst * c.R;
        src = (uint32_t)raw;
    } else {
        const uint32_t blk = key / c.RBN, rem = key - blk * c.RBN;
        dst = blk * c.BN + rem % c.BN;
        rel = rem / c.BN;
        src = (uint32_t)raw & (uint32_t)SRC_MASK;
    }
}

// ---- excluded edges (the *_excl calls; semantics and key encoding in include/ghf.h) ----------------------------------
// keys [n] ascending: (uint64)src << 32 | dst, or (typed) | dst * R + rel.  An edge is probed only once every cheaper test
// has passed (it would be taken otherwise), so the searches follow the subgraph, not E.  Whether an edge is excluded is a
// function of the edge alone: the "every writer writes the same value" arguments below stand.  The search never leaves
// [0, n) whatever the list's order; an unsorted list can only miss matches.
struct Excl {
    const uint64_t* keys;
    int64_t n;
    int typed;
};

__device__ __forceinline__ bool sub_excluded(const Excl x, uint32_t s, uint32_t t, uint32_t r, uint32_t R) {
    const uint64_t want = ((uint64_t)s << 32) | (uint64_t)(x.typed ? t * R + r : t);   // (t * R + r < 2^32: the plan's key space)
    int64_t lo = 0, hi = x.n;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (x.keys[mid] < want) lo = mid + 1;
        else hi = mid;
    }
    return lo < x.n && x.keys[lo] == want;
}

static Excl sub_excl(const uint64_t* keys, int64_t n, int typed) {
    Excl x;
    x.keys = keys;
    x.n = n;
    x.typed = typed;
    return x;
}

static unsigned sub_grid(int64_t n) {
    const int64_t g = cdiv(n > 0 ? n : 1, 256);
    return (unsigned)(g < 8192 ? g : 8192);
}

// ---- hops ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sub_dist_init_kernel(int32_t* __restrict__ dist, int64_t N, int k,
                                                            int32_t* __restrict__ found) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (int64_t v = t; v < N; v += stride) dist[v] = k + 1;
    if (t < k) found[t] = 0;
}

__global__ __launch_bounds__(256) void sub_dist_seeds_kernel(const int64_t* __restrict__ seeds, int64_t S, int64_t N,
                                                             int32_t* __restrict__ dist) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < S; i += stride) {
        const int64_t v = seeds[i];
        if (v >= 0 && v < N) dist[v] = 0;                   // (duplicates write the same value)
    }
}

// hop j: sources of edges into distance-j nodes that are still unvisited get distance j + 1 (X: unless the edge is excluded)
template <bool X>
__global__ __launch_bounds__(256) void sub_hop_kernel(const uint32_t* __restrict__ sorted_key, const int32_t* __restrict__ sorted_src,
                                                      int64_t N, int64_t E, EdgeCode c, int j, int k, int32_t* dist,
                                                      int32_t* found, Excl x) {
    if (j > 0 && found[j - 1] == 0) return;                 // hop j - 1 reached nobody: no node is at distance j
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    int any = 0;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < E; e += stride) {
        uint32_t s, t, r;
        sub_decode(sorted_key[e], sorted_src[e], c, s, t, r);
        if (t >= (uint64_t)N || s >= (uint64_t)N) continue;
        if (dist[t] == j && dist[s] > k) {
            if (X && sub_excluded(x, s, t, r, c.R)) continue;
            dist[s] = j + 1;                                // every writer of dist[s] in this pass writes j + 1
            any = 1;
        }
    }
    if (any) atomicOr(&found[j], 1);
}

// ---- nodes -----------------------------------------------------------------------------------------------------------
// f[v] = (dist[v] == j), f[N] = 0; the first level also clears new_id
__global__ __launch_bounds__(256) void sub_level_flags_kernel(const int32_t* __restrict__ dist, int64_t N, int j,
                                                              int32_t* __restrict__ f, int64_t* __restrict__ new_id) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v <= N; v += stride) {
        if (v == N) {
            f[v] = 0;
            continue;
        }
        f[v] = dist[v] == j;
        new_id[v] = -1;
    }
}

// the nodes at distance j go to node_list[m[j-1] + pos[v]]; m[j] = m[j-1] + count; f[] = the flags of distance j + 1
__global__ __launch_bounds__(256) void sub_level_scatter_kernel(const int32_t* __restrict__ dist, int64_t N, int j, int k,
                                                                const int32_t* __restrict__ pos, int32_t* __restrict__ f,
                                                                int64_t* __restrict__ node_list, int64_t* __restrict__ new_id,
                                                                int64_t* m) {
    const int64_t base = j > 0 ? m[j - 1] : 0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v <= N; v += stride) {
        if (v == N) {
            m[j] = base + pos[N];
            continue;
        }
        const int32_t dv = dist[v];
        if (dv == j) {
            const int64_t p = base + pos[v];
            node_list[p] = v;
            new_id[v] = p;
        }
        if (j < k) f[v] = dv == j + 1;                      // (f[N] stays 0)
    }
}

// ---- edges -----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool sub_keep(uint32_t s, uint32_t t, int64_t N, const int32_t* __restrict__ dist, int k) {
    return t < (uint64_t)N && s < (uint64_t)N && dist[t] <= k - 1;
}

template <bool X>
__global__ __launch_bounds__(256) void sub_edge_flags_kernel(const uint32_t* __restrict__ sorted_key,
                                                             const int32_t* __restrict__ sorted_src, int64_t N, int64_t E,
                                                             EdgeCode c, const int32_t* __restrict__ dist, int k,
                                                             int32_t* __restrict__ f, Excl x) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e <= E; e += stride) {
        if (e == E) {
            f[e] = 0;
            continue;
        }
        uint32_t s, t, r;
        sub_decode(sorted_key[e], sorted_src[e], c, s, t, r);
        f[e] = sub_keep(s, t, N, dist, k) && !(X && sub_excluded(x, s, t, r, c.R));
    }
}

// (X: the flags pass has probed the list; its flags f[] are read here instead of probing again)
template <bool X>
__global__ __launch_bounds__(256) void sub_edge_scatter_kernel(const uint32_t* __restrict__ sorted_key,
                                                               const int32_t* __restrict__ sorted_src, int64_t N, int64_t E,
                                                               EdgeCode c, const int32_t* __restrict__ dist,
                                                               const int64_t* __restrict__ new_id, int k,
                                                               const int32_t* __restrict__ f, const int32_t* __restrict__ pos,
                                                               int64_t* __restrict__ edge_out, int64_t* __restrict__ rel_out,
                                                               int64_t* __restrict__ num_edges) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e <= E; e += stride) {
        if (e == E) {
            num_edges[0] = pos[E];
            continue;
        }
        if (X && !f[e]) continue;
        uint32_t s, t, r;
        sub_decode(sorted_key[e], sorted_src[e], c, s, t, r);
        if (!X && !sub_keep(s, t, N, dist, k)) continue;
        const int64_t p = pos[e];
        edge_out[p] = new_id[s];
        edge_out[E + p] = new_id[t];
        rel_out[p] = r;
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------
static size_t sub_scan_bytes(int64_t n) {
    size_t tb = 0;
    hipcub::DeviceScan::ExclusiveSum(nullptr, tb, (const int32_t*)nullptr, (int32_t*)nullptr, (int)n, (hipStream_t)0);
    return tb;
}

// [found: k int32][f: n int32][pos: n int32][scan temp], n = max(N, E) + 1
size_t subgraph_workspace_bytes(int64_t N, int64_t E, int k) {
    if (N <= 0 || E < 0 || k < 1) return 0;
    const int64_t n = (N > E ? N : E) + 1;
    return align_up((size_t)k * 4, 256) + 2 * align_up((size_t)n * 4, 256) + align_up(sub_scan_bytes(n), 256);
}

struct SubWs {
    int32_t* found;
    int32_t* f;
    int32_t* pos;
    void* tmp;
    size_t tmp_bytes;
};

static SubWs sub_ws(void* ws, int64_t N, int64_t E, int k) {
    const int64_t n = (N > E ? N : E) + 1;
    char* p = (char*)ws;
    SubWs w;
    w.found = (int32_t*)p;  p += align_up((size_t)k * 4, 256);
    w.f = (int32_t*)p;      p += align_up((size_t)n * 4, 256);
    w.pos = (int32_t*)p;    p += align_up((size_t)n * 4, 256);
    w.tmp = p;
    w.tmp_bytes = sub_scan_bytes(n);
    return w;
}

static int sub_check(int64_t N, int64_t E, int R, int BN, int k, void* ws, size_t ws_bytes, const char* what) {
    GHF_REQUIRE(N > 0 && N < (1ll << 31) - 1 && E >= 0 && E < (1ll << 31) - 1, "%s: needs 0 < N < 2^31 - 1, 0 <= E < 2^31 - 1", what);
    GHF_REQUIRE(R > 0 && BN > 0 && k >= 1, "%s: R, block_nodes and k must be positive", what);
    GHF_REQUIRE((uint64_t)cdiv(N, BN) * (uint64_t)BN * (uint64_t)R < 0xFFFFFFFFull, "%s: not a plan's key space", what);
    GHF_REQUIRE(ws_bytes >= subgraph_workspace_bytes(N, E, k), "%s: workspace too small", what);
    GHF_REQUIRE(((uintptr_t)ws & 255) == 0, "%s: workspace must be 256-byte aligned", what);
    return GHF_OK;
}

static EdgeCode sub_code(int R, int BN) {
    EdgeCode c;
    c.R = (uint32_t)R;
    c.BN = (uint32_t)BN;
    c.RBN = (uint32_t)R * (uint32_t)BN;
    return c;
}

int launch_subgraph_hops(const uint32_t* sorted_key, const int32_t* sorted_src, int64_t N, int64_t E, int R, int BN,
                         const int64_t* seeds, int64_t S, int k, void* ws, size_t ws_bytes, int32_t* dist,
                         const uint64_t* excl, int64_t n_excl, int typed, hipStream_t stream) {
    const int rc = sub_check(N, E, R, BN, k, ws, ws_bytes, "subgraph_hops");
    if (rc) return rc;
    GHF_REQUIRE(S >= 0, "subgraph_hops: negative seed count");
    const SubWs w = sub_ws(ws, N, E, k);
    sub_dist_init_kernel<<<sub_grid(N > k ? N : k), 256, 0, stream>>>(dist, N, k, w.found);
    GHF_LAUNCH_CHECK();
    if (S > 0) {
        sub_dist_seeds_kernel<<<sub_grid(S), 256, 0, stream>>>(seeds, S, N, dist);
        GHF_LAUNCH_CHECK();
    }
    if (E == 0) return GHF_OK;
    const EdgeCode c = sub_code(R, BN);
    const Excl x = sub_excl(excl, n_excl, typed);
    for (int j = 0; j < k; ++j) {
        if (n_excl > 0)
            sub_hop_kernel<true><<<sub_grid(E), 256, 0, stream>>>(sorted_key, sorted_src, N, E, c, j, k, dist, w.found, x);
        else
            sub_hop_kernel<false><<<sub_grid(E), 256, 0, stream>>>(sorted_key, sorted_src, N, E, c, j, k, dist, w.found, x);
        GHF_LAUNCH_CHECK();
    }
    return GHF_OK;
}

int launch_subgraph_nodes(const int32_t* dist, int64_t N, int k, void* ws, size_t ws_bytes, int64_t* node_list,
                          int64_t* new_id, int64_t* m, hipStream_t stream) {
    GHF_REQUIRE(N > 0 && N < (1ll << 31) - 1 && k >= 1, "subgraph_nodes: needs 0 < N < 2^31 - 1 and k >= 1");
    GHF_REQUIRE(ws_bytes >= subgraph_workspace_bytes(N, 0, k), "subgraph_nodes: workspace too small");
    GHF_REQUIRE(((uintptr_t)ws & 255) == 0, "subgraph_nodes: workspace must be 256-byte aligned");
    SubWs w = sub_ws(ws, N, 0, k);
    // (the nodes stage only needs N + 1 entries of the flag and position arrays: a workspace sized for (N, E) also serves)
    const unsigned g = sub_grid(N + 1);
    sub_level_flags_kernel<<<g, 256, 0, stream>>>(dist, N, 0, w.f, new_id);
    GHF_LAUNCH_CHECK();
    for (int j = 0; j <= k; ++j) {
        GHF_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(w.tmp, w.tmp_bytes, (const int32_t*)w.f, w.pos, (int)(N + 1), stream));
        sub_level_scatter_kernel<<<g, 256, 0, stream>>>(dist, N, j, k, w.pos, w.f, node_list, new_id, m);
        GHF_LAUNCH_CHECK();
    }
    return GHF_OK;
}

int launch_subgraph_edges(const uint32_t* sorted_key, const int32_t* sorted_src, int64_t N, int64_t E, int R, int BN,
                          const int32_t* dist, const int64_t* new_id, int k, void* ws, size_t ws_bytes, int64_t* edge_out,
                          int64_t* rel_out, int64_t* num_edges, const uint64_t* excl, int64_t n_excl, int typed,
                          hipStream_t stream) {
    const int rc = sub_check(N, E, R, BN, k, ws, ws_bytes, "subgraph_edges");
    if (rc) return rc;
    SubWs w = sub_ws(ws, N, E, k);
    const EdgeCode c = sub_code(R, BN);
    const unsigned g = sub_grid(E + 1);
    const Excl x = sub_excl(excl, n_excl, typed);
    if (n_excl > 0)
        sub_edge_flags_kernel<true><<<g, 256, 0, stream>>>(sorted_key, sorted_src, N, E, c, dist, k, w.f, x);
    else
        sub_edge_flags_kernel<false><<<g, 256, 0, stream>>>(sorted_key, sorted_src, N, E, c, dist, k, w.f, x);
    GHF_LAUNCH_CHECK();
    GHF_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(w.tmp, w.tmp_bytes, (const int32_t*)w.f, w.pos, (int)(E + 1), stream));
    if (n_excl > 0)
        sub_edge_scatter_kernel<true><<<g, 256, 0, stream>>>(sorted_key, sorted_src, N, E, c, dist, new_id, k, w.f, w.pos,
                                                             edge_out, rel_out, num_edges);
    else
        sub_edge_scatter_kernel<false><<<g, 256, 0, stream>>>(sorted_key, sorted_src, N, E, c, dist, new_id, k, w.f, w.pos,
                                                              edge_out, rel_out, num_edges);
    GHF_LAUNCH_CHECK();
    return GHF_OK;
}

// ---- sampled hops (HyperGNN.forward_nodes with fanout caps; semantics in include/ghf.h) ------------------------------
// Hop j expands the nodes first reached at sampled distance j: of such a node's in-edges the fanout[j] with the smallest
// (priority, plan position) are kept, all of them when it has no more than that or fanout[j] == -1.  The in-edges of one
// destination are contiguous only in CSR plans, so a capped hop gathers them: flags (destination at distance j), an
// exclusive scan, a stable compaction into 64-bit keys (dst << 32 | priority) with the plan position as the value, one
// stable radix sort (equal keys stay in position order), then sorted entry i is kept unless entry i - fanout[j] has the same
// destination (its rank inside its destination's segment is then >= fanout[j]) — O(1) per edge whatever a hub's degree.  The
// sort's length is the one host read of a capped hop.  keep[] and dist[] only ever receive values that do not depend on which thread writes first.

// splitmix64 (Steele, Lea, Flood 2014; Vigna's constants) at state seed + (position + 1) * golden gamma: the high word
__host__ __device__ __forceinline__ uint32_t sample_priority(uint64_t seed, uint32_t position) {
    uint64_t z = seed + ((uint64_t)position + 1ull) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (uint32_t)(z >> 32);
}

__global__ __launch_bounds__(256) void sample_init_kernel(int32_t* __restrict__ dist, int32_t* __restrict__ keep, int64_t N,
                                                          int64_t E, int k, int32_t* __restrict__ found) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (int64_t v = t; v < N; v += stride) dist[v] = k + 1;
    for (int64_t e = t; e < E; e += stride) keep[e] = 0;
    if (t < k) found[t] = 0;
}

// a hop without a cap: sub_hop_kernel, which also marks the edges it walks (X: an excluded edge is not a candidate)
template <bool X>
__global__ __launch_bounds__(256) void sample_hop_all_kernel(const uint32_t* __restrict__ sorted_key,
                                                             const int32_t* __restrict__ sorted_src, int64_t N, int64_t E,
                                                             EdgeCode c, int j, int k, int32_t* dist,
                                                             int32_t* __restrict__ keep, int32_t* found, Excl x) {
    if (j > 0 && found[j - 1] == 0) return;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    int any = 0;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < E; e += stride) {
        uint32_t s, t, r;
        sub_decode(sorted_key[e], sorted_src[e], c, s, t, r);
        if (t >= (uint64_t)N || s >= (uint64_t)N) continue;
        if (dist[t] != j) continue;
        if (X && sub_excluded(x, s, t, r, c.R)) continue;
        keep[e] = 1;
        if (dist[s] > k) {
            dist[s] = j + 1;                                // every writer of dist[s] in this pass writes j + 1
            any = 1;
        }
    }
    if (any) atomicOr(&found[j], 1);
}

// f[e] = (the destination of edge e is at distance j) (X: and the edge is not excluded), f[E] = 0
template <bool X>
__global__ __launch_bounds__(256) void sample_cand_flags_kernel(const uint32_t* __restrict__ sorted_key,
                                                                const int32_t* __restrict__ sorted_src, int64_t N, int64_t E,
                                                                EdgeCode c, const int32_t* __restrict__ dist, int j,
                                                                int32_t* __restrict__ f, Excl x) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e <= E; e += stride) {
        if (e == E) {
            f[e] = 0;
            continue;
        }
        uint32_t s, t, r;
        sub_decode(sorted_key[e], sorted_src[e], c, s, t, r);
        f[e] = t < (uint64_t)N && s < (uint64_t)N && dist[t] == j && !(X && sub_excluded(x, s, t, r, c.R));
    }
}

__global__ __launch_bounds__(256) void sample_cand_scatter_kernel(const uint32_t* __restrict__ sorted_key,
                                                                  const int32_t* __restrict__ sorted_src, int64_t E, EdgeCode c,
                                                                  uint64_t seed, const int32_t* __restrict__ f,
                                                                  const int32_t* __restrict__ pos, uint64_t* __restrict__ keys,
                                                                  uint32_t* __restrict__ vals) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < E; e += stride) {
        if (!f[e]) continue;
        uint32_t s, t, r;
        sub_decode(sorted_key[e], sorted_src[e], c, s, t, r);
        const int32_t p = pos[e];
        keys[p] = ((uint64_t)t << 32) | sample_priority(seed, (uint32_t)e);
        vals[p] = (uint32_t)e;
    }
}

// entry i of the sorted candidates is among its destination's first `fan` unless entry i - fan has the same destination
__global__ __launch_bounds__(256) void sample_select_kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                                                            int64_t C, const int32_t* __restrict__ sorted_src, EdgeCode c,
                                                            int64_t N, int fan, int j, int k, int32_t* dist,
                                                            int32_t* __restrict__ keep, int32_t* found) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    int any = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < C; i += stride) {
        if (i >= fan) {                                     // (the first `fan` entries overall are kept whatever their rank)
            const uint64_t head = keys[i] & 0xFFFFFFFF00000000ull;
            if (keys[i - fan] >= head) continue;            // `fan` entries of this destination come before: rank >= fan
        }
        const uint32_t e = vals[i];
        keep[e] = 1;
        const uint32_t s = c.BN == 1 ? (uint32_t)sorted_src[e] : ((uint32_t)sorted_src[e] & (uint32_t)SRC_MASK);
        if (s < (uint64_t)N && dist[s] > k) {
            dist[s] = j + 1;                                // every writer of dist[s] in this pass writes j + 1
            any = 1;
        }
    }
    if (any) atomicOr(&found[j], 1);
}

// ---- edges by flag: the kept edges, renumbered, in the plan's order ----------------------------------------------------
__global__ __launch_bounds__(256) void sample_edge_flags_kernel(const uint32_t* __restrict__ sorted_key,
                                                                const int32_t* __restrict__ sorted_src, int64_t N, int64_t E,
                                                                EdgeCode c, const int32_t* __restrict__ keep,
                                                                int32_t* __restrict__ f) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e <= E; e += stride) {
        if (e == E) {
            f[e] = 0;
            continue;
        }
        uint32_t s, t, r;
        sub_decode(sorted_key[e], sorted_src[e], c, s, t, r);
        f[e] = keep[e] != 0 && t < (uint64_t)N && s < (uint64_t)N;
    }
}

__global__ __launch_bounds__(256) void sample_edge_scatter_kernel(const uint32_t* __restrict__ sorted_key,
                                                                  const int32_t* __restrict__ sorted_src, int64_t N, int64_t E,
                                                                  EdgeCode c, const int32_t* __restrict__ f,
                                                                  const int64_t* __restrict__ new_id,
                                                                  const int32_t* __restrict__ pos, int64_t* __restrict__ edge_out,
                                                                  int64_t* __restrict__ rel_out, int64_t* __restrict__ num_edges) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e <= E; e += stride) {
        if (e == E) {
            num_edges[0] = pos[E];
            continue;
        }
        if (!f[e]) continue;
        uint32_t s, t, r;
        sub_decode(sorted_key[e], sorted_src[e], c, s, t, r);
        const int64_t p = pos[e];
        edge_out[p] = new_id[s];
        edge_out[E + p] = new_id[t];
        rel_out[p] = r;
    }
}

// (double buffers: the sort ping-pongs between the workspace's two key and two value arrays, its temp stays small)
static hipError_t sample_sort_bytes(int64_t n, int end_bit, size_t* bytes) {
    hipcub::DoubleBuffer<uint64_t> keys(nullptr, nullptr);
    hipcub::DoubleBuffer<uint32_t> vals(nullptr, nullptr);
    *bytes = 0;
    return hipcub::DeviceRadixSort::SortPairs(nullptr, *bytes, keys, vals, (int)n, 0, end_bit, (hipStream_t)0);
}

static int sample_end_bit(int64_t N) {
    int b = 1;
    while (b < 31 && (1ll << b) < N) ++b;
    return 32 + b;
}

// the temp both library calls need: the scans over n = max(N, E) + 1 flags, one sort of up to E pairs
static hipError_t sample_tmp_bytes(int64_t N, int64_t E, size_t* bytes) {
    size_t a = 0, b = 0;
    *bytes = 0;
    hipError_t e = hipcub::DeviceScan::ExclusiveSum(nullptr, a, (const int32_t*)nullptr, (int32_t*)nullptr,
                                                    (int)((N > E ? N : E) + 1), (hipStream_t)0);
    if (e == hipSuccess) e = sample_sort_bytes(E, sample_end_bit(N), &b);
    if (e == hipSuccess) *bytes = a > b ? a : b;
    return e;
}

// [found: k int32][f: n int32][pos: n int32][scan / sort temp][keys: 2 x E uint64][vals: 2 x E uint32], n = max(N, E) + 1:
// the head is subgraph_workspace_bytes' layout (with more temp), so ghf_subgraph_nodes runs on the same workspace
static size_t sample_layout_bytes(int64_t N, int64_t E, int k, size_t tmp_bytes) {
    const int64_t n = (N > E ? N : E) + 1;
    return align_up((size_t)k * 4, 256) + 2 * align_up((size_t)n * 4, 256) + align_up(tmp_bytes, 256) +
           2 * align_up((size_t)E * 8, 256) + 2 * align_up((size_t)E * 4, 256);
}

// 0 for bad sizes or a failed size query.  A host without a device (the queries then report hipErrorNoDevice) gets the size
// without the temp: nothing can be launched there, and the launchers refuse to run after a failed query.
size_t subgraph_sample_workspace_bytes(int64_t N, int64_t E, int k) {
    if (N <= 0 || E < 0 || k < 1 || N >= (1ll << 31) - 1 || E >= (1ll << 31) - 1) return 0;
    size_t tmp = 0;
    const hipError_t e = sample_tmp_bytes(N, E, &tmp);
    if (e != hipSuccess && e != hipErrorNoDevice) return 0;
    return sample_layout_bytes(N, E, k, tmp);
}

struct SampleWs {
    SubWs s;
    uint64_t *keys_in, *keys_out;
    uint32_t *vals_in, *vals_out;
};

static SampleWs sample_ws(void* ws, int64_t N, int64_t E, int k, size_t tmp_bytes) {
    SampleWs w;
    w.s = sub_ws(ws, N, E, k);
    w.s.tmp_bytes = tmp_bytes;
    char* p = (char*)w.s.tmp + align_up(w.s.tmp_bytes, 256);
    w.keys_in = (uint64_t*)p;   p += align_up((size_t)E * 8, 256);
    w.keys_out = (uint64_t*)p;  p += align_up((size_t)E * 8, 256);
    w.vals_in = (uint32_t*)p;   p += align_up((size_t)E * 4, 256);
    w.vals_out = (uint32_t*)p;
    return w;
}

// the argument checks of both stages; *tmp_bytes: the temp size, queried once per call.  Bad arguments are reported before a
// failed query is (GHF_EINVAL needs no device), a failed query before anything is launched.
static int sample_check(int64_t N, int64_t E, int R, int BN, int k, void* ws, size_t ws_bytes, const char* what,
                        size_t* tmp_bytes) {
    GHF_REQUIRE(N > 0 && N < (1ll << 31) - 1 && E >= 0 && E < (1ll << 31) - 1, "%s: needs 0 < N < 2^31 - 1, 0 <= E < 2^31 - 1", what);
    GHF_REQUIRE(R > 0 && BN > 0 && k >= 1, "%s: R, block_nodes and k must be positive", what);
    GHF_REQUIRE((uint64_t)cdiv(N, BN) * (uint64_t)BN * (uint64_t)R < 0xFFFFFFFFull, "%s: not a plan's key space", what);
    const hipError_t query = sample_tmp_bytes(N, E, tmp_bytes);
    GHF_REQUIRE(ws_bytes >= sample_layout_bytes(N, E, k, *tmp_bytes), "%s: workspace too small", what);
    GHF_REQUIRE(((uintptr_t)ws & 255) == 0, "%s: workspace must be 256-byte aligned", what);
    GHF_HIP_CHECK(query);
    return GHF_OK;
}

int launch_subgraph_sample_hops(const uint32_t* sorted_key, const int32_t* sorted_src, int64_t N, int64_t E, int R, int BN,
                                const int64_t* seeds, int64_t S, int k, const int* fanout, uint64_t seed, void* ws,
                                size_t ws_bytes, int32_t* dist, int32_t* keep, int64_t* host_reads, const uint64_t* excl,
                                int64_t n_excl, int typed, hipStream_t stream) {
    GHF_REQUIRE(S >= 0, "subgraph_sample_hops: negative seed count");
    for (int j = 0; j < k; ++j)
        GHF_REQUIRE(fanout[j] == -1 || fanout[j] >= 1, "subgraph_sample_hops: fanout[%d] = %d (needs -1 or >= 1)", j, fanout[j]);
    size_t tmp_bytes = 0;
    const int rc = sample_check(N, E, R, BN, k, ws, ws_bytes, "subgraph_sample_hops", &tmp_bytes);
    if (rc) return rc;
    if (host_reads) *host_reads = 0;
    SampleWs w = sample_ws(ws, N, E, k, tmp_bytes);
    const int64_t ne = N > E ? N : E;
    sample_init_kernel<<<sub_grid(ne > k ? ne : k), 256, 0, stream>>>(dist, keep, N, E, k, w.s.found);
    GHF_LAUNCH_CHECK();
    if (S > 0) {
        sub_dist_seeds_kernel<<<sub_grid(S), 256, 0, stream>>>(seeds, S, N, dist);
        GHF_LAUNCH_CHECK();
    }
    if (E == 0) return GHF_OK;
    const EdgeCode c = sub_code(R, BN);
    const int end_bit = sample_end_bit(N);
    const Excl x = sub_excl(excl, n_excl, typed);
    for (int j = 0; j < k; ++j) {
        if (fanout[j] == -1) {
            if (n_excl > 0)
                sample_hop_all_kernel<true><<<sub_grid(E), 256, 0, stream>>>(sorted_key, sorted_src, N, E, c, j, k, dist, keep,
                                                                            w.s.found, x);
            else
                sample_hop_all_kernel<false><<<sub_grid(E), 256, 0, stream>>>(sorted_key, sorted_src, N, E, c, j, k, dist, keep,
                                                                             w.s.found, x);
            GHF_LAUNCH_CHECK();
            continue;
        }
        if (n_excl > 0)
            sample_cand_flags_kernel<true><<<sub_grid(E + 1), 256, 0, stream>>>(sorted_key, sorted_src, N, E, c, dist, j, w.s.f, x);
        else
            sample_cand_flags_kernel<false><<<sub_grid(E + 1), 256, 0, stream>>>(sorted_key, sorted_src, N, E, c, dist, j, w.s.f, x);
        GHF_LAUNCH_CHECK();
        GHF_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(w.s.tmp, w.s.tmp_bytes, (const int32_t*)w.s.f, w.s.pos, (int)(E + 1), stream));
        int32_t C = 0;                                      // the hop's one host read: the number of candidate edges
        GHF_HIP_CHECK(hipMemcpyAsync(&C, w.s.pos + E, sizeof(C), hipMemcpyDeviceToHost, stream));
        GHF_HIP_CHECK(hipStreamSynchronize(stream));
        if (host_reads) ++*host_reads;
        if (C <= 0) break;                                  // nobody at distance j has an in-edge: nor will anybody later
        GHF_REQUIRE(C <= E, "subgraph_sample_hops: candidate count %d out of range", (int)C);
        sample_cand_scatter_kernel<<<sub_grid(E), 256, 0, stream>>>(sorted_key, sorted_src, E, c, seed, w.s.f, w.s.pos, w.keys_in,
                                                                    w.vals_in);
        GHF_LAUNCH_CHECK();
        size_t need = 0;                                    // (C <= E pairs must fit the temp sized for E)
        GHF_HIP_CHECK(sample_sort_bytes(C, end_bit, &need));
        GHF_REQUIRE(need <= w.s.tmp_bytes, "subgraph_sample_hops: sort workspace %zu > %zu", need, w.s.tmp_bytes);
        need = w.s.tmp_bytes;
        hipcub::DoubleBuffer<uint64_t> keys(w.keys_in, w.keys_out);
        hipcub::DoubleBuffer<uint32_t> vals(w.vals_in, w.vals_out);
        GHF_HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(w.s.tmp, need, keys, vals, (int)C, 0, end_bit, stream));
        sample_select_kernel<<<sub_grid(C), 256, 0, stream>>>(keys.Current(), vals.Current(), C, sorted_src, c, N, fanout[j], j, k,
                                                              dist, keep, w.s.found);
        GHF_LAUNCH_CHECK();
    }
    return GHF_OK;
}

int launch_subgraph_sample_edges(const uint32_t* sorted_key, const int32_t* sorted_src, int64_t N, int64_t E, int R, int BN,
                                 const int32_t* keep, const int64_t* new_id, void* ws, size_t ws_bytes, int64_t* edge_out,
                                 int64_t* rel_out, int64_t* num_edges, hipStream_t stream) {
    size_t tmp_bytes = 0;
    const int rc = sample_check(N, E, R, BN, 1, ws, ws_bytes, "subgraph_sample_edges", &tmp_bytes);
    if (rc) return rc;
    SubWs w = sub_ws(ws, N, E, 1);
    w.tmp_bytes = tmp_bytes;
    const EdgeCode c = sub_code(R, BN);
    const unsigned g = sub_grid(E + 1);
    sample_edge_flags_kernel<<<g, 256, 0, stream>>>(sorted_key, sorted_src, N, E, c, keep, w.f);
    GHF_LAUNCH_CHECK();
    GHF_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(w.tmp, w.tmp_bytes, (const int32_t*)w.f, w.pos, (int)(E + 1), stream));
    sample_edge_scatter_kernel<<<g, 256, 0, stream>>>(sorted_key, sorted_src, N, E, c, w.f, new_id, w.pos, edge_out, rel_out,
                                                      num_edges);
    GHF_LAUNCH_CHECK();
    return GHF_OK;
}

}  // namespace ghf
