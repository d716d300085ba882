// rank.hip — link prediction against every node: filtered rank counts and top-k partners, the B x N scores never stored.
//
// What a user of the reference does after training (demo.py:79-101 trains on pair scores): score a query node against all
// N nodes, s(i, j) = q_i . c_j, and ask where the true partner ranks or which k partners score highest.  Both are one tiled
// q . c^T on the exact fp32 matrix instruction (v_mfma_f32_32x32x2_f32) whose epilogue consumes the accumulators in registers:
//
//   workgroup = 512 threads = 4 x 2 waves, block tile 256 candidates x 128 queries (d > 128: 256 threads, 128 x 128, so that
//   the LDS still holds the query tile), wave tile 64 x 64 = 2 x 2 MFMA tiles (64 accumulator registers: four independent
//   chains per wave).  Two waves share a SIMD: one multiplies while the other waits at the barrier or for LDS.
//   Candidates are the A operand (rows), queries the B operand (columns): the accumulator map of the 32x32 form puts the
//   COLUMN on the lane (col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)), so a lane compares its 16 registers
//   of one tile against ONE query's threshold and keeps one counter per query column.
//   The query tile (128 x d) is loaded once per workgroup and stays in LDS; candidate rows stream through two LDS buffers
//   of BK columns (BK = 32; 16 when d > 128), fetched into registers one step ahead of the step being multiplied: one
//   barrier per step.
//   LDS rows hold k permuted inside groups of 8 (position 4 (k & 1) + (k >> 1 & 3)) so that a lane's ONE 16-byte read gives
//   it k = h, h+2, h+4, h+6 (h = lane >> 5): the operands of four consecutive MFMAs, k ascending.
//   A workgroup owns (query tile, candidate slab); workgroups are numbered so that the ones an XCD runs together are the
//   query tiles of one slab, which then streams from HBM once and from that XCD's L2 after.
//
// Numerics: an accumulator is bit for bit the chain s = fmaf(q[k], c[k], s), k = 0 .. d-1, from s = 0 (zero padding of k
// adds fma(0, 0, s) = s).  dot_chain() below is that chain on the VALU: the target's score t_i and the filter corrections
// come from it and compare equal to the tile's value of the same pair.
//
// Rank:   greater / equal start at 0 (score_prep_kernel, which also computes t_i), every (query tile, candidate slab)
//         workgroup adds its integer counts with atomics (order-free, so reproducible), rank_filter_kernel takes the listed
//         known-true candidates out again by recomputing their scores, rank_finish_kernel takes the target out of `equal`
//         and writes -1 for a query with an id out of range.
// Top-k:  a workgroup keeps, per query, an append buffer of cap = k + (candidates per step) + 64 entries in the caller's
//         workspace and a threshold in LDS (the k-th best so far; candidates arrive in ascending id, so a tie with it
//         loses).  An entry is one 64-bit key ordered as (score descending, id ascending).  A candidate above the threshold
//         that is not in the query's (sorted) filter list is appended; when the next step could overflow the buffer a wave
//         selects the k best in place (select_in_place).  topk_merge_kernel merges the slabs' sorted lists: a key's
//         position is the number of keys above it, one binary search per slab.  A query with an id out of range
//         (score_prep_kernel, list_range_kernel) gets NaN scores and ids -1.
//
// The host side the four operations share (the prep kernel, the lists' range check, the checks that open a launch, the
// choice of the sweep's instantiation) is in rank_sweep.h.
#include "common.h"
#include "rank_sweep.h"

namespace ghf {

// four workgroups per CU over the call: the tail of the last round stays short; a slab still amortises its query-tile load
static inline bool rank_geom_rank(int64_t B, int64_t N, int d, RankGeom* g) { return rank_geom(B, N, d, 4 * RK_CUS, g); }
// one round: the longer the slab, the rarer an insertion (the threshold only rises) and the smaller the table to merge
static inline bool rank_geom_topk(int64_t B, int64_t N, int d, RankGeom* g) { return rank_geom(B, N, d, RK_CUS, g); }

size_t score_rank_workspace_bytes(int64_t B, int64_t N, int d) {
    RankGeom g;
    if (d <= 0 || d > RK_MAX_D || !rank_geom_rank(B, N, d, &g)) return 0;
    return rk_align((size_t)B * 4) + rk_align((size_t)B * 4);          // t [B] float, valid [B] int32
}

size_t score_topk_workspace_bytes(int64_t B, int64_t N, int d, int k) {
    RankGeom g;
    if (d <= 0 || d > RK_MAX_D || k < 1 || k > TOPK_MAX_K || !rank_geom_topk(B, N, d, &g)) return 0;
    const size_t entries = (size_t)B * (size_t)g.slabs * (size_t)topk_cap(d, k);
    return rk_align((size_t)B * 4) + rk_align(entries * 8);           // valid [B] int32, keys (8 bytes per entry)
}

// a candidate subset (candidates.hip): the all-node workspace for N := C, then the id map's
size_t score_rank_sub_workspace_bytes(int64_t B, int64_t C, int d, int64_t nnz) {
    const size_t base = score_rank_workspace_bytes(B, C, d), map = cand_workspace_bytes(B, nnz);
    return base && map ? base + map : 0;
}

size_t score_topk_sub_workspace_bytes(int64_t B, int64_t C, int d, int k, int64_t nnz) {
    const size_t base = score_topk_workspace_bytes(B, C, d, k), map = cand_workspace_bytes(B, nnz);
    return base && map ? base + map : 0;
}

// with a per-candidate bias: C = 0 is the all-node call (no id map), C > 0 adds the subset's gathered bias [C]
size_t score_rank_b_workspace_bytes(int64_t B, int64_t N, int64_t C, int d, int64_t nnz) {
    if (C <= 0) return score_rank_workspace_bytes(B, N, d);
    const size_t base = score_rank_sub_workspace_bytes(B, C, d, nnz);
    return base ? base + rk_align((size_t)C * 4) : 0;
}

size_t score_topk_b_workspace_bytes(int64_t B, int64_t N, int64_t C, int d, int k, int64_t nnz) {
    if (C <= 0) return score_topk_workspace_bytes(B, N, d, k);
    const size_t base = score_topk_sub_workspace_bytes(B, C, d, k, nnz);
    return base ? base + rk_align((size_t)C * 4) : 0;
}

// ---- rank: the small kernels around the sweep -----------------------------------------------------------------------------
// one thread per filter entry: an id out of range marks its query; any other entry's score is recomputed and taken out of the
// count it went into (lists are sorted: a repeat is the entry before; the target is taken out by rank_finish)
// (BIAS: the entry's score is the sweep's, s + bias[j], bias in the sweep's candidate space)
template <bool BIAS>
__device__ __forceinline__ void rank_filter_body(const float* __restrict__ q, const float* __restrict__ c,
                                                 const int64_t* __restrict__ iq, const int64_t* __restrict__ target,
                                                 const int64_t* __restrict__ filt_ptr, const int64_t* __restrict__ filt_idx,
                                                 int64_t nnz, int64_t N, int64_t B, int d, const float* __restrict__ t,
                                                 int* valid, unsigned long long* __restrict__ greater,
                                                 unsigned long long* __restrict__ equal, const int64_t* __restrict__ ic,
                                                 const float* __restrict__ bias) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= nnz) return;
    int64_t i;
    if (!list_owner(filt_ptr, B, e, &i)) return;
    const int64_t j = filt_idx[e];
    if (j < 0 || j >= N) {
        valid[i] = 0;
        return;
    }
    if (!valid[i]) return;
    if (j == target[i] || (e > filt_ptr[i] && filt_idx[e - 1] == j)) return;
    const int64_t r = iq ? iq[i] : i;                // in range: score_prep_kernel said so (valid[i] was 1)
    // over a candidate subset j and target[] are positions in ic (candidates.hip, which has checked ic)
    float s = dot_chain(q + (size_t)r * d, c + (size_t)(ic ? ic[j] : j) * d, d, rows_vec(q, d) && rows_vec(c, d));
    if constexpr (BIAS) s += bias[j];
    const float ti = t[i];
    if (s > ti) atomicAdd(&greater[i], ~0ull);
    else if (s == ti) atomicAdd(&equal[i], ~0ull);
}

__global__ __launch_bounds__(256) void rank_filter_kernel(const float* __restrict__ q, const float* __restrict__ c,
                                                          const int64_t* __restrict__ iq, const int64_t* __restrict__ target,
                                                          const int64_t* __restrict__ filt_ptr, const int64_t* __restrict__ filt_idx,
                                                          int64_t nnz, int64_t N, int64_t B, int d, const float* __restrict__ t,
                                                          int* valid, unsigned long long* __restrict__ greater,
                                                          unsigned long long* __restrict__ equal, const int64_t* __restrict__ ic) {
    rank_filter_body<false>(q, c, iq, target, filt_ptr, filt_idx, nnz, N, B, d, t, valid, greater, equal, ic, nullptr);
}

__global__ __launch_bounds__(256) void rank_filter_bias_kernel(const float* __restrict__ q, const float* __restrict__ c,
                                                               const int64_t* __restrict__ iq, const int64_t* __restrict__ target,
                                                               const int64_t* __restrict__ filt_ptr,
                                                               const int64_t* __restrict__ filt_idx, int64_t nnz, int64_t N, int64_t B,
                                                               int d, const float* __restrict__ t, int* valid,
                                                               unsigned long long* __restrict__ greater,
                                                               unsigned long long* __restrict__ equal,
                                                               const int64_t* __restrict__ ic, const float* __restrict__ bias) {
    rank_filter_body<true>(q, c, iq, target, filt_ptr, filt_idx, nnz, N, B, d, t, valid, greater, equal, ic, bias);
}

// one thread per query, behind the prep pass of a call with a bias: the target's score gets its own node's bias entry (the
// target need not be a candidate, so `bias` and `target` are the caller's, in node ids).  A query that is not valid keeps NaN.
__global__ __launch_bounds__(256) void rank_bias_target_kernel(const int64_t* __restrict__ target, const float* __restrict__ bias,
                                                               const int* __restrict__ valid, int64_t B, float* __restrict__ t) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= B || !valid[i]) return;
    t[i] += bias[target[i]];
}

__global__ __launch_bounds__(256) void rank_finish_kernel(const float* __restrict__ t, const int* __restrict__ valid, int64_t B,
                                                          long long* __restrict__ greater, long long* __restrict__ equal,
                                                          const int64_t* __restrict__ tpos) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= B) return;
    if (!valid[i]) {
        greater[i] = -1;
        equal[i] = -1;
    } else if (t[i] == t[i] && (!tpos || tpos[i] >= 0)) {
        equal[i] -= 1;                               // the target's own score, counted by the tile that holds it (over a
                                                     // candidate subset: when the target is a candidate)
    }
}

// ---- top-k: merge the slabs' sorted lists; one wave per query -------------------------------------------------------------
__global__ __launch_bounds__(256) void topk_merge_kernel(const uint64_t* __restrict__ ws_key, const int* __restrict__ valid,
                                                         int64_t B, int64_t slabs, int cap, int k, float* __restrict__ out_sc,
                                                         long long* __restrict__ out_id, const int64_t* __restrict__ ic) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= B) return;
    float* os = out_sc + (size_t)i * k;
    long long* oi = out_id + (size_t)i * k;
    if (!valid[i]) {                                 // an id out of range: NaN scores (as ghf_score_pairs_fwd), ids -1
        for (int p = lane; p < k; p += 64) {
            os[p] = __int_as_float(0x7FC00000);
            oi[p] = -1;
        }
        return;
    }
    const uint64_t* keys = ws_key + (size_t)i * slabs * cap;
    const int64_t m = slabs * k;
    int mine = 0;
    for (int64_t e = lane; e < m; e += 64) {
        const int64_t se = e / k;
        const uint64_t key = keys[se * cap + (e - se * k)];
        if (key == 0) continue;
        ++mine;
        int64_t rank = 0;
        for (int64_t sl = 0; sl < slabs && rank < k; ++sl) {
            // keys of slab sl above this one: its list is sorted downwards, empty slots last
            int lo = 0, hi = k;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (keys[sl * cap + mid] > key) lo = mid + 1; else hi = mid;
            }
            rank += lo;
        }
        if (rank < k) {
            os[rank] = key_score(key);
            oi[rank] = ic ? ic[key_id(key)] : key_id(key);      // a candidate subset: the position back to its node id
        }
    }
    // entries in all: positions from there on hold no candidate
    for (int off = 32; off; off >>= 1) mine += __shfl_xor(mine, off, 64);
    for (int64_t p = mine + lane; p < k; p += 64) {
        os[p] = -INFINITY;
        oi[p] = -1;
    }
}

// ---- launches -------------------------------------------------------------------------------------------------------------
int launch_score_rank(const float* q, const float* c, const int64_t* iq, const int64_t* target, const int64_t* filt_ptr,
                      const int64_t* filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d, void* ws,
                      size_t ws_bytes, int64_t* greater, int64_t* equal, hipStream_t stream, const int64_t* ic, int64_t C,
                      const float* bias) {
    RankArgs a;
    const int64_t M = ic ? C : N;                    // the candidates the sweep runs over
    GHF_REQUIRE(!ic || (C > 0 && C <= N), "score_rank: need 1 <= C <= N candidates");
    const size_t base = score_rank_workspace_bytes(B, M, d);
    const size_t need = ic ? score_rank_sub_workspace_bytes(B, C, d, nnz) : base;      // with a bias over a subset: + its [C] floats
    const size_t need_b = bias && ic && need ? need + rk_align((size_t)C * 4) : need;
    int rc = score_open("score_rank", rank_geom_rank, need_b, q, c, iq, filt_ptr, filt_idx, nnz, rows_q, M, B, d, ws_bytes, &a);
    if (rc != GHF_OK) return rc;
    float* t = (float*)ws;
    int* valid = (int*)((char*)ws + rk_align((size_t)B * 4));
    const unsigned qb = (unsigned)cdiv(B, 256);
    const float* bias_c = bias;                      // the bias in the sweep's candidate space
    if (bias && ic) {
        GHF_REQUIRE(need > 0, "candidates: B or nnz out of range");
        bias_c = (float*)((char*)ws + need);
        rc = launch_cand_bias(bias, ic, C, N, (float*)((char*)ws + need), stream);
        if (rc != GHF_OK) return rc;
    }
    const int64_t* target_nodes = target;
    CandMap m = {};
    if (ic) {
        rc = launch_cand_map(q, c, iq, target, false, filt_ptr, filt_idx, nnz, ic, C, rows_q, N, B, d, nullptr, t, valid, greater,
                             equal, (char*)ws + base, need > base ? need - base : 0, &m, stream);
        if (rc != GHF_OK) return rc;
        a.filt_ptr = m.ptr; a.filt_idx = m.idx;
        target = m.tpos; filt_ptr = m.ptr; filt_idx = m.idx;
    } else {
        score_prep_kernel<<<qb, 256, 0, stream>>>(q, c, iq, target, rows_q, N, B, d, t, valid, (long long*)greater, (long long*)equal);
        GHF_LAUNCH_CHECK();
    }
    if (bias) {
        rank_bias_target_kernel<<<qb, 256, 0, stream>>>(target_nodes, bias, valid, B, t);
        GHF_LAUNCH_CHECK();
    }
    a.t = t; a.greater = (unsigned long long*)greater; a.equal = (unsigned long long*)equal;
    rc = launch_rank_tiles<RK_RANK>(a, stream, ic, N, bias_c);
    if (rc != GHF_OK) return rc;
    if (nnz > 0 && bias) {
        rank_filter_bias_kernel<<<(unsigned)cdiv(nnz, 256), 256, 0, stream>>>(q, c, iq, target, filt_ptr, filt_idx, nnz, M, B, d, t,
                                                                             valid, a.greater, a.equal, ic, bias_c);
        GHF_LAUNCH_CHECK();
    } else if (nnz > 0) {
        rank_filter_kernel<<<(unsigned)cdiv(nnz, 256), 256, 0, stream>>>(q, c, iq, target, filt_ptr, filt_idx, nnz, M, B, d, t, valid,
                                                                        a.greater, a.equal, ic);
        GHF_LAUNCH_CHECK();
    }
    rank_finish_kernel<<<qb, 256, 0, stream>>>(t, valid, B, (long long*)greater, (long long*)equal, m.tpos);
    GHF_LAUNCH_CHECK();
    return GHF_OK;
}

int launch_score_topk(const float* q, const float* c, const int64_t* iq, const int64_t* filt_ptr, const int64_t* filt_idx,
                      int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d, int k, void* ws, size_t ws_bytes, float* scores,
                      int64_t* ids, hipStream_t stream, const int64_t* ic, int64_t C, const float* bias) {
    RankArgs a;
    const int64_t M = ic ? C : N;
    GHF_REQUIRE(k >= 1 && k <= TOPK_MAX_K, "score_topk: k = %d outside 1..%d", k, TOPK_MAX_K);
    GHF_REQUIRE(!ic || (C > 0 && C <= N), "score_topk: need 1 <= C <= N candidates");
    const size_t base = score_topk_workspace_bytes(B, M, d, k);
    const size_t need = ic ? score_topk_sub_workspace_bytes(B, C, d, k, nnz) : base;
    const size_t need_b = bias && ic && need ? need + rk_align((size_t)C * 4) : need;
    int rc = score_open("score_topk", rank_geom_topk, need_b, q, c, iq, filt_ptr, filt_idx, nnz, rows_q, M, B, d, ws_bytes, &a);
    if (rc != GHF_OK) return rc;
    const float* bias_c = bias;
    if (bias && ic) {
        GHF_REQUIRE(need > 0, "candidates: B or nnz out of range");
        bias_c = (float*)((char*)ws + need);
        rc = launch_cand_bias(bias, ic, C, N, (float*)((char*)ws + need), stream);
        if (rc != GHF_OK) return rc;
    }
    int* valid = (int*)ws;
    a.k = k; a.cap = topk_cap(d, k); a.ws_key = (uint64_t*)((char*)ws + rk_align((size_t)B * 4));
    if (ic) {
        CandMap m;
        rc = launch_cand_map(q, c, iq, nullptr, false, filt_ptr, filt_idx, nnz, ic, C, rows_q, N, B, d, nullptr, nullptr, valid,
                             nullptr, nullptr, (char*)ws + base, need > base ? need - base : 0, &m, stream);
        if (rc != GHF_OK) return rc;
        a.filt_ptr = m.ptr; a.filt_idx = m.idx;
    } else {
        score_prep_kernel<<<(unsigned)cdiv(B, 256), 256, 0, stream>>>(q, c, iq, nullptr, rows_q, N, B, d, nullptr, valid, nullptr, nullptr);
        GHF_LAUNCH_CHECK();
        if (nnz > 0) {
            list_range_kernel<<<(unsigned)cdiv(nnz, 256), 256, 0, stream>>>(filt_ptr, filt_idx, nnz, N, B, valid);
            GHF_LAUNCH_CHECK();
        }
    }
    rc = launch_rank_tiles<RK_TOPK>(a, stream, ic, N, bias_c);
    if (rc != GHF_OK) return rc;
    topk_merge_kernel<<<(unsigned)cdiv(B, 4), 256, 0, stream>>>(a.ws_key, valid, B, a.slabs, a.cap, k, scores, (long long*)ids, ic);
    GHF_LAUNCH_CHECK();
    return GHF_OK;
}

}  // namespace ghf
