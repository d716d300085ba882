// bce.hip — the multi-label 1-vs-all binary cross-entropy link-prediction loss against every node (the 1-N objective of ConvE,
// TuckER, CompGCN), forward; the B x N logits and labels never stored (include/ghf.h: ghf_score_bce_fwd / ghf_score_bce_bwd;
// DESIGN.md §14).  With z_ij = scale s(i, j), s the sweep's fp32 chain (rank_sweep.h), and P_i the ids of query i's list:
//
//   y_ij    = (1 - smoothing) [j in P_i] + smoothing / N
//   loss[i] = sum_j softplus(z_ij) - (1 - smoothing) sum_{j in P_i} z_ij - (smoothing / N) sum_j z_ij
//           = binary_cross_entropy_with_logits(z_i, y_i, reduction = "sum")
//
// Forward: rank_tile_kernel with its fourth epilogue.  A lane keeps three running sums per query column (softplus(z), z over
// the listed candidates, z) and folds a finished candidate tile's 32 registers of that column into them.  The list is walked
// by the softmax epilogue's cursor: a full tile without a listed id touches no memory, the others look every id up (a hit
// adds z to the positive sum; membership, so a repeated id counts once).  Candidates past N are left out, never scored as
// zero rows: softplus(0) = ln 2.  softplus keeps its tail: log(1 + t) is a short series below t = 2^-6 (rank_sweep.h).
// Partials merge as the softmax's: half-waves and waves through LDS, one triple per (query, slab) in the workspace,
// bce_finish_kernel over the slabs in slab order; the slabs are softmax_geom's (N and d alone), so a query's loss has the
// same bits whatever batch it is in.
//
// Backward: softmax_bwd_kernel with LOSS = SB_BCE (softmax.hip, which holds launch_score_bce_bwd).
#include "common.h"
#include "rank_sweep.h"

namespace ghf {

size_t score_bce_workspace_bytes(int64_t B, int64_t N, int d) {
    RankGeom g;
    if (d <= 0 || d > RK_MAX_D || !softmax_geom(B, N, d, &g)) return 0;
    // valid [B] int32, (softplus, positive z, z) [B, slabs]
    return rk_align((size_t)B * 4) + rk_align((size_t)B * (size_t)g.slabs * 12);
}

// a candidate subset (candidates.hip): the all-node workspace for N := C, then the id map's
size_t score_bce_sub_workspace_bytes(int64_t B, int64_t C, int d, int64_t nnz) {
    const size_t base = score_bce_workspace_bytes(B, C, d), map = cand_workspace_bytes(B, nnz);
    return base && map ? base + map : 0;
}

// with a per-candidate bias: C = 0 is the all-node call (no id map), C > 0 adds the subset's gathered bias [C]
size_t score_bce_b_workspace_bytes(int64_t B, int64_t N, int64_t C, int d, int64_t nnz) {
    if (C <= 0) return score_bce_workspace_bytes(B, N, d);
    const size_t base = score_bce_sub_workspace_bytes(B, C, d, nnz);
    return base ? base + rk_align((size_t)C * 4) : 0;
}

__global__ __launch_bounds__(256) void bce_finish_kernel(const float* __restrict__ part, const int* __restrict__ valid, int64_t B,
                                                         int64_t slabs, float pos_w, float neg_w, float* __restrict__ loss) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= B) return;
    const float* p = part + (size_t)i * slabs * 3;
    float sp = 0.f, pos = 0.f, sz = 0.f;
    for (int64_t s = 0; s < slabs; ++s) {
        sp += p[3 * s];
        pos += p[3 * s + 1];
        sz += p[3 * s + 2];
    }
    loss[i] = valid[i] ? (sp - pos_w * pos) - neg_w * sz : __int_as_float(0x7FC00000);
}

int launch_score_bce_fwd(const float* q, const float* c, const int64_t* iq, const int64_t* pos_ptr, const int64_t* pos_idx,
                         int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d, float scale, float smoothing, void* ws,
                         size_t ws_bytes, float* loss, hipStream_t stream, const int64_t* ic, int64_t C, const float* bias) {
    RankArgs a;
    const int64_t M = ic ? C : N;                    // the candidates the sweep runs over, and the labels' smoothing / M
    GHF_REQUIRE(!ic || (C > 0 && C <= N), "score_bce_fwd: need 1 <= C <= N candidates");
    const size_t base = score_bce_workspace_bytes(B, M, d);
    const size_t need = ic ? score_bce_sub_workspace_bytes(B, C, d, nnz) : base;      // with a bias over a subset: + its [C] floats
    const size_t need_b = bias && ic && need ? need + rk_align((size_t)C * 4) : need;
    int rc = score_open("score_bce_fwd", softmax_geom, need_b, q, c, iq, pos_ptr, pos_idx, nnz, rows_q, M, B, d, ws_bytes, &a);
    if (rc != GHF_OK) return rc;
    const float* bias_c = bias;                      // the bias in the sweep's candidate space
    if (bias && ic) {
        GHF_REQUIRE(need > 0, "candidates: B or nnz out of range");
        bias_c = (float*)((char*)ws + need);
        rc = launch_cand_bias(bias, ic, C, N, (float*)((char*)ws + need), stream);
        if (rc != GHF_OK) return rc;
    }
    int* valid = (int*)ws;
    const unsigned qb = (unsigned)cdiv(B, 256);
    if (ic) {
        CandMap m;
        rc = launch_cand_map(q, c, iq, nullptr, false, pos_ptr, pos_idx, nnz, ic, C, rows_q, N, B, d, nullptr, nullptr, valid, nullptr,
                             nullptr, (char*)ws + base, need > base ? need - base : 0, &m, stream);
        if (rc != GHF_OK) return rc;
        a.filt_ptr = m.ptr; a.filt_idx = m.idx;
    } else {
        // a query whose row id is out of range takes no part; list_range_kernel then clears the queries with a bad list id
        score_prep_kernel<<<qb, 256, 0, stream>>>(q, c, iq, nullptr, rows_q, N, B, d, nullptr, valid, nullptr, nullptr);
        GHF_LAUNCH_CHECK();
        if (nnz > 0) {
            list_range_kernel<<<(unsigned)cdiv(nnz, 256), 256, 0, stream>>>(pos_ptr, pos_idx, nnz, N, B, valid);
            GHF_LAUNCH_CHECK();
        }
    }
    a.scale = scale; a.ws_bce = (float*)((char*)ws + rk_align((size_t)B * 4));
    rc = launch_rank_tiles<RK_BCE>(a, stream, ic, N, bias_c);
    if (rc != GHF_OK) return rc;
    bce_finish_kernel<<<qb, 256, 0, stream>>>(a.ws_bce, valid, B, a.slabs, 1.f - smoothing, smoothing / (float)M, loss);
    GHF_LAUNCH_CHECK();
    return GHF_OK;
}

}  // namespace ghf
