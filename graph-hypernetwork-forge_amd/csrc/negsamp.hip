// negsamp.hip — the negative-sampling link-prediction loss with self-adversarial weighting (RotatE; PyKEEN's NSSALoss; the
// DGL-KE and OGB wikikg2 / biokg baselines) against every node or a candidate subset, forward; the B x C logits, weights and
// softplus terms never stored (include/ghf.h: ghf_score_negsamp_fwd / ghf_score_negsamp_bwd).  With
// z_ij = scale s(i, j) (+ bias[j]), s the sweep's fp32 chain (rank_sweep.h), J_i the candidates outside query i's list other
// than its target, gamma the margin and alpha >= 0 the adversarial temperature:
//
//   lw[i]   = log sum_{j in J_i} exp(alpha z_ij)                       (-inf when J_i is empty)
//   w_ij    = exp(alpha z_ij - lw[i])                                  (alpha = 0: 1 / |J_i|)
//   loss[i] = softplus(-(z_it + gamma)) + sum_{j in J_i} w_ij softplus(z_ij + gamma)
//
// Forward: rank_tile_kernel with its fifth epilogue.  A lane keeps a triple per query column — the running max of alpha z,
// S = sum exp(alpha z - max) and T = sum exp(alpha z - max) softplus(z + gamma) — and folds a finished candidate tile's 32
// registers of that column into it, both sums rescaled when the max rises (an online softmax whose value is a weighted sum).
// A listed candidate, the target and a candidate past N never enter; the list is walked by the softmax epilogue's cursor, and
// a full tile whose id range holds neither a listed id nor the target touches no memory.  Partials merge as the BCE's
// triples: half-waves and waves through LDS, one triple per (query, slab) in the workspace, negsamp_finish_kernel over the
// slabs in slab order, where loss = softplus(-(z_it + gamma)) + T / S and lw = max + log S.  The slabs are softmax_geom's (N
// and d alone): a query's loss has the same bits whatever batch it is in.  No floating-point atomics.
//
// Backward: softmax_bwd_kernel with LOSS = SB_NEGSAMP (softmax.hip, which holds launch_score_negsamp_bwd); the weights are
// constants there (detached), as in RotatE and PyKEEN.
#include "common.h"
#include "rank_sweep.h"

namespace ghf {

// C <= 0: every node.  C > 0: the subset's sweep over C candidates, the id map, and room for a gathered bias [C] (asked for
// whether or not the call has one: one size per shape)
size_t score_negsamp_workspace_bytes(int64_t B, int64_t N, int64_t C, int d, int64_t nnz) {
    RankGeom g;
    const int64_t M = C > 0 ? C : N;
    if (d <= 0 || d > RK_MAX_D || C > N || !softmax_geom(B, M, d, &g)) return 0;
    // t [B] float, valid [B] int32, (max, S, T) [B, slabs]
    const size_t base = 2 * rk_align((size_t)B * 4) + rk_align((size_t)B * (size_t)g.slabs * 12);
    if (C <= 0) return base;
    const size_t map = cand_workspace_bytes(B, nnz);
    return map ? base + map + rk_align((size_t)C * 4) : 0;
}

// target and bias in node ids (a query that is not valid may hold any target)
__global__ __launch_bounds__(256) void negsamp_finish_kernel(const float* __restrict__ part, const float* __restrict__ t,
                                                             const int* __restrict__ valid, int64_t B, int64_t slabs, float scale,
                                                             float margin, const int64_t* __restrict__ target,
                                                             const float* __restrict__ bias, float* __restrict__ loss,
                                                             float* __restrict__ lw) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= B) return;
    const float* p = part + (size_t)i * slabs * 3;
    NegTriple m = {p[0], p[1], p[2]};
    for (int64_t s = 1; s < slabs; ++s) m = neg_merge(m, NegTriple{p[3 * s], p[3 * s + 1], p[3 * s + 2]});
    float l = __int_as_float(0x7FC00000), w = l;
    if (valid[i]) {
#pragma clang fp contract(off)                           // z_it is rounded before the margin is added, as the sweep's logits
        const float zt = bias ? fmaf(scale, t[i], bias[target[i]]) : scale * t[i];
        const bool any = m.s > 0.f;                      // a query without negatives: the positive term alone, lw = -inf
        w = any ? m.m + logf(m.s) : -INFINITY;
        l = softplus(-(zt + margin)) + (any ? m.t / m.s : 0.f);
    }
    loss[i] = l;
    lw[i] = w;
}

int launch_score_negsamp_fwd(const float* q, const float* c, const int64_t* iq, const int64_t* target, const int64_t* filt_ptr,
                             const int64_t* filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d, float scale,
                             float margin, float alpha, const int64_t* ic, int64_t C, const float* bias, void* ws, size_t ws_bytes,
                             float* loss, float* lw, hipStream_t stream) {
    RankArgs a;
    const int64_t M = ic ? C : N;                    // the candidates the sweep runs over
    GHF_REQUIRE(ic ? (C > 0 && C <= N) : C == 0, "score_negsamp_fwd: need ic and 1 <= C <= N, or ic = NULL and C = 0");
    const size_t base = score_negsamp_workspace_bytes(B, M, 0, d, 0);
    const size_t need = score_negsamp_workspace_bytes(B, N, C, d, nnz);
    int rc = score_open("score_negsamp_fwd", softmax_geom, need, q, c, iq, filt_ptr, filt_idx, nnz, rows_q, M, B, d, ws_bytes, &a);
    if (rc != GHF_OK) return rc;
    GHF_REQUIRE(need > 0, "score_negsamp_fwd: B or nnz out of range");
    const size_t map_bytes = ic ? need - base - rk_align((size_t)C * 4) : 0;
    const float* bias_c = bias;                      // the bias in the sweep's candidate space
    if (bias && ic) {
        float* gathered = (float*)((char*)ws + base + map_bytes);
        bias_c = gathered;
        rc = launch_cand_bias(bias, ic, C, N, gathered, stream);
        if (rc != GHF_OK) return rc;
    }
    const int64_t* tpos = target;                    // the targets in the sweep's candidate space
    float* t = (float*)ws;
    int* valid = (int*)((char*)ws + rk_align((size_t)B * 4));
    const unsigned qb = (unsigned)cdiv(B, 256);
    if (ic) {                                        // a target that is no candidate: the query is not valid
        CandMap m;
        rc = launch_cand_map(q, c, iq, target, true, filt_ptr, filt_idx, nnz, ic, C, rows_q, N, B, d, nullptr, t, valid, nullptr,
                             nullptr, (char*)ws + base, map_bytes, &m, stream);
        if (rc != GHF_OK) return rc;
        a.filt_ptr = m.ptr; a.filt_idx = m.idx;
        tpos = m.tpos;
    } else {
        score_prep_kernel<<<qb, 256, 0, stream>>>(q, c, iq, target, rows_q, N, B, d, t, valid, nullptr, nullptr);
        GHF_LAUNCH_CHECK();
        if (nnz > 0) {
            list_range_kernel<<<(unsigned)cdiv(nnz, 256), 256, 0, stream>>>(filt_ptr, filt_idx, nnz, N, B, valid);
            GHF_LAUNCH_CHECK();
        }
    }
    a.target = tpos; a.scale = scale; a.ws_bce = (float*)((char*)ws + 2 * rk_align((size_t)B * 4));
    rc = launch_rank_tiles<RK_NEGSAMP>(a, stream, ic, N, bias_c, margin, alpha);
    if (rc != GHF_OK) return rc;
    negsamp_finish_kernel<<<qb, 256, 0, stream>>>(a.ws_bce, t, valid, B, a.slabs, scale, margin, target, bias, loss, lw);
    GHF_LAUNCH_CHECK();
    return GHF_OK;
}

}  // namespace ghf
