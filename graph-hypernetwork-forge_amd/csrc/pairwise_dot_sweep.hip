// pairwise_dot_sweep.hip — the pairwise ranking losses (hinge, logistic / BPR) by DOT PRODUCT against every node or a shared
// candidate subset, forward; the B x C scores, ids and coefficients never stored (include/ghf_pairwise_dot_sweep.h; DESIGN.md
// §28).  With z_ij = scale s(i, j) (+ bias[j]), s the sweep's fp32 chain (rank_sweep.h), J_i the candidates outside query i's
// list other than its target, and u_ij = (z_ij - z_it) + margin:
//
//   loss[i] = sum_{j in J_i} phi(u_ij) (/ n_i),   dsum[i] = sum_{j in J_i} phi'(u_ij),   count[i] = n_i,   active[i] = #{u_ij > 0}
//
// Forward: rank_tile_kernel with its sixth epilogue (RK_PAIR).  The target's z_it is known before the tiles start: t[i] comes
// from score_prep_kernel / launch_cand_map by the sweep's chain, pair_zt_kernel turns it into the logit the tile forms for that
// pair.  A lane keeps (sum phi, sum phi', n, active) per query column and folds a finished candidate tile's 32 registers of that
// column into them; a listed candidate, the target and a candidate past N add +0.f and 0 by select; the list is walked by the
// softmax epilogue's cursor, and a full tile whose id range holds neither a listed id nor the target touches no memory.
// Partials merge as the BCE's triples: half-waves and waves through LDS, one 16-byte partial per (query, slab) in the
// workspace, pair_finish_kernel over the slabs in slab order.  The slabs are softmax_geom's (the candidate count and d alone):
// a query's results have the same bits whatever batch it is in.  No floating-point atomics.  The public `kind` becomes the
// template flag HINGE once, in launch_score_pair_fwd's caller, and nothing else.
//
// Backward: softmax_bwd_kernel with LOSS = SB_PAIR (softmax.hip, which holds launch_score_pair_bwd).
#include "common.h"
#include "rank_sweep.h"

namespace ghf {

// the checks of both launches past the entry points' own, in the header's order; `need` is the call's *_workspace_bytes
int score_pair_open(const char* op, size_t need, const int64_t* iq, int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d,
                    const int64_t* ic, int64_t C, size_t ws_bytes) {
    GHF_REQUIRE(d > 0 && rows_q > 0 && N > 0 && B > 0 && nnz >= 0, "%s: bad shape", op);
    GHF_REQUIRE(iq || B <= rows_q, "%s: B exceeds the rows of q", op);
    GHF_REQUIRE(ic ? (C > 0 && C <= N) : C == 0, "%s: need ic and 1 <= C <= N, or ic = NULL and C = 0", op);
    GHF_REQUIRE(N < (int64_t)1 << 31, "%s: N = %lld rows, the sweep keeps row ids in 32 bits", op, (long long)N);
    GHF_REQUIRE(rows_q < (int64_t)1 << 31, "%s: rows_q = %lld rows of q, the sweep keeps row ids in 32 bits", op, (long long)rows_q);
    GHF_REQUIRE(B < (int64_t)1 << 31, "%s: B out of range", op);
    if (d > RK_MAX_D) return set_err(GHF_EUNSUPPORTED, "%s: d = %d exceeds %d", op, d, RK_MAX_D);
    GHF_REQUIRE(need > 0 && ws_bytes >= need, "%s: workspace of %zu bytes, need %zu", op, ws_bytes, need);
    return GHF_OK;
}

// C <= 0: every node.  C > 0: the subset's sweep over C candidates, the id map, and room for a gathered bias [C] (asked for
// whether or not the call has one: one size per shape)
size_t score_pair_workspace_bytes(int64_t B, int64_t N, int64_t C, int d, int64_t nnz) {
    RankGeom g;
    const int64_t M = C > 0 ? C : N;
    if (d <= 0 || d > RK_MAX_D || C < 0 || C > N || nnz < 0 || !softmax_geom(B, M, d, &g)) return 0;
    // t -> z_it [B] float, valid [B] int32, (sum phi, sum phi', n, active) [B, slabs]
    const size_t base = 2 * rk_align((size_t)B * 4) + rk_align((size_t)B * (size_t)g.slabs * sizeof(PairPart));
    if (C <= 0) return base;
    const size_t map = cand_workspace_bytes(B, nnz);
    return map ? base + map + rk_align((size_t)C * 4) : 0;
}

// one thread per query, behind the pass that formed t: the target's logit as the tile forms it, in place (target and bias in
// node ids; a query that is not valid keeps its NaN and may hold any target)
__global__ __launch_bounds__(256) void pair_zt_kernel(float* __restrict__ t, const int* __restrict__ valid, int64_t B, float scale,
                                                      const int64_t* __restrict__ target, const float* __restrict__ bias) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= B) return;
    float z = __int_as_float(0x7FC00000);
    if (valid[i]) z = bias ? fmaf(scale, t[i], bias[target[i]]) : scale * t[i];
    t[i] = z;
}

int launch_pair_zt(float* t, const int* valid, int64_t B, float scale, const int64_t* target, const float* bias, hipStream_t stream) {
    pair_zt_kernel<<<(unsigned)cdiv(B, 256), 256, 0, stream>>>(t, valid, B, scale, target, bias);
    GHF_LAUNCH_CHECK();
    return GHF_OK;
}

// one thread per query: the slabs' partials in slab order, then the outputs
__global__ __launch_bounds__(256) void pair_finish_kernel(const PairPart* __restrict__ part, const int* __restrict__ valid, int64_t B,
                                                          int64_t slabs, int hinge, int normalize, float* __restrict__ loss,
                                                          float* __restrict__ dsum, int* __restrict__ count, int* __restrict__ active) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= B) return;
    const PairPart* p = part + (size_t)i * slabs;
    PairPart m = p[0];
    for (int64_t s = 1; s < slabs; ++s) {
        m.f += p[s].f;
        m.g += p[s].g;
        m.n += p[s].n;
        m.a += p[s].a;
    }
    float l = m.f;
    if (normalize) l = m.n > 0 ? m.f * (1.f / (float)m.n) : 0.f;
    if (m.n <= 0) l = 0.f;                           // an empty J_i: exactly 0
    const bool ok = valid[i] != 0;
    loss[i] = ok ? l : __int_as_float(0x7FC00000);
    dsum[i] = ok ? (hinge ? (float)m.a : m.g) : __int_as_float(0x7FC00000);
    count[i] = ok ? m.n : -1;
    active[i] = ok ? m.a : -1;
}

int launch_score_pair_fwd(bool hinge, const float* q, const float* c, const int64_t* iq, const int64_t* target,
                          const int64_t* filt_ptr, const int64_t* filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d,
                          float scale, float margin, int normalize, const int64_t* ic, int64_t C, const float* bias, void* ws,
                          size_t ws_bytes, float* loss, float* dsum, int* count, int* active, hipStream_t stream) {
    const int64_t M = ic ? C : N;                    // the candidates the sweep runs over
    const bool sizes = d > 0 && d <= RK_MAX_D && B > 0 && N > 0;
    const size_t need = sizes ? score_pair_workspace_bytes(B, N, ic ? C : 0, d, nnz) : 0;
    int rc = score_pair_open("score_pair_fwd", need, iq, nnz, rows_q, N, B, d, ic, C, ws_bytes);
    if (rc != GHF_OK) return rc;
    RankArgs a;
    rc = score_open("score_pair_fwd", softmax_geom, need, q, c, iq, filt_ptr, filt_idx, nnz, rows_q, M, B, d, ws_bytes, &a);
    if (rc != GHF_OK) return rc;
    const size_t base = score_pair_workspace_bytes(B, M, 0, d, 0);
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
    rc = launch_pair_zt(t, valid, B, scale, target, bias, stream);
    if (rc != GHF_OK) return rc;
    RankPairArgs s = {};
    static_cast<RankArgs&>(s) = a;
    s.target = tpos; s.scale = scale; s.margin = margin; s.zt = t;
    s.ws_pair = (PairPart*)((char*)ws + 2 * rk_align((size_t)B * 4));
    rc = hinge ? launch_rank_pair_tiles<true>(s, stream, ic, N, bias_c) : launch_rank_pair_tiles<false>(s, stream, ic, N, bias_c);
    if (rc != GHF_OK) return rc;
    pair_finish_kernel<<<qb, 256, 0, stream>>>(s.ws_pair, valid, B, a.slabs, hinge ? 1 : 0, normalize, loss, dsum, count, active);
    GHF_LAUNCH_CHECK();
    return GHF_OK;
}

}  // namespace ghf
