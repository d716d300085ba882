/* ghf_distance.h — C ABI of libghf_hip.so, distance scores for per-query negative sets (csrc/distance.hip).
 *
 * A third header beside ghf.h and ghf_negatives.h, whose conventions and error codes it shares (device pointers owned by
 * the caller, inputs never written, every call enqueued on `stream`, a hipStream_t passed as void*; nothing allocates or
 * synchronises; 0 or a negative GHF_E* code, the message through ghf_last_error).  ghf.h, GHF_ABI_VERSION and
 * ghf_negatives.h are as they were: these entry points are additions that no existing caller sees.
 *
 * ghf_negatives.h scores query i against its own set neg[i, :] by the dot product q_i . c[v].  The calls below are the same
 * three operations and their backward under a DISTANCE, the score of the translational and rotational knowledge-graph
 * decoders (TransE: gamma - ||h + r - t||_1; RotatE: gamma - sum_k |h_k o r_k - t_k|, a complex modulus).  Everything that is
 * not restated here is ghf_negatives.h's, word for word: q, c, iq, target, the CSR filter lists, rows_q, N, B, d, scale; neg
 * [B, K] int64 with -1 "no entry", a multiset in the given order; the position set J_i; an invalid id makes its query alone
 * invalid (greater = equal = -1, loss = lse = lw = NaN, a NaN lse_or_lw[i] read as "no part": row i of coef and dq zero) and
 * no id is dereferenced before its range check; a query's outputs do not depend on its batch; no floating-point atomics, the
 * same call twice gives the same bits; d <= 256 (else GHF_EUNSUPPORTED), N < 2^31, B (K + 1) < 2^31.  There is no
 * per-candidate bias in these calls.
 *
 * With delta = q[iq[i]] - c[v] (one fp32 subtraction per element) and `metric` one of
 *
 *   GHF_DIST_L1       D(i, v) = sum_k |delta_k|                         g(i, v)_k = sign(delta_k), 0 at delta_k = 0
 *   GHF_DIST_L2       D(i, v) = sqrt(sum_k delta_k^2)                   g(i, v)_k = delta_k / D, all 0 where D = 0
 *   GHF_DIST_COMPLEX  D(i, v) = sum_p sqrt(delta_2p^2 + delta_2p+1^2)   g(i, v)_k = delta_k / rho_p, rho_p the modulus of k's
 *                     (re / im interleaved; d must be even, else        pair; both 0 where rho_p = 0
 *                     GHF_EINVAL)
 *
 * (g = dD / dq), the score of position j is s(i, j) = -D(i, n_ij) and the target's t_i = -D(i, target[i]), both formed by the
 * same code.  An unknown metric is GHF_EINVAL before anything is launched.
 *
 * ghf_dist_rank:        greater[i] = #{ j in J_i : s(i, j) > t_i }, equal[i] likewise with ==; int64 [B].
 * ghf_dist_softmax_fwd: ghf_neg_softmax_fwd's formulas with z = scale s; the target enters exactly once; J_i empty: loss
 *                       exactly 0.
 * ghf_dist_negsamp_fwd: ghf_neg_negsamp_fwd's formulas with z = scale s.  At scale = 1, margin = gamma the positive term
 *                       softplus(-(z_it + margin)) is -log sigmoid(gamma - D_t): RotatE's, as published.
 * ghf_dist_bwd:         mode GHF_DIST_SOFTMAX or GHF_DIST_NEGSAMP (the values of GHF_NEG_SOFTMAX / GHF_NEG_NEGSAMP); G_ij and
 *                       G_it exactly as ghf_neg_bwd defines them (gradients with respect to s, the weights detached);
 *                         coef [B, K + 1]: coef[i, j] = G_ij (0 outside J_i), coef[i, K] = G_it; every entry written; the
 *                                          same meaning under every metric
 *                         dq [B, d]:       dq[i] = -( sum_{j in J_i} G_ij g(i, n_ij) + G_it g(i, target[i]) ), positions
 *                                          ascending within a lane group, the target last; NOT scattered through iq
 *                       The gradient of c is  d c[v] = + sum_{(i, j): n_ij = v, j in J_i} G_ij g(i, v)
 *                                                      + sum_{i: target[i] = v} G_it g(i, v),
 *                       which is no multiple of q_i: ghf_segment_axpy cannot form it, ghf_dist_rows_grad does.
 * ghf_dist_rows_grad:   perm [B (K + 1)] and off [N + 1] are ghf_group_edges' outputs for the B (K + 1) node ids
 *                       [neg[i, :] | target[i]] of every query, a padding entry standing under its query's target (its
 *                       coefficient is 0).  Entry e belongs to query perm[e] / (K + 1), whose row is q[iq[.]] (q[.] without
 *                       iq).  dc [N, d] fp32:  dc[v] = sum_{e in off[v] .. off[v + 1]} coef[perm[e]] g(query of e, v),  e
 *                       ascending.  Every row of dc is written; an empty segment gives exact zeros; an entry whose
 *                       coefficient is 0 adds nothing, whatever its rows hold.  One wave per node: row v of c is read once
 *                       and kept in registers, a long segment is walked by its one wave, so the bits depend on the inputs
 *                       alone.  Values of perm, off and iq outside their ranges are skipped (off is clamped to
 *                       [0, B (K + 1)]), never dereferenced.  It takes no workspace.
 *
 * Accuracy — what is promised and no more.  The order of every sum depends on d and on the path alone: the vector path
 * (d % 4 == 0, q and c 16-byte aligned: a lane holds four adjacent floats) or the scalar path (a lane holds floats k, k + 64,
 * ...), chosen in the backward and in ghf_dist_rows_grad as in the forward.  L1 is exact where every difference and partial
 * sum is exactly representable.  The square roots are the hardware's (v_sqrt_f32, 1 ulp, not the IEEE sequence) and the
 * divisions of g are a multiplication by the hardware's reciprocal (v_rcp_f32, 1 ulp); a sum of squares in the subnormal
 * range may be read as 0, and g is then 0 by the rule above.  Equal arguments give equal bits: two candidates at the same
 * distance tie exactly, and that is all the rank counts rely on.
 *
 * workspace: ghf_dist_workspace_bytes(B, K, d, nnz) bytes, 256-byte aligned, one size for the four calls that take one; it
 * returns 0 for sizes the library cannot run (B, K or d < 1, nnz < 0, d > 256, B (K + 1) >= 2^31).  A workspace shorter
 * than that is GHF_EINVAL before anything is launched.  It is RESERVED AND NOT USED, as ghf_negatives.h's: one 256-byte
 * line that no kernel reads or writes. */
#ifndef GHF_DISTANCE_H
#define GHF_DISTANCE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GHF_DIST_L1 1
#define GHF_DIST_L2 2
#define GHF_DIST_COMPLEX 3

#define GHF_DIST_SOFTMAX 0
#define GHF_DIST_NEGSAMP 1

size_t ghf_dist_workspace_bytes(int64_t B, int64_t K, int d, int64_t nnz);
int ghf_dist_rank(int metric, const float* q, const float* c, const int64_t* iq, const int64_t* target,
                  const int64_t* filt_ptr, const int64_t* filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d,
                  const int64_t* neg /* [B, K] */, int64_t K, void* workspace, size_t workspace_bytes, int64_t* greater,
                  int64_t* equal, void* stream);
int ghf_dist_softmax_fwd(int metric, const float* q, const float* c, const int64_t* iq, const int64_t* target,
                         const int64_t* filt_ptr, const int64_t* filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B,
                         int d, float scale, const int64_t* neg /* [B, K] */, int64_t K, void* workspace,
                         size_t workspace_bytes, float* loss, float* lse, void* stream);
int ghf_dist_negsamp_fwd(int metric, const float* q, const float* c, const int64_t* iq, const int64_t* target,
                         const int64_t* filt_ptr, const int64_t* filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B,
                         int d, float scale, float margin, float adv_temperature, const int64_t* neg /* [B, K] */, int64_t K,
                         void* workspace, size_t workspace_bytes, float* loss, float* lw, void* stream);
int ghf_dist_bwd(int metric, int mode, const float* q, const float* c, const int64_t* iq, const int64_t* target,
                 const int64_t* filt_ptr, const int64_t* filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d,
                 float scale, float margin, float adv_temperature, const int64_t* neg /* [B, K] */, int64_t K,
                 const float* lse_or_lw, const float* grad_loss, void* workspace, size_t workspace_bytes, float* dq,
                 float* coef /* [B, K + 1] */, void* stream);
int ghf_dist_rows_grad(int metric, const float* q, const float* c, const int64_t* iq, int64_t rows_q, int64_t N, int64_t B,
                       int d, int64_t K, const float* coef /* [B, K + 1] */, const int64_t* perm /* [B (K + 1)] */,
                       const int64_t* off /* [N + 1] */, float* dc /* [N, d] */, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* GHF_DISTANCE_H */
