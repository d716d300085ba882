/* ghf_negatives.h — C ABI of libghf_hip.so, per-query negative sets (csrc/negatives.hip).
 *
 * A header of its own beside ghf.h, whose conventions and error codes it shares (device pointers owned by the caller,
 * inputs never written, every call enqueued on `stream`, a hipStream_t passed as void*; nothing allocates or
 * synchronises; 0 or a negative GHF_E* code, the message through ghf_last_error).  ghf.h and GHF_ABI_VERSION are as
 * they were: these entry points are additions that no existing caller sees.
 *
 * The scorers of ghf.h score a batch against ONE candidate set shared by all queries (every node, or ic [C]).  The
 * calls below score query i against ITS OWN set, row i of `neg` [B, K] int64, K >= 1: the K negatives per positive of
 * RotatE's and PyKEEN's samplers, the given 500 / 1,000 negatives per test triple of OGB wikikg2 / biokg / citation2.
 *
 * neg[i, j] is a node id in [0, N) or exactly -1, "no entry" (padding: ragged sets).  A row is a MULTISET IN THE
 * GIVEN ORDER: an id that occurs three times counts three times, as in F.cross_entropy(logits.gather(...)); nothing is
 * sorted or de-duplicated (unlike ic).  q, c, iq, target, the filter lists (CSR, each list ascending), rows_q, N, B, d
 * and scale are ghf_score_softmax_fwd's; bias [N] fp32 is the _b calls', or NULL for none.  With n_ij = neg[i, j],
 * list_i query i's filter list and
 *   J_i = { j < K : n_ij != -1, n_ij not in list_i, n_ij != target[i] }                    (a set of POSITIONS)
 *   s(i, j) = q[iq[i]] . c[n_ij]      fp32, summed in an order that depends on d (and on whether the rows can be read in
 *                                     16-byte pieces: d % 4 == 0, q and c 16-byte aligned) alone; NOT the matrix
 *                                     instruction's chain of the all-node sweeps — the two agree to rounding, and exactly
 *                                     where every product and partial sum is exact.  The target's score t_i is formed
 *                                     the same way from row target[i] of c.
 *
 * ghf_neg_rank:        greater[i] = #{ j in J_i : s(i, j) + bias[n_ij] > t_i + bias[target[i]] }, equal[i] likewise with
 *                      ==; int64 [B]; the bias one fp32 add behind the dot product; NaN counts in neither.
 * ghf_neg_softmax_fwd: z_ij = scale s(i, j), or fmaf(scale, s(i, j), bias[n_ij]) (the bias NOT multiplied by scale);
 *                      lse[i] = log(exp(z_it) + sum_{j in J_i} exp(z_ij)) — the target enters exactly once and always —
 *                      loss[i] = lse[i] - z_it; fp32 [B].  J_i empty: loss[i] is exactly 0.
 * ghf_neg_negsamp_fwd: ghf_score_negsamp_fwd's formulas over this J_i (margin finite, adv_temperature = alpha finite and
 *                      >= 0, the bias finite):  lw[i] = log sum_{J_i} exp(alpha z_ij)  (-inf when J_i is empty),
 *                      loss[i] = softplus(-(z_it + margin)) + sum_{J_i} exp(alpha z_ij - lw[i]) softplus(z_ij + margin);
 *                      J_i empty: the positive term alone.
 * ghf_neg_bwd:         mode GHF_NEG_SOFTMAX or GHF_NEG_NEGSAMP, lse_or_lw [B] the matching forward's second output,
 *                      grad_loss [B].  Per POSITION:
 *                        softmax:  G_ij = grad_i scale exp(z_ij - lse_i) on J_i,   G_it = grad_i scale (exp(z_it - lse_i) - 1)
 *                        negsamp:  G_ij = grad_i scale w_ij sigmoid(z_ij + margin) on J_i, w_ij = exp(alpha z_ij - lw_i) A
 *                                  CONSTANT (detached),   G_it = -grad_i scale sigmoid(-(z_it + margin))
 *                      coef [B, K + 1] fp32: coef[i, j] = G_ij (0 outside J_i), coef[i, K] = G_it; every entry written.
 *                      dq [B, d] fp32: dq[i] = sum_j G_ij c[n_ij] (j ascending) + G_it c[target[i]], NOT scattered
 *                      through iq.  margin and adv_temperature are ignored in softmax mode.  The gradient of c is
 *                      sum_{(i, j): n_ij = v} G_ij q[iq[i]] + sum_{i: target[i] = v} G_it q[iq[i]] — ghf_group_edges over
 *                      the B (K + 1) node ids and ghf_segment_axpy with coef, as for ghf_score_pairs_fwd's gradient — and
 *                      the bias's the same sum of coef / scale.
 *
 * A query whose iq / target / list id is outside its range, or with an entry of neg that is neither -1 nor in [0, N),
 * is invalid: greater = equal = -1, loss = lse = lw = NaN; the backward reads a NaN lse_or_lw[i] as "no part" (row i of
 * coef and dq all zero) and an lw[i] of -inf as "the target entry alone".  No id is dereferenced before its range check;
 * nothing faults.  The other queries are unaffected.
 *
 * A query is owned by one wave, or by the four waves of one workgroup where K > 256 — a number chosen from K alone: its
 * outputs (and dq) depend on its own row of q, its negatives in their order, its list, K and d, not on the batch or its
 * place in it.  No floating-point atomics, every sum in a fixed order: the
 * same call twice gives the same bits.
 *
 * workspace: ghf_neg_workspace_bytes(B, K, d, nnz) bytes, 256-byte aligned, one size for all four calls; it returns 0 for
 * sizes the library cannot run (B, K or d < 1, nnz < 0, d > 256, B (K + 1) >= 2^31).  A workspace shorter than that is
 * GHF_EINVAL before anything is launched.  It is RESERVED AND NOT USED: today it is one 256-byte line that no kernel reads
 * or writes, it carries nothing from the forward to the backward, and any buffer of that size serves every call.
 * Limits: d > 256 is GHF_EUNSUPPORTED; N >= 2^31 is GHF_EINVAL (the query is not told N: the kernels keep ids in 32 bits).
 * The summation order of s(i, j) is chosen from d and the alignment of q and c, in the backward as in the forward; a dq that
 * is not 16-byte aligned is written with narrower stores and changes no sum. */
#ifndef GHF_NEGATIVES_H
#define GHF_NEGATIVES_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GHF_NEG_SOFTMAX 0
#define GHF_NEG_NEGSAMP 1

size_t ghf_neg_workspace_bytes(int64_t B, int64_t K, int d, int64_t nnz);
int ghf_neg_rank(const float* q, const float* c, const int64_t* iq, const int64_t* target, const int64_t* filt_ptr,
                 const int64_t* filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d,
                 const int64_t* neg /* [B, K] */, int64_t K, const float* bias, void* workspace, size_t workspace_bytes,
                 int64_t* greater, int64_t* equal, void* stream);
int ghf_neg_softmax_fwd(const float* q, const float* c, const int64_t* iq, const int64_t* target, const int64_t* filt_ptr,
                        const int64_t* filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d, float scale,
                        const int64_t* neg /* [B, K] */, int64_t K, const float* bias, void* workspace,
                        size_t workspace_bytes, float* loss, float* lse, void* stream);
int ghf_neg_negsamp_fwd(const float* q, const float* c, const int64_t* iq, const int64_t* target, const int64_t* filt_ptr,
                        const int64_t* filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d, float scale,
                        float margin, float adv_temperature, const int64_t* neg /* [B, K] */, int64_t K, const float* bias,
                        void* workspace, size_t workspace_bytes, float* loss, float* lw, void* stream);
int ghf_neg_bwd(int mode, const float* q, const float* c, const int64_t* iq, const int64_t* target, const int64_t* filt_ptr,
                const int64_t* filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d, float scale, float margin,
                float adv_temperature, const int64_t* neg /* [B, K] */, int64_t K, const float* bias,
                const float* lse_or_lw, const float* grad_loss, void* workspace, size_t workspace_bytes, float* dq,
                float* coef /* [B, K + 1] */, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* GHF_NEGATIVES_H */
