/* ghf_pairwise.h — C ABI of libghf_hip.so, pairwise ranking losses (hinge, logistic / BPR) on per-query negative sets
 * (csrc/pairwise.hip).
 *
 * A sixth header beside ghf.h, ghf_negatives.h, ghf_distance.h, ghf_distance_sweep.h and ghf_distance_loss.h, whose
 * conventions and error codes it shares (device pointers owned by the caller, inputs never written, every call enqueued on
 * `stream`, a hipStream_t passed as void*; nothing allocates or synchronises; 0 or a negative GHF_E* code, the message
 * through ghf_last_error).  The five older headers and GHF_ABI_VERSION are as they were: these entry points are additions
 * that no existing caller sees.
 *
 * Everything that is not restated here is ghf_negatives.h's and ghf_distance.h's, word for word: q, c, iq, target, the CSR
 * filter lists, rows_q, N, B, d, scale; neg [B, K] int64 with -1 "no entry", a multiset in the given order; the position set
 * J_i (not -1, not the target, not listed); an invalid id makes its query alone invalid and no id is dereferenced before its
 * range check; a query's bits do not depend on its batch; no floating-point atomics, the same call twice gives the same bits;
 * d <= 256 (else GHF_EUNSUPPORTED), N < 2^31, B (K + 1) < 2^31.
 *
 * `metric` chooses the score: GHF_PAIR_DOT, s(i, j) = q[iq[i]] . c[n_ij] formed by the code of ghf_neg_rank, with `bias`
 * (fp32 [N] or NULL) entering as z = fmaf(scale, s, bias[n_ij]); or GHF_DIST_L1 / GHF_DIST_L2 / GHF_DIST_COMPLEX of
 * ghf_distance.h, s(i, j) = -D(i, n_ij) formed by the code of ghf_dist_rank, without a bias.  The target's t_i likewise.
 * `kind` chooses the loss.  With
 *
 *   z_ij = scale s(i, j)                         z_it = scale t_i      (dot with a bias: the fmaf above, the target too)
 *   u_ij = (z_ij - z_it) + margin                two fp32 operations in this order, not contracted
 *   GHF_PAIR_HINGE     phi(u) = u > 0 ? u : 0    (a NaN u stays NaN)   phi'(u) = u > 0 ? 1 : 0
 *   GHF_PAIR_LOGISTIC  phi(u) = softplus(u)                            phi'(u) = sigmoid(u)
 *   n_i = |J_i|
 *
 * ghf_pair_fwd:  loss[i]   = (normalize ? 1 / n_i : 1) sum_{j in J_i} phi(u_ij)   fp32 [B]; exactly 0 when J_i is empty
 *                count[i]  = n_i                                                 int32 [B]
 *                active[i] = #{ j in J_i : u_ij > 0 }                            int32 [B]: the violated pairs; at margin = 0
 *                                                                                and scale = 1 it is ghf_neg_rank's /
 *                                                                                ghf_dist_rank's greater[i]
 *                An invalid query has loss NaN and count = active = -1.
 *                Hinge at scale = 1 under GHF_DIST_L1 is max(0, margin + D(h + r, t) - D(h + r, t')): TransE's published loss,
 *                with q the translated rows.  Logistic at margin = 0 under GHF_PAIR_DOT is BPR.
 * ghf_pair_bwd:  `count` is the forward's.  With w_i = grad_loss[i] scale (normalize ? 1 / count[i] : 1):
 *                  G_ij = w_i phi'(u_ij) on J_i, 0 elsewhere;  G_it = -sum_j G_ij
 *                  coef [B, K + 1]: coef[i, j] = G_ij, coef[i, K] = G_it; every entry written
 *                  dq [B, d]: exactly as ghf_neg_bwd and ghf_dist_bwd define it from G — dot: sum_j G_ij c[n_ij] + G_it
 *                             c[target[i]]; distance: -(sum_j G_ij g(i, n_ij) + G_it g(i, target[i])) — positions
 *                             ascending within a lane group, the target last; NOT scattered through iq
 *                count[i] == -1: the query takes no part, row i of coef and of dq is zero.  count[i] == 0: likewise zero.
 *                The sum behind G_it has a fixed order that depends on K, d and the load path alone: a group of L lanes
 *                (L = 8, 16, 32, 64 for d <= 32, 64, 128, 256 on the vector path; 64 on the scalar path) adds the
 *                coefficients of its positions j, j + 64 / L steps apart, ascending; the 64 / L groups merge by a butterfly
 *                (partner group g ^ 1, then g ^ 2, ...); for K > 256 the positions are dealt to four waves in steps of
 *                8 * 64 / L and the four sums are added in wave order.
 *                The gradient of c (and of the bias: coef / scale) is formed from coef by ghf_group_edges +
 *                ghf_segment_axpy under GHF_PAIR_DOT and by ghf_dist_rows_grad under a distance, unchanged.
 *
 * Refusals, in this order, all before anything is launched: an unknown metric or an odd d under GHF_DIST_COMPLEX; an
 * unknown kind; a scale that is not finite and positive; a margin that is not finite; normalize outside {0, 1}; a bias
 * together with a distance (all GHF_EINVAL); then the per-query calls' own: null pointers, the lists, the workspace's
 * alignment, K < 1, the shape, d > 256 (GHF_EUNSUPPORTED), N, the workspace's size.
 *
 * workspace: ghf_pair_workspace_bytes(B, K, d, nnz) bytes, 256-byte aligned; 0 for sizes the library cannot run (B, K or
 * d < 1, nnz < 0, d > 256, B (K + 1) >= 2^31).  RESERVED AND NOT USED, as ghf_negatives.h's: one 256-byte line that no
 * kernel reads or writes. */
#ifndef GHF_PAIRWISE_H
#define GHF_PAIRWISE_H

#include <stddef.h>
#include <stdint.h>

#include "ghf_distance.h" /* GHF_DIST_L1, GHF_DIST_L2, GHF_DIST_COMPLEX */

#ifdef __cplusplus
extern "C" {
#endif

#define GHF_PAIR_DOT 0

#define GHF_PAIR_HINGE 1
#define GHF_PAIR_LOGISTIC 2

size_t ghf_pair_workspace_bytes(int64_t B, int64_t K, int d, int64_t nnz);
int ghf_pair_fwd(int metric, int kind, const float* q, const float* c, const int64_t* iq, const int64_t* target,
                 const int64_t* filt_ptr, const int64_t* filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d,
                 float scale, float margin, int normalize, const int64_t* neg /* [B, K] */, int64_t K, const float* bias,
                 void* workspace, size_t workspace_bytes, float* loss, int32_t* count, int32_t* active, void* stream);
int ghf_pair_bwd(int metric, int kind, const float* q, const float* c, const int64_t* iq, const int64_t* target,
                 const int64_t* filt_ptr, const int64_t* filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d,
                 float scale, float margin, int normalize, const int64_t* neg /* [B, K] */, int64_t K, const float* bias,
                 const int32_t* count, const float* grad_loss, void* workspace, size_t workspace_bytes, float* dq,
                 float* coef /* [B, K + 1] */, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* GHF_PAIRWISE_H */
