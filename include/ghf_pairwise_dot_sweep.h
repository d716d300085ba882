/* ghf_pairwise_dot_sweep.h — C ABI of libghf_hip.so, the pairwise ranking losses (hinge, logistic / BPR) by DOT PRODUCT against
 * every node or one candidate set shared by the batch, forward and backward (csrc/pairwise_dot_sweep.hip, csrc/rank_sweep.h,
 * csrc/softmax.hip).
 *
 * An eighth header beside ghf.h, ghf_negatives.h, ghf_distance.h, ghf_distance_sweep.h, ghf_distance_loss.h, ghf_pairwise.h
 * and ghf_pairwise_sweep.h, whose conventions and error codes it shares (device pointers owned by the caller, inputs never
 * written, every call enqueued on `stream`, a hipStream_t passed as void*; nothing allocates or synchronises; 0 or a negative
 * GHF_E* code, the message through ghf_last_error).  The seven older headers and GHF_ABI_VERSION are as they were: these entry
 * points are additions that no existing caller sees.
 *
 * ghf_pairwise.h's losses couple a query's target to the query's OWN negatives neg[i, :]; ghf_pairwise_sweep.h's couple it to
 * every row of c under a distance.  The calls below couple it to every row of c, or to one candidate set ic [C] shared by the
 * batch, under the dot product, on the fp32 matrix instruction; the B x C scores, ids and coefficients are never stored.
 *
 * Arguments.  q [rows_q, d], c [N, d] fp32 row-major; iq [B] int64 (NULL: query i is row i, B <= rows_q); target [B] node ids;
 * the CSR lists filt_ptr [B + 1] / filt_idx [nnz] of node ids, each list sorted ascending; rows_q, N, B, d; ic / C; bias: all
 * keep the meaning, the validity rules and the invalid-query behaviour of ghf_score_negsamp_fwd / ghf_score_negsamp_bwd (ghf.h):
 * ic == NULL with C == 0 means every node; otherwise ic [C] holds strictly ascending node ids in [0, N), 1 <= C <= N, ids stay
 * row ids of c, list entries outside the set take no part, and with ic the target must be in the set.  A bad ic (not strictly
 * ascending, or an id outside [0, N)) invalidates every query.  A query whose target is not in the set, or whose iq, target or
 * a list id is out of range, is invalid, it alone, and nothing faults because of it: no id is dereferenced before its range
 * check.  bias is fp32 [N] (one entry per node, also with ic) or NULL, and must be finite.  `kind` is ghf_pairwise.h's
 * GHF_PAIR_HINGE or GHF_PAIR_LOGISTIC.
 *
 * Scores.  s(i, j) is the sweep's accumulator chain: s = fmaf(q[iq[i]][k], c[j][k], s), k ascending from 0 (the matrix
 * instruction and its VALU restatement dot_chain give the same bits, on the vector and on the scalar load path alike).  With
 *
 *   z_ij = scale * s(i, j)                       with a bias: z_ij = fmaf(scale, s(i, j), bias[j])
 *   z_it = the same expression for j = target[i], from the chain of that pair: it has the tile's bits of that pair
 *   u_ij = (z_ij - z_it) + margin                two fp32 operations in this order, not contracted
 *   GHF_PAIR_HINGE     phi(u) = u > 0 ? u : 0    (a NaN u stays NaN)   phi'(u) = u > 0 ? 1 : 0
 *   GHF_PAIR_LOGISTIC  phi(u) = softplus(u)                            phi'(u) = sigmoid(u), by the hardware reciprocal
 *   J_i = the candidates outside query i's list, the target left out (ghf_pairwise_sweep.h's J_i);  n_i = |J_i|
 *
 * ghf_score_pair_fwd:  loss[i]   = sum_{j in J_i} phi(u_ij), times 1.f / (float)n_i with normalize    fp32 [B]; exactly 0 when
 *                                                                                                     J_i is empty
 *                      dsum[i]   = sum_{j in J_i} phi'(u_ij)                            fp32 [B]; hinge: (float)active[i]
 *                      count[i]  = n_i                                                  int32 [B]
 *                      active[i] = #{ j in J_i : u_ij > 0 }                             int32 [B]: the violated pairs; at margin
 *                                                                                       = 0, scale = 1, no bias it is
 *                                                                                       ghf_score_rank's greater[i]
 *                      An invalid query has loss = dsum = NaN and count = active = -1.
 *                      Logistic at margin = 0 is BPR on one negative set shared by the batch (in-batch / sampled negatives);
 *                      the hinge is the max-margin ranking loss.
 * ghf_score_pair_bwd:  `dsum` and `count` are the forward's.  With w_i = grad_loss[i] scale (normalize ? 1 / (float)count[i]
 *                      : 1):
 *                        G_ij = w_i phi'(u_ij) on J_i;  G_it = -w_i dsum[i] on the target pair, listed or not;  0 at a listed
 *                        pair.
 *                        dq [B, d]:  dq[i] = sum_j G_ij c[j]; NOT scattered through iq
 *                        dc [N, d] ([C, d] with ic, row j belonging to node ic[j]): dc[j] = sum_i G_ij q[iq[i]]
 *                        db [N] ([C] with ic): db[j] = (sum_i G_ij) / scale; NULL: not wanted; ignored without a bias
 *                      Every row of dq, dc and db is written, zeros included.  count[i] <= 0, or an invalid query: the query
 *                      takes no part.
 *                      The backward multiplies the same rows with the same matrix instruction in the same order of k (zeros
 *                      behind d add nothing), and forms z and u by the forward's expressions: u_ij in the backward has the
 *                      forward's bits.  For the hinge therefore sum_{j in J_i} G_ij = w_i active[i] = -G_it exactly, term by
 *                      term: every G_ij is w_i or 0, and exactly active[i] of them are w_i.
 *
 * The order of every sum is fixed.  Forward: a lane owns 32 candidates of every candidate tile (256 candidates, 128 for
 * d > 128) for each of its two query columns and adds its pairs tile by tile in ascending tile order, register order within a
 * tile, a pair outside J_i adding +0.f and 0 (the sums are never -0.f); the lanes' partials merge through LDS in the order
 * (wave along the candidates, half-wave) ascending; the slabs, which depend on the candidate count and d alone, are added in
 * ascending slab order.  Backward: streamed rows ascending within a slab, the slabs (again from the candidate count and d
 * alone) in ascending order.  No floating-point atomics: the same call twice gives the same bits (loss, dsum, count, active, dq,
 * dc, db), and a query's forward results do not depend on its batch.  A call with ic has the bits of the all-node call on a
 * contiguous copy c[ic] (bias[ic]).  A bias of zeros gives the bits of the call without one.
 *
 * Refusals, in this order, all before anything is launched: an unknown kind; a scale that is not finite and positive; a
 * margin that is not finite; normalize outside {0, 1}; null pointers (q, c, target, an output, the workspace, a list with
 * nnz > 0; the backward's dsum, count, grad_loss); a workspace that is not 256-byte aligned; bad shapes (d, rows_q, N, B < 1,
 * nnz < 0, B > rows_q without iq) and the pairing of ic and C (ic with 1 <= C <= N, or ic == NULL with C == 0); rows_q or
 * N >= 2^31 (all GHF_EINVAL); d > 256 (GHF_EUNSUPPORTED); a workspace shorter than the size query's answer (GHF_EINVAL).
 *
 * workspace: *_workspace_bytes(B, N, C, d, nnz) bytes, 256-byte aligned; C = 0 for every node.  It holds per-query values, one
 * 16-byte partial per (query, slab) (forward), per-slab dq partials (backward), and with ic the id map and a gathered bias [C]
 * (asked for whether or not the call has a bias: one size per shape): nothing of size B x C.  The queries return 0 for sizes
 * the library cannot run (B, N or d < 1, d > 256, C < 0 or C > N, nnz < 0, B or N >= 2^31). */
#ifndef GHF_PAIRWISE_DOT_SWEEP_H
#define GHF_PAIRWISE_DOT_SWEEP_H

#include <stddef.h>
#include <stdint.h>

#include "ghf_pairwise.h" /* GHF_PAIR_HINGE, GHF_PAIR_LOGISTIC */

#ifdef __cplusplus
extern "C" {
#endif

size_t ghf_score_pair_fwd_workspace_bytes(int64_t B, int64_t N, int64_t C, int d, int64_t nnz);
int ghf_score_pair_fwd(int kind, const float* q, const float* c, const int64_t* iq, const int64_t* target, const int64_t* filt_ptr,
                       const int64_t* filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d, float scale, float margin,
                       int normalize, const int64_t* ic /* [C] or NULL */, int64_t C, const float* bias /* [N] or NULL */,
                       void* workspace, size_t workspace_bytes, float* loss, float* dsum, int32_t* count, int32_t* active,
                       void* stream);
size_t ghf_score_pair_bwd_workspace_bytes(int64_t B, int64_t N, int64_t C, int d, int64_t nnz);
int ghf_score_pair_bwd(int kind, const float* q, const float* c, const int64_t* iq, const int64_t* target, const int64_t* filt_ptr,
                       const int64_t* filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d, float scale, float margin,
                       int normalize, const int64_t* ic /* [C] or NULL */, int64_t C, const float* bias /* [N] or NULL */,
                       const float* dsum, const int32_t* count, const float* grad_loss, void* workspace, size_t workspace_bytes,
                       float* dq /* [B, d] */, float* dc /* [N, d]; [C, d] with ic */, float* db /* [N]; [C] with ic; or NULL */,
                       void* stream);

#ifdef __cplusplus
}
#endif

#endif /* GHF_PAIRWISE_DOT_SWEEP_H */
