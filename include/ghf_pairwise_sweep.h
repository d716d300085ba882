/* ghf_pairwise_sweep.h — C ABI of libghf_hip.so, the pairwise ranking losses (hinge, logistic) under a distance score against
 * every node or one candidate set shared by the batch, forward and backward (csrc/pairwise_sweep.hip).
 *
 * A seventh header beside ghf.h, ghf_negatives.h, ghf_distance.h, ghf_distance_sweep.h, ghf_distance_loss.h and
 * ghf_pairwise.h, whose conventions and error codes it shares (device pointers owned by the caller, inputs never written,
 * every call enqueued on `stream`, a hipStream_t passed as void*; nothing allocates or synchronises; 0 or a negative GHF_E*
 * code, the message through ghf_last_error).  The six older headers and GHF_ABI_VERSION are as they were: these entry points
 * are additions that no existing caller sees.
 *
 * ghf_pairwise.h's losses couple a query's target to the query's OWN negatives neg[i, :].  The calls below couple it to all N
 * rows of c, or to one candidate set ic [C] shared by the batch; the B x C distances, ids and coefficients are never stored.
 *
 * Everything that is not restated here is ghf_distance_loss.h's, word for word: q [rows_q, d], c [N, d] fp32 row-major;
 * iq [B] int64 (NULL: query i is row i, B <= rows_q); target [B] node ids; the CSR lists filt_ptr [B + 1] / filt_idx [nnz] of
 * node ids, each list sorted ascending; the candidates (ic strictly ascending in [0, N), 1 <= C <= N; ic == NULL requires
 * C == N; ids stay row ids of c; a bad ic invalidates every query; list entries outside the set take no part; with ic the
 * target must be in the set); a query whose target is not in the set, or whose iq, target or a list id is out of range, is
 * invalid, it alone, and nothing faults because of it; no id is dereferenced before its range check.  D(i, j) under `metric`
 * = GHF_DIST_L1, GHF_DIST_L2 or GHF_DIST_COMPLEX is ghf_distance_sweep.h's ONE chain per pair, bit for bit, on the vector and
 * on the scalar load path alike; the target's z_it is formed by the same chain and equals the tile's value of that pair bit
 * for bit.  `kind` is ghf_pairwise.h's GHF_PAIR_HINGE or GHF_PAIR_LOGISTIC.  With
 *
 *   z_ij = scale * -D(q[iq[i]], c[j])            z_it = scale * -D(q[iq[i]], c[target[i]])
 *   u_ij = (z_ij - z_it) + margin                two fp32 operations in this order, not contracted
 *   GHF_PAIR_HINGE     phi(u) = u > 0 ? u : 0    (a NaN u stays NaN)   phi'(u) = u > 0 ? 1 : 0
 *   GHF_PAIR_LOGISTIC  phi(u) = softplus(u)                            phi'(u) = sigmoid(u), by the hardware reciprocal
 *   J_i = the candidates outside query i's list, the target left out (ghf_dist_loss_negsamp_fwd's J_i);  n_i = |J_i|
 *
 * ghf_dist_pair_fwd:  loss[i]   = (normalize ? 1 / n_i : 1) sum_{j in J_i} phi(u_ij)    fp32 [B]; exactly 0 when J_i is empty
 *                     dsum[i]   = sum_{j in J_i} phi'(u_ij)                            fp32 [B]; hinge: (float)active[i]
 *                     count[i]  = n_i                                                  int32 [B]
 *                     active[i] = #{ j in J_i : u_ij > 0 }                             int32 [B]: the violated pairs; at margin
 *                                                                                      = 0, scale = 1 it is ghf_dist_sweep_rank's
 *                                                                                      greater[i]
 *                     An invalid query has loss = dsum = NaN and count = active = -1.
 *                     Hinge at scale = 1 under GHF_DIST_L1 is max(0, margin + D(h + r, t) - D(h + r, t')), TransE's published
 *                     loss with q the translated rows, on one negative set shared by the batch.
 * ghf_dist_pair_bwd:  `dsum` and `count` are the forward's.  With w_i = grad_loss[i] scale (normalize ? 1 / (float)count[i]
 *                     : 1):
 *                       G_ij = w_i phi'(u_ij) on J_i;  G_it = -w_i dsum[i] on the target pair, listed or not;  0 for a listed
 *                       pair.  For the hinge sum_j G_ij = w_i active[i] = -G_it exactly.
 *                       dq [B, d]:  dq[i] = - sum_j G_ij g(i, j) over J_i and the target; NOT scattered through iq
 *                       dc [C, d] ([N, d] without ic): dc[j] = + sum_i G_ij g(i, j), row j belongs to candidate ic[j]
 *                     with g(i, j) = dD / dq exactly ghf_distance.h's, as ghf_dist_loss_bwd forms it.  Every row of dq and dc
 *                     is written, zeros included.  count[i] <= 0, or an invalid query: the query takes no part.  u_ij is
 *                     recomputed from the forward's chain and has the forward's bits.
 *
 * The order of every sum is fixed.  Forward: a lane owns candidates lane + 64 rc (rc = 0 .. 3) of every 256-candidate tile of
 * its slab and adds its pairs tile by tile in ascending tile order, rc ascending within a tile, a pair outside J_i adding
 * +0.f and 0; the 64 lanes merge by the xor butterfly (partner lane ^ 1, ^ 2, ... ^ 32); the slabs, which depend on C alone,
 * are added in ascending slab order.  Backward: the streamed side ascending, four rows a group, within a slab; the slabs in
 * ascending order.  No floating-point atomics: the same call twice gives the same bits (loss, dsum, count, active, dq, dc),
 * and a query's forward results do not depend on its batch.
 *
 * Refusals, in this order, all before anything is launched: an unknown metric (GHF_PAIR_DOT included) or an odd d under
 * GHF_DIST_COMPLEX; an unknown kind; a scale that is not finite and positive; a margin that is not finite; normalize outside
 * {0, 1} (all GHF_EINVAL); then null pointers, a workspace that is not 256-byte aligned, bad shapes, rows_q or N >= 2^31
 * (GHF_EINVAL); d > 256 (GHF_EUNSUPPORTED); a workspace shorter than the size query's answer (GHF_EINVAL).
 *
 * workspace: *_workspace_bytes(B, C, d, nnz) bytes, 256-byte aligned; C is the number of candidates (N without ic); one size
 * with and without ic.  It holds per-query values, one 16-byte partial per (query, slab), per-slab dq / dc partials and the id
 * map of a subset: nothing of size B x C.  The queries return 0 for sizes the library cannot run (B, C or d < 1, d > 256,
 * nnz < 0, B or C >= 2^31). */
#ifndef GHF_PAIRWISE_SWEEP_H
#define GHF_PAIRWISE_SWEEP_H

#include <stddef.h>
#include <stdint.h>

#include "ghf_distance.h" /* GHF_DIST_L1, GHF_DIST_L2, GHF_DIST_COMPLEX */
#include "ghf_pairwise.h" /* GHF_PAIR_HINGE, GHF_PAIR_LOGISTIC */

#ifdef __cplusplus
extern "C" {
#endif

size_t ghf_dist_pair_fwd_workspace_bytes(int64_t B, int64_t C, int d, int64_t nnz);
int ghf_dist_pair_fwd(int metric, int kind, const float* q, const float* c, const int64_t* iq, const int64_t* target,
                      const int64_t* filt_ptr, const int64_t* filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d,
                      float scale, float margin, int normalize, const int64_t* ic /* [C] or NULL */, int64_t C, void* workspace,
                      size_t workspace_bytes, float* loss, float* dsum, int32_t* count, int32_t* active, void* stream);
size_t ghf_dist_pair_bwd_workspace_bytes(int64_t B, int64_t C, int d, int64_t nnz);
int ghf_dist_pair_bwd(int metric, int kind, const float* q, const float* c, const int64_t* iq, const int64_t* target,
                      const int64_t* filt_ptr, const int64_t* filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d,
                      float scale, float margin, int normalize, const int64_t* ic /* [C] or NULL */, int64_t C, const float* dsum,
                      const int32_t* count, const float* grad_loss, void* workspace, size_t workspace_bytes,
                      float* dq /* [B, d] */, float* dc /* [C, d]; [N, d] without ic */, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* GHF_PAIRWISE_SWEEP_H */
