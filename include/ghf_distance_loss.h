/* ghf_distance_loss.h — C ABI of libghf_hip.so, the softmax and the negative-sampling loss under a distance score against
 * every node or a shared candidate subset, forward and backward (csrc/distance_loss.hip).
 *
 * A fifth header beside ghf.h, ghf_negatives.h, ghf_distance.h and ghf_distance_sweep.h, whose conventions and error codes it
 * shares (device pointers owned by the caller, inputs never written, every call enqueued on `stream`, a hipStream_t passed as
 * void*; nothing allocates or synchronises; 0 or a negative GHF_E* code, the message through ghf_last_error).  The four older
 * headers and GHF_ABI_VERSION are as they were: these entry points are additions that no existing caller sees.
 *
 * ghf_distance.h's losses score a query against its OWN negatives neg[i, :].  The calls below score it against all N rows of
 * c, or against one candidate set ic [C] shared by the batch, the B x C distances never stored:
 *
 *   s(i, j) = -D(q[iq[i]], c[j]),   z = scale * s,   D under `metric` = GHF_DIST_L1, GHF_DIST_L2 or GHF_DIST_COMPLEX.
 *
 * q [rows_q, d], c [N, d] fp32 row-major; iq [B] int64 (NULL: query i is row i, B <= rows_q); target [B] node ids; the CSR
 * lists filt_ptr [B + 1] / filt_idx [nnz] of node ids, each list sorted ascending, exactly ghf_distance_sweep.h's.  D is that
 * header's ONE chain per pair, bit for bit, on the vector and on the scalar load path alike; the target's z_it is formed by
 * the same chain and equals the tile's value of that pair bit for bit.
 *
 * Candidates: ghf_distance_sweep.h's rules (ic strictly ascending in [0, N), 1 <= C <= N; ic == NULL requires C == N; ids
 * stay row ids of c; a bad ic invalidates every query; list entries outside the set take no part) and, as
 * ghf_score_softmax_fwd_sub / ghf_score_negsamp_fwd: with ic the target must be in the set.  A query whose target is not in
 * the set, or whose iq, target or a list id is out of range, has loss = lse / lw = NaN; it takes no part in the backward,
 * and nothing faults because of it.  No id is dereferenced before its range check.
 *
 * ghf_dist_loss_softmax_fwd: J_i = the candidates outside query i's list; the target is always in the sum, listed or not.
 *                            lse[i] = log( sum_{j in J_i or j = target} exp z_ij ),  loss[i] = lse[i] - z_it.
 * ghf_dist_loss_negsamp_fwd: J_i = the candidates outside query i's list, the target left out.  With a = adv_temperature,
 *                            w_ij = exp(a z_ij) / sum_{J_i} exp(a z_ij)  (a = 0: the uniform mean),
 *                            loss[i] = softplus(-(z_it + margin)) + sum_{J_i} w_ij softplus(z_ij + margin),
 *                            lw[i] = log sum_{J_i} exp(a z_ij); J_i empty: the positive term alone and lw = -inf.
 *                            At scale = 1, margin = gamma the positive term is -log sigmoid(gamma - D_t).
 * Listed candidates are masked before they enter a sum, never subtracted afterwards.
 *
 * ghf_dist_loss_bwd: mode GHF_DIST_SOFTMAX or GHF_DIST_NEGSAMP; G_ij and G_it exactly as ghf_neg_bwd defines them per mode
 *                    (gradients with respect to s, the weights constants), g(i, j) = dD / dq exactly ghf_distance.h's (sign
 *                    (delta), 0 at 0; delta / D, 0 at D = 0; delta / rho_p, 0 at rho_p = 0; divisions by the hardware
 *                    reciprocal).
 *                      dq [B, d]:  dq[i] = - sum_j G_ij g(i, j) over J_i and the target; NOT scattered through iq
 *                      dc [C, d] ([N, d] without ic): dc[j] = + sum_i G_ij g(i, j), row j belongs to candidate ic[j]; every
 *                                  row is written, zeros included
 *                    A NaN lse_or_lw[i] means "query i takes no part", lw = -inf "the target entry alone".
 *
 * No floating-point atomics: the same call twice gives the same bits (loss, lse / lw, dq, dc).  A query's loss and lse / lw
 * do not depend on its batch: the candidate slabs are chosen from C alone.
 *
 * Errors, in this order: an unknown metric or an odd d under GHF_DIST_COMPLEX is GHF_EINVAL before anything else; then a bad
 * mode, a scale that is not finite and positive, a margin that is not finite, an adv_temperature that is not finite and
 * >= 0 (GHF_EINVAL); null pointers, a workspace that is not 256-byte aligned, bad shapes, rows_q or N >= 2^31 (GHF_EINVAL);
 * d > 256 is GHF_EUNSUPPORTED; a workspace shorter than the size query's answer is GHF_EINVAL.  Nothing is launched after a
 * refusal.
 *
 * workspace: *_workspace_bytes(B, C, d, nnz) bytes, 256-byte aligned; C is the number of candidates (N without ic); one size
 * with and without ic.  It holds per-(query, slab) partials, per-slab dq partials and the id map of a subset: nothing of size
 * B x C.  The queries return 0 for sizes the library cannot run (B, C or d < 1, d > 256, nnz < 0, C >= 2^31). */
#ifndef GHF_DISTANCE_LOSS_H
#define GHF_DISTANCE_LOSS_H

#include <stddef.h>
#include <stdint.h>

#include "ghf_distance.h"

#ifdef __cplusplus
extern "C" {
#endif

size_t ghf_dist_loss_fwd_workspace_bytes(int64_t B, int64_t C, int d, int64_t nnz);
int ghf_dist_loss_softmax_fwd(int metric, const float* q, const float* c, const int64_t* iq, const int64_t* target,
                              const int64_t* filt_ptr, const int64_t* filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B,
                              int d, float scale, const int64_t* ic /* [C] or NULL */, int64_t C, void* workspace,
                              size_t workspace_bytes, float* loss, float* lse, void* stream);
int ghf_dist_loss_negsamp_fwd(int metric, const float* q, const float* c, const int64_t* iq, const int64_t* target,
                              const int64_t* filt_ptr, const int64_t* filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B,
                              int d, float scale, float margin, float adv_temperature, const int64_t* ic /* [C] or NULL */,
                              int64_t C, void* workspace, size_t workspace_bytes, float* loss, float* lw, void* stream);
size_t ghf_dist_loss_bwd_workspace_bytes(int64_t B, int64_t C, int d, int64_t nnz);
int ghf_dist_loss_bwd(int metric, int mode, const float* q, const float* c, const int64_t* iq, const int64_t* target,
                      const int64_t* filt_ptr, const int64_t* filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d,
                      float scale, float margin, float adv_temperature, const int64_t* ic /* [C] or NULL */, int64_t C,
                      const float* lse_or_lw, const float* grad_loss, void* workspace, size_t workspace_bytes,
                      float* dq /* [B, d] */, float* dc /* [C, d]; [N, d] without ic */, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* GHF_DISTANCE_LOSS_H */
