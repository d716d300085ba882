/* ghf_distance_sweep.h — C ABI of libghf_hip.so, distance scores against every node or a candidate subset: filtered rank
 * counts and top-k (csrc/distance_sweep.hip).
 *
 * A fourth header beside ghf.h, ghf_negatives.h and ghf_distance.h, whose conventions and error codes it shares (device
 * pointers owned by the caller, inputs never written, every call enqueued on `stream`, a hipStream_t passed as void*; nothing
 * allocates or synchronises; 0 or a negative GHF_E* code, the message through ghf_last_error).  The three older headers and
 * GHF_ABI_VERSION are as they were: these entry points are additions that no existing caller sees.
 *
 * ghf_distance.h's ghf_dist_rank ranks a query against its OWN negatives neg[i, :].  The calls below rank it against all N
 * rows of c — the filtered rank every knowledge-graph leaderboard reports — or return its k nearest rows, the B x C distances
 * never stored.  They are ghf.h's ghf_score_rank and ghf_score_topk, and their _sub forms, with the score
 *
 *   s(i, j) = -D(q[iq[i]], c[j]),   D under `metric` = GHF_DIST_L1, GHF_DIST_L2 or GHF_DIST_COMPLEX of ghf_distance.h,
 *
 * and everything that is not restated here is theirs, word for word: q [rows_q, d], c [N, d] fp32 row-major; iq [B] int64
 * (NULL: query i is row i, B <= rows_q); target [B]; the CSR filter lists filt_ptr [B + 1] / filt_idx [nnz], each list sorted
 * ascending, a repeated id removed once, the target never removed by its list; greater[i] = #{ j : s(i, j) > t_i }, equal[i]
 * likewise with == (the target itself left out), int64 [B]; 1 <= k <= 128, scores [B, k] descending with ties towards the
 * lower id, (-inf, -1) where fewer candidates remain; NaN counts in neither count and is never returned; an out-of-range
 * iq, target or list id gives that query alone greater = equal = -1 / NaN scores and ids -1, without a fault, and no id is
 * dereferenced before its range check; the same call twice gives the same bits, and a query's outputs do not depend on its
 * batch; d <= 256 (else GHF_EUNSUPPORTED), N < 2^31, and — a limit of these calls alone — rows_q < 2^31 (else GHF_EINVAL ahead
 * of any launch: the sweep keeps a query's row number in 32 bits).
 *
 * Candidates.  ic == NULL: all N rows, and C == N is required.  Otherwise ic [C] int64 holds node ids, strictly ascending in
 * [0, N), 1 <= C <= N, with ghf_score_rank_sub / ghf_score_topk_sub's semantics: ids going in and coming out stay row ids of
 * c; the target may be any row (a target outside the set is compared, not counted); list entries outside the set take no
 * part; a bad ic makes every query invalid; no row outside c is ever read.
 *
 * The distance of a pair is ONE chain, bit for bit, whatever the path (vector: d % 4 == 0 and 16-byte aligned bases; scalar
 * otherwise), the tile position, the batch or the subset.  With delta_k = q_k - c_k (one fp32 subtraction), no contraction:
 *
 *   GHF_DIST_L1       acc = acc + |delta_k|,                 k = 0 .. d - 1 from acc = 0
 *   GHF_DIST_L2       acc = fmaf(delta_k, delta_k, acc),     k ascending, then D = sqrt(acc)
 *   GHF_DIST_COMPLEX  rho_p = sqrt(fmaf(delta_2p+1, delta_2p+1, delta_2p * delta_2p)),  acc = acc + rho_p,  p ascending
 *                     (re / im interleaved; an odd d is GHF_EINVAL)
 *
 * The square roots are the hardware's (v_sqrt_f32, 1 ulp), as in ghf_distance.h.  The target's distance and the filter
 * corrections are formed by the same chain: equal arguments give equal bits, two rows at the same distance tie exactly, and
 * that is all the counts rely on.  L1 is exact where every difference and partial sum is representable.  These sums are NOT
 * promised to equal ghf_dist_rank's bits: that kernel sums across a lane group.
 *
 * Errors, in this order: an unknown metric or an odd d under GHF_DIST_COMPLEX is GHF_EINVAL before anything else; then null
 * pointers, a workspace that is not 256-byte aligned, bad shapes (GHF_EINVAL); d > 256 is GHF_EUNSUPPORTED; a workspace
 * shorter than the size query's answer is GHF_EINVAL.  Nothing is launched after a refusal.
 *
 * workspace: *_workspace_bytes(B, C, d, [k,] nnz) bytes, 256-byte aligned; C is the number of candidates (N without ic).  One
 * size with and without ic.  The queries return 0 for sizes the library cannot run (B, C or d < 1, d > 256, nnz < 0, k outside
 * 1..128, C >= 2^31). */
#ifndef GHF_DISTANCE_SWEEP_H
#define GHF_DISTANCE_SWEEP_H

#include <stddef.h>
#include <stdint.h>

#include "ghf_distance.h"

#ifdef __cplusplus
extern "C" {
#endif

size_t ghf_dist_sweep_rank_workspace_bytes(int64_t B, int64_t C, int d, int64_t nnz);
int ghf_dist_sweep_rank(int metric, const float* q, const float* c, const int64_t* iq, const int64_t* target,
                        const int64_t* filt_ptr, const int64_t* filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B,
                        int d, const int64_t* ic /* [C] or NULL */, int64_t C, void* workspace, size_t workspace_bytes,
                        int64_t* greater, int64_t* equal, void* stream);
size_t ghf_dist_sweep_topk_workspace_bytes(int64_t B, int64_t C, int d, int k, int64_t nnz);
int ghf_dist_sweep_topk(int metric, const float* q, const float* c, const int64_t* iq, const int64_t* filt_ptr,
                        const int64_t* filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d, int k,
                        const int64_t* ic /* [C] or NULL */, int64_t C, void* workspace, size_t workspace_bytes,
                        float* scores /* [B, k] = -D */, int64_t* ids /* [B, k] */, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* GHF_DISTANCE_SWEEP_H */
