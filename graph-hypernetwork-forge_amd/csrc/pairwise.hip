// pairwise.hip — the pairwise ranking losses of a batch of queries against PER-QUERY negative sets neg [B, K]
// (include/ghf_pairwise.h), forward and backward, under the dot product or a distance:
//   u_ij = (z_ij - z_it) + margin,   loss_i = (1 / n_i) sum_{j in J_i} phi(u_ij),
//   phi(u) = max(u, 0) (hinge: TransE's margin ranking loss)  or  softplus(u) (logistic: BPR at margin 0).
// Every term couples one negative to its query's positive, so the target's coefficient is the negated sum of the row's:
// G_it = -sum_j G_ij.  None of negatives.hip's or distance.hip's epilogues has that form; the rest is theirs.
//
// The kernel is negatives_dev.h's pq_kernel (§23), its hinge and logistic arms: the geometry, the id walk and the row loads of
// negatives.hip, the score of a position formed by the policy of ghf_neg_rank (DotScore) or of ghf_dist_rank (DistScore<metric>,
// distance_dev.h), so `active` at margin 0 is that call's `greater`.  This unit turns the public metric into the policy and
// instantiates the two arms, forward and backward.
//
// Forward, one pass: z_it is known before the loop; the state is one float sum and two integer counts per lane (every lane
// of a group holds its group's), merged over the groups by the fixed butterfly and over the four waves through LDS in wave
// order.  No branch in the loop: a position outside J_i adds 0.f and 0.
// Backward, one pass: G_ij goes to coef as it is formed, dq_i and the running sum of G_ij accumulate together in registers,
// merge the same way, and the target's term — its coefficient is minus that sum — is applied after the merge.  1 / n_i comes
// from the saved count.  d embs and d bias are ghf_group_edges + ghf_segment_axpy (dot) or ghf_dist_rows_grad (distance) over
// coef (autograd.PerQueryLossFn).  No floating-point atomics.
#include "common.h"
#include "rank_sweep.h"
#include "negatives.h"
#include "negatives_dev.h"
#include "distance_dev.h"
#include "pairwise.h"

namespace ghf {

size_t pair_workspace_bytes(int64_t B, int64_t K, int d, int64_t nnz) { return neg_workspace_bytes(B, K, d, nnz); }

// the public metric, translated once into a score policy; the kind came as the kernels' epilogue
template <class P>
static int pair_launch_kind(PqEpi e, bool bwd, const NegArgs& a, hipStream_t stream) {
    if (e == PqEpi::Hinge) return bwd ? pq_launch<P, PqEpi::Hinge, true>(a, stream) : pq_launch<P, PqEpi::Hinge, false>(a, stream);
    if (e == PqEpi::Logistic) return bwd ? pq_launch<P, PqEpi::Logistic, true>(a, stream) : pq_launch<P, PqEpi::Logistic, false>(a, stream);
    return set_err(GHF_EINVAL, "pairwise launch: not a pairwise epilogue");
}

int launch_pair(int metric, PqEpi e, bool bwd, const char* op, const NegArgs& a, size_t ws_bytes, hipStream_t stream) {
    const int rc = pq_open_launch(op, e, bwd, a, ws_bytes);
    if (rc != GHF_OK) return rc;
    switch (metric) {
        case GHF_PAIR_DOT: return pair_launch_kind<DotScore>(e, bwd, a, stream);
        case GHF_DIST_L1: return pair_launch_kind<DistScore<GHF_DIST_L1>>(e, bwd, a, stream);
        case GHF_DIST_L2: return pair_launch_kind<DistScore<GHF_DIST_L2>>(e, bwd, a, stream);
        default: return pair_launch_kind<DistScore<GHF_DIST_COMPLEX>>(e, bwd, a, stream);
    }
}

}  // namespace ghf
