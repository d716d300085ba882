// negatives.hip — rank counts, the softmax loss and the negative-sampling loss of a batch of queries against PER-QUERY
// negative sets neg [B, K] (include/ghf_negatives.h), forward and backward.  The all-node sweeps
// (rank_sweep.h) multiply a query tile with a candidate tile that every query shares; here query i has its own K rows of c,
// so the work is a row gather and a dot product per (query, position), bound by the bytes in flight, not by the flops.
//
// A query is owned by one wave (K <= 256) or by the four waves of its workgroup (K > 256), the number chosen from K alone, so a
// query's bits do not depend on its batch; the four take the steps below round-robin and their partials merge through LDS in
// wave order.  The query's row q_i stays in registers: a GROUP of L lanes covers a row, each
// lane four floats of it — one 16-byte load, L = 8 (d <= 32), 16 (d <= 64), 32 (d <= 128) or 64 (d <= 256) — so one wave
// instruction reads 64 / L candidate rows and every lane works.  Where d % 4 != 0 or a base is not 16-byte aligned the
// group is the wave and a lane reads the floats lane, lane + 64, ... (the scalar path).  The wave walks its K positions
// NG_U x (64 / L) at a time: the ids of the NEXT step are loaded before the rows of this one (the id -> row dependence is
// otherwise exposed once per step), then all NG_U row loads of a lane are issued — eight 16-byte loads in flight per lane
// — then the filter-list searches of the step, and only then is the first row consumed.  No load of the loop stands under a
// branch (neg_row, neg_entry): a branch would end in a wait for everything outstanding.  A dot product is the
// lane's four fmas, then a butterfly over the group: DPP inside a row of 16 lanes, one ds_bpermute per level above.  Every
// lane of a group ends with the same bits.
//
// s(i, j) has an order that depends on d and the path alone; the target's score is formed by the same code from its own
// row.  An id is compared against its range before it addresses anything: a row that is absent loads as zeros.
//
// Epilogues, per group and merged over the groups by a fixed butterfly (each merge is symmetric in its two arguments, so
// every lane ends with the same bits): rank — two integer counts; softmax — a running max and a rescaled sum (lse_merge);
// negsamp — §19's triple (neg_merge), softplus / log1p_unit as negsamp.hip's and bce.hip's (rank_sweep.h).  The backward
// recomputes z_ij from the saved lse / lw, writes G_ij into coef [B, K + 1] and accumulates dq_i in registers over the
// positions in order; d embs and d bias are ghf_group_edges + ghf_segment_axpy over coef (autograd.PerQueryLossFn).
// No floating-point atomics.
//
// The kernel text is negatives_dev.h's pq_kernel, shared with distance.hip and pairwise.hip (§23): this unit instantiates it
// under DotScore for the rank and the two set losses.
#include "common.h"
#include "rank_sweep.h"
#include "negatives.h"
#include "negatives_dev.h"                       // the geometry, DotScore, the kernel template and its launch ladder

namespace ghf {

size_t neg_workspace_bytes(int64_t B, int64_t K, int d, int64_t nnz) {
    if (B <= 0 || K <= 0 || d <= 0 || d > RK_MAX_D || nnz < 0) return 0;
    if (B >= (int64_t)1 << 31 || K >= (int64_t)1 << 31 || B * (K + 1) >= (int64_t)1 << 31) return 0;
    return 256;                                  // one reserved line, not used: a query's state lives in registers and LDS
}

int launch_neg(PqEpi e, bool bwd, const char* op, const NegArgs& a, size_t ws_bytes, hipStream_t stream) {
    const int rc = pq_open_launch(op, e, bwd, a, ws_bytes);
    if (rc != GHF_OK) return rc;
    return pq_launch_set<DotScore>(e, bwd, a, stream);
}

}  // namespace ghf
