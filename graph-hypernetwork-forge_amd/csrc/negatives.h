// negatives.h — what capi.hip and the three units of the per-query family (negatives.hip, distance.hip, pairwise.hip;
// DESIGN.md §21, §22, §26, §23) agree on: the kernels' epilogue, the one place where each public constant set becomes it, the
// argument block, and negatives.hip's launcher.
#pragma once
#include "common.h"
#include "../../include/ghf_negatives.h"
#include "../../include/ghf_distance.h"
#include "../../include/ghf_pairwise.h"

namespace ghf {

// What a per-query kernel does with a query's scores.  GHF_NEG_SOFTMAX, GHF_DIST_SOFTMAX and GHF_PAIR_DOT are all 0 and the
// rank has no public number at all, so below the extern "C" functions nothing takes a public mode or kind: it is translated
// here, once per constant set, and the rank entry points name PqEpi::Rank.  A value outside its set never gets this far (the
// entry helper refuses it by its own message).
enum class PqEpi { Rank, Softmax, Negsamp, Hinge, Logistic };
constexpr PqEpi pq_of_neg_mode(int mode) { return mode == GHF_NEG_NEGSAMP ? PqEpi::Negsamp : PqEpi::Softmax; }
constexpr PqEpi pq_of_dist_mode(int mode) { return mode == GHF_DIST_NEGSAMP ? PqEpi::Negsamp : PqEpi::Softmax; }
constexpr PqEpi pq_of_pair_kind(int kind) { return kind == GHF_PAIR_HINGE ? PqEpi::Hinge : PqEpi::Logistic; }
static_assert(pq_of_neg_mode(GHF_NEG_SOFTMAX) == PqEpi::Softmax && pq_of_neg_mode(GHF_NEG_NEGSAMP) == PqEpi::Negsamp, "ghf_negatives.h");
static_assert(pq_of_dist_mode(GHF_DIST_SOFTMAX) == PqEpi::Softmax && pq_of_dist_mode(GHF_DIST_NEGSAMP) == PqEpi::Negsamp, "ghf_distance.h");
static_assert(pq_of_pair_kind(GHF_PAIR_HINGE) == PqEpi::Hinge && pq_of_pair_kind(GHF_PAIR_LOGISTIC) == PqEpi::Logistic, "ghf_pairwise.h");
constexpr bool pq_is_pair(PqEpi e) { return e == PqEpi::Hinge || e == PqEpi::Logistic; }

struct NegArgs {
    const float* q; const float* c; const int64_t* iq; const int64_t* target;
    const int64_t* filt_ptr; const int64_t* filt_idx; int64_t nnz;
    const int64_t* neg; int64_t K, rows_q, N, B;
    int d;
    const float* bias; float scale, margin, alpha;
    long long* greater; long long* equal; float* loss; float* aux;             // forward: counts, or loss and lse / lw
    const float* saved; const float* grad; float* dq; float* coef;             // backward
    int* count; int* active; const int* saved_n; int normalize;                // pairwise: n_i and the violated pairs, int32 [B]
};

size_t neg_workspace_bytes(int64_t B, int64_t K, int d, int64_t nnz);
// e: Rank (forward only), Softmax (aux = lse; margin and alpha unused) or Negsamp (aux = lw); filt_ptr null when nnz == 0
int launch_neg(PqEpi e, bool bwd, const char* op, const NegArgs& a, size_t ws_bytes, hipStream_t stream);

}  // namespace ghf
