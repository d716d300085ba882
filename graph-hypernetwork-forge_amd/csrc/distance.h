// distance.h — the launchers of distance.hip (distance scores for per-query negative sets; include/ghf_distance.h), called
// from capi.hip.
#pragma once
#include "negatives.h"

namespace ghf {

size_t dist_workspace_bytes(int64_t B, int64_t K, int d, int64_t nnz);
// metric: GHF_DIST_L1 / L2 / COMPLEX, checked by the caller; e, bwd, op and a as launch_neg's (no bias)
int launch_dist(int metric, PqEpi e, bool bwd, const char* op, const NegArgs& a, size_t ws_bytes, hipStream_t stream);
int launch_dist_rows_grad(int metric, const float* q, const float* c, const int64_t* iq, int64_t rows_q, int64_t N, int64_t B,
                          int d, int64_t K, const float* coef, const int64_t* perm, const int64_t* off, float* dc,
                          hipStream_t stream);

}  // namespace ghf
