// pairwise.h — the launcher of pairwise.hip (pairwise ranking losses on per-query negative sets; include/ghf_pairwise.h),
// called from capi.hip.
#pragma once
#include "negatives.h"

namespace ghf {

size_t pair_workspace_bytes(int64_t B, int64_t K, int d, int64_t nnz);
// metric: GHF_PAIR_DOT or GHF_DIST_L1 / L2 / COMPLEX, checked by the caller; e: Hinge or Logistic
int launch_pair(int metric, PqEpi e, bool bwd, const char* op, const NegArgs& a, size_t ws_bytes, hipStream_t stream);

}  // namespace ghf
