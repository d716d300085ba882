// pairwise.h — the launchers of pairwise.hip (pairwise ranking losses on per-query negative sets; include/ghf_pairwise.h),
// called from capi.hip.
#pragma once
#include "common.h"
#include "../../include/ghf_pairwise.h"

namespace ghf {

size_t pair_workspace_bytes(int64_t B, int64_t K, int d, int64_t nnz);
// metric: GHF_PAIR_DOT or GHF_DIST_L1 / L2 / COMPLEX; kind: GHF_PAIR_HINGE or GHF_PAIR_LOGISTIC — both checked by the caller
int launch_pair_fwd(int metric, int kind, const float* q, const float* c, const int64_t* iq, const int64_t* target,
                    const int64_t* filt_ptr, const int64_t* filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d,
                    float scale, float margin, int normalize, const int64_t* neg, int64_t K, const float* bias, void* ws,
                    size_t ws_bytes, float* loss, int32_t* count, int32_t* active, hipStream_t stream);
int launch_pair_bwd(int metric, int kind, const float* q, const float* c, const int64_t* iq, const int64_t* target,
                    const int64_t* filt_ptr, const int64_t* filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d,
                    float scale, float margin, int normalize, const int64_t* neg, int64_t K, const float* bias,
                    const int32_t* count, const float* grad, void* ws, size_t ws_bytes, float* dq, float* coef,
                    hipStream_t stream);

}  // namespace ghf
