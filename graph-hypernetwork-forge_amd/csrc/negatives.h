// negatives.h — the launchers of negatives.hip (per-query negative sets; include/ghf_negatives.h), called from capi.hip.
#pragma once
#include "common.h"
#include "../../include/ghf_negatives.h"

namespace ghf {

size_t neg_workspace_bytes(int64_t B, int64_t K, int d, int64_t nnz);
int launch_neg_rank(const float* q, const float* c, const int64_t* iq, const int64_t* target, const int64_t* filt_ptr,
                    const int64_t* filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d, const int64_t* neg,
                    int64_t K, const float* bias, void* ws, size_t ws_bytes, int64_t* greater, int64_t* equal,
                    hipStream_t stream);
// mode: GHF_NEG_SOFTMAX (aux = lse; margin and alpha unused) or GHF_NEG_NEGSAMP (aux = lw)
int launch_neg_loss_fwd(int mode, const float* q, const float* c, const int64_t* iq, const int64_t* target,
                        const int64_t* filt_ptr, const int64_t* filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d,
                        float scale, float margin, float alpha, const int64_t* neg, int64_t K, const float* bias, void* ws,
                        size_t ws_bytes, float* loss, float* aux, hipStream_t stream);
int launch_neg_bwd(int mode, const float* q, const float* c, const int64_t* iq, const int64_t* target, const int64_t* filt_ptr,
                   const int64_t* filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d, float scale, float margin,
                   float alpha, const int64_t* neg, int64_t K, const float* bias, const float* saved, const float* grad,
                   void* ws, size_t ws_bytes, float* dq, float* coef, hipStream_t stream);

}  // namespace ghf
