// distance.h — the launchers of distance.hip (distance scores for per-query negative sets; include/ghf_distance.h), called
// from capi.hip.
#pragma once
#include "common.h"
#include "../../include/ghf_distance.h"

namespace ghf {

size_t dist_workspace_bytes(int64_t B, int64_t K, int d, int64_t nnz);
int launch_dist_rank(int metric, const float* q, const float* c, const int64_t* iq, const int64_t* target,
                     const int64_t* filt_ptr, const int64_t* filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d,
                     const int64_t* neg, int64_t K, void* ws, size_t ws_bytes, int64_t* greater, int64_t* equal,
                     hipStream_t stream);
// mode: GHF_DIST_SOFTMAX (aux = lse; margin and alpha unused) or GHF_DIST_NEGSAMP (aux = lw)
int launch_dist_loss_fwd(int metric, int mode, const float* q, const float* c, const int64_t* iq, const int64_t* target,
                         const int64_t* filt_ptr, const int64_t* filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B,
                         int d, float scale, float margin, float alpha, const int64_t* neg, int64_t K, void* ws, size_t ws_bytes,
                         float* loss, float* aux, hipStream_t stream);
int launch_dist_bwd(int metric, int mode, const float* q, const float* c, const int64_t* iq, const int64_t* target,
                    const int64_t* filt_ptr, const int64_t* filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d,
                    float scale, float margin, float alpha, const int64_t* neg, int64_t K, const float* saved, const float* grad,
                    void* ws, size_t ws_bytes, float* dq, float* coef, hipStream_t stream);
int launch_dist_rows_grad(int metric, const float* q, const float* c, const int64_t* iq, int64_t rows_q, int64_t N, int64_t B,
                          int d, int64_t K, const float* coef, const int64_t* perm, const int64_t* off, float* dc,
                          hipStream_t stream);

}  // namespace ghf
