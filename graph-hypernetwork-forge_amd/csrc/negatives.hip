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
// positions in order; d embs and d bias are ghf_group_edges + ghf_segment_axpy over coef (autograd.NegativesLossFn).
// No floating-point atomics.
#include "common.h"
#include "rank_sweep.h"
#include "negatives.h"
#include "negatives_dev.h"                       // the geometry's device helpers, shared with distance.hip

namespace ghf {

size_t neg_workspace_bytes(int64_t B, int64_t K, int d, int64_t nnz) {
    if (B <= 0 || K <= 0 || d <= 0 || d > RK_MAX_D || nnz < 0) return 0;
    if (B >= (int64_t)1 << 31 || K >= (int64_t)1 << 31 || B * (K + 1) >= (int64_t)1 << 31) return 0;
    return 256;                                  // one reserved line, not used: a query's state lives in registers and LDS
}

__device__ __forceinline__ float neg_dot(f32x4 x, f32x4 y) {
    return fmaf(x[3], y[3], fmaf(x[2], y[2], fmaf(x[1], y[1], x[0] * y[0])));
}

// ---- forward ---------------------------------------------------------------------------------------------------------------
template <int L, bool VEC, int MODE, bool BIAS, int W>
__global__ __launch_bounds__(256) void neg_fwd_kernel(const NegArgs a) {
#pragma clang fp contract(off)                           // z is rounded before the margin is added, as in negsamp.hip
    constexpr int G = 64 / L;                            // rows per wave instruction
    constexpr int STEP = NG_U * G;                       // positions per step of a wave
    const int lane = threadIdx.x & 63, gl = lane & (L - 1), g = lane / L, wv = threadIdx.x >> 6;
    const int64_t i = W == 1 ? (int64_t)blockIdx.x * 4 + wv : (int64_t)blockIdx.x;
    const int sub = W == 1 ? 0 : wv;                     // the wave's place among the query's W
    if (W == 1 && i >= a.B) return;                      // the whole wave, and no barrier on this path
    const int d = a.d;
    NegQuery s = neg_open<VEC, BIAS>(a, i, gl);
    bool bad = false;                                    // a listed id or a negative outside its range
    for (int64_t e = s.lo + lane; e < s.hi; e += 64) bad |= (uint64_t)a.filt_idx[e] >= (uint64_t)a.N;
    const float t = group_sum<L>(neg_dot(s.qv, s.tv));
    const float tb = BIAS ? t + s.tb : t;                // rank: the target's score with its bias entry

    int ngt = 0, neq = 0;                                // K < 2^31
    float m = -INFINITY, S = 0.f, T = 0.f;               // softmax: (m, S); negsamp: (m, S, T) of alpha z

    const int64_t* __restrict__ nrow = a.neg + (size_t)i * a.K;
    int idn[NG_U];
#pragma unroll
    for (int u = 0; u < NG_U; ++u) idn[u] = neg_entry(nrow, sub * STEP + u * G + g, a.K, a.N);
    for (int64_t base = (int64_t)sub * STEP; base < a.K; base += W * STEP) {
        int id[NG_U];
        f32x4 row[NG_U];
        float b[NG_U];
        bool live[NG_U];
#pragma unroll
        for (int u = 0; u < NG_U; ++u) id[u] = idn[u];
#pragma unroll
        for (int u = 0; u < NG_U; ++u) {
            const int64_t j = base + W * STEP + u * G + g;
            idn[u] = neg_entry(nrow, j, a.K, a.N);
        }
#pragma unroll
        for (int u = 0; u < NG_U; ++u) {
            const bool in = id[u] >= 0;
            bad |= id[u] == -2;
            row[u] = neg_row<VEC>(a.c, id[u], gl, d);
            b[u] = 0.f;
            if constexpr (BIAS) { const float x = a.bias[in ? id[u] : 0]; b[u] = in ? x : 0.f; }
            live[u] = in;
        }
#pragma unroll
        for (int u = 0; u < NG_U; ++u)
            live[u] = live[u] && (int64_t)id[u] != s.tg && !(s.hi > s.lo && in_filter(a.filt_idx, s.lo, s.hi, (int64_t)id[u]));
#pragma unroll
        for (int u = 0; u < NG_U; ++u) {
            if constexpr (MODE == NG_RANK) {
                // One row at a time, as the losses' running sums force it.  Nothing else orders the eight dot products of a
                // step, and computed side by side they cost 30 VGPRs and with them the fourth wave per SIMD: the empty
                // statement makes row u wait for the count of row u - 1.
                float r0 = row[u][0];
                asm volatile("" : "+v"(r0), "+v"(ngt));
                row[u][0] = r0;
            }
            const float sc = group_sum<L>(neg_dot(s.qv, row[u]));
            if constexpr (MODE == NG_RANK) {
                const float sb = BIAS ? sc + b[u] : sc;
                ngt += live[u] && sb > tb ? 1 : 0;
                neq += live[u] && sb == tb ? 1 : 0;
            } else {
                float z;
                if constexpr (BIAS) z = fmaf(a.scale, sc, b[u]);
                else z = a.scale * sc;
                if (live[u]) {
                    const float x = MODE == NG_NEGSAMP ? a.alpha * z : z;
                    float sp = 0.f;
                    if constexpr (MODE == NG_NEGSAMP) sp = softplus(z + a.margin);
                    if (x > m) {                          // the max rises: rescale what is there (exp(-inf) = 0 at the first)
                        const float e = __expf(m - x);
                        S = fmaf(S, e, 1.f);
                        T = fmaf(T, e, sp);
                        m = x;
                    } else if (x > -INFINITY) {
                        const float w = __expf(x - m);
                        S += w;
                        T = fmaf(w, sp, T);
                    } else if (x != x) {                  // a NaN on its way out
                        m = S = T = x;
                    }
                }
            }
        }
    }
    bad = __any(bad);

    // the groups' partials, merged in a fixed tree; then the waves' (W > 1), in wave order, by wave 0
    __shared__ float shf[W][4];
    __shared__ int shi[W][4];
    if constexpr (MODE == NG_RANK) {
#pragma unroll
        for (int w = L; w < 64; w *= 2) {
            ngt += __shfl_xor(ngt, w, 64);
            neq += __shfl_xor(neq, w, 64);
        }
        if constexpr (W > 1) {
            if (lane == 0) { shi[wv][0] = ngt; shi[wv][1] = neq; shi[wv][2] = bad; }
            __syncthreads();
            if (wv != 0) return;
            for (int w = 1; w < W; ++w) { ngt += shi[w][0]; neq += shi[w][1]; bad |= shi[w][2] != 0; }
        }
        s.ok = s.ok && !bad;
        if (lane == 0) {
            a.greater[i] = s.ok ? ngt : -1;
            a.equal[i] = s.ok ? neq : -1;
        }
    } else if constexpr (MODE == NG_SOFTMAX) {
        f32x2 p = {m, S};
#pragma unroll
        for (int w = L; w < 64; w *= 2) p = lse_merge(p, f32x2{neg_xor(p[0], w), neg_xor(p[1], w)});
        if constexpr (W > 1) {
            if (lane == 0) { shf[wv][0] = p[0]; shf[wv][1] = p[1]; shi[wv][2] = bad; }
            __syncthreads();
            if (wv != 0) return;
            for (int w = 1; w < W; ++w) { p = lse_merge(p, f32x2{shf[w][0], shf[w][1]}); bad |= shi[w][2] != 0; }
        }
        s.ok = s.ok && !bad;
        float zt;
        if constexpr (BIAS) zt = fmaf(a.scale, t, s.tb);
        else zt = a.scale * t;
        p = lse_merge(p, f32x2{zt, 1.f});                // the target enters exactly once
        const float lse = p[0] + logf(p[1]);
        if (lane == 0) {
            a.loss[i] = s.ok ? lse - zt : __int_as_float(0x7FC00000);
            a.aux[i] = s.ok ? lse : __int_as_float(0x7FC00000);
        }
    } else {
        NegTriple p = {m, S, T};
#pragma unroll
        for (int w = L; w < 64; w *= 2) p = neg_merge(p, NegTriple{neg_xor(p.m, w), neg_xor(p.s, w), neg_xor(p.t, w)});
        if constexpr (W > 1) {
            if (lane == 0) { shf[wv][0] = p.m; shf[wv][1] = p.s; shf[wv][2] = p.t; shi[wv][2] = bad; }
            __syncthreads();
            if (wv != 0) return;
            for (int w = 1; w < W; ++w) { p = neg_merge(p, NegTriple{shf[w][0], shf[w][1], shf[w][2]}); bad |= shi[w][2] != 0; }
        }
        s.ok = s.ok && !bad;
        float zt;
        if constexpr (BIAS) zt = fmaf(a.scale, t, s.tb);
        else zt = a.scale * t;
        const bool any = p.s > 0.f;                      // no negatives: the positive term alone, lw = -inf
        const float lw = any ? p.m + logf(p.s) : -INFINITY;
        const float l = softplus(-(zt + a.margin)) + (any ? p.t / p.s : 0.f);
        if (lane == 0) {
            a.loss[i] = s.ok ? l : __int_as_float(0x7FC00000);
            a.aux[i] = s.ok ? lw : __int_as_float(0x7FC00000);
        }
    }
}

// ---- backward --------------------------------------------------------------------------------------------------------------
template <int L, bool VEC, int MODE, bool BIAS, int W>
__global__ __launch_bounds__(256) void neg_bwd_kernel(const NegArgs a) {
#pragma clang fp contract(off)
    constexpr int G = 64 / L;
    constexpr int STEP = NG_U * G;
    const int lane = threadIdx.x & 63, gl = lane & (L - 1), g = lane / L, wv = threadIdx.x >> 6;
    const int64_t i = W == 1 ? (int64_t)blockIdx.x * 4 + wv : (int64_t)blockIdx.x;
    const int sub = W == 1 ? 0 : wv;
    if (W == 1 && i >= a.B) return;
    const int d = a.d;
    const NegQuery s = neg_open<VEC, BIAS>(a, i, gl);
    const float sv = a.saved[i];                         // lse or lw: NaN = the query takes no part
    const bool part = s.ok && sv == sv;
    const float gs = a.grad[i] * a.scale;
    const float t = group_sum<L>(neg_dot(s.qv, s.tv));
    float* __restrict__ crow = a.coef + (size_t)i * (a.K + 1);

    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    const int64_t* __restrict__ nrow = a.neg + (size_t)i * a.K;
    int idn[NG_U];
#pragma unroll
    for (int u = 0; u < NG_U; ++u) idn[u] = neg_entry(nrow, sub * STEP + u * G + g, a.K, a.N);
    for (int64_t base = (int64_t)sub * STEP; base < a.K; base += W * STEP) {
        int id[NG_U];
        f32x4 row[NG_U];
        float b[NG_U];
        bool live[NG_U];
#pragma unroll
        for (int u = 0; u < NG_U; ++u) id[u] = idn[u];
#pragma unroll
        for (int u = 0; u < NG_U; ++u) {
            const int64_t j = base + W * STEP + u * G + g;
            idn[u] = neg_entry(nrow, j, a.K, a.N);
        }
#pragma unroll
        for (int u = 0; u < NG_U; ++u) {
            const bool in = part && id[u] >= 0;
            row[u] = neg_row<VEC>(a.c, in ? id[u] : -1, gl, d);
            b[u] = 0.f;
            if constexpr (BIAS) { const float x = a.bias[in ? id[u] : 0]; b[u] = in ? x : 0.f; }
            live[u] = in;
        }
#pragma unroll
        for (int u = 0; u < NG_U; ++u)
            live[u] = live[u] && (int64_t)id[u] != s.tg && !(s.hi > s.lo && in_filter(a.filt_idx, s.lo, s.hi, (int64_t)id[u]));
#pragma unroll
        for (int u = 0; u < NG_U; ++u) {
            const float sc = group_sum<L>(neg_dot(s.qv, row[u]));
            float z;
            if constexpr (BIAS) z = fmaf(a.scale, sc, b[u]);
            else z = a.scale * sc;
            float gv;
            if constexpr (MODE == NG_SOFTMAX) {
                gv = gs * __expf(z - sv);
            } else {
                const float y = z + a.margin;
                const float e = __expf(-fabsf(y)), rcp = __builtin_amdgcn_rcpf(1.f + e);
                const float w = sv > -INFINITY ? __expf(fmaf(a.alpha, z, -sv)) : 0.f;
                gv = gs * (w * (y >= 0.f ? rcp : e * rcp));
            }
            gv = live[u] ? gv : 0.f;
            const int64_t j = base + u * G + g;
            if (gl == 0 && j < a.K) crow[j] = gv;
            // positions in order within the group; a zero coefficient adds nothing, whatever the row holds
            const f32x4 nx = {fmaf(gv, row[u][0], acc[0]), fmaf(gv, row[u][1], acc[1]), fmaf(gv, row[u][2], acc[2]),
                              fmaf(gv, row[u][3], acc[3])};
            acc = gv != 0.f ? nx : acc;
        }
    }
#pragma unroll
    for (int w = L; w < 64; w *= 2) {
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] += neg_xor(acc[e], w);
    }
    if constexpr (W > 1) {                               // the waves' sums, in wave order, by wave 0
        __shared__ f32x4 shq[W][64];
        shq[wv][lane] = acc;
        __syncthreads();
        if (wv != 0) return;
        for (int w = 1; w < W; ++w) {
            const f32x4 o = shq[w][lane];
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] += o[e];
        }
    }
    // the target's entry, last
    float zt;
    if constexpr (BIAS) zt = fmaf(a.scale, t, s.tb);
    else zt = a.scale * t;
    float gt;
    if constexpr (MODE == NG_SOFTMAX) {
        gt = gs * (__expf(zt - sv) - 1.f);
    } else {
        const float y = zt + a.margin;
        const float e = __expf(-fabsf(y)), rcp = __builtin_amdgcn_rcpf(1.f + e);
        gt = -gs * (y >= 0.f ? e * rcp : rcp);
    }
    gt = part ? gt : 0.f;
    if (gt != 0.f) {
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] = fmaf(gt, s.tv[e], acc[e]);
    }
    if (lane == 0) crow[a.K] = gt;
    if (g == 0) {
        float* __restrict__ out = a.dq + (size_t)i * d;
        if constexpr (VEC) {                             // (a dq that is not 16-byte aligned takes four stores: the path, and with
            if (4 * gl < d) {                            // it the order of every sum, is the forward's — q, c and d choose it)
                if (((uintptr_t)out & 15) == 0) {
                    *(f32x4*)(out + 4 * gl) = acc;
                } else {
#pragma unroll
                    for (int m = 0; m < 4; ++m) out[4 * gl + m] = acc[m];
                }
            }
        } else {
#pragma unroll
            for (int m = 0; m < 4; ++m)
                if (gl + 64 * m < d) out[gl + 64 * m] = acc[m];
        }
    }
}

// ---- launches --------------------------------------------------------------------------------------------------------------
static int neg_open_launch(const char* op, const NegArgs& a, size_t ws_bytes) {
    GHF_REQUIRE(a.d > 0 && a.rows_q > 0 && a.N > 0 && a.B > 0 && a.K > 0 && a.nnz >= 0, "%s: bad shape", op);
    if (a.d > RK_MAX_D) return set_err(GHF_EUNSUPPORTED, "%s: d = %d exceeds %d", op, a.d, RK_MAX_D);
    GHF_REQUIRE(a.N < (int64_t)1 << 31, "%s: N out of range", op);            // the loops keep ids in 32 bits (neg_id32)
    const size_t need = neg_workspace_bytes(a.B, a.K, a.d, a.nnz);
    GHF_REQUIRE(need > 0, "%s: B (K + 1) out of range", op);
    GHF_REQUIRE(a.iq || a.B <= a.rows_q, "%s: B exceeds the rows of q", op);
    GHF_REQUIRE(ws_bytes >= need, "%s: workspace of %zu bytes, need %zu", op, ws_bytes, need);
    return GHF_OK;
}

template <bool BWD, int MODE, bool BIAS, int W>
static int neg_launch_path(const NegArgs& a, hipStream_t stream) {
    const unsigned grid = (unsigned)(W == 1 ? cdiv(a.B, 4) : a.B);
    const bool vec = (a.d & 3) == 0 && (((uintptr_t)a.q | (uintptr_t)a.c) & 15) == 0;      // forward and backward alike
#define GHF_NEG_GO(LL, VV)                                                                  \
    do {                                                                                    \
        if constexpr (BWD) neg_bwd_kernel<LL, VV, MODE, BIAS, W><<<grid, 256, 0, stream>>>(a); \
        else neg_fwd_kernel<LL, VV, MODE, BIAS, W><<<grid, 256, 0, stream>>>(a);               \
    } while (0)
    if (!vec) GHF_NEG_GO(64, false);
    else if (a.d <= 32) GHF_NEG_GO(8, true);
    else if (a.d <= 64) GHF_NEG_GO(16, true);
    else if (a.d <= 128) GHF_NEG_GO(32, true);
    else GHF_NEG_GO(64, true);
#undef GHF_NEG_GO
    GHF_LAUNCH_CHECK();
    return GHF_OK;
}

template <bool BWD, int MODE>
static int neg_launch(const NegArgs& a, hipStream_t stream) {
    if (neg_waves(a.K) == 1) return a.bias ? neg_launch_path<BWD, MODE, true, 1>(a, stream) : neg_launch_path<BWD, MODE, false, 1>(a, stream);
    return a.bias ? neg_launch_path<BWD, MODE, true, 4>(a, stream) : neg_launch_path<BWD, MODE, false, 4>(a, stream);
}

int launch_neg_rank(const float* q, const float* c, const int64_t* iq, const int64_t* target, const int64_t* filt_ptr,
                    const int64_t* filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d, const int64_t* neg,
                    int64_t K, const float* bias, void* ws, size_t ws_bytes, int64_t* greater, int64_t* equal,
                    hipStream_t stream) {
    NegArgs a{};
    a.q = q; a.c = c; a.iq = iq; a.target = target; a.filt_ptr = nnz > 0 ? filt_ptr : nullptr; a.filt_idx = filt_idx; a.nnz = nnz;
    a.neg = neg; a.K = K; a.rows_q = rows_q; a.N = N; a.B = B; a.d = d; a.bias = bias; a.scale = 1.f;
    a.greater = (long long*)greater; a.equal = (long long*)equal;
    const int rc = neg_open_launch("neg_rank", a, ws_bytes);
    if (rc != GHF_OK) return rc;
    return neg_launch<false, NG_RANK>(a, stream);
}

int launch_neg_loss_fwd(int mode, const float* q, const float* c, const int64_t* iq, const int64_t* target,
                        const int64_t* filt_ptr, const int64_t* filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d,
                        float scale, float margin, float alpha, const int64_t* neg, int64_t K, const float* bias, void* ws,
                        size_t ws_bytes, float* loss, float* aux, hipStream_t stream) {
    NegArgs a{};
    a.q = q; a.c = c; a.iq = iq; a.target = target; a.filt_ptr = nnz > 0 ? filt_ptr : nullptr; a.filt_idx = filt_idx; a.nnz = nnz;
    a.neg = neg; a.K = K; a.rows_q = rows_q; a.N = N; a.B = B; a.d = d; a.bias = bias;
    a.scale = scale; a.margin = margin; a.alpha = alpha; a.loss = loss; a.aux = aux;
    const int rc = neg_open_launch(mode == GHF_NEG_NEGSAMP ? "neg_negsamp_fwd" : "neg_softmax_fwd", a, ws_bytes);
    if (rc != GHF_OK) return rc;
    return mode == GHF_NEG_NEGSAMP ? neg_launch<false, NG_NEGSAMP>(a, stream) : neg_launch<false, NG_SOFTMAX>(a, stream);
}

int launch_neg_bwd(int mode, const float* q, const float* c, const int64_t* iq, const int64_t* target, const int64_t* filt_ptr,
                   const int64_t* filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d, float scale, float margin,
                   float alpha, const int64_t* neg, int64_t K, const float* bias, const float* saved, const float* grad,
                   void* ws, size_t ws_bytes, float* dq, float* coef, hipStream_t stream) {
    NegArgs a{};
    a.q = q; a.c = c; a.iq = iq; a.target = target; a.filt_ptr = nnz > 0 ? filt_ptr : nullptr; a.filt_idx = filt_idx; a.nnz = nnz;
    a.neg = neg; a.K = K; a.rows_q = rows_q; a.N = N; a.B = B; a.d = d; a.bias = bias;
    a.scale = scale; a.margin = margin; a.alpha = alpha; a.saved = saved; a.grad = grad; a.dq = dq; a.coef = coef;
    const int rc = neg_open_launch("neg_bwd", a, ws_bytes);
    if (rc != GHF_OK) return rc;
    return mode == GHF_NEG_NEGSAMP ? neg_launch<true, NG_NEGSAMP>(a, stream) : neg_launch<true, NG_SOFTMAX>(a, stream);
}

}  // namespace ghf
