// pairwise.hip — the pairwise ranking losses of a batch of queries against PER-QUERY negative sets neg [B, K]
// (include/ghf_pairwise.h), forward and backward, under the dot product or a distance:
//   u_ij = (z_ij - z_it) + margin,   loss_i = (1 / n_i) sum_{j in J_i} phi(u_ij),
//   phi(u) = max(u, 0) (hinge: TransE's margin ranking loss)  or  softplus(u) (logistic: BPR at margin 0).
// Every term couples one negative to its query's positive, so the target's coefficient is the negated sum of the row's:
// G_it = -sum_j G_ij.  None of negatives.hip's or distance.hip's epilogues has that form; the rest is theirs.
//
// The geometry is negatives.hip's, through negatives_dev.h: one wave (K <= 256) or the four waves of a workgroup per query, a
// group of L lanes per row with four floats a lane, ids of the next step before this step's rows, all NG_U row loads of a lane
// issued before the first is consumed, no load under a branch, ids in 32 bits.  The score of a position is formed by the code
// of ghf_neg_rank (pair_dot = negatives.hip's neg_dot) or of ghf_dist_rank (distance_dev.h), so `active` at margin 0 is that
// call's `greater`.  One kernel text per direction over the score policy M (0: dot; GHF_DIST_L1 / L2 / COMPLEX) and the kind.
//
// Forward, one pass: z_it is known before the loop; the state is one float sum and two integer counts per lane (every lane
// of a group holds its group's), merged over the groups by the fixed butterfly and over the four waves through LDS in wave
// order.  No branch in the loop: a position outside J_i adds 0.f and 0.
// Backward, one pass: G_ij goes to coef as it is formed, dq_i and the running sum of G_ij accumulate together in registers,
// merge the same way, and the target's term — its coefficient is minus that sum — is applied after the merge.  1 / n_i comes
// from the saved count.  d embs and d bias are ghf_group_edges + ghf_segment_axpy (dot) or ghf_dist_rows_grad (distance) over
// coef (autograd.PairwiseLossFn).  No floating-point atomics.
#include "common.h"
#include "rank_sweep.h"
#include "negatives.h"
#include "negatives_dev.h"
#include "distance_dev.h"
#include "pairwise.h"

namespace ghf {

size_t pair_workspace_bytes(int64_t B, int64_t K, int d, int64_t nnz) { return neg_workspace_bytes(B, K, d, nnz); }

constexpr int PR_DOT = GHF_PAIR_DOT;             // the score policy M: 0, or a metric of distance_dev.h (1, 2, 3)

struct PairArgs {
    NegArgs n;                                   // q .. K, scale, margin as the per-query kernels read them; loss, grad, dq, coef
    int* count; int* active;                     // forward: n_i and the violated pairs, int32 [B]
    const int* saved;                            // backward: the forward's count
    int normalize;
};

// negatives.hip's neg_dot, restated: the same four operations in the same order
__device__ __forceinline__ float pair_dot(f32x4 x, f32x4 y) {
    return fmaf(x[3], y[3], fmaf(x[2], y[2], fmaf(x[1], y[1], x[0] * y[0])));
}

// s(x, y) in every lane of the group
template <int M, int L, bool VEC>
__device__ __forceinline__ float pair_score(const f32x4 x, const f32x4 y, int gl) {
    if constexpr (M == PR_DOT) return group_sum<L>(pair_dot(x, y));
    else return dist_score<M, L, VEC>(x, y, gl);
}

// ---- forward ---------------------------------------------------------------------------------------------------------------
template <int M, int L, bool VEC, bool HINGE, bool BIAS, int W>
__global__ __launch_bounds__(256) void pair_fwd_kernel(const PairArgs p) {
#pragma clang fp contract(off)                           // u = (z - z_t) + margin: two roundings, as the header says
    static_assert(M == PR_DOT || !BIAS, "no bias under a distance");
    const NegArgs& a = p.n;
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
    const float t = pair_score<M, L, VEC>(s.qv, s.tv, gl);
    float zt;
    if constexpr (BIAS) zt = fmaf(a.scale, t, s.tb);
    else zt = a.scale * t;

    float S = 0.f;                                       // sum of phi(u) over the group's positions, in order
    int cnt = 0, act = 0;                                // K < 2^31

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
            // One row at a time (negatives.hip's rank mode): the loop has no branch to order the eight scores of a step, and
            // side by side they cost the registers of eight reductions: row u waits for the sum of row u - 1.
            float r0 = row[u][0];
            asm volatile("" : "+v"(r0), "+v"(S));
            row[u][0] = r0;
            const float sc = pair_score<M, L, VEC>(s.qv, row[u], gl);
            float z;
            if constexpr (BIAS) z = fmaf(a.scale, sc, b[u]);
            else z = a.scale * sc;
            const float y = (z - zt) + a.margin;
            float phi;
            if constexpr (HINGE) phi = y <= 0.f ? 0.f : y;          // not fmaxf: a NaN stays a NaN
            else phi = softplus(y);
            S += live[u] ? phi : 0.f;
            cnt += live[u] ? 1 : 0;
            act += live[u] && y > 0.f ? 1 : 0;
        }
    }
    bad = __any(bad);

    // the groups' partials, merged in a fixed tree; then the waves' (W > 1), in wave order, by wave 0
#pragma unroll
    for (int w = L; w < 64; w *= 2) {
        S += neg_xor(S, w);
        cnt += __shfl_xor(cnt, w, 64);
        act += __shfl_xor(act, w, 64);
    }
    if constexpr (W > 1) {
        __shared__ float shf[W];
        __shared__ int shi[W][4];
        if (lane == 0) { shf[wv] = S; shi[wv][0] = cnt; shi[wv][1] = act; shi[wv][2] = bad; }
        __syncthreads();
        if (wv != 0) return;
        for (int w = 1; w < W; ++w) { S += shf[w]; cnt += shi[w][0]; act += shi[w][1]; bad |= shi[w][2] != 0; }
    }
    s.ok = s.ok && !bad;
    float l = S;
    if (p.normalize) l = cnt > 0 ? S * (1.f / (float)cnt) : 0.f;
    if (lane == 0) {
        a.loss[i] = s.ok ? l : __int_as_float(0x7FC00000);
        p.count[i] = s.ok ? cnt : -1;
        p.active[i] = s.ok ? act : -1;
    }
}

// ---- backward --------------------------------------------------------------------------------------------------------------
template <int M, int L, bool VEC, bool HINGE, bool BIAS, int W>
__global__ __launch_bounds__(256) void pair_bwd_kernel(const PairArgs p) {
#pragma clang fp contract(off)
    static_assert(M == PR_DOT || !BIAS, "no bias under a distance");
    const NegArgs& a = p.n;
    constexpr int G = 64 / L;
    constexpr int STEP = NG_U * G;
    const int lane = threadIdx.x & 63, gl = lane & (L - 1), g = lane / L, wv = threadIdx.x >> 6;
    const int64_t i = W == 1 ? (int64_t)blockIdx.x * 4 + wv : (int64_t)blockIdx.x;
    const int sub = W == 1 ? 0 : wv;
    if (W == 1 && i >= a.B) return;
    const int d = a.d;
    const NegQuery s = neg_open<VEC, BIAS>(a, i, gl);
    const int n = p.saved[i];                            // -1: the query takes no part; 0: no pair, an all-zero row
    const bool part = s.ok && n >= 0;
    const float gs = a.grad[i] * a.scale;
    const float wi = p.normalize ? gs * (n > 0 ? 1.f / (float)n : 0.f) : gs;
    f32x4 tdl = {0.f, 0.f, 0.f, 0.f}, trho = tdl;
    float tD = 0.f, t;
    if constexpr (M == PR_DOT) {
        t = group_sum<L>(pair_dot(s.qv, s.tv));
    } else {
        tD = dist_eval<M, L, VEC>(s.qv, s.tv, gl, tdl, trho);
        t = -tD;
    }
    float zt;
    if constexpr (BIAS) zt = fmaf(a.scale, t, s.tb);
    else zt = a.scale * t;
    float* __restrict__ crow = a.coef + (size_t)i * (a.K + 1);

    f32x4 acc = {0.f, 0.f, 0.f, 0.f};                    // dq of the lane's floats
    float Gs = 0.f;                                      // sum of G_ij over the group's positions, in order
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
            f32x4 dl, rho;
            float D = 0.f, sc;
            if constexpr (M == PR_DOT) {
                sc = group_sum<L>(pair_dot(s.qv, row[u]));
            } else {
                D = dist_eval<M, L, VEC>(s.qv, row[u], gl, dl, rho);
                sc = -D;
            }
            float z;
            if constexpr (BIAS) z = fmaf(a.scale, sc, b[u]);
            else z = a.scale * sc;
            const float y = (z - zt) + a.margin;
            float gv;
            if constexpr (HINGE) {
                gv = y > 0.f ? wi : 0.f;
            } else {                                     // sigmoid(y), as neg_bwd forms it
                const float e = __expf(-fabsf(y)), rcp = __builtin_amdgcn_rcpf(1.f + e);
                gv = wi * (y >= 0.f ? rcp : e * rcp);
            }
            gv = live[u] ? gv : 0.f;
            const int64_t j = base + u * G + g;
            if (gl == 0 && j < a.K) crow[j] = gv;
            Gs += gv;
            // positions in order within the group; a zero coefficient adds nothing, whatever the row holds
            f32x4 nx;
            if constexpr (M == PR_DOT) {
                nx = f32x4{fmaf(gv, row[u][0], acc[0]), fmaf(gv, row[u][1], acc[1]), fmaf(gv, row[u][2], acc[2]),
                           fmaf(gv, row[u][3], acc[3])};
            } else {
                const f32x4 gr = dist_grad<M>(dl, rho, D);
                const float ng = -gv;
                nx = f32x4{fmaf(ng, gr[0], acc[0]), fmaf(ng, gr[1], acc[1]), fmaf(ng, gr[2], acc[2]), fmaf(ng, gr[3], acc[3])};
            }
            acc = gv != 0.f ? nx : acc;
        }
    }
#pragma unroll
    for (int w = L; w < 64; w *= 2) {
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] += neg_xor(acc[e], w);
        Gs += neg_xor(Gs, w);
    }
    if constexpr (W > 1) {                               // the waves' sums, in wave order, by wave 0
        __shared__ f32x4 shq[W][64];
        __shared__ float shg[W];
        shq[wv][lane] = acc;
        if (lane == 0) shg[wv] = Gs;
        __syncthreads();
        if (wv != 0) return;
        for (int w = 1; w < W; ++w) {
            const f32x4 o = shq[w][lane];
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] += o[e];
            Gs += shg[w];
        }
    }
    // the target's entry, last: minus the row's sum
    const float gt = part ? 0.f - Gs : 0.f;
    if (gt != 0.f) {
        if constexpr (M == PR_DOT) {
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] = fmaf(gt, s.tv[e], acc[e]);
        } else {
            const f32x4 gr = dist_grad<M>(tdl, trho, tD);
            const float ng = -gt;
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] = fmaf(ng, gr[e], acc[e]);
        }
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
static int pair_open_launch(const char* op, const NegArgs& a, size_t ws_bytes) {
    GHF_REQUIRE(a.d > 0 && a.rows_q > 0 && a.N > 0 && a.B > 0 && a.K > 0 && a.nnz >= 0, "%s: bad shape", op);
    if (a.d > RK_MAX_D) return set_err(GHF_EUNSUPPORTED, "%s: d = %d exceeds %d", op, a.d, RK_MAX_D);
    GHF_REQUIRE(a.N < (int64_t)1 << 31, "%s: N out of range", op);            // the loops keep ids in 32 bits (neg_id32)
    const size_t need = pair_workspace_bytes(a.B, a.K, a.d, a.nnz);
    GHF_REQUIRE(need > 0, "%s: B (K + 1) out of range", op);
    GHF_REQUIRE(a.iq || a.B <= a.rows_q, "%s: B exceeds the rows of q", op);
    GHF_REQUIRE(ws_bytes >= need, "%s: workspace of %zu bytes, need %zu", op, ws_bytes, need);
    return GHF_OK;
}

template <int M, bool BWD, bool HINGE, bool BIAS, int W>
static int pair_launch_path(const PairArgs& p, hipStream_t stream) {
    const NegArgs& a = p.n;
    const unsigned grid = (unsigned)(W == 1 ? cdiv(a.B, 4) : a.B);
    const bool vec = (a.d & 3) == 0 && (((uintptr_t)a.q | (uintptr_t)a.c) & 15) == 0;      // forward and backward alike
#define GHF_PAIR_GO(LL, VV)                                                                        \
    do {                                                                                           \
        if constexpr (BWD) pair_bwd_kernel<M, LL, VV, HINGE, BIAS, W><<<grid, 256, 0, stream>>>(p); \
        else pair_fwd_kernel<M, LL, VV, HINGE, BIAS, W><<<grid, 256, 0, stream>>>(p);               \
    } while (0)
    if (!vec) GHF_PAIR_GO(64, false);
    else if (a.d <= 32) GHF_PAIR_GO(8, true);
    else if (a.d <= 64) GHF_PAIR_GO(16, true);
    else if (a.d <= 128) GHF_PAIR_GO(32, true);
    else GHF_PAIR_GO(64, true);
#undef GHF_PAIR_GO
    GHF_LAUNCH_CHECK();
    return GHF_OK;
}

template <int M, bool BWD, bool HINGE>
static int pair_launch_metric(const PairArgs& p, hipStream_t stream) {
    const bool one = neg_waves(p.n.K) == 1;
    if constexpr (M == PR_DOT) {
        if (p.n.bias) return one ? pair_launch_path<M, BWD, HINGE, true, 1>(p, stream) : pair_launch_path<M, BWD, HINGE, true, 4>(p, stream);
    }
    return one ? pair_launch_path<M, BWD, HINGE, false, 1>(p, stream) : pair_launch_path<M, BWD, HINGE, false, 4>(p, stream);
}

// the public metric and kind, translated once into template parameters
template <bool BWD>
static int pair_launch(int metric, int kind, const PairArgs& p, hipStream_t stream) {
    const bool hinge = kind == GHF_PAIR_HINGE;
    switch (metric) {
        case GHF_PAIR_DOT: return hinge ? pair_launch_metric<PR_DOT, BWD, true>(p, stream) : pair_launch_metric<PR_DOT, BWD, false>(p, stream);
        case GHF_DIST_L1: return hinge ? pair_launch_metric<GHF_DIST_L1, BWD, true>(p, stream) : pair_launch_metric<GHF_DIST_L1, BWD, false>(p, stream);
        case GHF_DIST_L2: return hinge ? pair_launch_metric<GHF_DIST_L2, BWD, true>(p, stream) : pair_launch_metric<GHF_DIST_L2, BWD, false>(p, stream);
        default: return hinge ? pair_launch_metric<GHF_DIST_COMPLEX, BWD, true>(p, stream) : pair_launch_metric<GHF_DIST_COMPLEX, BWD, false>(p, stream);
    }
}

static int pair_selectors_check(const char* op, int metric, int kind, int d, const float* bias) {
    GHF_REQUIRE(metric == GHF_PAIR_DOT || metric == GHF_DIST_L1 || metric == GHF_DIST_L2 || metric == GHF_DIST_COMPLEX,
                "%s: metric must be GHF_PAIR_DOT, GHF_DIST_L1, GHF_DIST_L2 or GHF_DIST_COMPLEX, got %d", op, metric);
    GHF_REQUIRE(metric != GHF_DIST_COMPLEX || (d & 1) == 0, "%s: GHF_DIST_COMPLEX needs an even d (re / im interleaved), got %d", op, d);
    GHF_REQUIRE(kind == GHF_PAIR_HINGE || kind == GHF_PAIR_LOGISTIC, "%s: kind must be GHF_PAIR_HINGE or GHF_PAIR_LOGISTIC, got %d", op, kind);
    GHF_REQUIRE(metric == GHF_PAIR_DOT || !bias, "%s: no per-candidate bias under a distance", op);
    return GHF_OK;
}

int launch_pair_fwd(int metric, int kind, const float* q, const float* c, const int64_t* iq, const int64_t* target,
                    const int64_t* filt_ptr, const int64_t* filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d,
                    float scale, float margin, int normalize, const int64_t* neg, int64_t K, const float* bias, void* ws,
                    size_t ws_bytes, float* loss, int32_t* count, int32_t* active, hipStream_t stream) {
    PairArgs p{};
    NegArgs& a = p.n;
    a.q = q; a.c = c; a.iq = iq; a.target = target; a.filt_ptr = nnz > 0 ? filt_ptr : nullptr; a.filt_idx = filt_idx; a.nnz = nnz;
    a.neg = neg; a.K = K; a.rows_q = rows_q; a.N = N; a.B = B; a.d = d; a.bias = bias;
    a.scale = scale; a.margin = margin; a.loss = loss;
    p.count = count; p.active = active; p.normalize = normalize;
    int rc = pair_selectors_check("pair_fwd", metric, kind, d, bias);
    if (rc != GHF_OK) return rc;
    rc = pair_open_launch("pair_fwd", a, ws_bytes);
    if (rc != GHF_OK) return rc;
    return pair_launch<false>(metric, kind, p, stream);
}

int launch_pair_bwd(int metric, int kind, const float* q, const float* c, const int64_t* iq, const int64_t* target,
                    const int64_t* filt_ptr, const int64_t* filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d,
                    float scale, float margin, int normalize, const int64_t* neg, int64_t K, const float* bias,
                    const int32_t* count, const float* grad, void* ws, size_t ws_bytes, float* dq, float* coef,
                    hipStream_t stream) {
    PairArgs p{};
    NegArgs& a = p.n;
    a.q = q; a.c = c; a.iq = iq; a.target = target; a.filt_ptr = nnz > 0 ? filt_ptr : nullptr; a.filt_idx = filt_idx; a.nnz = nnz;
    a.neg = neg; a.K = K; a.rows_q = rows_q; a.N = N; a.B = B; a.d = d; a.bias = bias;
    a.scale = scale; a.margin = margin; a.grad = grad; a.dq = dq; a.coef = coef;
    p.saved = count; p.normalize = normalize;
    int rc = pair_selectors_check("pair_bwd", metric, kind, d, bias);
    if (rc != GHF_OK) return rc;
    rc = pair_open_launch("pair_bwd", a, ws_bytes);
    if (rc != GHF_OK) return rc;
    return pair_launch<true>(metric, kind, p, stream);
}

}  // namespace ghf
