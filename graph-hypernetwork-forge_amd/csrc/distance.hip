// distance.hip — negatives.hip's three operations (rank counts, the softmax loss, the negative-sampling loss; forward and
// backward) under a DISTANCE score instead of the dot product (include/ghf_distance.h):
//   s(i, j) = -D(q_i, c[n_ij]),   D = sum |delta| (L1),  sqrt(sum delta^2) (L2)  or  sum_p |delta_2p + i delta_2p+1| (COMPLEX),
// delta = q_i - c[v].  The geometry is negatives.hip's, through negatives_dev.h: one wave (K <= 256) or the four waves of a
// workgroup per query, a group of L lanes per row with four floats a lane, ids of the next step before this step's rows, all
// NG_U row loads of a lane issued before the first is consumed, no load under a branch, ids in 32 bits, fixed merge trees.
// Only the reduction differs: per lane |delta| or delta^2 summed (L1, L2) or the moduli of the lane's two pairs (COMPLEX),
// then group_sum<L>, and for L2 one square root behind it.  Lanes past d and absent rows load as zeros on both sides and add
// 0 to every distance.  On the scalar path (floats gl, gl + 64, ...) a complex pair sits in two adjacent lanes of the same
// register: the partner's delta^2 comes through the quad-perm DPP of group_sum (the sum is symmetric, so both lanes hold the
// same modulus) and the even lane carries it into the distance.
//
// The backward accumulates dq_i = -sum G g in registers, g = dD / dq: sign(delta) (L1), delta / D (L2), delta / rho_pair
// (COMPLEX), each 0 where its denominator is 0.  The gradient of a candidate row is +sum G g over the entries that name it,
// which is no multiple of q_i — ghf_segment_axpy cannot form it: dist_rows_grad_kernel does, one wave per node over
// ghf_group_edges' grouping, the node's row in registers, the entries of its segment in order.
//
// Square roots are v_sqrt_f32 and the divisions a multiplication by v_rcp_f32 (1 ulp each): the kernels are bound by the
// bytes in flight, and the IEEE sequences would add ten VALU instructions per root for bits nothing relies on — equal
// arguments give equal bits, which is what the rank counts need.  No floating-point atomics.
#include "common.h"
#include "rank_sweep.h"
#include "negatives.h"
#include "negatives_dev.h"
#include "distance.h"
#include "distance_dev.h"                        // dist_eval / dist_score / dist_grad, shared with pairwise.hip

namespace ghf {

size_t dist_workspace_bytes(int64_t B, int64_t K, int d, int64_t nnz) { return neg_workspace_bytes(B, K, d, nnz); }

// ---- forward ---------------------------------------------------------------------------------------------------------------
template <int M, int L, bool VEC, int MODE, int W>
__global__ __launch_bounds__(256) void dist_fwd_kernel(const NegArgs a) {
#pragma clang fp contract(off)                           // z is rounded before the margin is added, as in negatives.hip
    constexpr int G = 64 / L;                            // rows per wave instruction
    constexpr int STEP = NG_U * G;                       // positions per step of a wave
    const int lane = threadIdx.x & 63, gl = lane & (L - 1), g = lane / L, wv = threadIdx.x >> 6;
    const int64_t i = W == 1 ? (int64_t)blockIdx.x * 4 + wv : (int64_t)blockIdx.x;
    const int sub = W == 1 ? 0 : wv;                     // the wave's place among the query's W
    if (W == 1 && i >= a.B) return;                      // the whole wave, and no barrier on this path
    const int d = a.d;
    NegQuery s = neg_open<VEC, false>(a, i, gl);
    bool bad = false;                                    // a listed id or a negative outside its range
    for (int64_t e = s.lo + lane; e < s.hi; e += 64) bad |= (uint64_t)a.filt_idx[e] >= (uint64_t)a.N;
    const float t = dist_score<M, L, VEC>(s.qv, s.tv, gl);

    int ngt = 0, neq = 0;                                // K < 2^31
    float m = -INFINITY, S = 0.f, T = 0.f;               // softmax: (m, S); negsamp: (m, S, T) of alpha z

    const int64_t* __restrict__ nrow = a.neg + (size_t)i * a.K;
    int idn[NG_U];
#pragma unroll
    for (int u = 0; u < NG_U; ++u) idn[u] = neg_entry(nrow, sub * STEP + u * G + g, a.K, a.N);
    for (int64_t base = (int64_t)sub * STEP; base < a.K; base += W * STEP) {
        int id[NG_U];
        f32x4 row[NG_U];
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
            bad |= id[u] == -2;
            row[u] = neg_row<VEC>(a.c, id[u], gl, d);
            live[u] = id[u] >= 0;
        }
#pragma unroll
        for (int u = 0; u < NG_U; ++u)
            live[u] = live[u] && (int64_t)id[u] != s.tg && !(s.hi > s.lo && in_filter(a.filt_idx, s.lo, s.hi, (int64_t)id[u]));
#pragma unroll
        for (int u = 0; u < NG_U; ++u) {
            if constexpr (MODE == NG_RANK) {             // one row at a time (negatives.hip): row u waits for the count of row u - 1
                float r0 = row[u][0];
                asm volatile("" : "+v"(r0), "+v"(ngt));
                row[u][0] = r0;
            }
            const float sc = dist_score<M, L, VEC>(s.qv, row[u], gl);
            if constexpr (MODE == NG_RANK) {
                ngt += live[u] && sc > t ? 1 : 0;
                neq += live[u] && sc == t ? 1 : 0;
            } else {
                const float z = a.scale * sc;
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
        const float zt = a.scale * t;
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
        const float zt = a.scale * t;
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
template <int M, int L, bool VEC, int MODE, int W>
__global__ __launch_bounds__(256) void dist_bwd_kernel(const NegArgs a) {
#pragma clang fp contract(off)
    constexpr int G = 64 / L;
    constexpr int STEP = NG_U * G;
    const int lane = threadIdx.x & 63, gl = lane & (L - 1), g = lane / L, wv = threadIdx.x >> 6;
    const int64_t i = W == 1 ? (int64_t)blockIdx.x * 4 + wv : (int64_t)blockIdx.x;
    const int sub = W == 1 ? 0 : wv;
    if (W == 1 && i >= a.B) return;
    const int d = a.d;
    const NegQuery s = neg_open<VEC, false>(a, i, gl);
    const float sv = a.saved[i];                         // lse or lw: NaN = the query takes no part
    const bool part = s.ok && sv == sv;
    const float gs = a.grad[i] * a.scale;
    f32x4 tdl, trho;
    const float tD = dist_eval<M, L, VEC>(s.qv, s.tv, gl, tdl, trho);
    const float t = -tD;
    float* __restrict__ crow = a.coef + (size_t)i * (a.K + 1);

    f32x4 acc = {0.f, 0.f, 0.f, 0.f};                    // -sum G g of the lane's floats
    const int64_t* __restrict__ nrow = a.neg + (size_t)i * a.K;
    int idn[NG_U];
#pragma unroll
    for (int u = 0; u < NG_U; ++u) idn[u] = neg_entry(nrow, sub * STEP + u * G + g, a.K, a.N);
    for (int64_t base = (int64_t)sub * STEP; base < a.K; base += W * STEP) {
        int id[NG_U];
        f32x4 row[NG_U];
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
            live[u] = in;
        }
#pragma unroll
        for (int u = 0; u < NG_U; ++u)
            live[u] = live[u] && (int64_t)id[u] != s.tg && !(s.hi > s.lo && in_filter(a.filt_idx, s.lo, s.hi, (int64_t)id[u]));
#pragma unroll
        for (int u = 0; u < NG_U; ++u) {
            f32x4 dl, rho;
            const float D = dist_eval<M, L, VEC>(s.qv, row[u], gl, dl, rho);
            const float z = a.scale * -D;
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
            const f32x4 gr = dist_grad<M>(dl, rho, D);
            const float ng = -gv;
            const f32x4 nx = {fmaf(ng, gr[0], acc[0]), fmaf(ng, gr[1], acc[1]), fmaf(ng, gr[2], acc[2]), fmaf(ng, gr[3], acc[3])};
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
    const float zt = a.scale * t;
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
        const f32x4 gr = dist_grad<M>(tdl, trho, tD);
        const float ng = -gt;
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] = fmaf(ng, gr[e], acc[e]);
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

// ---- the gradient of the candidate rows ------------------------------------------------------------------------------------
// dc[v] = sum_{e in off[v] .. off[v + 1]} coef[perm[e]] g(q of entry perm[e], c[v]), e ascending.  One wave per node, the node's
// row in registers (the wave is one group: a lane holds four floats of it, as above), RG_U entries' loads in flight: perm,
// then coef and iq, then the query's row — none under a branch; an entry past the segment's end, or one whose perm / iq value
// is outside its range, repeats a load inside the arrays and counts with coefficient 0.  Whether there is an iq is a template
// parameter: as a test inside the loop it was a branch around the iq load, and the listing showed the four entries' loads
// one after the other, each behind its own wait.
constexpr int RG_U = 4;

struct RowsGradArgs {
    const float* q; const float* c; const int64_t* iq; int64_t rows_q, N, total;
    int d; unsigned K1;
    const float* coef; const int64_t* perm; const int64_t* off; float* dc;
};

template <int M, bool VEC, bool IQ>
__global__ __launch_bounds__(256) void dist_rows_grad_kernel(const RowsGradArgs a) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int64_t v = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (v >= a.N) return;                                // the whole wave
    const int d = a.d;
    const f32x4 cv = neg_slice<VEC>(a.c + (size_t)v * d, lane, d);
    int64_t e0 = a.off[v], e1 = a.off[v + 1];
    e0 = e0 < 0 ? 0 : (e0 > a.total ? a.total : e0);
    e1 = e1 < e0 ? e0 : (e1 > a.total ? a.total : e1);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int64_t e = e0; e < e1; e += RG_U) {
        float w[RG_U];
        f32x4 row[RG_U];
#pragma unroll
        for (int u = 0; u < RG_U; ++u) {
            const bool in = e + u < e1;
            const int64_t p = a.perm[in ? e + u : e1 - 1];
            const bool okp = in && (uint64_t)p < (uint64_t)a.total;
            const unsigned pp = okp ? (unsigned)p : 0u;
            const float x = a.coef[pp];
            const int64_t i = pp / a.K1;
            int64_t r = i;
            if constexpr (IQ) r = a.iq[i];
            const bool ok = okp && (uint64_t)r < (uint64_t)a.rows_q;
            row[u] = neg_row<VEC>(a.q, ok ? (int)r : -1, lane, d);
            w[u] = ok ? x : 0.f;
        }
#pragma unroll
        for (int u = 0; u < RG_U; ++u) {
            f32x4 dl, rho;
            const float D = dist_eval<M, 64, VEC>(row[u], cv, lane, dl, rho);
            const f32x4 gr = dist_grad<M>(dl, rho, D);
            const f32x4 nx = {fmaf(w[u], gr[0], acc[0]), fmaf(w[u], gr[1], acc[1]), fmaf(w[u], gr[2], acc[2]), fmaf(w[u], gr[3], acc[3])};
            acc = w[u] != 0.f ? nx : acc;
        }
    }
    float* __restrict__ out = a.dc + (size_t)v * d;
    if constexpr (VEC) {
        if (4 * lane < d) {
            if (((uintptr_t)out & 15) == 0) {
                *(f32x4*)(out + 4 * lane) = acc;
            } else {
#pragma unroll
                for (int m = 0; m < 4; ++m) out[4 * lane + m] = acc[m];
            }
        }
    } else {
#pragma unroll
        for (int m = 0; m < 4; ++m)
            if (lane + 64 * m < d) out[lane + 64 * m] = acc[m];
    }
}

// ---- launches --------------------------------------------------------------------------------------------------------------
static int dist_metric_check(const char* op, int metric, int d) {
    GHF_REQUIRE(metric == GHF_DIST_L1 || metric == GHF_DIST_L2 || metric == GHF_DIST_COMPLEX,
                "%s: metric must be GHF_DIST_L1, GHF_DIST_L2 or GHF_DIST_COMPLEX, got %d", op, metric);
    GHF_REQUIRE(metric != GHF_DIST_COMPLEX || (d & 1) == 0, "%s: GHF_DIST_COMPLEX needs an even d (re / im interleaved), got %d", op, d);
    return GHF_OK;
}

static int dist_open_launch(const char* op, int metric, const NegArgs& a, size_t ws_bytes) {
    GHF_REQUIRE(a.d > 0 && a.rows_q > 0 && a.N > 0 && a.B > 0 && a.K > 0 && a.nnz >= 0, "%s: bad shape", op);
    const int rc = dist_metric_check(op, metric, a.d);
    if (rc != GHF_OK) return rc;
    if (a.d > RK_MAX_D) return set_err(GHF_EUNSUPPORTED, "%s: d = %d exceeds %d", op, a.d, RK_MAX_D);
    GHF_REQUIRE(a.N < (int64_t)1 << 31, "%s: N out of range", op);            // the loops keep ids in 32 bits (neg_id32)
    const size_t need = dist_workspace_bytes(a.B, a.K, a.d, a.nnz);
    GHF_REQUIRE(need > 0, "%s: B (K + 1) out of range", op);
    GHF_REQUIRE(a.iq || a.B <= a.rows_q, "%s: B exceeds the rows of q", op);
    GHF_REQUIRE(ws_bytes >= need, "%s: workspace of %zu bytes, need %zu", op, ws_bytes, need);
    return GHF_OK;
}

template <int M, bool BWD, int MODE, int W>
static int dist_launch_path(const NegArgs& a, hipStream_t stream) {
    const unsigned grid = (unsigned)(W == 1 ? cdiv(a.B, 4) : a.B);
    const bool vec = (a.d & 3) == 0 && (((uintptr_t)a.q | (uintptr_t)a.c) & 15) == 0;      // forward and backward alike
#define GHF_DIST_GO(LL, VV)                                                              \
    do {                                                                                 \
        if constexpr (BWD) dist_bwd_kernel<M, LL, VV, MODE, W><<<grid, 256, 0, stream>>>(a); \
        else dist_fwd_kernel<M, LL, VV, MODE, W><<<grid, 256, 0, stream>>>(a);               \
    } while (0)
    if (!vec) GHF_DIST_GO(64, false);
    else if (a.d <= 32) GHF_DIST_GO(8, true);
    else if (a.d <= 64) GHF_DIST_GO(16, true);
    else if (a.d <= 128) GHF_DIST_GO(32, true);
    else GHF_DIST_GO(64, true);
#undef GHF_DIST_GO
    GHF_LAUNCH_CHECK();
    return GHF_OK;
}

template <bool BWD, int MODE>
static int dist_launch(int metric, const NegArgs& a, hipStream_t stream) {
    const bool one = neg_waves(a.K) == 1;
    switch (metric) {
        case GHF_DIST_L1: return one ? dist_launch_path<GHF_DIST_L1, BWD, MODE, 1>(a, stream) : dist_launch_path<GHF_DIST_L1, BWD, MODE, 4>(a, stream);
        case GHF_DIST_L2: return one ? dist_launch_path<GHF_DIST_L2, BWD, MODE, 1>(a, stream) : dist_launch_path<GHF_DIST_L2, BWD, MODE, 4>(a, stream);
        default: return one ? dist_launch_path<GHF_DIST_COMPLEX, BWD, MODE, 1>(a, stream) : dist_launch_path<GHF_DIST_COMPLEX, BWD, MODE, 4>(a, stream);
    }
}

int launch_dist_rank(int metric, const float* q, const float* c, const int64_t* iq, const int64_t* target,
                     const int64_t* filt_ptr, const int64_t* filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d,
                     const int64_t* neg, int64_t K, void* ws, size_t ws_bytes, int64_t* greater, int64_t* equal,
                     hipStream_t stream) {
    NegArgs a{};
    a.q = q; a.c = c; a.iq = iq; a.target = target; a.filt_ptr = nnz > 0 ? filt_ptr : nullptr; a.filt_idx = filt_idx; a.nnz = nnz;
    a.neg = neg; a.K = K; a.rows_q = rows_q; a.N = N; a.B = B; a.d = d; a.scale = 1.f;
    a.greater = (long long*)greater; a.equal = (long long*)equal;
    const int rc = dist_open_launch("dist_rank", metric, a, ws_bytes);
    if (rc != GHF_OK) return rc;
    return dist_launch<false, NG_RANK>(metric, a, stream);
}

int launch_dist_loss_fwd(int metric, int mode, const float* q, const float* c, const int64_t* iq, const int64_t* target,
                         const int64_t* filt_ptr, const int64_t* filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B,
                         int d, float scale, float margin, float alpha, const int64_t* neg, int64_t K, void* ws, size_t ws_bytes,
                         float* loss, float* aux, hipStream_t stream) {
    NegArgs a{};
    a.q = q; a.c = c; a.iq = iq; a.target = target; a.filt_ptr = nnz > 0 ? filt_ptr : nullptr; a.filt_idx = filt_idx; a.nnz = nnz;
    a.neg = neg; a.K = K; a.rows_q = rows_q; a.N = N; a.B = B; a.d = d;
    a.scale = scale; a.margin = margin; a.alpha = alpha; a.loss = loss; a.aux = aux;
    const int rc = dist_open_launch(mode == GHF_DIST_NEGSAMP ? "dist_negsamp_fwd" : "dist_softmax_fwd", metric, a, ws_bytes);
    if (rc != GHF_OK) return rc;
    return mode == GHF_DIST_NEGSAMP ? dist_launch<false, NG_NEGSAMP>(metric, a, stream) : dist_launch<false, NG_SOFTMAX>(metric, a, stream);
}

int launch_dist_bwd(int metric, int mode, const float* q, const float* c, const int64_t* iq, const int64_t* target,
                    const int64_t* filt_ptr, const int64_t* filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d,
                    float scale, float margin, float alpha, const int64_t* neg, int64_t K, const float* saved, const float* grad,
                    void* ws, size_t ws_bytes, float* dq, float* coef, hipStream_t stream) {
    NegArgs a{};
    a.q = q; a.c = c; a.iq = iq; a.target = target; a.filt_ptr = nnz > 0 ? filt_ptr : nullptr; a.filt_idx = filt_idx; a.nnz = nnz;
    a.neg = neg; a.K = K; a.rows_q = rows_q; a.N = N; a.B = B; a.d = d;
    a.scale = scale; a.margin = margin; a.alpha = alpha; a.saved = saved; a.grad = grad; a.dq = dq; a.coef = coef;
    const int rc = dist_open_launch("dist_bwd", metric, a, ws_bytes);
    if (rc != GHF_OK) return rc;
    return mode == GHF_DIST_NEGSAMP ? dist_launch<true, NG_NEGSAMP>(metric, a, stream) : dist_launch<true, NG_SOFTMAX>(metric, a, stream);
}

template <int M>
static int dist_rows_grad_go(const RowsGradArgs& a, hipStream_t stream) {
    const unsigned grid = (unsigned)cdiv(a.N, 4);
    const bool vec = (a.d & 3) == 0 && (((uintptr_t)a.q | (uintptr_t)a.c) & 15) == 0;
    if (vec && a.iq) dist_rows_grad_kernel<M, true, true><<<grid, 256, 0, stream>>>(a);
    else if (vec) dist_rows_grad_kernel<M, true, false><<<grid, 256, 0, stream>>>(a);
    else if (a.iq) dist_rows_grad_kernel<M, false, true><<<grid, 256, 0, stream>>>(a);
    else dist_rows_grad_kernel<M, false, false><<<grid, 256, 0, stream>>>(a);
    GHF_LAUNCH_CHECK();
    return GHF_OK;
}

int launch_dist_rows_grad(int metric, const float* q, const float* c, const int64_t* iq, int64_t rows_q, int64_t N, int64_t B,
                          int d, int64_t K, const float* coef, const int64_t* perm, const int64_t* off, float* dc,
                          hipStream_t stream) {
    GHF_REQUIRE(d > 0 && rows_q > 0 && N > 0 && B > 0 && K > 0, "dist_rows_grad: bad shape");
    const int rc = dist_metric_check("dist_rows_grad", metric, d);
    if (rc != GHF_OK) return rc;
    if (d > RK_MAX_D) return set_err(GHF_EUNSUPPORTED, "dist_rows_grad: d = %d exceeds %d", d, RK_MAX_D);
    GHF_REQUIRE(N < (int64_t)1 << 31 && rows_q < (int64_t)1 << 31, "dist_rows_grad: N or rows_q out of range");
    GHF_REQUIRE(dist_workspace_bytes(B, K, d, 0) > 0, "dist_rows_grad: B (K + 1) out of range");
    GHF_REQUIRE(iq || B <= rows_q, "dist_rows_grad: B exceeds the rows of q");
    RowsGradArgs a{};
    a.q = q; a.c = c; a.iq = iq; a.rows_q = rows_q; a.N = N; a.total = B * (K + 1); a.d = d; a.K1 = (unsigned)(K + 1);
    a.coef = coef; a.perm = perm; a.off = off; a.dc = dc;
    switch (metric) {
        case GHF_DIST_L1: return dist_rows_grad_go<GHF_DIST_L1>(a, stream);
        case GHF_DIST_L2: return dist_rows_grad_go<GHF_DIST_L2>(a, stream);
        default: return dist_rows_grad_go<GHF_DIST_COMPLEX>(a, stream);
    }
}

}  // namespace ghf
