// distance.hip — negatives.hip's three operations (rank counts, the softmax loss, the negative-sampling loss; forward and
// backward) under a DISTANCE score instead of the dot product (include/ghf_distance.h):
//   s(i, j) = -D(q_i, c[n_ij]),   D = sum |delta| (L1),  sqrt(sum delta^2) (L2)  or  sum_p |delta_2p + i delta_2p+1| (COMPLEX),
// delta = q_i - c[v].  The kernel is negatives.hip's too — negatives_dev.h's pq_kernel under DistScore<metric> (distance_dev.h;
// §23) — and so is the geometry: one wave (K <= 256) or the four waves of a
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
#include "distance_dev.h"                        // dist_eval / dist_grad / DistScore, shared with pairwise.hip

namespace ghf {

size_t dist_workspace_bytes(int64_t B, int64_t K, int d, int64_t nnz) { return neg_workspace_bytes(B, K, d, nnz); }

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

int launch_dist(int metric, PqEpi e, bool bwd, const char* op, const NegArgs& a, size_t ws_bytes, hipStream_t stream) {
    int rc = dist_metric_check(op, metric, a.d);
    if (rc == GHF_OK) rc = pq_open_launch(op, e, bwd, a, ws_bytes);
    if (rc != GHF_OK) return rc;
    switch (metric) {
        case GHF_DIST_L1: return pq_launch_set<DistScore<GHF_DIST_L1>>(e, bwd, a, stream);
        case GHF_DIST_L2: return pq_launch_set<DistScore<GHF_DIST_L2>>(e, bwd, a, stream);
        default: return pq_launch_set<DistScore<GHF_DIST_COMPLEX>>(e, bwd, a, stream);
    }
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
