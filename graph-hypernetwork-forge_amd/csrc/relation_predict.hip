// relation_predict.hip — which relation holds between two given nodes: the score of EVERY relation for every pair
// (ghf.h: ghf_relation_scores, ghf_relation_scores_bwd_rows, ghf_relation_scores_bwd_weights).
//
//   out[i][u] = sum_l q_l b_l,   q = [a] + a . op(W[u]) + [bias[u]],   a = x[ia[i]],  b = x[ib[i]]
//
// q is the row ghf_relation_rows builds for (ix = ia[i], rel = u), bit for bit; it is never stored: nothing of size
// B x U x d exists, forward or backward.
//
// rp_sweep_kernel (tile, streamed W slices, LDS layout and the chain of q: relation_sweep.h, shared with
// relation_rows_kernel):
//   one workgroup per (64-row query tile, run of consecutive relations), striding over its grid.  No grouping: every row
//   meets every relation.  The a tile is gathered once per item; the slices are fetched one ahead ACROSS relations (the
//   first slice of relation u + 1 is in flight while the last of u is multiplied).  After a relation's last slice:
//     MODE 0 (scores): q = (a + s) + bias in the D layout, times the lane's b values (4 DC / 16 registers, loaded once per
//       tile), summed per lane over its columns c, c + 16, c + 32, .. ascending (one fmaf chain from 0), then across the 16
//       column lanes in four data-parallel-primitive steps: lane ^ 1, lane ^ 2, the other quad of the half row, the other
//       half row.  One fixed order: an entry depends on its own two rows, W[u] and bias[u] only.  The scores of the run
//       (at most 32 relations) are staged in LDS and written as runs of consecutive u.
//     MODE 1 (row gradients): rows[i] += G[i][u] q (one fmaf per element, u ascending); the tile's [64, d] sum is written
//       once, to the output or — when the relations of a tile are split over workgroups — to the split's partial, and
//       launch_ordered_sum adds the partials in split order.
//
// rp_wgrad_kernel: dW[u] = sum_i G[i][u] a_i^T b_i, dbias[u] = sum_i G[i][u] b_i, i ascending: a GEMM whose contraction
//   runs over the QUERIES.  workgroup = (slab of queries, relation, 64 rows of dW[u]); blocks of 16 queries go through two
//   LDS buffers, the G-scaled a rows (64 columns of them) as the A operand, the b rows as the B operand; ids and G values
//   are fetched one block further ahead than the rows they name (REL_BK is also the queries per block).  Slabs are reduced
//   in slab order by launch_ordered_sum.
//
// Every id is clamped (tested against its range) before an address is formed from it: an id out of range reads nothing;
// its row of the scores / row gradients is NaN, and it adds nothing to the weight gradients.
#include <algorithm>

#include "relation_sweep.h"

namespace ghf {

constexpr int RP_CH = 32;                    // relations whose scores are staged before they are written
constexpr int RP_LDS_SC = RP_CH + 1;
constexpr int RP_WG_MIN_SLAB = 64;           // fewest queries per slab of the weight gradient

static inline bool rp_sizes_ok(int64_t B, int64_t U, int d) {
    return B > 0 && B < ((int64_t)1 << 31) && U > 0 && U < (1 << 23) && d > 0 && d <= REL_MAX_D;
}
// relations per workgroup of the sweep.  Scores: at most RP_CH (the staging tile), fewer when there are few tiles (an entry does not depend on
// the split).  Row gradients: all of them unless the tiles alone leave the machine idle; then the partials cost
// (number of splits) x B x d floats, which the split count bounds by 512 tiles' worth.
static inline int rp_span(int64_t B, int U, bool scores) {
    const int64_t tiles = cdiv(B, REL_ROWS);
    int64_t splits = scores ? std::max<int64_t>(cdiv(U, RP_CH), cdiv(1024, tiles)) : std::max<int64_t>(1, 512 / tiles);
    splits = std::min<int64_t>(splits, U);
    return (int)cdiv(U, splits);
}
static inline int64_t rp_wgrad_slab(int64_t B, int U, int d) {     // queries per slab: a multiple of 16
    const int64_t items = (int64_t)U * cdiv(d, 64);
    int64_t slabs = std::max<int64_t>(1, std::min<int64_t>(cdiv(512, items), cdiv(B, RP_WG_MIN_SLAB)));
    return cdiv(cdiv(B, slabs), REL_BK) * REL_BK;
}

size_t relation_scores_bwd_rows_workspace_bytes(int64_t B, int U, int d) {
    if (!rp_sizes_ok(B, U, d)) return 0;
    const int64_t splits = cdiv(U, rp_span(B, U, false));
    return align_up(splits > 1 ? (size_t)splits * (size_t)B * d * sizeof(float) : 1, 256);
}
size_t relation_scores_bwd_weights_workspace_bytes(int64_t B, int U, int d) {
    if (!rp_sizes_ok(B, U, d)) return 0;
    const int64_t slabs = cdiv(B, rp_wgrad_slab(B, U, d));
    return align_up(slabs > 1 ? (size_t)slabs * (size_t)U * ((size_t)d * d + d) * sizeof(float) : 1, 256);
}

struct SweepArgs {
    const float* x; const int64_t* ia; const int64_t* ib; const float* W; const float* bias; const float* G;
    int64_t rows_x, B, tiles, items;
    int U, d, add_x, span;
    float* out;                              // MODE 0: [B, U]; MODE 1: [splits][B, d] (one split: the output itself)
};

template <int NCT, bool TR, int MODE>
__global__ __launch_bounds__(REL_NT) void rp_sweep_kernel(const SweepArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    using G = RelGeom<NCT>;
    float* Xs = lds;
    float* Ws = Xs + G::XS;
    float* Sc = Ws + G::WS;                                 // MODE 0: the staged scores [row][relation of the run]
    int64_t* rowa = (int64_t*)(Sc + REL_ROWS * RP_LDS_SC);   // the row of x behind a, -1: none (a row of zeros)
    int64_t* rowb = rowa + REL_ROWS;                         // the row of x behind b, -1: none
    int* rowbad = (int*)(rowb + REL_ROWS);                   // an id out of range: the row of out is NaN
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int d = a.d, U = a.U;
    const int nsl = (d + REL_BK - 1) / REL_BK;
    const bool vx = rows_vec(a.x, d), vw = rows_vec(a.W, d);
    const float nan = __int_as_float(0x7FC00000);

    for (int64_t item = blockIdx.x; item < a.items; item += gridDim.x) {
        const int64_t row0 = (item % a.tiles) * REL_ROWS;    // tiles fastest: neighbouring workgroups stream the same relations
        const int64_t split = item / a.tiles;
        const int u_lo = (int)(split * a.span), u_hi = u_lo + a.span < U ? u_lo + a.span : U;
        const int nrows = (int)(a.B - row0 < REL_ROWS ? a.B - row0 : REL_ROWS);

        if (tid < REL_ROWS) {
            int64_t ra = -1, rb = -1;
            int bad = 0;
            if (tid < nrows) {
                const int64_t va = a.ia[row0 + tid];
                if (va >= 0 && va < a.rows_x) ra = va; else bad = 1;
                if constexpr (MODE == 0) {
                    const int64_t vb = a.ib[row0 + tid];
                    if (vb >= 0 && vb < a.rows_x) rb = vb; else bad = 1;
                }
            }
            rowa[tid] = ra;
            rowb[tid] = rb;
            rowbad[tid] = bad;
        }
        __syncthreads();

        rel_gather<NCT>(Xs, rowa, a.x, d, vx, tid);

        float bv[MODE == 0 ? NCT : 1][4];                   // MODE 0: the lane's b values, in the D layout
        if constexpr (MODE == 0) {
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int64_t xb = rowb[rel_drow(wave, lane, reg)];
#pragma unroll
                for (int ct = 0; ct < NCT; ++ct) {
                    const int col = rel_dcol(ct, lane);
                    bv[ct][reg] = (xb >= 0 && col < d) ? a.x[(size_t)xb * d + col] : 0.f;
                }
            }
        }

        f32x4 pre[G::NL];
        auto fetch = [&](int u, int s) { rel_fetch<NCT, TR>(pre, a.W + (size_t)u * d * d, s, d, vw, tid); };

        f32x4 acc[NCT], racc[MODE == 1 ? NCT : 1];
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) acc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
        if constexpr (MODE == 1) {
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) racc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        float bpre[NCT];                                     // bias[u] of the lane's columns, requested at the first slice
        float g[4] = {0.f, 0.f, 0.f, 0.f};                   // MODE 1: G[row][u] of the lane's four rows

        fetch(u_lo, 0);
        rel_stash<NCT, TR>(pre, Ws, 0, tid);
        __syncthreads();
        int buf = 0, u = u_lo, s = 0;
        for (;;) {
            int un = u, sn = s + 1;
            if (sn == nsl) { sn = 0; un = u + 1; }
            const bool more = un < u_hi;
            if (more) fetch(un, sn);
            if (s == 0) {
                const float* bu = a.bias ? a.bias + (size_t)u * d : nullptr;
#pragma unroll
                for (int ct = 0; ct < NCT; ++ct) bpre[ct] = rel_bias(bu, rel_dcol(ct, lane), d);
                if constexpr (MODE == 1) {
#pragma unroll
                    for (int reg = 0; reg < 4; ++reg) {
                        const int row = rel_drow(wave, lane, reg);
                        g[reg] = row < nrows ? a.G[(size_t)(row0 + row) * U + u] : 0.f;
                    }
                }
            }
            rel_multiply<NCT>(acc, Xs, Ws, buf, s, lane, wave);
            if (more) rel_stash<NCT, TR>(pre, Ws, buf ^ 1, tid);
            if (s == nsl - 1) {                              // the relation's epilogue
                float p[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ct = 0; ct < NCT; ++ct) {
#pragma unroll
                    for (int reg = 0; reg < 4; ++reg) {
                        const float v = rel_value(acc[ct][reg], Xs + rel_drow(wave, lane, reg) * G::LDX + rel_dcol(ct, lane), a.add_x,
                                                  a.bias, bpre[ct]);
                        if constexpr (MODE == 0) p[reg] = fmaf(v, bv[ct][reg], p[reg]);
                        else racc[ct][reg] = fmaf(g[reg], v, racc[ct][reg]);
                    }
                    acc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
                }
                if constexpr (MODE == 0) {
#pragma unroll
                    for (int reg = 0; reg < 4; ++reg) {
                        float v = p[reg];
                        v += dpp_take<0xB1, 0xF>(v);         // lane ^ 1
                        v += dpp_take<0x4E, 0xF>(v);         // lane ^ 2
                        v += dpp_take<0x141, 0xF>(v);        // row_half_mirror: the other quad of the half row
                        v += dpp_take<0x140, 0xF>(v);        // row_mirror: the other half row
                        if ((lane & 15) == 0) Sc[rel_drow(wave, lane, reg) * RP_LDS_SC + (u - u_lo)] = v;
                    }
                }
            }
            __syncthreads();
            buf ^= 1;
            if (!more) break;
            u = un;
            s = sn;
        }

        if constexpr (MODE == 0) {                                     // the run's scores (span <= RP_CH): runs of consecutive u per row
            const int cnt = u_hi - u_lo;
            for (int idx = tid; idx < nrows * cnt; idx += REL_NT) {
                const int row = idx / cnt, j = idx - row * cnt;
                a.out[(size_t)(row0 + row) * U + u_lo + j] = rowbad[row] ? nan : Sc[row * RP_LDS_SC + j];
            }
        }
        if constexpr (MODE == 1) {                                     // the tile's sums: through the wave's own rows of the a tile
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
                for (int reg = 0; reg < 4; ++reg)
                    Xs[rel_drow(wave, lane, reg) * G::LDX + rel_dcol(ct, lane)] = racc[ct][reg];
            __syncthreads();
            float* dst = a.out + (size_t)split * (size_t)a.B * d;
            rel_store_rows<NCT>(Xs, rowbad, nrows, d, dst, rows_vec(dst, d), tid, [&](int row) { return row0 + row; });
        }
        __syncthreads();                                     // the next item rewrites the tile and the row tables
    }
}

template <int NCT, bool TR, int MODE>
static int launch_sweep(const SweepArgs& a, hipStream_t stream) {
    const size_t lds = (size_t)(RelGeom<NCT>::XS + RelGeom<NCT>::WS + REL_ROWS * RP_LDS_SC) * 4 + REL_ROWS * (8 + 8 + 4);   // + Sc; rowa, rowb, rowbad
    GHF_SET_MAX_LDS((rp_sweep_kernel<NCT, TR, MODE>), lds);
    rp_sweep_kernel<NCT, TR, MODE><<<(unsigned)std::min<int64_t>(a.items, MAX_GRID), REL_NT, lds, stream>>>(a);
    GHF_LAUNCH_CHECK();
    return GHF_OK;
}

template <int MODE>
static int dispatch_sweep(const SweepArgs& a, bool transpose, hipStream_t stream) {
    return rel_dispatch(a.d, transpose, [&](auto nct, auto tr) {
        return launch_sweep<decltype(nct)::value, decltype(tr)::value, MODE>(a, stream);
    });
}

static int rp_check(const char* what, int64_t rows_x, int64_t B, int64_t U, int d, int flags, int allowed) {
    if (int rc = rel_check(what, rows_x, B, U, d, flags, allowed)) return rc;
    GHF_REQUIRE(rp_sizes_ok(B, U, d), "%s: B or U out of range", what);
    return GHF_OK;
}

int launch_relation_scores(const float* x, const int64_t* ia, const int64_t* ib, const float* W, const float* bias,
                           int64_t rows_x, int64_t B, int64_t U, int d, int flags, float* out, hipStream_t stream) {
    if (int rc = rp_check("relation_scores", rows_x, B, U, d, flags, GHF_REL_ADD_X | GHF_REL_TRANSPOSE)) return rc;
    SweepArgs a = {};
    a.x = x; a.ia = ia; a.ib = ib; a.W = W; a.bias = bias; a.rows_x = rows_x; a.B = B; a.U = (int)U; a.d = d;
    a.add_x = (flags & GHF_REL_ADD_X) ? 1 : 0; a.out = out;
    a.tiles = cdiv(B, REL_ROWS);
    a.span = rp_span(B, a.U, true);
    a.items = a.tiles * cdiv(U, a.span);
    return dispatch_sweep<0>(a, (flags & GHF_REL_TRANSPOSE) != 0, stream);
}

int launch_relation_scores_bwd_rows(const float* x, const int64_t* ia, const float* G, const float* W, const float* bias,
                                    int64_t rows_x, int64_t B, int64_t U, int d, int flags, void* ws, size_t ws_bytes, float* out,
                                    hipStream_t stream) {
    if (int rc = rp_check("relation_scores_bwd_rows", rows_x, B, U, d, flags, GHF_REL_ADD_X | GHF_REL_TRANSPOSE)) return rc;
    const size_t need = relation_scores_bwd_rows_workspace_bytes(B, (int)U, d);
    GHF_REQUIRE(ws_bytes >= need, "relation_scores_bwd_rows: workspace of %zu bytes, need %zu", ws_bytes, need);
    SweepArgs a = {};
    a.x = x; a.ia = ia; a.G = G; a.W = W; a.bias = bias; a.rows_x = rows_x; a.B = B; a.U = (int)U; a.d = d;
    a.add_x = (flags & GHF_REL_ADD_X) ? 1 : 0;
    a.tiles = cdiv(B, REL_ROWS);
    a.span = rp_span(B, a.U, false);
    const int64_t splits = cdiv(U, a.span);
    a.items = a.tiles * splits;
    a.out = splits > 1 ? (float*)ws : out;
    if (int rc = dispatch_sweep<1>(a, (flags & GHF_REL_TRANSPOSE) != 0, stream)) return rc;
    return splits > 1 ? launch_ordered_sum((const float*)ws, splits, B * d, out, stream) : GHF_OK;
}

// ---- the weight gradients ---------------------------------------------------------------------------------------------
struct WgradArgs {
    const float* x; const int64_t* ia; const int64_t* ib; const float* G;
    int64_t rows_x, B, slab, items;
    int U, d, nkt;
    float* dW; float* dbias;                 // [slabs][U, d, d] and [slabs][U, d] (one slab: the outputs themselves)
};

template <int NCT>
__global__ __launch_bounds__(REL_NT) void rp_wgrad_kernel(const WgradArgs a) {
    using G = RelGeom<NCT>;                                 // the b rows are staged as the sweep stages a slice of W
    constexpr int DC = G::DC, LDA = 64 + 16, LDB = G::LDW, F4 = G::F4, NL = G::NL;
    __shared__ __attribute__((aligned(16))) float As[2][REL_BK * LDA];     // [query of the block][64 columns of a], times G
    __shared__ __attribute__((aligned(16))) float Bs[2][REL_BK * LDB];     // [query of the block][all columns of b]
    __shared__ float Gs[2][REL_BK];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int d = a.d, U = a.U;
    const bool vx = rows_vec(a.x, d);

    for (int64_t item = blockIdx.x; item < a.items; item += gridDim.x) {
        const int kt = (int)(item % a.nkt);
        const int u = (int)((item / a.nkt) % U);
        const int64_t slab = item / ((int64_t)a.nkt * U);
        const int64_t q_lo = slab * a.slab, q_hi = q_lo + a.slab < a.B ? q_lo + a.slab : a.B;
        const int nblk = (int)((q_hi - q_lo + REL_BK - 1) / REL_BK);
        const bool do_bias = a.dbias && kt == 0;

        // the ids and the G value of the thread's rows of a block: a row past the slab or an id out of range is -1 (zeros)
        int64_t ra, rb[NL];
        float gr, gpre = 0.f;
        auto ids = [&](int blk) {
            const int64_t qa = q_lo + (int64_t)blk * REL_BK + (tid >> 4);
            ra = -1;
            gr = 0.f;
            if (qa < q_hi) {
                const int64_t v = a.ia[qa];
                if (v >= 0 && v < a.rows_x) { ra = v; gr = a.G[(size_t)qa * U + u]; }
            }
#pragma unroll
            for (int i = 0; i < NL; ++i) {
                const int64_t qb = q_lo + (int64_t)blk * REL_BK + (tid + REL_NT * i) / F4;
                rb[i] = -1;
                if (qb < q_hi) {
                    const int64_t v = a.ib[qb];
                    if (v >= 0 && v < a.rows_x) rb[i] = v;
                }
            }
        };
        f32x4 prea, preb[NL];
        auto fetch = [&]() {
            prea = load_k4(ra >= 0 ? a.x + (size_t)ra * d : nullptr, kt * 64 + (tid & 15) * 4, d, vx);
            gpre = gr;
#pragma unroll
            for (int i = 0; i < NL; ++i) {
                const int idx = tid + REL_NT * i, qi = idx / F4, c4 = idx - qi * F4;
                preb[i] = load_k4(rb[i] >= 0 ? a.x + (size_t)rb[i] * d : nullptr, c4 * 4, d, vx);
            }
        };
        auto stash = [&](int buf) {
            *(f32x4*)(&As[buf][(tid >> 4) * LDA + (tid & 15) * 4]) = prea * gpre;
            if ((tid & 15) == 0) Gs[buf][tid >> 4] = gpre;
#pragma unroll
            for (int i = 0; i < NL; ++i) {
                const int idx = tid + REL_NT * i, qi = idx / F4, c4 = idx - qi * F4;
                *(f32x4*)(&Bs[buf][qi * LDB + c4 * 4]) = preb[i];
            }
        };

        f32x4 acc[NCT];
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) acc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
        float bsum = 0.f;

        ids(0);
        fetch();
        ids(1);
        stash(0);
        __syncthreads();
        int buf = 0;
        for (int blk = 0; blk < nblk; ++blk) {
            const bool more = blk + 1 < nblk;
            if (more) {
                fetch();                                     // the rows of block blk + 1, by the ids requested a block ago
                ids(blk + 2);
            }
            const float* pa = &As[buf][(lane >> 4) * LDA + wave * 16 + (lane & 15)];
            const float* pb = &Bs[buf][(lane >> 4) * LDB + (lane & 15)];
#pragma unroll
            for (int kq = 0; kq < REL_BK / 4; ++kq) {
                const float av = pa[4 * kq * LDA];
#pragma unroll
                for (int ct = 0; ct < NCT; ++ct)
                    acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, pb[4 * kq * LDB + ct * 16], acc[ct], 0, 0, 0);
            }
            if (do_bias && tid < DC) {
#pragma unroll
                for (int i = 0; i < REL_BK; ++i) bsum = fmaf(Gs[buf][i], Bs[buf][i * LDB + tid], bsum);
            }
            if (more) stash(buf ^ 1);
            __syncthreads();
            buf ^= 1;
        }

        float* dw = a.dW + ((size_t)slab * U + u) * (size_t)d * d;
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) {
            const int col = ct * 16 + (lane & 15);
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int k = kt * 64 + wave * 16 + 4 * (lane >> 4) + reg;
                if (k < d && col < d) dw[(size_t)k * d + col] = acc[ct][reg];
            }
        }
        if (do_bias && tid < d) a.dbias[((size_t)slab * U + u) * d + tid] = bsum;
    }
}

template <int NCT>
static int launch_wgrad(const WgradArgs& a, hipStream_t stream) {
    rp_wgrad_kernel<NCT><<<(unsigned)std::min<int64_t>(a.items, MAX_GRID), REL_NT, 0, stream>>>(a);
    GHF_LAUNCH_CHECK();
    return GHF_OK;
}

int launch_relation_scores_bwd_weights(const float* x, const int64_t* ia, const int64_t* ib, const float* G, int64_t rows_x,
                                       int64_t B, int64_t U, int d, int flags, void* ws, size_t ws_bytes, float* dW, float* dbias,
                                       hipStream_t stream) {
    if (int rc = rp_check("relation_scores_bwd_weights", rows_x, B, U, d, flags, 0)) return rc;
    const size_t need = relation_scores_bwd_weights_workspace_bytes(B, (int)U, d);
    GHF_REQUIRE(ws_bytes >= need, "relation_scores_bwd_weights: workspace of %zu bytes, need %zu", ws_bytes, need);
    WgradArgs a = {};
    a.x = x; a.ia = ia; a.ib = ib; a.G = G; a.rows_x = rows_x; a.B = B; a.U = (int)U; a.d = d;
    a.nkt = (int)cdiv(d, 64);
    a.slab = rp_wgrad_slab(B, a.U, d);
    const int64_t slabs = cdiv(B, a.slab);
    a.items = slabs * U * a.nkt;
    const size_t nW = (size_t)U * d * d, nb = (size_t)U * d;
    float* pW = (float*)ws;
    float* pb = pW + (size_t)slabs * nW;
    a.dW = slabs > 1 ? pW : dW;
    a.dbias = dbias ? (slabs > 1 ? pb : dbias) : nullptr;
    int rc = rel_dispatch(d, [&](auto nct) { return launch_wgrad<decltype(nct)::value>(a, stream); });
    if (rc || slabs == 1) return rc;
    if ((rc = launch_ordered_sum(pW, slabs, (int64_t)nW, dW, stream))) return rc;
    return dbias ? launch_ordered_sum(pb, slabs, (int64_t)nb, dbias, stream) : GHF_OK;
}

}  // namespace ghf
