// relation_predict.hip — which relation holds between two given nodes: the score of EVERY relation for every pair
// (ghf.h: ghf_relation_scores, ghf_relation_scores_bwd_rows, ghf_relation_scores_bwd_weights).
//
//   out[i][u] = sum_l q_l b_l,   q = [a] + a . op(W[u]) + [bias[u]],   a = x[ia[i]],  b = x[ib[i]]
//
// q is the row ghf_relation_rows builds for (ix = ia[i], rel = u), bit for bit; it is never stored: nothing of size
// B x U x d exists, forward or backward.
//
// rp_sweep_kernel (a close cousin of relation_rows_kernel: same tile, same streamed W slices, same fp32 chain):
//   workgroup = 256 threads = 4 waves, one (64-row query tile, run of consecutive relations).  No grouping: every row
//   meets every relation.  The a tile is gathered into LDS once; op(W[u]) streams through two LDS buffers of 16 rows of k,
//   fetched into registers one slice ahead, ACROSS relations (the first slice of relation u + 1 is in flight while the last
//   of u is multiplied).  Wave w owns rows 16 w .. 16 w + 15 and all columns: DC / 16 accumulators of
//   v_mfma_f32_16x16x4_f32 (layouts as in relation.hip).  After a relation's last slice:
//     MODE 0 (scores): q = (a + s) + bias in the D layout, times the lane's b values (4 DC / 16 registers, loaded once per
//       tile), summed per lane over its columns c, c + 16, c + 32, .. ascending (one fmaf chain from 0), then across the 16
//       column lanes in four data-parallel-primitive steps: lane ^ 1, lane ^ 2, the other quad of the half row, the other
//       half row.  One fixed order: an entry depends on its own two rows, W[u] and bias[u] only.  The scores of the run
//       (at most 32 relations) are staged in LDS and written as runs of consecutive u.
//     MODE 1 (row gradients): rows[i] += G[i][u] q (one fmaf per element, u ascending); the tile's [64, d] sum is written
//       once, to the output or — when the relations of a tile are split over workgroups — to the split's partial, and
//       rp_sum_kernel adds the partials in split order.
//   The padded columns and the padded tail of k are multiplied as zeros (no test around the matrix instruction).
//
// rp_wgrad_kernel: dW[u] = sum_i G[i][u] a_i^T b_i, dbias[u] = sum_i G[i][u] b_i, i ascending: a GEMM whose contraction
//   runs over the QUERIES.  workgroup = (slab of queries, relation, 64 rows of dW[u]); blocks of 16 queries go through two
//   LDS buffers, the G-scaled a rows (64 columns of them) as the A operand, the b rows as the B operand; ids and G values
//   are fetched one block further ahead than the rows they name.  Slabs are reduced in slab order by rp_sum_kernel.
//
// Every id is clamped (tested against its range) before an address is formed from it: an id out of range reads nothing;
// its row of the scores / row gradients is NaN, and it adds nothing to the weight gradients.
#include <algorithm>

#include "common.h"
#include "rank_sweep.h"

namespace ghf {

constexpr int RP_ROWS = 64;                  // query rows per workgroup
constexpr int RP_BK = 16;                    // rows of k per weight slice / queries per block of the weight gradient
constexpr int RP_NT = 256;
constexpr int RP_MAX_D = 256;
constexpr int RP_CH = 32;                    // relations whose scores are staged before they are written
constexpr int RP_LDS_SC = RP_CH + 1;
constexpr int64_t RP_MAX_GRID = 1 << 20;     // workgroups per launch; the kernels stride over their work items
constexpr int RP_WG_MIN_SLAB = 64;           // fewest queries per slab of the weight gradient

static inline bool rp_sizes_ok(int64_t B, int64_t U, int d) {
    return B > 0 && B < ((int64_t)1 << 31) && U > 0 && U < (1 << 23) && d > 0 && d <= RP_MAX_D;
}
// relations per workgroup of the sweep.  Scores: at most RP_CH (the staging tile), fewer when there are few tiles (an entry does not depend on
// the split).  Row gradients: all of them unless the tiles alone leave the machine idle; then the partials cost
// (number of splits) x B x d floats, which the split count bounds by 512 tiles' worth.
static inline int rp_span(int64_t B, int U, bool scores) {
    const int64_t tiles = cdiv(B, RP_ROWS);
    int64_t splits = scores ? std::max<int64_t>(cdiv(U, RP_CH), cdiv(1024, tiles)) : std::max<int64_t>(1, 512 / tiles);
    splits = std::min<int64_t>(splits, U);
    return (int)cdiv(U, splits);
}
static inline int64_t rp_wgrad_slab(int64_t B, int U, int d) {     // queries per slab: a multiple of 16
    const int64_t items = (int64_t)U * cdiv(d, 64);
    int64_t slabs = std::max<int64_t>(1, std::min<int64_t>(cdiv(512, items), cdiv(B, RP_WG_MIN_SLAB)));
    return cdiv(cdiv(B, slabs), RP_BK) * RP_BK;
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

static inline size_t rp_lds_bytes(int NCT) {
    const int DC = NCT * 16;
    return ((size_t)RP_ROWS * (DC + 4) + 2 * (size_t)RP_BK * (DC + 16) + (size_t)RP_ROWS * RP_LDS_SC) * 4 + RP_ROWS * (8 + 8 + 4);
}

template <int NCT, bool TR, int MODE>
__global__ __launch_bounds__(RP_NT) void rp_sweep_kernel(const SweepArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int DC = NCT * 16, LDX = DC + 4, LDW = DC + 16, F4 = DC / 4, NL = RP_BK * F4 / RP_NT;
    float* Xs = lds;
    float* Ws = Xs + RP_ROWS * LDX;
    float* Sc = Ws + 2 * RP_BK * LDW;                       // MODE 0: the staged scores [row][relation of the run]
    int64_t* rowa = (int64_t*)(Sc + RP_ROWS * RP_LDS_SC);   // the row of x behind a, -1: none (a row of zeros)
    int64_t* rowb = rowa + RP_ROWS;                         // the row of x behind b, -1: none
    int* rowbad = (int*)(rowb + RP_ROWS);                   // an id out of range: the row of out is NaN
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int d = a.d, U = a.U;
    const int nsl = (d + RP_BK - 1) / RP_BK;
    const bool vx = rows_vec(a.x, d), vw = rows_vec(a.W, d);
    const float nan = __int_as_float(0x7FC00000);

    for (int64_t item = blockIdx.x; item < a.items; item += gridDim.x) {
        const int64_t row0 = (item % a.tiles) * RP_ROWS;    // tiles fastest: neighbouring workgroups stream the same relations
        const int64_t split = item / a.tiles;
        const int u_lo = (int)(split * a.span), u_hi = u_lo + a.span < U ? u_lo + a.span : U;
        const int nrows = (int)(a.B - row0 < RP_ROWS ? a.B - row0 : RP_ROWS);

        if (tid < RP_ROWS) {
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

        for (int idx = tid; idx < RP_ROWS * F4; idx += RP_NT) {
            const int row = idx / F4, c4 = idx - row * F4;
            const int64_t xr = rowa[row];
            *(f32x4*)(Xs + row * LDX + c4 * 4) = load_k4(xr >= 0 ? a.x + (size_t)xr * d : nullptr, c4 * 4, d, vx);
        }

        float bv[MODE == 0 ? NCT : 1][4];                   // MODE 0: the lane's b values, in the D layout
        if constexpr (MODE == 0) {
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int64_t xb = rowb[wave * 16 + 4 * (lane >> 4) + reg];
#pragma unroll
                for (int ct = 0; ct < NCT; ++ct) {
                    const int col = ct * 16 + (lane & 15);
                    bv[ct][reg] = (xb >= 0 && col < d) ? a.x[(size_t)xb * d + col] : 0.f;
                }
            }
        }

        f32x4 pre[NL];
        // slice s of relation u holds k = 16 s .. 16 s + 15 of op(W[u]) as [k][column], zeros past d either way
        auto fetch = [&](int u, int s) {
            const float* Wr = a.W + (size_t)u * d * d;
#pragma unroll
            for (int i = 0; i < NL; ++i) {
                const int idx = tid + RP_NT * i;
                if (TR) {
                    const int l = idx >> 2, c4 = idx & 3;
                    pre[i] = load_k4(l < d ? Wr + (size_t)l * d : nullptr, s * RP_BK + c4 * 4, d, vw);
                } else {
                    const int kk = idx / F4, c4 = idx - kk * F4, k = s * RP_BK + kk;
                    pre[i] = load_k4(k < d ? Wr + (size_t)k * d : nullptr, c4 * 4, d, vw);
                }
            }
        };
        auto stash = [&](int buf) {
            float* w = Ws + buf * RP_BK * LDW;
#pragma unroll
            for (int i = 0; i < NL; ++i) {
                const int idx = tid + RP_NT * i;
                if (TR) {
                    const int l = idx >> 2, c4 = idx & 3;
#pragma unroll
                    for (int e = 0; e < 4; ++e) w[(c4 * 4 + e) * LDW + l] = pre[i][e];
                } else {
                    const int kk = idx / F4, c4 = idx - kk * F4;
                    *(f32x4*)(w + kk * LDW + c4 * 4) = pre[i];
                }
            }
        };

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
        stash(0);
        __syncthreads();
        int buf = 0, u = u_lo, s = 0;
        for (;;) {
            int un = u, sn = s + 1;
            if (sn == nsl) { sn = 0; un = u + 1; }
            const bool more = un < u_hi;
            if (more) fetch(un, sn);
            if (s == 0) {
#pragma unroll
                for (int ct = 0; ct < NCT; ++ct) {
                    const int col = ct * 16 + (lane & 15);
                    bpre[ct] = (a.bias && col < d) ? a.bias[(size_t)u * d + col] : 0.f;
                }
                if constexpr (MODE == 1) {
#pragma unroll
                    for (int reg = 0; reg < 4; ++reg) {
                        const int row = wave * 16 + 4 * (lane >> 4) + reg;
                        g[reg] = row < nrows ? a.G[(size_t)(row0 + row) * U + u] : 0.f;
                    }
                }
            }
            const float* xa = Xs + (wave * 16 + (lane & 15)) * LDX + s * RP_BK + (lane >> 4);
            const float* wb = Ws + buf * RP_BK * LDW + (lane >> 4) * LDW + (lane & 15);
#pragma unroll
            for (int kq = 0; kq < RP_BK / 4; ++kq) {
                const float av = xa[4 * kq];
#pragma unroll
                for (int ct = 0; ct < NCT; ++ct)             // every tile, also the ones past d (zeros)
                    acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, wb[4 * kq * LDW + ct * 16], acc[ct], 0, 0, 0);
            }
            if (more) stash(buf ^ 1);
            if (s == nsl - 1) {                              // the relation's epilogue
                float p[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ct = 0; ct < NCT; ++ct) {
                    const int col = ct * 16 + (lane & 15);
#pragma unroll
                    for (int reg = 0; reg < 4; ++reg) {
                        float v = acc[ct][reg];
                        if (a.add_x) v = Xs[(wave * 16 + 4 * (lane >> 4) + reg) * LDX + col] + v;
                        if (a.bias) v += bpre[ct];
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
                        if ((lane & 15) == 0) Sc[(wave * 16 + 4 * (lane >> 4) + reg) * RP_LDS_SC + (u - u_lo)] = v;
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
            for (int idx = tid; idx < nrows * cnt; idx += RP_NT) {
                const int row = idx / cnt, j = idx - row * cnt;
                a.out[(size_t)(row0 + row) * U + u_lo + j] = rowbad[row] ? nan : Sc[row * RP_LDS_SC + j];
            }
        }
        if constexpr (MODE == 1) {                                     // the tile's sums: through the wave's own rows of the a tile
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
                for (int reg = 0; reg < 4; ++reg)
                    Xs[(wave * 16 + 4 * (lane >> 4) + reg) * LDX + ct * 16 + (lane & 15)] = racc[ct][reg];
            __syncthreads();
            float* dst = a.out + (size_t)split * (size_t)a.B * d;
            const bool vo = rows_vec(dst, d);
            const int nf4 = (d + 3) >> 2;
            for (int idx = tid; idx < nrows * nf4; idx += RP_NT) {
                const int row = idx / nf4, c4 = idx - row * nf4;
                f32x4 v = *(const f32x4*)(Xs + row * LDX + c4 * 4);
                if (rowbad[row]) v = f32x4{nan, nan, nan, nan};
                float* o = dst + (size_t)(row0 + row) * d + c4 * 4;
                if (vo) {
                    *(f32x4*)o = v;
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (c4 * 4 + e < d) o[e] = v[e];
                }
            }
        }
        __syncthreads();                                     // the next item rewrites the tile and the row tables
    }
}

// out[j] = part[0][j] + part[1][j] + .. in that order, j < n
__global__ __launch_bounds__(256) void rp_sum_kernel(const float* __restrict__ part, int64_t nparts, int64_t n, float* __restrict__ out) {
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < n; j += (int64_t)gridDim.x * 256) {
        float s = part[j];
        for (int64_t p = 1; p < nparts; ++p) s += part[p * n + j];
        out[j] = s;
    }
}

static int launch_rp_sum(const float* part, int64_t nparts, int64_t n, float* out, hipStream_t stream) {
    const unsigned grid = (unsigned)std::min<int64_t>(cdiv(n, 256), RP_MAX_GRID);
    rp_sum_kernel<<<grid, 256, 0, stream>>>(part, nparts, n, out);
    GHF_LAUNCH_CHECK();
    return GHF_OK;
}

template <int NCT, bool TR, int MODE>
static int launch_sweep(const SweepArgs& a, hipStream_t stream) {
    const size_t lds = rp_lds_bytes(NCT);
    GHF_SET_MAX_LDS((rp_sweep_kernel<NCT, TR, MODE>), lds);
    rp_sweep_kernel<NCT, TR, MODE><<<(unsigned)std::min<int64_t>(a.items, RP_MAX_GRID), RP_NT, lds, stream>>>(a);
    GHF_LAUNCH_CHECK();
    return GHF_OK;
}

template <int MODE>
static int dispatch_sweep(const SweepArgs& a, bool tr, hipStream_t stream) {
    const int d = a.d;
    if (d <= 64) return tr ? launch_sweep<4, true, MODE>(a, stream) : launch_sweep<4, false, MODE>(a, stream);
    if (d <= 128) return tr ? launch_sweep<8, true, MODE>(a, stream) : launch_sweep<8, false, MODE>(a, stream);
    if (d <= 192) return tr ? launch_sweep<12, true, MODE>(a, stream) : launch_sweep<12, false, MODE>(a, stream);
    return tr ? launch_sweep<16, true, MODE>(a, stream) : launch_sweep<16, false, MODE>(a, stream);
}

static int rp_check(const char* what, int64_t rows_x, int64_t B, int64_t U, int d, int flags, int allowed) {
    GHF_REQUIRE(d > 0 && rows_x > 0 && B > 0 && U > 0, "%s: bad shape", what);
    if (d > RP_MAX_D) return set_err(GHF_EUNSUPPORTED, "%s: d = %d exceeds %d", what, d, RP_MAX_D);
    GHF_REQUIRE((flags & ~allowed) == 0, "%s: unknown flags %d", what, flags);
    GHF_REQUIRE(rp_sizes_ok(B, U, d), "%s: B or U out of range", what);
    return GHF_OK;
}

int launch_relation_scores(const float* x, const int64_t* ia, const int64_t* ib, const float* W, const float* bias,
                           int64_t rows_x, int64_t B, int64_t U, int d, int flags, float* out, hipStream_t stream) {
    if (int rc = rp_check("relation_scores", rows_x, B, U, d, flags, GHF_REL_ADD_X | GHF_REL_TRANSPOSE)) return rc;
    SweepArgs a = {};
    a.x = x; a.ia = ia; a.ib = ib; a.W = W; a.bias = bias; a.rows_x = rows_x; a.B = B; a.U = (int)U; a.d = d;
    a.add_x = (flags & GHF_REL_ADD_X) ? 1 : 0; a.out = out;
    a.tiles = cdiv(B, RP_ROWS);
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
    a.tiles = cdiv(B, RP_ROWS);
    a.span = rp_span(B, a.U, false);
    const int64_t splits = cdiv(U, a.span);
    a.items = a.tiles * splits;
    a.out = splits > 1 ? (float*)ws : out;
    if (int rc = dispatch_sweep<1>(a, (flags & GHF_REL_TRANSPOSE) != 0, stream)) return rc;
    return splits > 1 ? launch_rp_sum((const float*)ws, splits, B * d, out, stream) : GHF_OK;
}

// ---- the weight gradients ---------------------------------------------------------------------------------------------
struct WgradArgs {
    const float* x; const int64_t* ia; const int64_t* ib; const float* G;
    int64_t rows_x, B, slab, items;
    int U, d, nkt;
    float* dW; float* dbias;                 // [slabs][U, d, d] and [slabs][U, d] (one slab: the outputs themselves)
};

template <int NCT>
__global__ __launch_bounds__(RP_NT) void rp_wgrad_kernel(const WgradArgs a) {
    constexpr int DC = NCT * 16, LDA = 64 + 16, LDB = DC + 16, F4 = DC / 4, NL = RP_BK * F4 / RP_NT;
    __shared__ __attribute__((aligned(16))) float As[2][RP_BK * LDA];     // [query of the block][64 columns of a], times G
    __shared__ __attribute__((aligned(16))) float Bs[2][RP_BK * LDB];     // [query of the block][all columns of b]
    __shared__ float Gs[2][RP_BK];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int d = a.d, U = a.U;
    const bool vx = rows_vec(a.x, d);

    for (int64_t item = blockIdx.x; item < a.items; item += gridDim.x) {
        const int kt = (int)(item % a.nkt);
        const int u = (int)((item / a.nkt) % U);
        const int64_t slab = item / ((int64_t)a.nkt * U);
        const int64_t q_lo = slab * a.slab, q_hi = q_lo + a.slab < a.B ? q_lo + a.slab : a.B;
        const int nblk = (int)((q_hi - q_lo + RP_BK - 1) / RP_BK);
        const bool do_bias = a.dbias && kt == 0;

        // the ids and the G value of the thread's rows of a block: a row past the slab or an id out of range is -1 (zeros)
        int64_t ra, rb[NL];
        float gr, gpre = 0.f;
        auto ids = [&](int blk) {
            const int64_t qa = q_lo + (int64_t)blk * RP_BK + (tid >> 4);
            ra = -1;
            gr = 0.f;
            if (qa < q_hi) {
                const int64_t v = a.ia[qa];
                if (v >= 0 && v < a.rows_x) { ra = v; gr = a.G[(size_t)qa * U + u]; }
            }
#pragma unroll
            for (int i = 0; i < NL; ++i) {
                const int64_t qb = q_lo + (int64_t)blk * RP_BK + (tid + RP_NT * i) / F4;
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
                const int idx = tid + RP_NT * i, qi = idx / F4, c4 = idx - qi * F4;
                preb[i] = load_k4(rb[i] >= 0 ? a.x + (size_t)rb[i] * d : nullptr, c4 * 4, d, vx);
            }
        };
        auto stash = [&](int buf) {
            *(f32x4*)(&As[buf][(tid >> 4) * LDA + (tid & 15) * 4]) = prea * gpre;
            if ((tid & 15) == 0) Gs[buf][tid >> 4] = gpre;
#pragma unroll
            for (int i = 0; i < NL; ++i) {
                const int idx = tid + RP_NT * i, qi = idx / F4, c4 = idx - qi * F4;
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
            for (int kq = 0; kq < RP_BK / 4; ++kq) {
                const float av = pa[4 * kq * LDA];
#pragma unroll
                for (int ct = 0; ct < NCT; ++ct)
                    acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, pb[4 * kq * LDB + ct * 16], acc[ct], 0, 0, 0);
            }
            if (do_bias && tid < DC) {
#pragma unroll
                for (int i = 0; i < RP_BK; ++i) bsum = fmaf(Gs[buf][i], Bs[buf][i * LDB + tid], bsum);
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
    rp_wgrad_kernel<NCT><<<(unsigned)std::min<int64_t>(a.items, RP_MAX_GRID), RP_NT, 0, stream>>>(a);
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
    int rc;
    if (d <= 64) rc = launch_wgrad<4>(a, stream);
    else if (d <= 128) rc = launch_wgrad<8>(a, stream);
    else if (d <= 192) rc = launch_wgrad<12>(a, stream);
    else rc = launch_wgrad<16>(a, stream);
    if (rc || slabs == 1) return rc;
    if ((rc = launch_rp_sum(pW, slabs, (int64_t)nW, dW, stream))) return rc;
    return dbias ? launch_rp_sum(pb, slabs, (int64_t)nb, dbias, stream) : GHF_OK;
}

}  // namespace ghf
