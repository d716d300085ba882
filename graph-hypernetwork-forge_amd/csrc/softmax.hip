// softmax.hip — the 1-vs-all softmax link-prediction loss against every node, forward and backward, the B x N logits never
// stored (include/ghf.h: ghf_score_softmax_fwd / ghf_score_softmax_bwd).
//
//   lse[i] = log sum_{j in J_i} exp(scale s(i, j)),   loss[i] = lse[i] - scale s(i, target[i])
//
// with s(i, j) the sweep's fp32 chain (rank_sweep.h) and J_i every candidate outside query i's filter list, the target
// always inside.
//
// Forward: rank_tile_kernel with its third epilogue.  A lane keeps a running (max, sum) per query column and folds a
// finished candidate tile's 32 registers of that column into it; a listed candidate is masked BEFORE it enters the sum
// (a query's known partners are the candidates that score highest: taking their terms out of a total afterwards cancels
// catastrophically).  Lists are sorted and candidates arrive in ascending id, so a lane carries a cursor into its query's
// list and only a tile whose id range holds a listed id looks ids up.  Partials merge in a fixed order: the half-waves and
// waves of a workgroup through LDS, one (max, sum) per (query, slab) in the workspace, softmax_finish_kernel over the
// slabs in slab order.  The slabs depend on N and d alone, so a query's loss has the same bits whatever batch it is in.
//
// Backward: softmax_bwd_kernel recomputes score tiles from the saved lse, as an attention backward does:
//   G_ij = grad[i] scale (p_ij - [j = target[i]]),   p_ij = exp(scale s(i,j) - lse[i]) on J_i, 0 outside
//   dq[i] = sum_j G_ij c[j]       a workgroup owns (query tile, candidate slab): candidates stream, one partial per slab,
//                                  the partials summed in slab order (launch_ordered_sum)
//   dc[j] = sum_i G_ij q[iq[i]]   a workgroup owns a candidate tile, streams ALL query tiles in ascending order and
//                                  writes its rows once
// One kernel serves both: 256 threads, an owner tile (128 rows; 64 for d > 128) resident in LDS, streamed tiles of 64
// whole-d rows in a second LDS buffer.  Per streamed tile: the score product (candidates the A operand, queries the B
// operand, so a lane holds ONE query's lse / gradient / target for its accumulator column), G into LDS as [streamed k]
// [owner row], then the second product out[owner, d] += G^T-or-G . Y on the same fp32 matrix instruction, the streamed
// rows read across (the k permutation of their groups of 8 undone in the column index).  Sums run over streamed rows in
// ascending order: no floating-point atomics, bit-reproducible.
// Masking in the backward: the dq sweep uses the forward's cursor.  The dc sweep's queries change every step, so a
// workgroup first collects the (query, candidate) pairs of all lists that fall
// into ITS candidate tile (one coalesced pass over filt_idx) and zeroes those entries of G in LDS after each step's
// epilogue; a tile that more than SB_HCAP pairs fall into (a hub listed by thousands of queries) looks every id up instead.
//
// The multi-label BCE loss (bce.hip) runs its backward through the same kernel (LOSS = SB_BCE): only G differs,
//   G_ij = grad[i] scale (sigma(scale s(i,j)) - smoothing / N - (1 - smoothing) [j listed]),
// the lists naming positives, not masks: the dq sweep's cursor says which steps hold listed ids, and the dc sweep's collected
// pairs SUBTRACT grad scale (1 - smoothing) from their entries of G instead of zeroing them.
//
// The self-adversarial negative-sampling loss (negsamp.hip) is the kernel's third loss (LOSS = SB_NEGSAMP), the
// saved per-query value being lw = log sum_{j in J_i} exp(alpha z_ij) (-inf: no negatives) and the weights constants:
//   G_ij = grad[i] scale exp(alpha z_ij - lw[i]) sigma(z_ij + margin) on J_i,   G_it = -grad[i] scale sigma(-(z_it + margin)),
// 0 at a listed candidate; lists, cursor and the dc sweep's zeroed pairs are the softmax's, the target never a negative.
//
// The pairwise ranking losses by dot product (pairwise_dot_sweep.hip; include/ghf_pairwise_dot_sweep.h) are the
// kernel's fourth loss (LOSS = SB_PAIR, HINGE choosing between the two), with three saved per-query values where the others
// have two — z_it (NaN: the query takes no part), w_i and G_it, formed once for both passes by pair_saved_kernel — and an
// argument struct of its own for them and the margin:
//   G_ij = w_i phi'((z_ij - z_it) + margin) on J_i,   G_it = -w_i dsum_i on the target pair, listed or not,
// 0 at a listed candidate; the hinge's phi' is a compare.  Lists, cursor and the dc sweep's zeroed pairs are the softmax's.
//
// A per-candidate bias (BIAS instantiations; include/ghf.h: the _b calls): every logit is fmaf(scale, s(i,j), b_j),
// forward (rank_sweep.h) and backward, where the softmax forms p_ij = exp(fmaf(scale, s, b_j - lse[i])) so that a zero bias keeps
// the bits.  The dq sweep stages the 64 bias values of a step with its streamed rows, the dc sweep loads its owner rows' once;
// db[j] = sum_i G_ij / scale falls out of the dc sweep's second product, whose A operand is G itself (ascending query order).
#include "common.h"
#include "rank_sweep.h"

namespace ghf {

constexpr int SB_ST = 64;                    // backward: streamed rows per step
constexpr int SB_NT = 256;                   // backward: threads
constexpr int SB_HCAP = 1024;                // backward, dc: listed pairs a candidate tile keeps in LDS
constexpr int SB_MIN_SLAB_TILES = 64;        // backward, dq: a slab is at least 4,096 candidates, so that the partials stay
                                             // below 1/32 of a score matrix at d = 128
static inline int sb_otile(int d) { return d <= 128 ? 128 : 64; }

// dq: two workgroups per CU over the call where the slabs' minimum length allows
static inline bool softmax_bwd_geom(int64_t B, int64_t N, int d, RankGeom* g) {
    if (B <= 0 || N <= 0 || N >= (int64_t)1 << 31 || B >= (int64_t)1 << 31) return false;
    g->qtiles = cdiv(B, sb_otile(d));
    g->ctiles = cdiv(N, SB_ST);
    int64_t slabs = cdiv(2 * RK_CUS, g->qtiles);
    if (slabs > g->ctiles / SB_MIN_SLAB_TILES) slabs = g->ctiles / SB_MIN_SLAB_TILES;
    if (slabs < 1) slabs = 1;
    g->slab_tiles = cdiv(g->ctiles, slabs);
    g->slabs = cdiv(g->ctiles, g->slab_tiles);
    return g->qtiles * g->slabs < (int64_t)1 << 31;
}

size_t score_softmax_workspace_bytes(int64_t B, int64_t N, int d) {
    RankGeom g;
    if (d <= 0 || d > RK_MAX_D || !softmax_geom(B, N, d, &g)) return 0;
    // t [B] float, valid [B] int32, (max, sum) [B, slabs]
    return 2 * rk_align((size_t)B * 4) + rk_align((size_t)B * (size_t)g.slabs * 8);
}

size_t score_softmax_bwd_workspace_bytes(int64_t B, int64_t N, int d) {
    RankGeom g;
    if (d <= 0 || d > RK_MAX_D || !softmax_bwd_geom(B, N, d, &g)) return 0;
    return rk_align((size_t)g.slabs * (size_t)B * (size_t)d * 4);      // dq partials [slabs, B, d]
}

// a candidate subset (candidates.hip): the all-node workspace for N := C, then the id map's
size_t score_softmax_sub_workspace_bytes(int64_t B, int64_t C, int d, int64_t nnz) {
    const size_t base = score_softmax_workspace_bytes(B, C, d), map = cand_workspace_bytes(B, nnz);
    return base && map ? base + map : 0;
}

size_t score_softmax_bwd_sub_workspace_bytes(int64_t B, int64_t C, int d, int64_t nnz) {
    const size_t base = score_softmax_bwd_workspace_bytes(B, C, d), map = cand_workspace_bytes(B, nnz);
    return base && map ? base + map : 0;
}

// with a per-candidate bias: C = 0 is the all-node call (no id map), C > 0 adds the subset's gathered bias [C]
size_t score_softmax_b_workspace_bytes(int64_t B, int64_t N, int64_t C, int d, int64_t nnz) {
    if (C <= 0) return score_softmax_workspace_bytes(B, N, d);
    const size_t base = score_softmax_sub_workspace_bytes(B, C, d, nnz);
    return base ? base + rk_align((size_t)C * 4) : 0;
}

size_t score_softmax_bwd_b_workspace_bytes(int64_t B, int64_t N, int64_t C, int d, int64_t nnz) {
    if (C <= 0) return score_softmax_bwd_workspace_bytes(B, N, d);
    const size_t base = score_softmax_bwd_sub_workspace_bytes(B, C, d, nnz);
    return base ? base + rk_align((size_t)C * 4) : 0;
}

// ---- forward: the sweep between score_prep_kernel / list_range_kernel (rank_sweep.h) and the merge over the slabs ---------
__global__ __launch_bounds__(256) void softmax_finish_kernel(const f32x2* __restrict__ ms, const float* __restrict__ t,
                                                             const int* __restrict__ valid, int64_t B, int64_t slabs, float scale,
                                                             float* __restrict__ loss, float* __restrict__ lse) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= B) return;
    f32x2 m = ms[(size_t)i * slabs];
    for (int64_t s = 1; s < slabs; ++s) m = lse_merge(m, ms[(size_t)i * slabs + s]);
    const float l = valid[i] ? m[0] + logf(m[1]) : __int_as_float(0x7FC00000);
    lse[i] = l;
    loss[i] = l - scale * t[i];
}

// with a bias: the target's logit is fmaf(scale, t, bias[target]), as the sweep forms it (target and bias in node ids; a query
// that is not valid may hold any target)
__global__ __launch_bounds__(256) void softmax_finish_bias_kernel(const f32x2* __restrict__ ms, const float* __restrict__ t,
                                                                  const int* __restrict__ valid, int64_t B, int64_t slabs,
                                                                  float scale, const int64_t* __restrict__ target,
                                                                  const float* __restrict__ bias, float* __restrict__ loss,
                                                                  float* __restrict__ lse) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= B) return;
    f32x2 m = ms[(size_t)i * slabs];
    for (int64_t s = 1; s < slabs; ++s) m = lse_merge(m, ms[(size_t)i * slabs + s]);
    const bool ok = valid[i] != 0;
    const float l = ok ? m[0] + logf(m[1]) : __int_as_float(0x7FC00000);
    lse[i] = l;
    loss[i] = ok ? l - fmaf(scale, t[i], bias[target[i]]) : l;
}

int launch_score_softmax_fwd(const float* q, const float* c, const int64_t* iq, const int64_t* target, const int64_t* filt_ptr,
                             const int64_t* filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d, float scale,
                             void* ws, size_t ws_bytes, float* loss, float* lse, hipStream_t stream, const int64_t* ic,
                             int64_t C, const float* bias) {
    RankArgs a;
    const int64_t M = ic ? C : N;                    // the candidates the sweep runs over
    GHF_REQUIRE(!ic || (C > 0 && C <= N), "score_softmax_fwd: need 1 <= C <= N candidates");
    const size_t base = score_softmax_workspace_bytes(B, M, d);
    const size_t need = ic ? score_softmax_sub_workspace_bytes(B, C, d, nnz) : base;      // with a bias over a subset: + its [C] floats
    const size_t need_b = bias && ic && need ? need + rk_align((size_t)C * 4) : need;
    int rc = score_open("score_softmax_fwd", softmax_geom, need_b, q, c, iq, filt_ptr, filt_idx, nnz, rows_q, M, B, d, ws_bytes, &a);
    if (rc != GHF_OK) return rc;
    const float* bias_c = bias;                      // the bias in the sweep's candidate space
    if (bias && ic) {
        GHF_REQUIRE(need > 0, "candidates: B or nnz out of range");
        bias_c = (float*)((char*)ws + need);
        rc = launch_cand_bias(bias, ic, C, N, (float*)((char*)ws + need), stream);
        if (rc != GHF_OK) return rc;
    }
    const int64_t* target_nodes = target;
    float* t = (float*)ws;
    int* valid = (int*)((char*)ws + rk_align((size_t)B * 4));
    const unsigned qb = (unsigned)cdiv(B, 256);
    if (ic) {                                        // a target that is no candidate: the query is not valid
        CandMap m;
        rc = launch_cand_map(q, c, iq, target, true, filt_ptr, filt_idx, nnz, ic, C, rows_q, N, B, d, nullptr, t, valid, nullptr,
                             nullptr, (char*)ws + base, need > base ? need - base : 0, &m, stream);
        if (rc != GHF_OK) return rc;
        a.filt_ptr = m.ptr; a.filt_idx = m.idx;
        target = m.tpos;
    } else {
        score_prep_kernel<<<qb, 256, 0, stream>>>(q, c, iq, target, rows_q, N, B, d, t, valid, nullptr, nullptr);
        GHF_LAUNCH_CHECK();
        if (nnz > 0) {
            list_range_kernel<<<(unsigned)cdiv(nnz, 256), 256, 0, stream>>>(filt_ptr, filt_idx, nnz, N, B, valid);
            GHF_LAUNCH_CHECK();
        }
    }
    a.target = target; a.scale = scale; a.ws_ms = (f32x2*)((char*)ws + 2 * rk_align((size_t)B * 4));
    rc = launch_rank_tiles<RK_SOFTMAX>(a, stream, ic, N, bias_c);
    if (rc != GHF_OK) return rc;
    if (bias) softmax_finish_bias_kernel<<<qb, 256, 0, stream>>>(a.ws_ms, t, valid, B, a.slabs, scale, target_nodes, bias, loss, lse);
    else softmax_finish_kernel<<<qb, 256, 0, stream>>>(a.ws_ms, t, valid, B, a.slabs, scale, loss, lse);
    GHF_LAUNCH_CHECK();
    return GHF_OK;
}

// ---- backward -------------------------------------------------------------------------------------------------------------
struct SmBwdArgs {
    const float* q; const float* c; const int64_t* iq; const int64_t* target;
    const int64_t* filt_ptr; const int64_t* filt_idx; int64_t nnz;
    int64_t rows_q, N, B;
    int d;
    float scale;
    const float* lse; const float* grad;     // bce: lse is the forward's loss (only its NaNs are read), target is NULL
    int64_t qtiles, slab_tiles, slabs;       // dq
    float* dq_part;                          // dq: [slabs, B, d]
    float* dc;                               // dc: [N, d]
    float pos_w, neg_w;                      // bce: 1 - smoothing, smoothing / N; negsamp: the margin, the adversarial temperature
};
// SUB: candidate j is row ic[j] of c, which has Nn rows (rank_sweep.h: sub_row, RankSubArgs)
struct SmBwdSubArgs : SmBwdArgs { const int64_t* ic; int64_t Nn; };
template <bool SUB, bool BIAS = false, bool PAIR = false> struct SmBwdKernelArgs { typedef SmBwdArgs type; };
template <> struct SmBwdKernelArgs<true, false> { typedef SmBwdSubArgs type; };
// BIAS: bias[j] is the term of the sweeps' candidate j (rank_sweep.h: RankBiasArgs),
// the logit fmaf(scale, s, bias[j]); db [N] (may be NULL) gets sum_i G_ij / scale from the dc pass
struct SmBwdBiasArgs : SmBwdSubArgs { const float* bias; float* db; };
template <bool SUB> struct SmBwdKernelArgs<SUB, true, false> { typedef SmBwdBiasArgs type; };
// SB_PAIR: `lse` holds z_it (NaN: the query takes no part); w and gt are the query's w_i and G_it.  One type
// for its (SUB, BIAS, HINGE) variants, and a type of its own: every other instantiation keeps its argument block.
struct SmBwdPairArgs : SmBwdBiasArgs { const float* w; const float* gt; float margin; };
template <bool SUB, bool BIAS> struct SmBwdKernelArgs<SUB, BIAS, true> { typedef SmBwdPairArgs type; };

constexpr int SB_BIAS = 128;                 // backward: bias values in LDS (the owner tile's, or the streamed tile's)
static inline size_t sb_lds_bytes(int d, int OT, bool bias = false) {
    const int dpad = (d + 31) & ~31;
    return ((size_t)(OT + SB_ST) * (dpad + 4) + (size_t)SB_ST * (OT + 1)) * 4 + (size_t)SB_HCAP * 8 + 16 + (bias ? SB_BIAS * 4 : 0);
}

// what a lane knows of the query in its accumulator column
struct SmQuery {
    float lse, gs;                           // lse NaN: the query takes no part; gs = grad * scale
    int64_t tgt, f0, f1;                     // target, filter list [f0, f1)
};

// the loss whose G the backward forms
constexpr int SB_SOFTMAX = 0, SB_BCE = 1, SB_NEGSAMP = 2, SB_PAIR = 3;

template <int OT, int DMAX, bool DC, int LOSS, bool SUB = false, bool BIAS = false, bool HINGE = false>
__global__ __launch_bounds__(SB_NT) void softmax_bwd_kernel(const typename SmBwdKernelArgs<SUB, BIAS, LOSS == SB_PAIR>::type a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr bool BCE = LOSS == SB_BCE, NEG = LOSS == SB_NEGSAMP, PAIR = LOSS == SB_PAIR;
    constexpr int ST = SB_ST, NT = SB_NT, LDG = OT + 1;
    constexpr int QR = DC ? ST : OT, CR = DC ? OT : ST;             // query / candidate rows of a step's score tile
    constexpr int QT = QR / 32, NTW = QT * (CR / 32) / 4;           // a wave: one query column tile, NTW candidate row tiles
    constexpr int RT = OT / 32, NC = DMAX * RT / 128;               // second product: one owner row tile, NC column tiles of d
    constexpr int NL = ST * (DMAX / 4) / NT;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 31, lh = lane >> 5;
    const int d = a.d, dpad = (d + 31) & ~31, LDX = dpad + 4, nf4 = dpad >> 2;
    float* Xs = lds;                             // the owner tile, resident
    float* Ys = Xs + OT * LDX;                   // the streamed tile
    float* Gs = Ys + ST * LDX;                   // G of the step: [streamed row][owner row]
    long long* hits = (long long*)(Gs + ST * LDG);
    int* hcnt = (int*)(hits + SB_HCAP);
    // BIAS: the bias of the step's candidates — dc: the owner tile's, loaded once; dq: the streamed tile's, staged with it
    float* Bs = (float*)(hcnt + 4);
    const bool vq = rows_vec(a.q, d), vc = rows_vec(a.c, d);

    int64_t own0, tile0, tile1, slab = 0;
    if (DC) {
        own0 = (int64_t)blockIdx.x * OT;
        tile0 = 0;
        tile1 = (a.B + ST - 1) / ST;
    } else {
        int64_t wg = blockIdx.x;                 // as rank_tile_kernel: an XCD's workgroups are the query tiles of one slab
        const int64_t per_xcd = gridDim.x / 8;
        if (wg < per_xcd * 8) wg = (wg % 8) * per_xcd + wg / 8;
        const int64_t qt = wg % a.qtiles, ctiles = (a.N + ST - 1) / ST;
        slab = wg / a.qtiles;
        own0 = qt * OT;
        tile0 = slab * a.slab_tiles;
        tile1 = tile0 + a.slab_tiles < ctiles ? tile0 + a.slab_tiles : ctiles;
    }

    auto qrow = [&](int64_t qi) -> const float* {
        if (qi >= a.B) return nullptr;
        const int64_t r = a.iq ? a.iq[qi] : qi;
        return r >= 0 && r < a.rows_q ? a.q + (size_t)r * d : nullptr;
    };
    auto crow = [&](int64_t j) -> const float* {
        if constexpr (SUB) return sub_row(a.c, a.ic, j, a.N, a.Nn, d);
        else return j < a.N ? a.c + (size_t)j * d : nullptr;
    };
    auto query = [&](int64_t qi) {
        SmQuery m = {__int_as_float(0x7FC00000), 0.f, -1, 0, 0};
        if (qi < a.B) {
            const int64_t r = a.iq ? a.iq[qi] : qi;
            const float l = a.lse[qi];
            if (!BCE) m.tgt = a.target[qi];
            if (r >= 0 && r < a.rows_q && l == l) {
                m.lse = l;
                if constexpr (PAIR) m.gs = a.w[qi];
                else m.gs = a.grad[qi] * a.scale;
            }
            if (a.filt_ptr) {
                int64_t lo = a.filt_ptr[qi], hi = a.filt_ptr[qi + 1];
                lo = lo < 0 ? 0 : (lo > a.nnz ? a.nnz : lo);
                hi = hi < lo ? lo : (hi > a.nnz ? a.nnz : hi);
                m.f0 = lo;
                m.f1 = hi;
            }
        }
        return m;
    };

    for (int idx = tid; idx < OT * nf4; idx += NT) {
        const int row = idx / nf4, c4 = idx - row * nf4;
        const float* src = DC ? crow(own0 + row) : qrow(own0 + row);
        store_perm(Xs + row * LDX, c4, load_k4(src, c4 * 4, d, DC ? vc : vq));
    }
    if constexpr (BIAS && DC) {
        if (tid < OT) Bs[tid] = own0 + tid < a.N ? a.bias[own0 + tid] : 0.f;
    }

    // dc: the listed (query, candidate) pairs inside this candidate tile, the targets' own left out.  bce: the pairs of the
    // queries that take part, an id that repeats its predecessor in the list left out (a positive counts once)
    if (DC) {
        if (tid == 0) *hcnt = 0;
        __syncthreads();
        if (a.filt_ptr) {
            for (int64_t e = tid; e < a.nnz; e += NT) {
                const int64_t j = a.filt_idx[e];
                if (j < own0 || j >= own0 + OT) continue;
                int64_t lo;
                if (!list_owner(a.filt_ptr, a.B, e, &lo)) continue;
                if (BCE) {
                    if (e > 0 && e > a.filt_ptr[lo] && a.filt_idx[e - 1] == j) continue;
                    const int64_t r = a.iq ? a.iq[lo] : lo;
                    const float l = a.lse[lo];
                    if (r < 0 || r >= a.rows_q || l != l) continue;
                } else {
                    if (a.target[lo] == j) continue;
                }
                const int pos = atomicAdd(hcnt, 1);
                if (pos < SB_HCAP) hits[pos] = (long long)(lo * 256 + (j - own0));
            }
        }
    }

    const int ct = wave % QT, rt0 = (wave / QT) * NTW;          // score tiles of this wave
    const int rt2 = wave % RT, cb = (wave / RT) * NC;           // output tiles of this wave
    const int ql = ct * 32 + lr;                                // the lane's query row inside the step's query rows
    const int pl = (lr & ~7) + 4 * (lr & 1) + ((lr >> 1) & 3);  // where store_perm put column lr of a group of 32

    SmQuery cur = query(DC ? tile0 * ST + ql : own0 + ql), nxtq = cur;
    // pair: the G_it of the lane's query (read only where the query is live, whose gt is then a number)
    float cgt = 0.f, ngt = 0.f;
    auto query_gt = [&](int64_t qi) -> float {
        if constexpr (PAIR) return qi < a.B ? a.gt[qi] : 0.f;
        else return 0.f;
    };
    if constexpr (PAIR) cgt = query_gt(DC ? tile0 * ST + ql : own0 + ql);
    int64_t nxt = INT64_MAX;                                    // dq: the first listed id not yet behind the sweep
    if (!DC) {
        cur.f0 = filter_lower_bound(a.filt_idx, cur.f0, cur.f1, tile0 * ST);
        if (cur.f0 < cur.f1) nxt = a.filt_idx[cur.f0];
    }

    f32x4 pre[NL];
    float bpre = 0.f, dbacc = 0.f;
    auto fetch = [&](int64_t tile) {
#pragma unroll
        for (int i = 0; i < NL; ++i) {
            const int idx = tid + NT * i;
            if (idx < ST * nf4) {
                const int row = idx / nf4, c4 = idx - row * nf4;
                const float* src = DC ? qrow(tile * ST + row) : crow(tile * ST + row);
                pre[i] = load_k4(src, c4 * 4, d, DC ? vq : vc);
            }
        }
        if constexpr (BIAS && !DC) {
            if (tid < ST) bpre = tile * ST + tid < a.N ? a.bias[tile * ST + tid] : 0.f;
        }
    };
    auto stash = [&]() {
#pragma unroll
        for (int i = 0; i < NL; ++i) {
            const int idx = tid + NT * i;
            if (idx < ST * nf4) {
                const int row = idx / nf4, c4 = idx - row * nf4;
                store_perm(Ys + row * LDX, c4, pre[i]);
            }
        }
        if constexpr (BIAS && !DC) {
            if (tid < ST) Bs[tid] = bpre;
        }
    };

    f32x16 out[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int r = 0; r < 16; ++r) out[c][r] = 0.f;

    fetch(tile0);
    stash();
    __syncthreads();
    const bool over = DC && *hcnt > SB_HCAP;
    // (bce subtracts at the kept pairs: a tile that looks every id up must not apply them as well)
    const int nh = DC && !(BCE && over) ? (*hcnt < SB_HCAP ? *hcnt : SB_HCAP) : 0;

    for (int64_t tile = tile0; tile < tile1; ++tile) {
        const bool more = tile + 1 < tile1;
        if (more) {
            fetch(tile + 1);
            if (DC) nxtq = query((tile + 1) * ST + ql);
            if constexpr (PAIR && DC) ngt = query_gt((tile + 1) * ST + ql);
        }

        // scores of the step: candidates x queries, the chain of the forward
        f32x16 s[NTW];
#pragma unroll
        for (int t = 0; t < NTW; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) s[t][r] = 0.f;
        const float* cA = (DC ? Xs : Ys) + (rt0 * 32 + lr) * LDX + 4 * lh;
        const float* qB = (DC ? Ys : Xs) + ql * LDX + 4 * lh;
        for (int g = 0; g < (dpad >> 3); ++g) {
            const f32x4 b = *(const f32x4*)(qB + 8 * g);
            f32x4 av[NTW];
#pragma unroll
            for (int t = 0; t < NTW; ++t) av[t] = *(const f32x4*)(cA + t * 32 * LDX + 8 * g);
#pragma unroll
            for (int m = 0; m < 4; ++m)
#pragma unroll
                for (int t = 0; t < NTW; ++t) s[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[t][m], b[m], s[t], 0, 0, 0);
        }

        // G of the step, into LDS
        const int64_t cand0 = DC ? own0 : tile * ST;
        const bool live = cur.lse == cur.lse;
        bool look;                                   // whether one of the query's listed ids can be among the step's candidates
        if (DC) {
            look = false;
            if (over && live) {
                const int64_t lb = filter_lower_bound(a.filt_idx, cur.f0, cur.f1, cand0);
                look = lb < cur.f1 && a.filt_idx[lb] < cand0 + CR;
            }
        } else {
            look = nxt < cand0 + CR;
        }
#pragma unroll
        for (int t = 0; t < NTW; ++t) {
            f32x4 bq[4];                             // BIAS: the bias of the lane's 16 candidates of this tile, bq[r >> 2][r & 3]
            if constexpr (BIAS) {
#pragma unroll
                for (int g = 0; g < 4; ++g) bq[g] = *(const f32x4*)(Bs + (rt0 + t) * 32 + 8 * g + 4 * lh);
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int cl = (rt0 + t) * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                const int64_t cand = cand0 + cl;
                float gv = 0.f;
                if (live && cand < a.N) {
                    if constexpr (PAIR) {
#pragma clang fp contract(off)                           // z and u by the forward's expressions: u has the forward's bits
                        float z;
                        if constexpr (BIAS) z = fmaf(a.scale, s[t][r], bq[r >> 2][r & 3]);
                        else z = a.scale * s[t][r];
                        const float u = (z - cur.lse) + a.margin;
                        float g;
                        if constexpr (HINGE) g = u > 0.f ? cur.gs : 0.f;
                        else g = cur.gs * pair_sigmoid(u);
                        if (cand == cur.tgt) {
                            gv = cgt;
                        } else {
                            const bool masked = look && in_filter(a.filt_idx, cur.f0, cur.f1, cand);
                            gv = masked ? 0.f : g;
                        }
                    } else if constexpr (NEG) {
#pragma clang fp contract(off)                           // z is rounded before the margin is added, as in the forward
                        // sigma(y), y = z + margin, from e = exp(-|y|) as the BCE's; the target's entry is -gs sigma(-y), a
                        // negative's gs w sigma(y) with w = exp(alpha z - lw), 0 for a query without negatives (lw = -inf)
                        float z;
                        if constexpr (BIAS) z = fmaf(a.scale, s[t][r], bq[r >> 2][r & 3]);
                        else z = a.scale * s[t][r];
                        const float y = z + a.pos_w;
                        const float e = __expf(-fabsf(y)), rcp = __builtin_amdgcn_rcpf(1.f + e);
                        const float hi = rcp, lo = e * rcp;              // sigma(|y|), sigma(-|y|)
                        if (cand == cur.tgt) {
                            gv = -cur.gs * (y >= 0.f ? lo : hi);
                        } else {
                            const bool masked = look && in_filter(a.filt_idx, cur.f0, cur.f1, cand);
                            const float w = cur.lse > -INFINITY ? __expf(fmaf(a.neg_w, z, -cur.lse)) : 0.f;
                            gv = masked ? 0.f : cur.gs * (w * (y >= 0.f ? hi : lo));
                        }
                    } else if (BCE) {
                        // sigma(z) from e = exp(-|z|) in (0, 1]: 1 / (1 + e) for z >= 0, e / (1 + e) below
                        float z;
                        if constexpr (BIAS) z = fmaf(a.scale, s[t][r], bq[r >> 2][r & 3]);
                        else z = a.scale * s[t][r];
                        const float e = __expf(-fabsf(z)), rcp = __builtin_amdgcn_rcpf(1.f + e);
                        const float p = z >= 0.f ? rcp : e * rcp;
                        const bool listed = look && in_filter(a.filt_idx, cur.f0, cur.f1, cand);
                        gv = cur.gs * ((p - a.neg_w) - (listed ? a.pos_w : 0.f));
                    } else {
                        const bool masked = look && cand != cur.tgt && in_filter(a.filt_idx, cur.f0, cur.f1, cand);
                        // BIAS: bias - lse first, so that a zero bias leaves the one rounding of the line below it
                        float p;
                        if constexpr (BIAS) p = masked ? 0.f : __expf(fmaf(a.scale, s[t][r], bq[r >> 2][r & 3] - cur.lse));
                        else p = masked ? 0.f : __expf(fmaf(a.scale, s[t][r], -cur.lse));
                        gv = cur.gs * (p - (cand == cur.tgt ? 1.f : 0.f));
                    }
                }
                Gs[DC ? ql * LDG + cl : cl * LDG + ql] = gv;
            }
        }
        if (!DC) {
            while (nxt < cand0 + CR) {
                ++cur.f0;
                nxt = cur.f0 < cur.f1 ? a.filt_idx[cur.f0] : INT64_MAX;
            }
        }
        __syncthreads();
        if (DC && nh > 0) {                          // the listed pairs of this candidate tile whose query is in the step
            for (int h = tid; h < nh; h += NT) {
                const int64_t qi = hits[h] >> 8;
                if (BCE) {                           // one pair, one entry: no two threads meet
                    if (qi >= tile * ST && qi < tile * ST + ST)
                        Gs[(int)(qi - tile * ST) * LDG + (int)(hits[h] & 255)] -= a.grad[qi] * a.scale * a.pos_w;
                } else {
                    if (qi >= tile * ST && qi < tile * ST + ST) Gs[(int)(qi - tile * ST) * LDG + (int)(hits[h] & 255)] = 0.f;
                }
            }
            __syncthreads();
        }

        // out[owner rows, d] += G . (streamed rows): k = the streamed row, ascending
        const float* gA = Gs + lh * LDG + rt2 * 32 + lr;
        const float* yB = Ys + lh * LDX + pl;
#pragma unroll 4
        for (int k = 0; k < ST; k += 2) {
            const float av = gA[k * LDG];
            if constexpr (BIAS && DC) {
                // db falls out of the operand this loop loads anyway: av is G[query k + lh][owner row rt2 * 32 + lr], so the
                // lower half-wave adds its own entry (query k), then the upper one's (query k + 1, fetched by one 32-lane
                // swap): every owner column sums its G over the queries in ascending order, in the shadow of the MFMAs
                const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(av), __float_as_uint(av), false, false);
                dbacc = (dbacc + av) + __uint_as_float(sw[1]);
            }
#pragma unroll
            for (int c = 0; c < NC; ++c)
                if ((cb + c) * 32 < d) out[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, yB[k * LDX + (cb + c) * 32], out[c], 0, 0, 0);
        }
        __syncthreads();
        if (more) {
            stash();
            if (DC) cur = nxtq;
            if constexpr (PAIR && DC) cgt = ngt;
        }
        __syncthreads();
    }

#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const int col = (cb + c) * 32 + lr;
        if (col < d) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int64_t row = own0 + rt2 * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                if (DC) {
                    if (row < a.N) a.dc[(size_t)row * d + col] = out[c][r];
                } else {
                    if (row < a.B) a.dq_part[((size_t)slab * a.B + row) * d + col] = out[c][r];
                }
            }
        }
    }
    if constexpr (BIAS && DC) {
        // the lower half-waves of the waves with the first column block hold one owner row each; G carries grad * scale and
        // the bias enters the logit unscaled
        const int64_t row = own0 + rt2 * 32 + lr;
        if (a.db && cb == 0 && lh == 0 && row < a.N) a.db[row] = dbacc / a.scale;
    }
}

template <int OT, int DMAX, int LOSS, bool SUB = false>
static int launch_bwd_tiles(const typename SmBwdKernelArgs<SUB>::type& a, hipStream_t stream) {
    const size_t lds = sb_lds_bytes(a.d, OT);
    GHF_SET_MAX_LDS((softmax_bwd_kernel<OT, DMAX, false, LOSS, SUB>), lds);
    GHF_SET_MAX_LDS((softmax_bwd_kernel<OT, DMAX, true, LOSS, SUB>), lds);
    softmax_bwd_kernel<OT, DMAX, false, LOSS, SUB><<<(unsigned)(a.qtiles * a.slabs), SB_NT, lds, stream>>>(a);
    GHF_LAUNCH_CHECK();
    softmax_bwd_kernel<OT, DMAX, true, LOSS, SUB><<<(unsigned)cdiv(a.N, OT), SB_NT, lds, stream>>>(a);
    GHF_LAUNCH_CHECK();
    return GHF_OK;
}

template <int OT, int DMAX, int LOSS, bool SUB>
static int launch_bwd_bias_tiles(const SmBwdBiasArgs& a, hipStream_t stream) {
    const size_t lds = sb_lds_bytes(a.d, OT, true);
    GHF_SET_MAX_LDS((softmax_bwd_kernel<OT, DMAX, false, LOSS, SUB, true>), lds);
    GHF_SET_MAX_LDS((softmax_bwd_kernel<OT, DMAX, true, LOSS, SUB, true>), lds);
    softmax_bwd_kernel<OT, DMAX, false, LOSS, SUB, true><<<(unsigned)(a.qtiles * a.slabs), SB_NT, lds, stream>>>(a);
    GHF_LAUNCH_CHECK();
    softmax_bwd_kernel<OT, DMAX, true, LOSS, SUB, true><<<(unsigned)cdiv(a.N, OT), SB_NT, lds, stream>>>(a);
    GHF_LAUNCH_CHECK();
    return GHF_OK;
}

// the three losses' backward: the lists are the softmax's / negsamp's filter lists or the BCE's positives, `lse` the forward's
// lse, (negsamp) its lw or (BCE, of which only the NaNs are read) its loss; target, smoothing and (margin, alpha) belong to
// one loss each
template <int LOSS>
static int launch_score_loss_bwd(const float* q, const float* c, const int64_t* iq, const int64_t* target, const int64_t* list_ptr,
                                 const int64_t* list_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d, float scale,
                                 float smoothing, const float* lse, const float* grad_loss, void* ws, size_t ws_bytes, float* dq,
                                 float* dc, hipStream_t stream, const int64_t* ic, int64_t C, const float* bias, float* db,
                                 float margin = 0.f, float alpha = 0.f) {
    RankArgs r;
    const char* op = LOSS == SB_BCE ? "score_bce_bwd" : LOSS == SB_NEGSAMP ? "score_negsamp_bwd" : "score_softmax_bwd";
    const int64_t M = ic ? C : N;                    // the candidates the sweeps run over: dc is [M, d]
    GHF_REQUIRE(!ic || (C > 0 && C <= N), "%s: need 1 <= C <= N candidates", op);
    const size_t base = score_softmax_bwd_workspace_bytes(B, M, d);
    const size_t need = ic ? score_softmax_bwd_sub_workspace_bytes(B, C, d, nnz) : base;      // with a bias over a subset: + [C] floats
    // (ghf_score_negsamp_bwd_workspace_bytes is one size per shape: a subset's workspace holds the gathered bias's room, asked
    // for or not, and the call refuses less)
    const size_t need_b = (bias || LOSS == SB_NEGSAMP) && ic && need ? need + rk_align((size_t)C * 4) : need;
    int rc = score_open(op, softmax_bwd_geom, need_b, q, c, iq, list_ptr, list_idx, nnz, rows_q, M, B, d, ws_bytes, &r);
    if (rc != GHF_OK) return rc;
    SmBwdBiasArgs a = {};
    a.bias = bias; a.db = db;
    if (bias && ic) {
        GHF_REQUIRE(need > 0, "candidates: B or nnz out of range");
        a.bias = (float*)((char*)ws + need);
        rc = launch_cand_bias(bias, ic, C, N, (float*)((char*)ws + need), stream);
        if (rc != GHF_OK) return rc;
    }
    if (ic) {      // targets and lists as positions in ic; a query that a bad ic or a target outside it rules out has lse NaN
        CandMap m;
        rc = launch_cand_map(q, c, iq, target, LOSS != SB_BCE, list_ptr, list_idx, nnz, ic, C, rows_q, N, B, d, lse, nullptr, nullptr,
                             nullptr, nullptr, (char*)ws + base, need > base ? need - base : 0, &m, stream);
        if (rc != GHF_OK) return rc;
        a.ic = ic; a.Nn = N;
        target = LOSS == SB_BCE ? nullptr : m.tpos; lse = m.lse; r.filt_ptr = m.ptr; list_idx = m.idx;
    }
    a.q = q; a.c = c; a.iq = iq; a.target = target;
    a.filt_ptr = r.filt_ptr; a.filt_idx = list_idx; a.nnz = nnz;
    a.rows_q = rows_q; a.N = M; a.B = B; a.d = d; a.scale = scale; a.lse = lse; a.grad = grad_loss;
    if (LOSS == SB_BCE) { a.pos_w = 1.f - smoothing; a.neg_w = smoothing / (float)M; }
    if (LOSS == SB_NEGSAMP) { a.pos_w = margin; a.neg_w = alpha; }
    a.qtiles = r.qtiles; a.slab_tiles = r.slab_tiles; a.slabs = r.slabs;
    a.dq_part = (float*)ws; a.dc = dc;
    if (bias && ic) rc = sb_otile(d) == 128 ? launch_bwd_bias_tiles<128, 128, LOSS, true>(a, stream) : launch_bwd_bias_tiles<64, 256, LOSS, true>(a, stream);
    else if (bias) rc = sb_otile(d) == 128 ? launch_bwd_bias_tiles<128, 128, LOSS, false>(a, stream) : launch_bwd_bias_tiles<64, 256, LOSS, false>(a, stream);
    else if (ic) rc = sb_otile(d) == 128 ? launch_bwd_tiles<128, 128, LOSS, true>(a, stream) : launch_bwd_tiles<64, 256, LOSS, true>(a, stream);
    else rc = sb_otile(d) == 128 ? launch_bwd_tiles<128, 128, LOSS>(a, stream) : launch_bwd_tiles<64, 256, LOSS>(a, stream);
    if (rc != GHF_OK) return rc;
    return launch_ordered_sum(a.dq_part, a.slabs, B * (int64_t)d, dq, stream);
}

int launch_score_softmax_bwd(const float* q, const float* c, const int64_t* iq, const int64_t* target, const int64_t* filt_ptr,
                             const int64_t* filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d, float scale,
                             const float* lse, const float* grad_loss, void* ws, size_t ws_bytes, float* dq, float* dc,
                             hipStream_t stream, const int64_t* ic, int64_t C, const float* bias, float* db) {
    return launch_score_loss_bwd<SB_SOFTMAX>(q, c, iq, target, filt_ptr, filt_idx, nnz, rows_q, N, B, d, scale, 0.f, lse, grad_loss, ws,
                                             ws_bytes, dq, dc, stream, ic, C, bias, db);
}

// the multi-label BCE loss's backward (bce.hip holds its forward): the same two sweeps and workspace, G formed for that loss
size_t score_bce_bwd_workspace_bytes(int64_t B, int64_t N, int d) { return score_softmax_bwd_workspace_bytes(B, N, d); }
size_t score_bce_bwd_sub_workspace_bytes(int64_t B, int64_t C, int d, int64_t nnz) {
    return score_softmax_bwd_sub_workspace_bytes(B, C, d, nnz);
}
size_t score_bce_bwd_b_workspace_bytes(int64_t B, int64_t N, int64_t C, int d, int64_t nnz) {
    return score_softmax_bwd_b_workspace_bytes(B, N, C, d, nnz);
}

int launch_score_bce_bwd(const float* q, const float* c, const int64_t* iq, const int64_t* pos_ptr, const int64_t* pos_idx,
                         int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d, float scale, float smoothing, const float* loss,
                         const float* grad_loss, void* ws, size_t ws_bytes, float* dq, float* dc, hipStream_t stream,
                         const int64_t* ic, int64_t C, const float* bias, float* db) {
    return launch_score_loss_bwd<SB_BCE>(q, c, iq, nullptr, pos_ptr, pos_idx, nnz, rows_q, N, B, d, scale, smoothing, loss, grad_loss,
                                         ws, ws_bytes, dq, dc, stream, ic, C, bias, db);
}

// the negative-sampling loss's backward (negsamp.hip holds its forward): the same two sweeps; the workspace is the softmax's
// general form (a subset's always with room for its gathered bias)
size_t score_negsamp_bwd_workspace_bytes(int64_t B, int64_t N, int64_t C, int d, int64_t nnz) {
    return C > N ? 0 : score_softmax_bwd_b_workspace_bytes(B, N, C, d, nnz);
}

int launch_score_negsamp_bwd(const float* q, const float* c, const int64_t* iq, const int64_t* target, const int64_t* filt_ptr,
                             const int64_t* filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d, float scale,
                             float margin, float alpha, const float* lw, const float* grad_loss, const int64_t* ic, int64_t C,
                             const float* bias, void* ws, size_t ws_bytes, float* dq, float* dc, float* db, hipStream_t stream) {
    return launch_score_loss_bwd<SB_NEGSAMP>(q, c, iq, target, filt_ptr, filt_idx, nnz, rows_q, N, B, d, scale, 0.f, lw, grad_loss, ws,
                                             ws_bytes, dq, dc, stream, ic, C, bias, db, margin, alpha);
}

// ---- the pairwise ranking losses by dot product (pairwise_dot_sweep.hip holds their forward) -----------------
// The same two sweeps, G formed for that loss.  A sibling of launch_score_loss_bwd, not a fourth arm of it: this call forms
// the per-query t and valid itself (the others read the forward's lse, whose NaNs say which queries take part), has three
// saved values and a workspace of its own layout, and its refusals come in its header's order (score_pair_open).
int score_pair_open(const char* op, size_t need, const int64_t* iq, int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d,
                    const int64_t* ic, int64_t C, size_t ws_bytes);
int launch_pair_zt(float* t, const int* valid, int64_t B, float scale, const int64_t* target, const float* bias, hipStream_t stream);

// the softmax's general form (a subset's always with room for its gathered bias), then t -> z_it, valid, w and G_it [B]
size_t score_pair_bwd_workspace_bytes(int64_t B, int64_t N, int64_t C, int d, int64_t nnz) {
    if (C < 0 || C > N || nnz < 0) return 0;
    const size_t base = score_softmax_bwd_b_workspace_bytes(B, N, C, d, nnz);
    return base ? base + 4 * rk_align((size_t)B * 4) : 0;
}

// one thread per query, behind launch_pair_zt: what both passes read of a query — z_it (NaN: the query takes no part: not
// valid, or count <= 0), w_i and G_it
__global__ __launch_bounds__(256) void pair_saved_kernel(const int* __restrict__ valid, const float* __restrict__ dsum,
                                                         const int* __restrict__ count, const float* __restrict__ grad, int64_t B,
                                                         float scale, int normalize, float* __restrict__ zt, float* __restrict__ w,
                                                         float* __restrict__ gt) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= B) return;
    const int n = count[i];
    const bool part = valid[i] != 0 && n > 0;
    const float gs = grad[i] * scale;
    const float wi = normalize ? gs * (n > 0 ? 1.f / (float)n : 0.f) : gs;
    zt[i] = part ? zt[i] : __int_as_float(0x7FC00000);
    w[i] = part ? wi : 0.f;
    gt[i] = part ? -(wi * dsum[i]) : 0.f;
}

template <int OT, int DMAX, bool SUB, bool BIAS, bool HINGE>
static int launch_pair_bwd_tiles(const SmBwdPairArgs& a, hipStream_t stream) {
    const size_t lds = sb_lds_bytes(a.d, OT, BIAS);
    GHF_SET_MAX_LDS((softmax_bwd_kernel<OT, DMAX, false, SB_PAIR, SUB, BIAS, HINGE>), lds);
    GHF_SET_MAX_LDS((softmax_bwd_kernel<OT, DMAX, true, SB_PAIR, SUB, BIAS, HINGE>), lds);
    softmax_bwd_kernel<OT, DMAX, false, SB_PAIR, SUB, BIAS, HINGE><<<(unsigned)(a.qtiles * a.slabs), SB_NT, lds, stream>>>(a);
    GHF_LAUNCH_CHECK();
    softmax_bwd_kernel<OT, DMAX, true, SB_PAIR, SUB, BIAS, HINGE><<<(unsigned)cdiv(a.N, OT), SB_NT, lds, stream>>>(a);
    GHF_LAUNCH_CHECK();
    return GHF_OK;
}

template <bool HINGE>
static int launch_pair_bwd_shape(const SmBwdPairArgs& a, bool sub, bool biased, hipStream_t stream) {
    const bool wide = sb_otile(a.d) == 128;
#define GHF_PAIR_BWD(SUBSET, BIASED) \
    (wide ? launch_pair_bwd_tiles<128, 128, SUBSET, BIASED, HINGE>(a, stream) : launch_pair_bwd_tiles<64, 256, SUBSET, BIASED, HINGE>(a, stream))
    if (sub && biased) return GHF_PAIR_BWD(true, true);
    if (sub) return GHF_PAIR_BWD(true, false);
    if (biased) return GHF_PAIR_BWD(false, true);
    return GHF_PAIR_BWD(false, false);
#undef GHF_PAIR_BWD
}

int launch_score_pair_bwd(bool hinge, const float* q, const float* c, const int64_t* iq, const int64_t* target,
                          const int64_t* filt_ptr, const int64_t* filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d,
                          float scale, float margin, int normalize, const int64_t* ic, int64_t C, const float* bias, const float* dsum,
                          const int* count, const float* grad_loss, void* ws, size_t ws_bytes, float* dq, float* dc, float* db,
                          hipStream_t stream) {
    const int64_t M = ic ? C : N;                    // the candidates the sweeps run over: dc is [M, d]
    const bool sizes = d > 0 && d <= RK_MAX_D && B > 0 && N > 0;
    const size_t need = sizes ? score_pair_bwd_workspace_bytes(B, N, ic ? C : 0, d, nnz) : 0;
    int rc = score_pair_open("score_pair_bwd", need, iq, nnz, rows_q, N, B, d, ic, C, ws_bytes);
    if (rc != GHF_OK) return rc;
    RankArgs r;
    rc = score_open("score_pair_bwd", softmax_bwd_geom, need, q, c, iq, filt_ptr, filt_idx, nnz, rows_q, M, B, d, ws_bytes, &r);
    if (rc != GHF_OK) return rc;
    // dq partials; with ic the id map and the gathered bias [C]; then the four per-query arrays
    const size_t base = score_softmax_bwd_workspace_bytes(B, M, d);
    const size_t sub = ic ? score_softmax_bwd_sub_workspace_bytes(B, C, d, nnz) : base;
    const size_t front = need - 4 * rk_align((size_t)B * 4);
    char* tail = (char*)ws + front;
    float* zt = (float*)tail;
    int* valid = (int*)(tail + rk_align((size_t)B * 4));
    float* w = (float*)(tail + 2 * rk_align((size_t)B * 4));
    float* gt = (float*)(tail + 3 * rk_align((size_t)B * 4));
    SmBwdPairArgs a = {};
    a.bias = bias; a.db = bias ? db : nullptr;
    if (bias && ic) {
        a.bias = (float*)((char*)ws + sub);
        rc = launch_cand_bias(bias, ic, C, N, (float*)((char*)ws + sub), stream);
        if (rc != GHF_OK) return rc;
    }
    const int64_t* tpos = target;
    const int64_t* list_idx = filt_idx;
    const unsigned qb = (unsigned)cdiv(B, 256);
    if (ic) {      // targets and lists as positions in ic; a bad ic or a target outside it rules the query out
        CandMap m;
        rc = launch_cand_map(q, c, iq, target, true, filt_ptr, filt_idx, nnz, ic, C, rows_q, N, B, d, nullptr, zt, valid, nullptr,
                             nullptr, (char*)ws + base, sub - base, &m, stream);
        if (rc != GHF_OK) return rc;
        a.ic = ic; a.Nn = N;
        tpos = m.tpos; r.filt_ptr = m.ptr; list_idx = m.idx;
    } else {
        score_prep_kernel<<<qb, 256, 0, stream>>>(q, c, iq, target, rows_q, N, B, d, zt, valid, nullptr, nullptr);
        GHF_LAUNCH_CHECK();
        if (nnz > 0) {
            list_range_kernel<<<(unsigned)cdiv(nnz, 256), 256, 0, stream>>>(filt_ptr, filt_idx, nnz, N, B, valid);
            GHF_LAUNCH_CHECK();
        }
    }
    rc = launch_pair_zt(zt, valid, B, scale, target, bias, stream);
    if (rc != GHF_OK) return rc;
    pair_saved_kernel<<<qb, 256, 0, stream>>>(valid, dsum, count, grad_loss, B, scale, normalize, zt, w, gt);
    GHF_LAUNCH_CHECK();
    a.q = q; a.c = c; a.iq = iq; a.target = tpos;
    a.filt_ptr = r.filt_ptr; a.filt_idx = list_idx; a.nnz = nnz;
    a.rows_q = rows_q; a.N = M; a.B = B; a.d = d; a.scale = scale; a.lse = zt; a.grad = grad_loss;
    a.w = w; a.gt = gt; a.margin = margin;
    a.qtiles = r.qtiles; a.slab_tiles = r.slab_tiles; a.slabs = r.slabs;
    a.dq_part = (float*)ws; a.dc = dc;
    rc = hinge ? launch_pair_bwd_shape<true>(a, ic != nullptr, bias != nullptr, stream)
               : launch_pair_bwd_shape<false>(a, ic != nullptr, bias != nullptr, stream);
    if (rc != GHF_OK) return rc;
    return launch_ordered_sum(a.dq_part, a.slabs, B * (int64_t)d, dq, stream);
}

}  // namespace ghf
