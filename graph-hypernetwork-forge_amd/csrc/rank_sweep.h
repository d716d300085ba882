// rank_sweep.h — the tiled q . c^T sweep on the exact fp32 matrix instruction that rank.hip (rank counts, top-k),
// softmax.hip (1-vs-all softmax loss) and bce.hip (multi-label 1-vs-all BCE loss) share: geometry, the VALU form of the
// accumulator's chain, the LDS layout and rank_tile_kernel with its six epilogues (the fifth: negsamp.hip's negative-sampling
// loss, with an argument struct of its own for its two extra floats; the sixth: pairwise_dot_sweep.hip's pairwise ranking
// losses, again with a struct of its own), and the host side around it: the two
// kernels that validate ids ahead of a sweep, the checks that open a launch (score_open) and the choice of the instantiation
// (launch_rank_tiles).  rank.hip's header comment describes the sweep.  Two template flags select a variant of it, each with an
// argument struct of its own so that the others keep theirs: SUB (a candidate subset, candidates.hip) and BIAS (a per-candidate
// fp32 term on every score).
#pragma once
#include "common.h"

namespace ghf {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int RK_TILE = 128;                 // queries per workgroup
constexpr int RK_MAX_D = 256;
constexpr int RK_CUS = 256;                  // MI355X: the grid is sized against it, on the host, without asking a device
constexpr int TOPK_MAX_K = 128;
// candidates per step: 256 (eight waves, two per SIMD: one multiplies while the other waits at a barrier or for LDS) where
// the LDS holds it next to the query tile, 128 (four waves) for d > 128
static inline int rank_ctile(int d) { return d <= 128 ? 256 : 128; }
// free slots behind the k kept entries of a top-k list: one step appends at most its candidates, per query
static inline int topk_cap(int d, int k) { return k + rank_ctile(d) + 64; }
constexpr int TOPK_EPL = (TOPK_MAX_K + 256 + 64 + 63) / 64;   // entries per lane when a wave selects in place

static inline size_t rk_align(size_t x) { return align_up(x, 256); }

// ---- geometry shared by the workspace queries and the launches ------------------------------------------------------------
struct RankGeom { int64_t qtiles, ctiles, slab_tiles, slabs; };

static inline bool rank_geom(int64_t B, int64_t N, int d, int blocks_wanted, RankGeom* g) {
    if (B <= 0 || N <= 0 || N >= (int64_t)1 << 31 || B >= (int64_t)1 << 31) return false;
    g->qtiles = cdiv(B, RK_TILE);
    g->ctiles = cdiv(N, rank_ctile(d));
    int64_t slabs = cdiv(blocks_wanted, g->qtiles);
    if (slabs > g->ctiles) slabs = g->ctiles;
    if (slabs < 1) slabs = 1;
    g->slab_tiles = cdiv(g->ctiles, slabs);
    g->slabs = cdiv(g->ctiles, g->slab_tiles);       // every slab holds at least one tile
    return g->qtiles * g->slabs < (int64_t)1 << 31;
}

// the two losses: a fixed number of candidate slabs (fewer when N is small), whatever B is — the slabs depend on N and d
// alone, so a query's partial sums, and with them its loss, have the same bits whatever batch it is in
constexpr int SM_SLABS = 128;
static inline bool softmax_geom(int64_t B, int64_t N, int d, RankGeom* g) {
    if (B <= 0 || N <= 0 || N >= (int64_t)1 << 31 || B >= (int64_t)1 << 31) return false;
    g->qtiles = cdiv(B, RK_TILE);
    g->ctiles = cdiv(N, rank_ctile(d));
    g->slab_tiles = cdiv(g->ctiles, SM_SLABS);
    g->slabs = cdiv(g->ctiles, g->slab_tiles);
    return g->qtiles * g->slabs < (int64_t)1 << 31;
}

// ---- the chain the matrix instruction computes, on the VALU ---------------------------------------------------------------
__device__ __forceinline__ float dot_chain(const float* __restrict__ x, const float* __restrict__ y, int d, bool vec) {
    float s = 0.f;
    if (vec) {
        for (int k = 0; k < d; k += 4) {
            const f32x4 a = *(const f32x4*)(x + k), b = *(const f32x4*)(y + k);
            s = fmaf(a[3], b[3], fmaf(a[2], b[2], fmaf(a[1], b[1], fmaf(a[0], b[0], s))));
        }
    } else {
        for (int k = 0; k < d; ++k) s = fmaf(x[k], y[k], s);
    }
    return s;
}

__device__ __forceinline__ bool rows_vec(const float* p, int d) { return (d & 3) == 0 && ((uintptr_t)p & 15) == 0; }

// four consecutive k of a row (zeros past d, or when the row is absent)
__device__ __forceinline__ f32x4 load_k4(const float* __restrict__ row, int k, int d, bool vec) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (row) {
        if (vec) {
            if (k < d) v = *(const f32x4*)(row + k);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (k + e < d) v[e] = row[k + e];
        }
    }
    return v;
}

// float4 number c4 of an LDS row, k permuted inside its group of 8: k = 8g + 4x + e  ->  position 8g + 4 (e & 1) + 2x + (e >> 1)
__device__ __forceinline__ void store_perm(float* lds_row, int c4, f32x4 v) {
    float* p = lds_row + (c4 >> 1) * 8 + (c4 & 1) * 2;
    *(f32x2*)p = f32x2{v[0], v[2]};
    *(f32x2*)(p + 4) = f32x2{v[1], v[3]};
}

// A top-k entry is ONE 64-bit key whose unsigned order is (score descending, id ascending) read downwards: the score's bits
// made monotone, then 2^31 - 1 - id.  Keys of different candidates differ; 0 is below every key (an empty slot).
__device__ __forceinline__ uint64_t topk_key(float s, int id) {
    const uint32_t b = __float_as_uint(s + 0.f);                      // -0 -> +0: the two compare equal as scores
    const uint32_t ord = b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
    return ((uint64_t)ord << 32) | (uint32_t)(0x7FFFFFFF - id);
}
__device__ __forceinline__ float key_score(uint64_t key) {
    const uint32_t ord = (uint32_t)(key >> 32);
    return __uint_as_float(ord ^ ((ord >> 31) ? 0x80000000u : 0xFFFFFFFFu));
}
__device__ __forceinline__ int key_id(uint64_t key) { return 0x7FFFFFFF - (int)(uint32_t)key; }
__device__ __forceinline__ uint64_t readlane64(uint64_t v, int l) {
    return ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(v >> 32), l) << 32) |
           (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, l);
}

__device__ __forceinline__ bool in_filter(const int64_t* __restrict__ idx, int64_t lo, int64_t hi, int64_t cand) {
    const int64_t end = hi;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (idx[mid] < cand) lo = mid + 1; else hi = mid;
    }
    return lo < end && idx[lo] == cand;
}

// One wave keeps the k best of the m <= TOPK_EPL * 64 keys at `keys`, in place.  Every lane takes its keys into registers
// (all loads are consumed before the first store is issued); the k-th largest key is found bit by bit from the top (64
// rounds of "how many keys are at least this": a compare and a population count per 64 keys); the keys at or above it move
// to the front — in any order while the sweep goes on, sorted (each kept key counts the kept keys above it) at the slab's
// end, where the list is also padded with empty slots up to k.
static __device__ void select_in_place(uint64_t* keys, int m, int k, int lane, float* thr, int* cnt, bool last) {
    uint64_t key[TOPK_EPL];
#pragma unroll
    for (int u = 0; u < TOPK_EPL; ++u) key[u] = lane + 64 * u < m ? keys[lane + 64 * u] : 0;
    uint64_t kth = 1;                                   // m < k: every key stays
    if (m >= k) {
        kth = 0;
        for (int b = 63; b >= 0; --b) {
            const uint64_t cand = kth | (1ull << b);
            int n = 0;
#pragma unroll
            for (int u = 0; u < TOPK_EPL; ++u)
                if (64 * u < m) n += __popcll(__ballot(key[u] >= cand));
            if (n >= k) kth = cand;
        }
    }
    const int kept = m < k ? m : k;
    if (!last) {
        int base = 0;
#pragma unroll
        for (int u = 0; u < TOPK_EPL; ++u) {
            if (64 * u < m) {
                const bool keep = key[u] >= kth;
                const uint64_t mask = __ballot(keep);
                if (keep) keys[base + __popcll(mask & ((1ull << lane) - 1))] = key[u];
                base += __popcll(mask);
            }
        }
    } else {
        int rk[TOPK_EPL];
#pragma unroll
        for (int u = 0; u < TOPK_EPL; ++u) rk[u] = 0;
#pragma unroll
        for (int v = 0; v < TOPK_EPL; ++v) {
            if (64 * v < m) {
                const int n = m - 64 * v < 64 ? m - 64 * v : 64;
                for (int l = 0; l < n; ++l) {
                    const uint64_t kf = readlane64(key[v], l);
                    if (kf >= kth) {
#pragma unroll
                        for (int u = 0; u < TOPK_EPL; ++u) rk[u] += kf > key[u] ? 1 : 0;
                    }
                }
            }
        }
#pragma unroll
        for (int u = 0; u < TOPK_EPL; ++u)
            if (key[u] >= kth) keys[rk[u]] = key[u];
        for (int p = kept + lane; p < k; p += 64) keys[p] = 0;
    }
    if (lane == 0) {
        *cnt = kept;
        *thr = m >= k ? key_score(kth) : -INFINITY;
    }
}

struct RankArgs {
    const float* q; const float* c; const int64_t* iq;
    int64_t rows_q, N, B;
    int d;
    int64_t qtiles, slab_tiles, slabs;
    // rank
    const float* t; unsigned long long* greater; unsigned long long* equal;
    // top-k
    const int64_t* filt_ptr; const int64_t* filt_idx; int64_t nnz;
    int k, cap; uint64_t* ws_key;
    // softmax (lists as for top-k)
    const int64_t* target; float scale; f32x2* ws_ms;
    // bce (the lists name each query's positives; scale as for softmax)
    float* ws_bce;
};

// a candidate subset (the SUB instantiations; candidates.hip): the sweep's candidate j is row ic[j] of c, which has Nn rows;
// N, the lists and the targets are then the count of, and positions in, ic.  A type of its own, so that the all-node
// instantiations keep their argument block, and with it their code, as they are.
struct RankSubArgs : RankArgs { const int64_t* ic; int64_t Nn; };
template <bool SUB, bool BIAS = false, bool NEG = false, bool PAIR = false> struct RankKernelArgs { typedef RankArgs type; };
template <> struct RankKernelArgs<true, false> { typedef RankSubArgs type; };

// a per-candidate bias (the BIAS instantiations): bias[j] is the fp32 term of the
// sweep's candidate j, i.e. of node j in an all-node sweep (ic and Nn are then unused) and of node ic[j] over a subset, where
// candidates.hip has gathered it into position space ahead of the sweep.  Rank and top-k compare s(i, j) + bias[j], the two
// losses use fmaf(scale, s(i, j), bias[j]).  Again a type of its own: every other instantiation keeps its argument block.
struct RankBiasArgs : RankSubArgs { const float* bias; };
template <bool SUB> struct RankKernelArgs<SUB, true, false, false> { typedef RankBiasArgs type; };

// the negative-sampling loss (the RK_NEGSAMP instantiations; negsamp.hip): its margin and adversarial
// temperature.  One type for its four (SUB, BIAS) variants (ic / Nn / bias unused where the flag is off), and a type of its
// own once more: every other instantiation keeps its argument block.
struct RankNegArgs : RankBiasArgs { float margin, alpha; };
template <bool SUB, bool BIAS> struct RankKernelArgs<SUB, BIAS, true, false> { typedef RankNegArgs type; };

// the pairwise ranking losses (the RK_PAIR instantiations; pairwise_dot_sweep.hip): the margin, every query's
// z_it (the target's logit, formed ahead of the sweep from the t[i] of score_prep_kernel / launch_cand_map) and the 16-byte
// partial per (query, slab).  One type for the (SUB, BIAS, HINGE) variants, and once more a type of its own.
struct __attribute__((aligned(16))) PairPart { float f, g; int n, a; };   // sum phi, sum phi', |J_i|, #{u > 0}
struct RankPairArgs : RankBiasArgs { float margin; const float* zt; PairPart* ws_pair; };
template <bool SUB, bool BIAS> struct RankKernelArgs<SUB, BIAS, false, true> { typedef RankPairArgs type; };

// row j of a sweep over the candidate subset ic [C] of a table of `rows` rows: absent past C or when the id is outside the
// table (candidates.hip reports such a list; the sweep only has to read nothing outside c)
__device__ __forceinline__ const float* sub_row(const float* __restrict__ c, const int64_t* __restrict__ ic, int64_t j, int64_t C,
                                                int64_t rows, int d) {
    if (j >= C) return nullptr;
    const int64_t id = ic[j];
    return (uint64_t)id < (uint64_t)rows ? c + (size_t)id * d : nullptr;
}

// the epilogue of rank_tile_kernel
constexpr int RK_RANK = 0, RK_TOPK = 1, RK_SOFTMAX = 2, RK_BCE = 3, RK_NEGSAMP = 4, RK_PAIR = 5;

// first entry of the sorted list [lo, hi) that is not below `first`
__device__ __forceinline__ int64_t filter_lower_bound(const int64_t* __restrict__ idx, int64_t lo, int64_t hi, int64_t first) {
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (idx[mid] < first) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// (max, sum of exp(. - max)) of two disjoint sets of logits; (-inf, 0) is the empty set
__device__ __forceinline__ f32x2 lse_merge(f32x2 x, f32x2 y) {
    const float m = fmaxf(x[0], y[0]);
    if (!(m > -INFINITY)) return m == m ? f32x2{-INFINITY, 0.f} : f32x2{m, m};     // both empty, or a NaN on its way out
    return f32x2{m, x[1] * expf(x[0] - m) + y[1] * expf(y[0] - m)};
}

// (max, S, T) of two disjoint sets of negatives (RK_NEGSAMP): max of a = alpha z, S = sum exp(a - max), T = sum exp(a - max)
// softplus(z + margin); (-inf, 0, 0) is the empty set
struct NegTriple { float m, s, t; };
__device__ __forceinline__ NegTriple neg_merge(NegTriple x, NegTriple y) {
    const float m = fmaxf(x.m, y.m);
    if (!(m > -INFINITY)) return m == m ? NegTriple{-INFINITY, 0.f, 0.f} : NegTriple{m, m, m};
    const float ex = expf(x.m - m), ey = expf(y.m - m);
    return NegTriple{m, x.s * ex + y.s * ey, x.t * ex + y.t * ey};
}

// log(1 + t) for t = exp(-|z|) in (0, 1].  Forming 1 + t rounds t to a multiple of 2^-24: 4e-6 of the result at t = 2^-6,
// 2 % at 6e-6, all of it below 6e-8.  Below 2^-6 the series t - t^2/2 + t^3/3 stands in (its next term is below 1e-6 of it).
__device__ __forceinline__ float log1p_unit(float t) {
    const float series = t * fmaf(t, fmaf(t, 1.f / 3.f, -0.5f), 1.f);
    return t < 0.015625f ? series : __logf(1.f + t);
}
// softplus(z) = log(1 + exp(z)) = max(z, 0) + log(1 + exp(-|z|)): no overflow at either end
__device__ __forceinline__ float softplus(float z) { return fmaxf(z, 0.f) + log1p_unit(__expf(-fabsf(z))); }
// sigmoid(u) from e = exp(-|u|) in (0, 1] and the hardware reciprocal, as ghf_pairwise_sweep.h's phi' of the logistic loss
__device__ __forceinline__ float pair_sigmoid(float u) {
#pragma clang fp contract(off)
    const float e = __expf(-fabsf(u)), rcp = __builtin_amdgcn_rcpf(1.f + e);
    return u >= 0.f ? rcp : e * rcp;
}

// *owner = the query whose list holds entry e, i.e. the last i with filt_ptr[i] <= e; false when e lies inside no list (a
// malformed pointer array).  A flag, not a -1 owner: the caller's test is then a branch on the two comparisons themselves,
// and softmax_bwd_kernel's dc pass keeps the instruction stream it had with the search written out.
__device__ __forceinline__ bool list_owner(const int64_t* __restrict__ filt_ptr, int64_t B, int64_t e, int64_t* owner) {
    int64_t lo = 0, hi = B;
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (filt_ptr[mid] <= e) lo = mid; else hi = mid;
    }
    *owner = lo;
    return filt_ptr[lo] <= e && filt_ptr[lo + 1] > e;
}

// one thread per list entry: an id out of range marks the query whose list holds it
static __global__ __launch_bounds__(256) void list_range_kernel(const int64_t* __restrict__ filt_ptr, const int64_t* __restrict__ filt_idx,
                                                                int64_t nnz, int64_t N, int64_t B, int* valid) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= nnz) return;
    const int64_t j = filt_idx[e];
    if (j >= 0 && j < N) return;
    int64_t i;
    if (list_owner(filt_ptr, B, e, &i)) valid[i] = 0;
}

// one thread per query, ahead of every sweep: valid[i] says whether the query's row id, and its target where the call has
// one, are in range.  With `t` (which needs `target`): the target's score by the sweep's chain, NaN for a query that is not
// valid (it compares false with every score, so a bad query counts nothing).  With the rank counters: their reset.
static __global__ __launch_bounds__(256) void score_prep_kernel(const float* __restrict__ q, const float* __restrict__ c,
                                                                const int64_t* __restrict__ iq, const int64_t* __restrict__ target,
                                                                int64_t rows_q, int64_t N, int64_t B, int d, float* __restrict__ t,
                                                                int* __restrict__ valid, long long* __restrict__ greater,
                                                                long long* __restrict__ equal) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= B) return;
    const int64_t r = iq ? iq[i] : i;
    bool ok = r >= 0 && r < rows_q;
    if (target) {
        const int64_t tg = target[i];
        ok = ok && tg >= 0 && tg < N;
        if (t) t[i] = ok ? dot_chain(q + (size_t)r * d, c + (size_t)tg * d, d, rows_vec(q, d) && rows_vec(c, d)) : __int_as_float(0x7FC00000);
    }
    if (greater) {
        greater[i] = 0;
        equal[i] = 0;
    }
    valid[i] = ok ? 1 : 0;
}

// `bias`: the two buffers of CT bias values behind the counters (the BIAS instantiations)
static inline size_t rank_lds_bytes(int d, int BK, int CT, bool bias = false) {
    const int dpad = (d + 7) & ~7;
    return ((size_t)RK_TILE * (dpad + 4) + 2 * (size_t)CT * (BK + 4) + 2 * RK_TILE + (bias ? 2 * CT : 0)) * 4;
}

// HINGE: which of the two pairwise losses the RK_PAIR epilogue forms (set once, in the entry point, from the public kind)
template <int BK, int CT, int MODE, bool SUB = false, bool BIAS = false, bool HINGE = false>
__global__ __launch_bounds__(CT * 2) void rank_tile_kernel(const typename RankKernelArgs<SUB, BIAS, MODE == RK_NEGSAMP, MODE == RK_PAIR>::type a) {
    constexpr bool TOPK = MODE == RK_TOPK, RANK = MODE == RK_RANK, SOFTMAX = MODE == RK_SOFTMAX, BCE = MODE == RK_BCE;
    constexpr bool NEGSAMP = MODE == RK_NEGSAMP, PAIR = MODE == RK_PAIR;
    constexpr bool CURSOR = SOFTMAX || BCE || NEGSAMP || PAIR;  // the lists are walked by a cursor, in step with the sweep
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int NT = CT * 2, NW = NT / 64;            // a wave per 64 candidates x 64 queries
    constexpr int LDC = BK + 4, F4 = BK / 4, NL = CT * F4 / NT;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
    const int lr = lane & 31, lh = lane >> 5;
    const int d = a.d, dpad = (d + 7) & ~7, LDQ = dpad + 4;
    float* Qs = lds;
    float* Cs = Qs + RK_TILE * LDQ;
    int* sm0 = (int*)(Cs + 2 * CT * LDC);      // rank: greater counts; top-k: entry counts
    int* sm1 = sm0 + RK_TILE;                       // rank: equal counts;   top-k: thresholds (float bits)
    float* thrS = (float*)sm1;
    // BIAS: the bias of the tile being multiplied and of the next one, CT values each; a tile's values are requested with its
    // first chunk of rows (a register per thread of the first CT) and stored with it, so the epilogue reads them from LDS
    float* Bs = (float*)(sm1 + RK_TILE);

    // Workgroups are dealt to the 8 XCDs round-robin; number them so that the ones an XCD runs at the same time are
    // neighbours, i.e. the query tiles of ONE candidate slab: the slab then comes from that XCD's L2 for all but the first.
    int64_t wg = blockIdx.x;
    const int64_t per_xcd = gridDim.x / 8;
    if (wg < per_xcd * 8) wg = (wg % 8) * per_xcd + wg / 8;
    const int64_t qt = wg % a.qtiles, slab = wg / a.qtiles;
    const int64_t q0 = qt * RK_TILE;
    const int64_t ctiles = (a.N + CT - 1) / CT;
    const int64_t tile0 = slab * a.slab_tiles;
    const int64_t tile1 = tile0 + a.slab_tiles < ctiles ? tile0 + a.slab_tiles : ctiles;
    const bool vq = rows_vec(a.q, d), vc = rows_vec(a.c, d);

    // the query tile: resident for the whole slab; a query past B or with an id out of range is a row of zeros
    const int nf4 = dpad >> 2;
    for (int idx = tid; idx < RK_TILE * nf4; idx += NT) {
        const int row = idx / nf4, c4 = idx - row * nf4;
        const int64_t qi = q0 + row;
        const float* src = nullptr;
        if (qi < a.B) {
            const int64_t r = a.iq ? a.iq[qi] : qi;
            if (r >= 0 && r < a.rows_q) src = a.q + (size_t)r * d;
        }
        store_perm(Qs + row * LDQ, c4, load_k4(src, c4 * 4, d, vq));
    }
    if (tid < RK_TILE) {
        sm0[tid] = 0;
        if (TOPK) thrS[tid] = q0 + tid < a.B ? -INFINITY : INFINITY;
        else sm1[tid] = 0;
    }

    // per-lane state of its two query columns
    float tq[2];
    int gt[2] = {0, 0}, eq[2] = {0, 0};
    int64_t f0[2] = {0, 0}, f1[2] = {0, 0};
    // softmax: running (max, sum) of the column's logits, its target, and the first listed id not yet behind the sweep
    float rm[2] = {-INFINITY, -INFINITY}, rs[2] = {0.f, 0.f};
    int64_t tgt[2] = {-1, -1}, nxt[2] = {INT64_MAX, INT64_MAX};
    // bce: running sums of softplus(z), of z, and of z over the column's listed candidates (its positives)
    float bsp[2] = {0.f, 0.f}, bsz[2] = {0.f, 0.f}, bpos[2] = {0.f, 0.f};
    // negsamp: rm / rs are the running max of alpha z and the sum S of exp(alpha z - max) over the column's negatives, nT the
    // same sum weighted by softplus(z + margin); tgt and the cursor as for the softmax
    float nT[2] = {0.f, 0.f};
    // pair: tq is the column's z_it; bsp / bsz are its running sums of phi and phi', gt / eq its pairs of J_i and those with
    // u > 0; tgt and the cursor as for the softmax
#pragma unroll
    for (int tn = 0; tn < 2; ++tn) {
        const int64_t qi = q0 + wn * 64 + tn * 32 + lr;
        tq[tn] = __int_as_float(0x7FC00000);
        if (qi < a.B) {
            if (RANK) tq[tn] = a.t[qi];
            if constexpr (PAIR) tq[tn] = a.zt[qi];
            if (SOFTMAX || NEGSAMP || PAIR) tgt[tn] = a.target[qi];
            if (!RANK && a.filt_ptr) {
                int64_t lo = a.filt_ptr[qi], hi = a.filt_ptr[qi + 1];
                lo = lo < 0 ? 0 : (lo > a.nnz ? a.nnz : lo);
                hi = hi < lo ? lo : (hi > a.nnz ? a.nnz : hi);
                f0[tn] = lo;
                f1[tn] = hi;
                if (CURSOR) {                        // the cursor starts at the slab's first candidate
                    f0[tn] = filter_lower_bound(a.filt_idx, lo, hi, tile0 * CT);
                    if (f0[tn] < hi) nxt[tn] = a.filt_idx[f0[tn]];
                }
            }
        }
    }

    const int nch = (dpad + BK - 1) / BK;
    const int64_t total = (tile1 - tile0) * nch;

    f32x4 pre[NL];
    // SUB: a row's address needs its id first, two loads in a row where the all-node sweep has one.  The ids of the rows this
    // thread fetches (the same NL rows of a tile for every chunk of it) are therefore loaded a whole tile ahead: cid for the
    // tile being fetched, nid for the one after it; -1 = no row (past C, or an id outside the table).
    int cid[NL], nid[NL];
    auto load_ids = [&](int64_t tile, int* out) {
#pragma unroll
        for (int i = 0; i < NL; ++i) {
            if constexpr (SUB) {
                const int64_t cand = tile * CT + (tid + NT * i) / F4;
                const int64_t id = cand < a.N ? a.ic[cand] : -1;
                out[i] = (uint64_t)id < (uint64_t)a.Nn ? (int)id : -1;
            }
        }
    };
    auto fetch = [&](int64_t tile, int kc) {
#pragma unroll
        for (int i = 0; i < NL; ++i) {
            const int idx = tid + NT * i, row = idx / F4, c4 = idx % F4;
            const int64_t cand = tile * CT + row;
            if constexpr (SUB) pre[i] = load_k4(cid[i] >= 0 ? a.c + (size_t)cid[i] * d : nullptr, kc * BK + c4 * 4, d, vc);
            else pre[i] = load_k4(cand < a.N ? a.c + (size_t)cand * d : nullptr, kc * BK + c4 * 4, d, vc);
        }
    };
    auto stash = [&](int buf) {
#pragma unroll
        for (int i = 0; i < NL; ++i) {
            const int idx = tid + NT * i, row = idx / F4, c4 = idx % F4;
            store_perm(Cs + (buf * CT + row) * LDC, c4, pre[i]);
        }
    };

    float bpre = 0.f;
    int bb = 0;                                         // the bias buffer of the tile being multiplied
    auto fetch_bias = [&](int64_t tile) {               // a candidate past N: 0 (the epilogues leave it out themselves)
        if constexpr (BIAS) {
            const int64_t cand = tile * CT + tid;
            if (tid < CT) bpre = cand < a.N ? a.bias[cand] : 0.f;
        }
    };

    f32x16 acc[2][2];
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[x][y][r] = 0.f;

    if constexpr (SUB) {
        load_ids(tile0, cid);
        load_ids(tile0 + 1, nid);
    }
    if constexpr (BIAS) fetch_bias(tile0);
    fetch(tile0, 0);
    stash(0);
    if constexpr (BIAS) {
        if (tid < CT) Bs[tid] = bpre;
    }
    __syncthreads();

    int64_t tile = tile0;
    int kc = 0, buf = 0;
    for (int64_t step = 0; step < total; ++step) {
        int64_t ntile = tile;
        int nkc = kc + 1;
        if (nkc == nch) { nkc = 0; ++ntile; }
        const bool more = step + 1 < total;
        if constexpr (SUB) {
            if (more && nkc == 0) {                     // the next fetch opens a tile: its ids are here, request the one after
#pragma unroll
                for (int i = 0; i < NL; ++i) cid[i] = nid[i];
                load_ids(ntile + 1, nid);
            }
        }
        if constexpr (BIAS) {
            if (more && nkc == 0) fetch_bias(ntile);
        }
        if (more) fetch(ntile, nkc);

        const int k0 = kc * BK;
        const int ng = (dpad - k0) >> 3;
        const float* cA = Cs + (buf * CT + wm * 64 + lr) * LDC + 4 * lh;
        const float* qB = Qs + (wn * 64 + lr) * LDQ + k0 + 4 * lh;
#pragma unroll
        for (int g = 0; g < BK / 8; ++g) {      // 8 columns: one 16-byte read per operand tile, four MFMAs per accumulator
            if (g < ng) {
                const f32x4 a0 = *(const f32x4*)(cA + 8 * g), a1 = *(const f32x4*)(cA + 32 * LDC + 8 * g);
                const f32x4 b0 = *(const f32x4*)(qB + 8 * g), b1 = *(const f32x4*)(qB + 32 * LDQ + 8 * g);
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[m], b0[m], acc[0][0], 0, 0, 0);
                    acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[m], b1[m], acc[0][1], 0, 0, 0);
                    acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[m], b0[m], acc[1][0], 0, 0, 0);
                    acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[m], b1[m], acc[1][1], 0, 0, 0);
                }
            }
        }

        const bool tile_done = kc == nch - 1;
        if (tile_done) {
            const int64_t base = tile * CT + wm * 64 + 4 * lh;     // + 32 tm + (r & 3) + 8 (r >> 2): the register's candidate
            const bool full = tile * CT + CT <= a.N;
            // BIAS: the bias of the lane's 32 candidates (the same for both query columns), register e = 16 tm + r, read from
            // LDS four at a time where it is used.  Rank and top-k add it to the scores where they stand; the losses fuse it
            // into the multiply by scale.
            auto bias4 = [&](int g) -> f32x4 {          // registers e = 4 g .. 4 g + 3
                return *(const f32x4*)(Bs + bb * CT + wm * 64 + 4 * lh + 32 * (g >> 2) + 8 * (g & 3));
            };
            if constexpr (BIAS && (RANK || TOPK)) {
#pragma unroll
                for (int g = 0; g < 8; ++g) {
                    const f32x4 b4 = bias4(g);
#pragma unroll
                    for (int tn = 0; tn < 2; ++tn)
#pragma unroll
                        for (int i = 0; i < 4; ++i) acc[g >> 2][tn][4 * (g & 3) + i] += b4[i];
                }
            }
            auto logit = [&](int tn, int e) -> float {
                if constexpr (BIAS) return fmaf(a.scale, acc[e >> 4][tn][e & 15], bias4(e >> 2)[e & 3]);
                else return a.scale * acc[e >> 4][tn][e & 15];
            };
            if (SOFTMAX) {
                // online softmax: once per finished tile, a column's 32 registers enter its running (max, sum).  A tile whose
                // id range holds none of the query's listed ids (the cursor says so) takes the plain path; the others look
                // every id up, and a listed candidate other than the target never enters the sum.
                const int64_t tile_end = tile * CT + CT;
#pragma unroll
                for (int tn = 0; tn < 2; ++tn) {
                    float v[32];
                    if (full && nxt[tn] >= tile_end) {
#pragma unroll
                        for (int e = 0; e < 32; ++e) v[e] = logit(tn, e);
                    } else {
#pragma unroll
                        for (int e = 0; e < 32; ++e) {
                            const int64_t cand = base + 32 * (e >> 4) + (e & 3) + 8 * ((e & 15) >> 2);
                            const bool out = cand >= a.N || (cand != tgt[tn] && in_filter(a.filt_idx, f0[tn], f1[tn], cand));
                            v[e] = out ? -INFINITY : logit(tn, e);
                        }
                        while (nxt[tn] < tile_end) {
                            ++f0[tn];
                            nxt[tn] = f0[tn] < f1[tn] ? a.filt_idx[f0[tn]] : INT64_MAX;
                        }
                    }
                    float mx = rm[tn];
#pragma unroll
                    for (int e = 0; e < 32; ++e) mx = fmaxf(mx, v[e]);
                    if (mx > -INFINITY) {
                        float sum = rs[tn] * __expf(rm[tn] - mx);
#pragma unroll
                        for (int e = 0; e < 32; ++e) sum += __expf(v[e] - mx);
                        rs[tn] = sum;
                        rm[tn] = mx;
                    }
                }
            } else if (BCE) {
                // the tile's 32 logits of a column enter its three sums in register order, whichever path the tile takes (a
                // term left out adds +0): a full tile without a listed id touches no memory.  A candidate past N is left out,
                // not scored as a zero row: softplus(0) = ln 2.
                const int64_t tile_end = tile * CT + CT;
#pragma unroll
                for (int tn = 0; tn < 2; ++tn) {
                    float tsp = 0.f, tsz = 0.f, tpos = 0.f;
                    if (full && nxt[tn] >= tile_end) {
#pragma unroll
                        for (int e = 0; e < 32; ++e) {
                            const float z = logit(tn, e);
                            tsp += softplus(z);
                            tsz += z;
                        }
                    } else {
                        const bool look = nxt[tn] < tile_end;
#pragma unroll
                        for (int e = 0; e < 32; ++e) {
                            const int64_t cand = base + 32 * (e >> 4) + (e & 3) + 8 * ((e & 15) >> 2);
                            const float z = logit(tn, e);
                            const bool in = cand < a.N;
                            tsp += in ? softplus(z) : 0.f;
                            tsz += in ? z : 0.f;
                            tpos += (in && look && in_filter(a.filt_idx, f0[tn], f1[tn], cand)) ? z : 0.f;
                        }
                        while (nxt[tn] < tile_end) {
                            ++f0[tn];
                            nxt[tn] = f0[tn] < f1[tn] ? a.filt_idx[f0[tn]] : INT64_MAX;
                        }
                    }
                    bsp[tn] += tsp;
                    bsz[tn] += tsz;
                    bpos[tn] += tpos;
                }
            } else if constexpr (NEGSAMP) {
                // no contraction in this arm: z is rounded once before the margin is added, with a bias (fmaf(scale, s, b)) as
                // without (scale * s), so that a bias of zeros keeps the bits
#pragma clang fp contract(off)
                // The column's negatives of this tile enter (max, S, T) in two passes over its 32 registers: the max of
                // alpha z (and, where the tile's id range holds a listed id, the target or the end of the candidates, a bit
                // per register that is no negative), then the two sums.  A register left out adds +0 to both.
                const int64_t tile_end = tile * CT + CT;
#pragma unroll
                for (int tn = 0; tn < 2; ++tn) {
                    uint32_t outm = 0;
                    float mx = rm[tn];
                    if (full && nxt[tn] >= tile_end && (tgt[tn] < tile * CT || tgt[tn] >= tile_end)) {
#pragma unroll
                        for (int e = 0; e < 32; ++e) mx = fmaxf(mx, a.alpha * logit(tn, e));
                    } else {
                        const bool look = nxt[tn] < tile_end;
#pragma unroll
                        for (int e = 0; e < 32; ++e) {
                            const int64_t cand = base + 32 * (e >> 4) + (e & 3) + 8 * ((e & 15) >> 2);
                            const bool out = cand >= a.N || cand == tgt[tn] || (look && in_filter(a.filt_idx, f0[tn], f1[tn], cand));
                            outm |= out ? 1u << e : 0u;
                            mx = out ? mx : fmaxf(mx, a.alpha * logit(tn, e));
                        }
                        while (nxt[tn] < tile_end) {
                            ++f0[tn];
                            nxt[tn] = f0[tn] < f1[tn] ? a.filt_idx[f0[tn]] : INT64_MAX;
                        }
                    }
                    if (mx > -INFINITY) {
                        const float r = __expf(rm[tn] - mx);
                        float S = rs[tn] * r, T = nT[tn] * r;
#pragma unroll
                        for (int e = 0; e < 32; ++e) {
                            const float z = logit(tn, e);
                            const float w = (outm >> e) & 1 ? 0.f : __expf(fmaf(a.alpha, z, -mx));
                            S += w;
                            T = fmaf(w, softplus(z + a.margin), T);
                        }
                        rs[tn] = S;
                        nT[tn] = T;
                        rm[tn] = mx;
                    }
                }
            } else if constexpr (PAIR) {
                // no contraction in this arm: z is rounded once (scale * s, or the one fmaf with a bias), then u = (z - z_it) +
                // margin in two operations, so that a bias of zeros keeps the bits and the backward can form the same u
#pragma clang fp contract(off)
                // As the negsamp arm: a bit per register that is no pair of J_i where the tile's id range holds a listed id,
                // the target or the end of the candidates, none on the plain path; then the column's 32 registers enter its
                // sums in register order, a register left out adding +0.f and 0 by select (the sums are never -0.f).  The
                // one branch around a column's group skips nothing that counts and keeps the two columns' temporaries from
                // being scheduled side by side.
                const int64_t tile_end = tile * CT + CT;
#pragma unroll
                for (int tn = 0; tn < 2; ++tn) {
                    uint32_t outm = 0;
                    if (!(full && nxt[tn] >= tile_end && (tgt[tn] < tile * CT || tgt[tn] >= tile_end))) {
                        const bool look = nxt[tn] < tile_end;
#pragma unroll
                        for (int e = 0; e < 32; ++e) {
                            const int64_t cand = base + 32 * (e >> 4) + (e & 3) + 8 * ((e & 15) >> 2);
                            const bool out = cand >= a.N || cand == tgt[tn] || (look && in_filter(a.filt_idx, f0[tn], f1[tn], cand));
                            outm |= out ? 1u << e : 0u;
                        }
                        while (nxt[tn] < tile_end) {
                            ++f0[tn];
                            nxt[tn] = f0[tn] < f1[tn] ? a.filt_idx[f0[tn]] : INT64_MAX;
                        }
                    }
                    if (outm != 0xFFFFFFFFu) {
                        float f = bsp[tn], g = bsz[tn];
                        int ac = eq[tn];
#pragma unroll
                        for (int e = 0; e < 32; ++e) {
                            const bool out = (outm >> e) & 1;
                            const float u = (logit(tn, e) - tq[tn]) + a.margin;
                            float phi;
                            if constexpr (HINGE) phi = u <= 0.f ? 0.f : u;      // not fmaxf: a NaN stays a NaN
                            else phi = softplus(u);
                            f += out ? 0.f : phi;
                            if constexpr (!HINGE) g += out ? 0.f : pair_sigmoid(u);
                            ac += !out && u > 0.f ? 1 : 0;
                        }
                        bsp[tn] = f;
                        bsz[tn] = g;
                        eq[tn] = ac;
                        gt[tn] += 32 - __popc(outm);
                    }
                }
            } else if (RANK) {
#pragma unroll
                for (int tm = 0; tm < 2; ++tm)
#pragma unroll
                    for (int tn = 0; tn < 2; ++tn)
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const float s = acc[tm][tn][r];
                            const bool in = full || base + 32 * tm + (r & 3) + 8 * (r >> 2) < a.N;
                            gt[tn] += (in && s > tq[tn]) ? 1 : 0;
                            eq[tn] += (in && s == tq[tn]) ? 1 : 0;
                        }
            } else {
                __syncthreads();        // the selections that followed the previous tile are done: counts and thresholds stand
#pragma unroll
                for (int tn = 0; tn < 2; ++tn) {
                    const int qc = wn * 64 + tn * 32 + lr;
                    const float thr = thrS[qc];
                    bool any = false;
#pragma unroll
                    for (int tm = 0; tm < 2; ++tm)
#pragma unroll
                        for (int r = 0; r < 16; ++r) any |= acc[tm][tn][r] > thr;
                    if (any) {
                        const size_t row = ((size_t)(q0 + qc) * a.slabs + slab) * a.cap;
#pragma unroll
                        for (int tm = 0; tm < 2; ++tm)
#pragma unroll
                            for (int r = 0; r < 16; ++r) {
                                const float s = acc[tm][tn][r];
                                const int64_t cand = base + 32 * tm + (r & 3) + 8 * (r >> 2);
                                if (s > thr && cand < a.N && !in_filter(a.filt_idx, f0[tn], f1[tn], cand)) {
                                    const int pos = atomicAdd(&sm0[qc], 1);
                                    if (pos < a.cap) a.ws_key[row + pos] = topk_key(s, (int)cand);
                                }
                            }
                    }
                }
            }
#pragma unroll
            for (int x = 0; x < 2; ++x)
#pragma unroll
                for (int y = 0; y < 2; ++y)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[x][y][r] = 0.f;
        }

        if (more) stash(buf ^ 1);
        if constexpr (BIAS) {
            if (more && nkc == 0 && tid < CT) Bs[(bb ^ 1) * CT + tid] = bpre;
            if (tile_done) bb ^= 1;
        }
        __syncthreads();
        if (TOPK && tile_done && more) {
            // a query whose buffer could overflow in the next tile keeps its k best now (wave w: queries w, w + 4, ...)
            for (int qc = wave; qc < RK_TILE; qc += NW) {
                const int m = sm0[qc] < a.cap ? sm0[qc] : a.cap;
                if (m > a.cap - CT) {
                    const size_t row = ((size_t)(q0 + qc) * a.slabs + slab) * a.cap;
                    select_in_place(a.ws_key + row, m, a.k, lane, &thrS[qc], &sm0[qc], false);
                }
            }
        }
        tile = ntile;
        kc = nkc;
        buf ^= 1;
    }

    if (SOFTMAX) {
        // a column's partials (two half-waves x the waves along the candidates) merge in that fixed order: one (max, sum)
        // per (query, slab); the loop's last barrier has retired every read of the candidate buffers
        constexpr int NP = NW;                          // NW / 2 waves along the candidates, two half-waves each
        f32x2* part = (f32x2*)Cs;
#pragma unroll
        for (int tn = 0; tn < 2; ++tn) part[(wn * 64 + tn * 32 + lr) * NP + wm * 2 + lh] = f32x2{rm[tn], rs[tn]};
        __syncthreads();
        if (tid < RK_TILE && q0 + tid < a.B) {
            f32x2 m = part[tid * NP];
            for (int p = 1; p < NP; ++p) m = lse_merge(m, part[tid * NP + p]);
            a.ws_ms[(size_t)(q0 + tid) * a.slabs + slab] = m;
        }
    } else if (BCE) {
        // as the softmax's partials: the column's NP triples through LDS, added in that fixed order, one triple per (query,
        // slab) in the workspace
        constexpr int NP = NW;
        float* part = Cs;
#pragma unroll
        for (int tn = 0; tn < 2; ++tn) {
            float* p = part + ((wn * 64 + tn * 32 + lr) * NP + wm * 2 + lh) * 3;
            p[0] = bsp[tn];
            p[1] = bpos[tn];
            p[2] = bsz[tn];
        }
        __syncthreads();
        if (tid < RK_TILE && q0 + tid < a.B) {
            float sp = 0.f, pos = 0.f, sz = 0.f;
            for (int p = 0; p < NP; ++p) {
                sp += part[(tid * NP + p) * 3];
                pos += part[(tid * NP + p) * 3 + 1];
                sz += part[(tid * NP + p) * 3 + 2];
            }
            float* w = a.ws_bce + ((size_t)(q0 + tid) * a.slabs + slab) * 3;
            w[0] = sp;
            w[1] = pos;
            w[2] = sz;
        }
    } else if constexpr (NEGSAMP) {
        // as the BCE's partials: the column's NP triples through LDS, merged in that fixed order, one per (query, slab)
        constexpr int NP = NW;
        float* part = Cs;
#pragma unroll
        for (int tn = 0; tn < 2; ++tn) {
            float* p = part + ((wn * 64 + tn * 32 + lr) * NP + wm * 2 + lh) * 3;
            p[0] = rm[tn];
            p[1] = rs[tn];
            p[2] = nT[tn];
        }
        __syncthreads();
        if (tid < RK_TILE && q0 + tid < a.B) {
            NegTriple m = {part[tid * NP * 3], part[tid * NP * 3 + 1], part[tid * NP * 3 + 2]};
            for (int p = 1; p < NP; ++p)
                m = neg_merge(m, NegTriple{part[(tid * NP + p) * 3], part[(tid * NP + p) * 3 + 1], part[(tid * NP + p) * 3 + 2]});
            float* w = a.ws_bce + ((size_t)(q0 + tid) * a.slabs + slab) * 3;
            w[0] = m.m;
            w[1] = m.s;
            w[2] = m.t;
        }
    } else if constexpr (PAIR) {
        // as the BCE's triples: the column's NP partials of 16 bytes through LDS, added in that fixed order, one per (query, slab)
        constexpr int NP = NW;
        PairPart* part = (PairPart*)Cs;
#pragma unroll
        for (int tn = 0; tn < 2; ++tn) part[(wn * 64 + tn * 32 + lr) * NP + wm * 2 + lh] = PairPart{bsp[tn], bsz[tn], gt[tn], eq[tn]};
        __syncthreads();
        if (tid < RK_TILE && q0 + tid < a.B) {
            PairPart m = part[tid * NP];
            for (int p = 1; p < NP; ++p) {
                const PairPart x = part[tid * NP + p];
                m.f += x.f;
                m.g += x.g;
                m.n += x.n;
                m.a += x.a;
            }
            a.ws_pair[(size_t)(q0 + tid) * a.slabs + slab] = m;
        }
    } else if (RANK) {
#pragma unroll
        for (int tn = 0; tn < 2; ++tn) {
            const int qc = wn * 64 + tn * 32 + lr;
            if (gt[tn]) atomicAdd(&sm0[qc], gt[tn]);
            if (eq[tn]) atomicAdd(&sm1[qc], eq[tn]);
        }
        __syncthreads();
        if (tid < RK_TILE && q0 + tid < a.B) {
            if (sm0[tid]) atomicAdd(&a.greater[q0 + tid], (unsigned long long)sm0[tid]);
            if (sm1[tid]) atomicAdd(&a.equal[q0 + tid], (unsigned long long)sm1[tid]);
        }
    } else {
        // the slab's list of every query: k entries, sorted, padded with (-inf, -1)
        for (int qc = wave; qc < RK_TILE; qc += NW) {
            if (q0 + qc >= a.B) break;
            const int m = sm0[qc] < a.cap ? sm0[qc] : a.cap;
            const size_t row = ((size_t)(q0 + qc) * a.slabs + slab) * a.cap;
            select_in_place(a.ws_key + row, m, a.k, lane, &thrS[qc], &sm0[qc], true);
        }
    }
}

// ---- the host side every operation shares ---------------------------------------------------------------------------------
// the sweep with epilogue MODE over a.qtiles x a.slabs workgroups: the one place that picks the instantiation.  With `ic`
// (node ids of the a.N candidates, rows of a table of Nn rows) the sweep over that subset.
// With `bias` (one value per candidate of the sweep: per node, or gathered through ic) the BIAS instantiations.
// RK_NEGSAMP: the same 2 x 2 x 2 choice among its own instantiations, which all take RankNegArgs (margin, alpha).
// RK_PAIR goes through launch_rank_pair_tiles below.
template <int MODE>
static int launch_rank_tiles(const RankArgs& a, hipStream_t stream, const int64_t* ic = nullptr, int64_t Nn = 0,
                             const float* bias = nullptr, float margin = 0.f, float alpha = 0.f) {
    const unsigned grid = (unsigned)(a.qtiles * a.slabs);
    if constexpr (MODE == RK_NEGSAMP) {
        RankNegArgs s;
        static_cast<RankArgs&>(s) = a;
        s.ic = ic; s.Nn = Nn; s.bias = bias; s.margin = margin; s.alpha = alpha;
        const bool wide = rank_ctile(a.d) == 256;
        const size_t lds = wide ? rank_lds_bytes(a.d, 32, 256, bias != nullptr) : rank_lds_bytes(a.d, 16, 128, bias != nullptr);
#define GHF_RANK_NEG_LAUNCH(BK, CT, SUBSET, BIASED)                                              \
    do {                                                                                          \
        GHF_SET_MAX_LDS((rank_tile_kernel<BK, CT, MODE, SUBSET, BIASED>), lds);                   \
        rank_tile_kernel<BK, CT, MODE, SUBSET, BIASED><<<grid, CT * 2, lds, stream>>>(s);         \
    } while (0)
#define GHF_RANK_NEG_SHAPE(BK, CT)                                                                \
    do {                                                                                          \
        if (ic && bias) GHF_RANK_NEG_LAUNCH(BK, CT, true, true);                                  \
        else if (ic) GHF_RANK_NEG_LAUNCH(BK, CT, true, false);                                    \
        else if (bias) GHF_RANK_NEG_LAUNCH(BK, CT, false, true);                                  \
        else GHF_RANK_NEG_LAUNCH(BK, CT, false, false);                                           \
    } while (0)
        if (wide) GHF_RANK_NEG_SHAPE(32, 256); else GHF_RANK_NEG_SHAPE(16, 128);
#undef GHF_RANK_NEG_SHAPE
#undef GHF_RANK_NEG_LAUNCH
    } else if (bias) {
        RankBiasArgs s;
        static_cast<RankArgs&>(s) = a;
        s.ic = ic; s.Nn = Nn; s.bias = bias;
        const bool wide = rank_ctile(a.d) == 256;
        const size_t lds = wide ? rank_lds_bytes(a.d, 32, 256, true) : rank_lds_bytes(a.d, 16, 128, true);
#define GHF_RANK_BIAS_LAUNCH(BK, CT, SUBSET)                                                  \
    do {                                                                                       \
        GHF_SET_MAX_LDS((rank_tile_kernel<BK, CT, MODE, SUBSET, true>), lds);                  \
        rank_tile_kernel<BK, CT, MODE, SUBSET, true><<<grid, CT * 2, lds, stream>>>(s);        \
    } while (0)
        if (wide) { if (ic) GHF_RANK_BIAS_LAUNCH(32, 256, true); else GHF_RANK_BIAS_LAUNCH(32, 256, false); }
        else { if (ic) GHF_RANK_BIAS_LAUNCH(16, 128, true); else GHF_RANK_BIAS_LAUNCH(16, 128, false); }
#undef GHF_RANK_BIAS_LAUNCH
    } else if (ic) {                                           // the same two shapes, rows through ic
        RankSubArgs s;
        static_cast<RankArgs&>(s) = a;
        s.ic = ic; s.Nn = Nn;
        if (rank_ctile(a.d) == 256) {
            const size_t lds = rank_lds_bytes(a.d, 32, 256);
            GHF_SET_MAX_LDS((rank_tile_kernel<32, 256, MODE, true>), lds);
            rank_tile_kernel<32, 256, MODE, true><<<grid, 512, lds, stream>>>(s);
        } else {
            const size_t lds = rank_lds_bytes(a.d, 16, 128);
            GHF_SET_MAX_LDS((rank_tile_kernel<16, 128, MODE, true>), lds);
            rank_tile_kernel<16, 128, MODE, true><<<grid, 256, lds, stream>>>(s);
        }
    } else if (rank_ctile(a.d) == 256) {
        const size_t lds = rank_lds_bytes(a.d, 32, 256);
        GHF_SET_MAX_LDS((rank_tile_kernel<32, 256, MODE>), lds);
        rank_tile_kernel<32, 256, MODE><<<grid, 512, lds, stream>>>(a);
    } else {
        const size_t lds = rank_lds_bytes(a.d, 16, 128);
        GHF_SET_MAX_LDS((rank_tile_kernel<16, 128, MODE>), lds);
        rank_tile_kernel<16, 128, MODE><<<grid, 256, lds, stream>>>(a);
    }
    GHF_LAUNCH_CHECK();
    return GHF_OK;
}

// RK_PAIR: the 2 x 2 x 2 choice of launch_rank_tiles<RK_NEGSAMP> among the instantiations of one loss (HINGE or not), which
// all take RankPairArgs; `s` comes with every field but ic / Nn / bias
template <bool HINGE>
static int launch_rank_pair_tiles(RankPairArgs s, hipStream_t stream, const int64_t* ic, int64_t Nn, const float* bias) {
    const unsigned grid = (unsigned)(s.qtiles * s.slabs);
    s.ic = ic; s.Nn = Nn; s.bias = bias;
    const bool wide = rank_ctile(s.d) == 256;
    const size_t lds = wide ? rank_lds_bytes(s.d, 32, 256, bias != nullptr) : rank_lds_bytes(s.d, 16, 128, bias != nullptr);
#define GHF_RANK_PAIR_LAUNCH(BK, CT, SUBSET, BIASED)                                                      \
    do {                                                                                                   \
        GHF_SET_MAX_LDS((rank_tile_kernel<BK, CT, RK_PAIR, SUBSET, BIASED, HINGE>), lds);                  \
        rank_tile_kernel<BK, CT, RK_PAIR, SUBSET, BIASED, HINGE><<<grid, CT * 2, lds, stream>>>(s);        \
    } while (0)
#define GHF_RANK_PAIR_SHAPE(BK, CT)                                                                        \
    do {                                                                                                   \
        if (ic && bias) GHF_RANK_PAIR_LAUNCH(BK, CT, true, true);                                          \
        else if (ic) GHF_RANK_PAIR_LAUNCH(BK, CT, true, false);                                            \
        else if (bias) GHF_RANK_PAIR_LAUNCH(BK, CT, false, true);                                          \
        else GHF_RANK_PAIR_LAUNCH(BK, CT, false, false);                                                   \
    } while (0)
    if (wide) GHF_RANK_PAIR_SHAPE(32, 256); else GHF_RANK_PAIR_SHAPE(16, 128);
#undef GHF_RANK_PAIR_SHAPE
#undef GHF_RANK_PAIR_LAUNCH
    GHF_LAUNCH_CHECK();
    return GHF_OK;
}

// What every launch_score_* opens with: the shape checks (`op` names the operation in the messages), the geometry by the
// operation's own function, the workspace against `need` (the operation's *_workspace_bytes).  On success *a holds what
// every sweep reads (rows, sizes, geometry, the lists: absent when they are empty); the caller sets its own fields.
static inline int score_open(const char* op, bool (*geom)(int64_t, int64_t, int, RankGeom*), size_t need, const float* q,
                             const float* c, const int64_t* iq, const int64_t* filt_ptr, const int64_t* filt_idx, int64_t nnz,
                             int64_t rows_q, int64_t N, int64_t B, int d, size_t ws_bytes, RankArgs* a) {
    RankGeom g;
    GHF_REQUIRE(d > 0 && rows_q > 0 && N > 0 && B > 0 && nnz >= 0, "%s: bad shape", op);
    if (d > RK_MAX_D) return set_err(GHF_EUNSUPPORTED, "%s: d = %d exceeds %d", op, d, RK_MAX_D);
    GHF_REQUIRE(geom(B, N, d, &g), "%s: B or N out of range", op);
    GHF_REQUIRE(iq || B <= rows_q, "%s: B exceeds the rows of q", op);
    GHF_REQUIRE(ws_bytes >= need, "%s: workspace of %zu bytes, need %zu", op, ws_bytes, need);
    *a = RankArgs{};
    a->q = q; a->c = c; a->iq = iq; a->rows_q = rows_q; a->N = N; a->B = B; a->d = d;
    a->qtiles = g.qtiles; a->slab_tiles = g.slab_tiles; a->slabs = g.slabs;
    a->filt_ptr = nnz > 0 ? filt_ptr : nullptr; a->filt_idx = filt_idx; a->nnz = nnz;
    return GHF_OK;
}

// ---- candidate subsets (candidates.hip) -----------------------------------------------------------------------------------
// What a sweep over the subset ic [C] reads in place of the caller's node ids: every query's target as a position in ic
// (-1: not a candidate), its list cut down to the candidates and renumbered the same way (a new CSR pair, each list still
// ascending; NULL where the call has no lists), and for a backward the forward's lse with NaN for a query that takes no part.
struct CandMap { const int64_t* tpos; const int64_t* ptr; const int64_t* idx; const float* lse; };

size_t cand_workspace_bytes(int64_t B, int64_t nnz);
// The pass ahead of every sweep over a subset, in place of score_prep_kernel / list_range_kernel: checks ic (strictly
// ascending, inside [0, N)), writes valid [B] (the query's row id in range, its target a node — with `target_in` a
// candidate —, no listed id outside [0, N), ic good), t [B] where given (the target's score from its own row of c, NaN for a
// query that is not valid), resets the rank counters where given, and fills *m from `ws` (ws_bytes = cand_workspace_bytes,
// 0 where the sizes are out of range).
int launch_cand_map(const float* q, const float* c, const int64_t* iq, const int64_t* target, bool target_in,
                    const int64_t* list_ptr, const int64_t* list_idx, int64_t nnz, const int64_t* ic, int64_t C, int64_t rows_q,
                    int64_t N, int64_t B, int d, const float* lse, float* t, int* valid, int64_t* greater, int64_t* equal, void* ws,
                    size_t ws_bytes, CandMap* m, hipStream_t stream);
// out[j] = bias[ic[j]], j < C: a per-node bias in the position space of a sweep over ic (0 where ic[j] is outside [0, N))
int launch_cand_bias(const float* bias, const int64_t* ic, int64_t C, int64_t N, float* out, hipStream_t stream);

}  // namespace ghf
