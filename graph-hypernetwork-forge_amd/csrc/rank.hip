// rank.hip — link prediction against every node: filtered rank counts and top-k partners, the B x N scores never stored.
//
// What a user of the reference does after training (demo.py:79-101 trains on pair scores): score a query node against all
// N nodes, s(i, j) = q_i . c_j, and ask where the true partner ranks or which k partners score highest.  Both are one tiled
// q . c^T on the exact fp32 matrix instruction (v_mfma_f32_32x32x2_f32) whose epilogue consumes the accumulators in registers:
//
//   workgroup = 512 threads = 4 x 2 waves, block tile 256 candidates x 128 queries (d > 128: 256 threads, 128 x 128, so that
//   the LDS still holds the query tile), wave tile 64 x 64 = 2 x 2 MFMA tiles (64 accumulator registers: four independent
//   chains per wave).  Two waves share a SIMD: one multiplies while the other waits at the barrier or for LDS.
//   Candidates are the A operand (rows), queries the B operand (columns): the accumulator map of the 32x32 form puts the
//   COLUMN on the lane (col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)), so a lane compares its 16 registers
//   of one tile against ONE query's threshold and keeps one counter per query column.
//   The query tile (128 x d) is loaded once per workgroup and stays in LDS; candidate rows stream through two LDS buffers
//   of BK columns (BK = 32; 16 when d > 128), fetched into registers one step ahead of the step being multiplied: one
//   barrier per step.
//   LDS rows hold k permuted inside groups of 8 (position 4 (k & 1) + (k >> 1 & 3)) so that a lane's ONE 16-byte read gives
//   it k = h, h+2, h+4, h+6 (h = lane >> 5): the operands of four consecutive MFMAs, k ascending.
//   A workgroup owns (query tile, candidate slab); workgroups are numbered so that the ones an XCD runs together are the
//   query tiles of one slab, which then streams from HBM once and from that XCD's L2 after.
//
// Numerics: an accumulator is bit for bit the chain s = fmaf(q[k], c[k], s), k = 0 .. d-1, from s = 0 (zero padding of k
// adds fma(0, 0, s) = s).  dot_chain() below is that chain on the VALU: the target's score t_i and the filter corrections
// come from it and compare equal to the tile's value of the same pair.
//
// Rank:   greater / equal start at 0 (rank_prep_kernel, which also computes t_i), every (query tile, candidate slab)
//         workgroup adds its integer counts with atomics (order-free, so reproducible), rank_filter_kernel takes the listed
//         known-true candidates out again by recomputing their scores, rank_finish_kernel takes the target out of `equal`
//         and writes -1 for a query with an id out of range.
// Top-k:  a workgroup keeps, per query, an append buffer of cap = k + (candidates per step) + 64 entries in the caller's
//         workspace and a threshold in LDS (the k-th best so far; candidates arrive in ascending id, so a tie with it
//         loses).  An entry is one 64-bit key ordered as (score descending, id ascending).  A candidate above the threshold
//         that is not in the query's (sorted) filter list is appended; when the next step could overflow the buffer a wave
//         selects the k best in place (select_in_place).  topk_merge_kernel merges the slabs' sorted lists: a key's
//         position is the number of keys above it, one binary search per slab.
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

// four workgroups per CU over the call: the tail of the last round stays short; a slab still amortises its query-tile load
static inline bool rank_geom_rank(int64_t B, int64_t N, int d, RankGeom* g) { return rank_geom(B, N, d, 4 * RK_CUS, g); }
// one round: the longer the slab, the rarer an insertion (the threshold only rises) and the smaller the table to merge
static inline bool rank_geom_topk(int64_t B, int64_t N, int d, RankGeom* g) { return rank_geom(B, N, d, RK_CUS, g); }

size_t score_rank_workspace_bytes(int64_t B, int64_t N, int d) {
    RankGeom g;
    if (d <= 0 || d > RK_MAX_D || !rank_geom_rank(B, N, d, &g)) return 0;
    return rk_align((size_t)B * 4) + rk_align((size_t)B * 4);          // t [B] float, valid [B] int32
}

size_t score_topk_workspace_bytes(int64_t B, int64_t N, int d, int k) {
    RankGeom g;
    if (d <= 0 || d > RK_MAX_D || k < 1 || k > TOPK_MAX_K || !rank_geom_topk(B, N, d, &g)) return 0;
    const size_t entries = (size_t)B * (size_t)g.slabs * (size_t)topk_cap(d, k);
    return rk_align((size_t)B * 4) + rk_align(entries * 8);           // valid [B] int32, keys (8 bytes per entry)
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
__device__ void select_in_place(uint64_t* keys, int m, int k, int lane, float* thr, int* cnt, bool last) {
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
};

static inline size_t rank_lds_bytes(int d, int BK, int CT) {
    const int dpad = (d + 7) & ~7;
    return ((size_t)RK_TILE * (dpad + 4) + 2 * (size_t)CT * (BK + 4) + 2 * RK_TILE) * 4;
}

template <int BK, int CT, bool TOPK>
__global__ __launch_bounds__(CT * 2) void rank_tile_kernel(const RankArgs a) {
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
#pragma unroll
    for (int tn = 0; tn < 2; ++tn) {
        const int64_t qi = q0 + wn * 64 + tn * 32 + lr;
        tq[tn] = __int_as_float(0x7FC00000);
        if (qi < a.B) {
            if (!TOPK) tq[tn] = a.t[qi];
            if (TOPK && a.filt_ptr) {
                int64_t lo = a.filt_ptr[qi], hi = a.filt_ptr[qi + 1];
                lo = lo < 0 ? 0 : (lo > a.nnz ? a.nnz : lo);
                hi = hi < lo ? lo : (hi > a.nnz ? a.nnz : hi);
                f0[tn] = lo;
                f1[tn] = hi;
            }
        }
    }

    const int nch = (dpad + BK - 1) / BK;
    const int64_t total = (tile1 - tile0) * nch;

    f32x4 pre[NL];
    auto fetch = [&](int64_t tile, int kc) {
#pragma unroll
        for (int i = 0; i < NL; ++i) {
            const int idx = tid + NT * i, row = idx / F4, c4 = idx % F4;
            const int64_t cand = tile * CT + row;
            pre[i] = load_k4(cand < a.N ? a.c + (size_t)cand * d : nullptr, kc * BK + c4 * 4, d, vc);
        }
    };
    auto stash = [&](int buf) {
#pragma unroll
        for (int i = 0; i < NL; ++i) {
            const int idx = tid + NT * i, row = idx / F4, c4 = idx % F4;
            store_perm(Cs + (buf * CT + row) * LDC, c4, pre[i]);
        }
    };

    f32x16 acc[2][2];
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[x][y][r] = 0.f;

    fetch(tile0, 0);
    stash(0);
    __syncthreads();

    int64_t tile = tile0;
    int kc = 0, buf = 0;
    for (int64_t step = 0; step < total; ++step) {
        int64_t ntile = tile;
        int nkc = kc + 1;
        if (nkc == nch) { nkc = 0; ++ntile; }
        const bool more = step + 1 < total;
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
            if (!TOPK) {
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

    if (!TOPK) {
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

// ---- rank: the small kernels around the sweep -----------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rank_prep_kernel(const float* __restrict__ q, const float* __restrict__ c,
                                                        const int64_t* __restrict__ iq, const int64_t* __restrict__ target,
                                                        int64_t rows_q, int64_t N, int64_t B, int d, float* __restrict__ t,
                                                        int* __restrict__ valid, long long* __restrict__ greater,
                                                        long long* __restrict__ equal) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= B) return;
    const int64_t r = iq ? iq[i] : i;
    bool ok = r >= 0 && r < rows_q;
    float ti = __int_as_float(0x7FC00000);          // NaN: compares false with every score, so a bad query counts nothing
    if (target) {
        const int64_t tg = target[i];
        ok = ok && tg >= 0 && tg < N;
        if (ok) ti = dot_chain(q + (size_t)r * d, c + (size_t)tg * d, d, rows_vec(q, d) && rows_vec(c, d));
        greater[i] = 0;
        equal[i] = 0;
        t[i] = ti;
    }
    valid[i] = ok ? 1 : 0;
}

// one thread per filter entry: an id out of range marks its query; in the rank call the entry's score is recomputed and taken
// out of the count it went into (lists are sorted: a repeat is the entry before; the target is taken out by rank_finish)
__global__ __launch_bounds__(256) void rank_filter_kernel(const float* __restrict__ q, const float* __restrict__ c,
                                                          const int64_t* __restrict__ iq, const int64_t* __restrict__ target,
                                                          const int64_t* __restrict__ filt_ptr, const int64_t* __restrict__ filt_idx,
                                                          int64_t nnz, int64_t N, int64_t B, int d, const float* __restrict__ t,
                                                          int* valid, unsigned long long* __restrict__ greater,
                                                          unsigned long long* __restrict__ equal) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= nnz) return;
    int64_t lo = 0, hi = B;                          // the query whose list holds e: last i with filt_ptr[i] <= e
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (filt_ptr[mid] <= e) lo = mid; else hi = mid;
    }
    const int64_t i = lo;
    if (filt_ptr[i] > e || filt_ptr[i + 1] <= e) return;      // not inside any list (a malformed pointer array)
    const int64_t j = filt_idx[e];
    if (j < 0 || j >= N) {
        valid[i] = 0;
        return;
    }
    if (!target || !valid[i]) return;
    if (j == target[i] || (e > filt_ptr[i] && filt_idx[e - 1] == j)) return;
    const int64_t r = iq ? iq[i] : i;                // in range: rank_prep_kernel said so (valid[i] was 1)
    const float s = dot_chain(q + (size_t)r * d, c + (size_t)j * d, d, rows_vec(q, d) && rows_vec(c, d));
    const float ti = t[i];
    if (s > ti) atomicAdd(&greater[i], ~0ull);
    else if (s == ti) atomicAdd(&equal[i], ~0ull);
}

__global__ __launch_bounds__(256) void rank_finish_kernel(const float* __restrict__ t, const int* __restrict__ valid, int64_t B,
                                                          long long* __restrict__ greater, long long* __restrict__ equal) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= B) return;
    if (!valid[i]) {
        greater[i] = -1;
        equal[i] = -1;
    } else if (t[i] == t[i]) {
        equal[i] -= 1;                               // the target's own score, counted by the tile that holds it
    }
}

// ---- top-k: merge the slabs' sorted lists; one wave per query -------------------------------------------------------------
__global__ __launch_bounds__(256) void topk_merge_kernel(const uint64_t* __restrict__ ws_key, const int* __restrict__ valid,
                                                         int64_t B, int64_t slabs, int cap, int k, float* __restrict__ out_sc,
                                                         long long* __restrict__ out_id) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= B) return;
    float* os = out_sc + (size_t)i * k;
    long long* oi = out_id + (size_t)i * k;
    if (!valid[i]) {                                 // an id out of range: NaN scores (as ghf_score_pairs_fwd), ids -1
        for (int p = lane; p < k; p += 64) {
            os[p] = __int_as_float(0x7FC00000);
            oi[p] = -1;
        }
        return;
    }
    const uint64_t* keys = ws_key + (size_t)i * slabs * cap;
    const int64_t m = slabs * k;
    int mine = 0;
    for (int64_t e = lane; e < m; e += 64) {
        const int64_t se = e / k;
        const uint64_t key = keys[se * cap + (e - se * k)];
        if (key == 0) continue;
        ++mine;
        int64_t rank = 0;
        for (int64_t sl = 0; sl < slabs && rank < k; ++sl) {
            // keys of slab sl above this one: its list is sorted downwards, empty slots last
            int lo = 0, hi = k;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (keys[sl * cap + mid] > key) lo = mid + 1; else hi = mid;
            }
            rank += lo;
        }
        if (rank < k) {
            os[rank] = key_score(key);
            oi[rank] = key_id(key);
        }
    }
    // entries in all: positions from there on hold no candidate
    for (int off = 32; off; off >>= 1) mine += __shfl_xor(mine, off, 64);
    for (int64_t p = mine + lane; p < k; p += 64) {
        os[p] = -INFINITY;
        oi[p] = -1;
    }
}

// ---- launches -------------------------------------------------------------------------------------------------------------
template <bool TOPK>
static int launch_tiles(const RankArgs& a, hipStream_t stream) {
    const unsigned grid = (unsigned)(a.qtiles * a.slabs);
    if (rank_ctile(a.d) == 256) {
        const size_t lds = rank_lds_bytes(a.d, 32, 256);
        GHF_SET_MAX_LDS((rank_tile_kernel<32, 256, TOPK>), lds);
        rank_tile_kernel<32, 256, TOPK><<<grid, 512, lds, stream>>>(a);
    } else {
        const size_t lds = rank_lds_bytes(a.d, 16, 128);
        GHF_SET_MAX_LDS((rank_tile_kernel<16, 128, TOPK>), lds);
        rank_tile_kernel<16, 128, TOPK><<<grid, 256, lds, stream>>>(a);
    }
    GHF_LAUNCH_CHECK();
    return GHF_OK;
}

int launch_score_rank(const float* q, const float* c, const int64_t* iq, const int64_t* target, const int64_t* filt_ptr,
                      const int64_t* filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d, void* ws,
                      size_t ws_bytes, int64_t* greater, int64_t* equal, hipStream_t stream) {
    RankGeom g;
    GHF_REQUIRE(d > 0 && rows_q > 0 && N > 0 && B > 0 && nnz >= 0, "score_rank: bad shape");
    if (d > RK_MAX_D) return set_err(GHF_EUNSUPPORTED, "score_rank: d = %d exceeds %d", d, RK_MAX_D);
    GHF_REQUIRE(rank_geom_rank(B, N, d, &g), "score_rank: B or N out of range");
    GHF_REQUIRE(iq || B <= rows_q, "score_rank: B exceeds the rows of q");
    GHF_REQUIRE(ws_bytes >= score_rank_workspace_bytes(B, N, d), "score_rank: workspace of %zu bytes, need %zu", ws_bytes,
                score_rank_workspace_bytes(B, N, d));
    float* t = (float*)ws;
    int* valid = (int*)((char*)ws + rk_align((size_t)B * 4));
    const unsigned qb = (unsigned)cdiv(B, 256);
    rank_prep_kernel<<<qb, 256, 0, stream>>>(q, c, iq, target, rows_q, N, B, d, t, valid, (long long*)greater, (long long*)equal);
    GHF_LAUNCH_CHECK();
    RankArgs a = {};
    a.q = q; a.c = c; a.iq = iq; a.rows_q = rows_q; a.N = N; a.B = B; a.d = d;
    a.qtiles = g.qtiles; a.slab_tiles = g.slab_tiles; a.slabs = g.slabs;
    a.t = t; a.greater = (unsigned long long*)greater; a.equal = (unsigned long long*)equal;
    const int rc = launch_tiles<false>(a, stream);
    if (rc != GHF_OK) return rc;
    if (nnz > 0) {
        rank_filter_kernel<<<(unsigned)cdiv(nnz, 256), 256, 0, stream>>>(q, c, iq, target, filt_ptr, filt_idx, nnz, N, B, d, t, valid,
                                                                        a.greater, a.equal);
        GHF_LAUNCH_CHECK();
    }
    rank_finish_kernel<<<qb, 256, 0, stream>>>(t, valid, B, (long long*)greater, (long long*)equal);
    GHF_LAUNCH_CHECK();
    return GHF_OK;
}

int launch_score_topk(const float* q, const float* c, const int64_t* iq, const int64_t* filt_ptr, const int64_t* filt_idx,
                      int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d, int k, void* ws, size_t ws_bytes, float* scores,
                      int64_t* ids, hipStream_t stream) {
    RankGeom g;
    GHF_REQUIRE(d > 0 && rows_q > 0 && N > 0 && B > 0 && nnz >= 0, "score_topk: bad shape");
    GHF_REQUIRE(k >= 1 && k <= TOPK_MAX_K, "score_topk: k = %d outside 1..%d", k, TOPK_MAX_K);
    if (d > RK_MAX_D) return set_err(GHF_EUNSUPPORTED, "score_topk: d = %d exceeds %d", d, RK_MAX_D);
    GHF_REQUIRE(rank_geom_topk(B, N, d, &g), "score_topk: B or N out of range");
    GHF_REQUIRE(iq || B <= rows_q, "score_topk: B exceeds the rows of q");
    GHF_REQUIRE(ws_bytes >= score_topk_workspace_bytes(B, N, d, k), "score_topk: workspace of %zu bytes, need %zu", ws_bytes,
                score_topk_workspace_bytes(B, N, d, k));
    const int cap = topk_cap(d, k);
    int* valid = (int*)ws;
    uint64_t* ws_key = (uint64_t*)((char*)ws + rk_align((size_t)B * 4));
    rank_prep_kernel<<<(unsigned)cdiv(B, 256), 256, 0, stream>>>(q, c, iq, nullptr, rows_q, N, B, d, nullptr, valid, nullptr, nullptr);
    GHF_LAUNCH_CHECK();
    if (nnz > 0) {
        rank_filter_kernel<<<(unsigned)cdiv(nnz, 256), 256, 0, stream>>>(q, c, iq, nullptr, filt_ptr, filt_idx, nnz, N, B, d, nullptr,
                                                                        valid, nullptr, nullptr);
        GHF_LAUNCH_CHECK();
    }
    RankArgs a = {};
    a.q = q; a.c = c; a.iq = iq; a.rows_q = rows_q; a.N = N; a.B = B; a.d = d;
    a.qtiles = g.qtiles; a.slab_tiles = g.slab_tiles; a.slabs = g.slabs;
    a.filt_ptr = nnz > 0 ? filt_ptr : nullptr; a.filt_idx = filt_idx; a.nnz = nnz;
    a.k = k; a.cap = cap; a.ws_key = ws_key;
    const int rc = launch_tiles<true>(a, stream);
    if (rc != GHF_OK) return rc;
    topk_merge_kernel<<<(unsigned)cdiv(B, 4), 256, 0, stream>>>(ws_key, valid, B, g.slabs, cap, k, scores, (long long*)ids);
    GHF_LAUNCH_CHECK();
    return GHF_OK;
}

}  // namespace ghf
