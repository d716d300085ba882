// distance_sweep.hip — distance scores against EVERY node (or a candidate subset): filtered rank counts and top-k, the B x C
// distances never stored (include/ghf_distance_sweep.h).  rank.hip's two operations under ghf_distance.h's
// metrics, s(i, j) = -D(q_i, c_j).  L1 and the complex modulus have no matrix form, and L2 through |q|^2 + |c|^2 - 2 q.c loses
// its accuracy exactly where ranks are decided, so this sweep is a register-tiled VALU kernel of its own:
//
//   workgroup = 256 threads = 4 waves; block tile DS_CT = 256 candidates x DS_TQ = 64 queries.  THE LANE OWNS CANDIDATES (lane
//   l: candidates l, l + 64, l + 128, l + 192 of the tile), THE WAVE OWNS QUERIES (wave w: queries 16 w .. 16 w + 15 of the
//   tile): 16 x 4 = 64 accumulators a lane, one per (query, candidate) pair, every one an independent chain.
//   Candidate rows stream through two LDS buffers of DS_BK = 16 columns (rows through ic[j] when a subset is given), fetched
//   into registers one step ahead of the step being consumed: one barrier per step.  An LDS row is 20 floats, so that the 16
//   lanes of a 16-byte read phase touch all 64 banks once.  A lane reads 4 candidates x 4 k (four 16-byte reads) per 16
//   queries x 4 candidates x 4 k = 256 distance elements.
//   The wave's 16 query rows are wave-uniform: they are read from the constant address space at a readfirstlane'd row
//   offset, i.e. with scalar loads, and reach the VALU as SGPR operands — no LDS traffic and no VGPRs for the queries.
//   A workgroup owns (query tile, candidate slab); workgroups are numbered as in rank.hip so that an XCD runs the query tiles of
//   one slab together.
//
// Numerics: an accumulator is bit for bit dist_chain() of distance_sweep_dev.h — delta_k = q_k - c_k (one fp32 subtraction), then
//   L1       acc = acc + |delta_k|,                          k ascending from acc = 0
//   L2       acc = fmaf(delta_k, delta_k, acc),              k ascending, then one hardware root
//   COMPLEX  rho_p = sqrt(fmaf(delta_2p+1, delta_2p+1, delta_2p * delta_2p)),  acc = acc + rho_p,  p ascending
// with contraction off and the hardware's square root (ghf_distance.h).  Zero padding of k adds exactly 0.  The tile and
// dist_chain() run the same dist_step4(), four k at a time; the target's distance and the filter corrections come from
// dist_chain() and so compare equal to the tile's value of the same pair.  The vector and the scalar path differ in how the
// floats are loaded, not in the chain.  (ghf_dist_rank sums across a lane group: its bits are NOT these.)
//
// Rank:   as rank.hip — the prep pass validates ids and resets the counters, dist_target_kernel forms t_i, the sweep counts
//         popc(ballot(s > t_i)) / (s == t_i) per query into scalar registers and adds them once per (query, workgroup) with an
//         integer atomic, dsweep_filter_kernel takes the listed candidates out again, dsweep_finish_kernel the target.
// Top-k:  rank_sweep.h's keys, append buffers and select_in_place.  A query belongs to ONE wave, so its entry count and threshold
//         are wave-private: appends are a ballot and a prefix population count, no atomics.  Candidates of a query are
//         appended in ascending id (rc outer, lane inner) and the threshold moves only between steps, so a tie with it loses.
//         dsweep_merge_kernel merges the slabs' lists as topk_merge_kernel does.
#include "common.h"
#include "rank_sweep.h"
#include "distance_sweep_dev.h"
#include "../../include/ghf_distance_sweep.h"

namespace ghf {

static inline int dsweep_cap(int k) { return k + DS_CT + 64; }
static_assert(TOPK_MAX_K + DS_CT + 64 <= TOPK_EPL * 64, "select_in_place holds a whole append buffer");

struct DsGeom { int64_t qtiles, ctiles, slab_tiles, slabs; };

static inline bool dsweep_geom(int64_t B, int64_t C, int blocks_wanted, DsGeom* g) {
    if (B <= 0 || C <= 0 || C >= (int64_t)1 << 31 || B >= (int64_t)1 << 31) return false;
    g->qtiles = cdiv(B, DS_TQ);
    g->ctiles = cdiv(C, DS_CT);
    int64_t slabs = cdiv(blocks_wanted, g->qtiles);
    if (slabs > g->ctiles) slabs = g->ctiles;
    if (slabs < 1) slabs = 1;
    g->slab_tiles = cdiv(g->ctiles, slabs);
    // a slab is at least DS_MIN_TILES tiles (all of them when there are fewer): a workgroup's prologue (query ids, thresholds,
    // the first fetch) is then paid once per 1,024 candidates at the least
    if (g->slab_tiles < DS_MIN_TILES) g->slab_tiles = g->ctiles < DS_MIN_TILES ? g->ctiles : DS_MIN_TILES;
    g->slabs = cdiv(g->ctiles, g->slab_tiles);
    return g->qtiles * g->slabs < (int64_t)1 << 31;
}
// three workgroups fit a CU (LDS): two rounds for the counts, one for the lists (the longer the slab, the rarer an insertion)
static inline bool dsweep_geom_rank(int64_t B, int64_t C, DsGeom* g) { return dsweep_geom(B, C, 6 * RK_CUS, g); }
static inline bool dsweep_geom_topk(int64_t B, int64_t C, DsGeom* g) { return dsweep_geom(B, C, 3 * RK_CUS, g); }

static size_t dsweep_rank_workspace_bytes(int64_t B, int64_t C, int d, int64_t nnz) {
    DsGeom g;
    if (d <= 0 || d > RK_MAX_D || nnz < 0 || !dsweep_geom_rank(B, C, &g)) return 0;
    const size_t map = cand_workspace_bytes(B, nnz);
    if (!map) return 0;
    return rk_align((size_t)B * 4) + rk_align((size_t)B * 4) + map;       // t [B] float, valid [B] int32, the id map's
}

static size_t dsweep_topk_workspace_bytes(int64_t B, int64_t C, int d, int k, int64_t nnz) {
    DsGeom g;
    if (d <= 0 || d > RK_MAX_D || nnz < 0 || k < 1 || k > TOPK_MAX_K || !dsweep_geom_topk(B, C, &g)) return 0;
    const size_t map = cand_workspace_bytes(B, nnz);
    if (!map) return 0;
    const size_t entries = (size_t)B * (size_t)g.slabs * (size_t)dsweep_cap(k);
    return rk_align((size_t)B * 4) + rk_align(entries * 8) + map;         // valid [B] int32, keys, the id map's
}


// ---- the sweep --------------------------------------------------------------------------------------------------------------
struct DsweepArgs {
    const float* q; const float* c; const int64_t* iq; const int64_t* ic;
    int64_t rows_q, Nn, C, B;                // Nn rows of c; C candidates (the sweep's positions 0 .. C - 1)
    int d;
    int64_t qtiles, slab_tiles, slabs;
    // rank
    const float* t; unsigned long long* greater; unsigned long long* equal;
    // top-k (lists in position space)
    const int64_t* filt_ptr; const int64_t* filt_idx; int64_t nnz;
    int k, cap; uint64_t* ws_key;
};


template <int M, bool VEC, bool TOPK>
__global__ __launch_bounds__(256) void dsweep_tile_kernel(const DsweepArgs a) {
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(16))) float Cs[2 * DS_CT * DS_LDC];
    __shared__ int cntS[DS_TQ];
    __shared__ float thrS[DS_TQ];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int d = a.d, dpad = (d + 3) & ~3;

    int64_t wg = blockIdx.x;
    const int64_t per_xcd = gridDim.x / 8;
    if (wg < per_xcd * 8) wg = (wg % 8) * per_xcd + wg / 8;
    const int64_t qt = wg % a.qtiles, slab = wg / a.qtiles;
    const int64_t q0 = qt * DS_TQ + wave * DS_RQ;           // the wave's first query
    const int64_t ctiles = (a.C + DS_CT - 1) / DS_CT;
    const int64_t tile0 = slab * a.slab_tiles;
    const int64_t tile1 = tile0 + a.slab_tiles < ctiles ? tile0 + a.slab_tiles : ctiles;
    const bool vc = rows_vec(a.c, d);

    // the wave's query rows: a uniform row number each (a query past B or with an id out of range reads row 0: its results
    // are never used), the row itself through the constant address space, i.e. scalar loads into SGPRs
    ds_cfloat* qc = (ds_cfloat*)a.q;
    int qrow[DS_RQ];
    float tq[DS_RQ];
    int gt[DS_RQ], eq[DS_RQ];
#pragma unroll
    for (int rq = 0; rq < DS_RQ; ++rq) {
        const int64_t qi = q0 + rq;
        int64_t r = 0;
        float t = __int_as_float(0x7FC00000);
        if (qi < a.B) {
            r = a.iq ? a.iq[qi] : qi;
            if ((uint64_t)r >= (uint64_t)a.rows_q) r = 0;
            if (!TOPK) t = a.t[qi];
        }
        qrow[rq] = __builtin_amdgcn_readfirstlane((int)r);
        tq[rq] = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(t)));
        gt[rq] = 0;
        eq[rq] = 0;
    }
    if (TOPK && tid < DS_TQ) {
        cntS[tid] = 0;
        thrS[tid] = qt * DS_TQ + tid < a.B ? -INFINITY : INFINITY;
    }

    const int nch = (dpad + DS_BK - 1) / DS_BK;
    const int64_t total = (tile1 - tile0) * nch;

    // the rows this thread fetches are the same DS_NL of a tile for every chunk of it: their row ids (through ic when given) are
    // loaded a whole tile ahead, cid for the tile being fetched, nid for the one after; -1 = no row
    f32x4 pre[DS_NL];
    int cid[DS_NL], nid[DS_NL];
    const int frow = tid >> 2, fc4 = tid & 3;                // thread -> (row frow + 64 i, floats 4 fc4 .. 4 fc4 + 3)
    auto load_ids = [&](int64_t tile, int* out) {
#pragma unroll
        for (int i = 0; i < DS_NL; ++i) {
            const int64_t cand = tile * DS_CT + frow + 64 * i;
            int64_t id = -1;
            if (cand < a.C) id = a.ic ? a.ic[cand] : cand;
            out[i] = (uint64_t)id < (uint64_t)a.Nn ? (int)id : -1;
        }
    };
    auto fetch = [&](int kc) {
#pragma unroll
        for (int i = 0; i < DS_NL; ++i)
            pre[i] = load_k4(cid[i] >= 0 ? a.c + (size_t)cid[i] * d : nullptr, kc * DS_BK + fc4 * 4, d, vc);
    };
    auto stash = [&](int buf) {
#pragma unroll
        for (int i = 0; i < DS_NL; ++i) *(f32x4*)(Cs + (buf * DS_CT + frow + 64 * i) * DS_LDC + fc4 * 4) = pre[i];
    };

    float acc[DS_RQ][DS_RC];
#pragma unroll
    for (int rq = 0; rq < DS_RQ; ++rq)
#pragma unroll
        for (int rc = 0; rc < DS_RC; ++rc) acc[rq][rc] = 0.f;

    load_ids(tile0, cid);
    load_ids(tile0 + 1, nid);
    fetch(0);
    stash(0);
    __syncthreads();

    int64_t tile = tile0;
    int kc = 0, buf = 0;
    for (int64_t step = 0; step < total; ++step) {
        int64_t ntile = tile;
        int nkc = kc + 1;
        if (nkc == nch) { nkc = 0; ++ntile; }
        const bool more = step + 1 < total;
        if (more && nkc == 0) {
#pragma unroll
            for (int i = 0; i < DS_NL; ++i) cid[i] = nid[i];
            load_ids(ntile + 1, nid);
        }
        if (more) fetch(nkc);

        const int k0 = kc * DS_BK;
        const float* cs = Cs + (buf * DS_CT + lane) * DS_LDC;
#pragma unroll 1
        for (int k4 = 0; k4 < DS_BK / 4; ++k4) {
            const int k = k0 + 4 * k4;
            if (k >= dpad) break;
            f32x4 cv[DS_RC];
#pragma unroll
            for (int rc = 0; rc < DS_RC; ++rc) cv[rc] = *(const f32x4*)(cs + rc * 64 * DS_LDC + 4 * k4);
#pragma unroll
            for (int rq = 0; rq < DS_RQ; ++rq) {
                const size_t off = (size_t)qrow[rq] * d + k;
                f32x4 qv;
                if constexpr (VEC) {
                    qv = *(ds_cf32x4*)(qc + off);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) qv[e] = k + e < d ? qc[off + e] : 0.f;
                }
#pragma unroll
                for (int rc = 0; rc < DS_RC; ++rc) acc[rq][rc] = dist_step4<M>(acc[rq][rc], qv, cv[rc]);
            }
        }

        const bool tile_done = kc == nch - 1;
        if (tile_done) {
            const int64_t base = tile * DS_CT + lane;           // + 64 rc: the accumulator's candidate
            if constexpr (!TOPK) {
#pragma unroll
                for (int rq = 0; rq < DS_RQ; ++rq)
#pragma unroll
                    for (int rc = 0; rc < DS_RC; ++rc) {
                        const float s = -dist_finish<M>(acc[rq][rc]);
                        const bool in = base + 64 * rc < a.C;
                        gt[rq] += __popcll(__ballot(in && s > tq[rq]));
                        eq[rq] += __popcll(__ballot(in && s == tq[rq]));
                    }
            } else {
                __syncthreads();        // the selections that followed the previous tile are done: counts and thresholds stand
#pragma unroll
                for (int rq = 0; rq < DS_RQ; ++rq) {
                    const int qcol = wave * DS_RQ + rq;
                    const float thr = thrS[qcol];
                    float s[DS_RC];
                    bool pass[DS_RC], any = false;
#pragma unroll
                    for (int rc = 0; rc < DS_RC; ++rc) {
                        s[rc] = -dist_finish<M>(acc[rq][rc]);
                        pass[rc] = s[rc] > thr && base + 64 * rc < a.C;
                        any |= pass[rc];
                    }
                    if (__ballot(any) != 0) {                   // the whole wave: thr is +inf for a query past B
                        const int64_t qi = q0 + rq;
                        int64_t f0 = 0, f1 = 0;
                        if (a.filt_ptr) {
                            int64_t lo = a.filt_ptr[qi], hi = a.filt_ptr[qi + 1];
                            lo = lo < 0 ? 0 : (lo > a.nnz ? a.nnz : lo);
                            hi = hi < lo ? lo : (hi > a.nnz ? a.nnz : hi);
                            f0 = lo;
                            f1 = hi;
                        }
                        const size_t row = ((size_t)qi * a.slabs + slab) * a.cap;
                        int cnt = cntS[qcol];
#pragma unroll
                        for (int rc = 0; rc < DS_RC; ++rc) {
                            const int64_t cand = base + 64 * rc;
                            const bool keep = pass[rc] && !(f1 > f0 && in_filter(a.filt_idx, f0, f1, cand));
                            const uint64_t mask = __ballot(keep);
                            const int pos = cnt + __popcll(mask & ((1ull << lane) - 1));
                            if (keep && pos < a.cap) a.ws_key[row + pos] = topk_key(s[rc], (int)cand);
                            cnt += __popcll(mask);
                        }
                        if (lane == 0) cntS[qcol] = cnt;
                    }
                }
            }
#pragma unroll
            for (int rq = 0; rq < DS_RQ; ++rq)
#pragma unroll
                for (int rc = 0; rc < DS_RC; ++rc) acc[rq][rc] = 0.f;
        }

        if (more) stash(buf ^ 1);
        __syncthreads();
        if (TOPK && tile_done && more) {
            // a query whose buffer could overflow in the next tile keeps its k best now; the wave's own queries
            for (int rq = 0; rq < DS_RQ; ++rq) {
                const int qcol = wave * DS_RQ + rq;
                const int m = cntS[qcol] < a.cap ? cntS[qcol] : a.cap;
                if (m > a.cap - DS_CT) {
                    const size_t row = ((size_t)(q0 + rq) * a.slabs + slab) * a.cap;
                    select_in_place(a.ws_key + row, m, a.k, lane, &thrS[qcol], &cntS[qcol], false);
                }
            }
        }
        tile = ntile;
        kc = nkc;
        buf ^= 1;
    }

    if constexpr (!TOPK) {
        // one integer atomic per (query, workgroup) and counter: order-free, so reproducible
        if (lane == 0) {
#pragma unroll
            for (int rq = 0; rq < DS_RQ; ++rq) {
                if (q0 + rq < a.B) {
                    if (gt[rq]) atomicAdd(&a.greater[q0 + rq], (unsigned long long)gt[rq]);
                    if (eq[rq]) atomicAdd(&a.equal[q0 + rq], (unsigned long long)eq[rq]);
                }
            }
        }
    } else {
        // the slab's list of every query: k entries, sorted, padded with empty slots
        for (int rq = 0; rq < DS_RQ; ++rq) {
            if (q0 + rq >= a.B) break;
            const int qcol = wave * DS_RQ + rq;
            const int m = cntS[qcol] < a.cap ? cntS[qcol] : a.cap;
            const size_t row = ((size_t)(q0 + rq) * a.slabs + slab) * a.cap;
            select_in_place(a.ws_key + row, m, a.k, lane, &thrS[qcol], &cntS[qcol], true);
        }
    }
}

// ---- the small kernels around the sweep -------------------------------------------------------------------------------------
// one thread per filter entry, as rank_filter_kernel: an id out of range marks its query; any other entry's score is recomputed
// and taken out of the count it went into.  Over a subset the lists and `tpos` are positions in ic (candidates.hip).
__global__ __launch_bounds__(256) void dsweep_filter_kernel(int metric, const float* __restrict__ q, const float* __restrict__ c,
                                                            const int64_t* __restrict__ iq, const int64_t* __restrict__ tpos,
                                                            const int64_t* __restrict__ filt_ptr, const int64_t* __restrict__ filt_idx,
                                                            int64_t nnz, int64_t M, int64_t B, int d, const float* __restrict__ t,
                                                            int* valid, unsigned long long* __restrict__ greater,
                                                            unsigned long long* __restrict__ equal, const int64_t* __restrict__ ic) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= nnz) return;
    int64_t i;
    if (!list_owner(filt_ptr, B, e, &i)) return;
    const int64_t j = filt_idx[e];
    if (j < 0 || j >= M) {
        valid[i] = 0;
        return;
    }
    if (!valid[i]) return;
    if (j == tpos[i] || (e > filt_ptr[i] && filt_idx[e - 1] == j)) return;
    const int64_t r = iq ? iq[i] : i;                // in range: the prep pass said so (valid[i] was 1)
    const float s = -dist_chain(metric, q + (size_t)r * d, c + (size_t)(ic ? ic[j] : j) * d, d, rows_vec(q, d) && rows_vec(c, d));
    const float ti = t[i];
    if (s > ti) atomicAdd(&greater[i], ~0ull);
    else if (s == ti) atomicAdd(&equal[i], ~0ull);
}

__global__ __launch_bounds__(256) void dsweep_finish_kernel(const float* __restrict__ t, const int* __restrict__ valid, int64_t B,
                                                            long long* __restrict__ greater, long long* __restrict__ equal,
                                                            const int64_t* __restrict__ tpos) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= B) return;
    if (!valid[i]) {
        greater[i] = -1;
        equal[i] = -1;
    } else if (t[i] == t[i] && (!tpos || tpos[i] >= 0)) {
        equal[i] -= 1;                               // the target's own score, counted by the tile that holds it
    }
}

// merge the slabs' sorted lists, one wave per query: topk_merge_kernel's scheme (a key's position is the number of keys above it)
__global__ __launch_bounds__(256) void dsweep_merge_kernel(const uint64_t* __restrict__ ws_key, const int* __restrict__ valid,
                                                           int64_t B, int64_t slabs, int cap, int k, float* __restrict__ out_sc,
                                                           long long* __restrict__ out_id, const int64_t* __restrict__ ic) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= B) return;
    float* os = out_sc + (size_t)i * k;
    long long* oi = out_id + (size_t)i * k;
    if (!valid[i]) {
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
            int lo = 0, hi = k;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (keys[sl * cap + mid] > key) lo = mid + 1; else hi = mid;
            }
            rank += lo;
        }
        if (rank < k) {
            os[rank] = key_score(key);
            oi[rank] = ic ? ic[key_id(key)] : key_id(key);
        }
    }
    for (int off = 32; off; off >>= 1) mine += __shfl_xor(mine, off, 64);
    for (int64_t p = mine + lane; p < k; p += 64) {
        os[p] = -INFINITY;
        oi[p] = -1;
    }
}

// ---- launches ---------------------------------------------------------------------------------------------------------------
template <bool TOPK>
static int launch_dsweep_tiles(int metric, const DsweepArgs& a, hipStream_t stream) {
    const unsigned grid = (unsigned)(a.qtiles * a.slabs);
    const bool vec = (a.d & 3) == 0 && ((uintptr_t)a.q & 15) == 0;
#define GHF_DSWEEP_LAUNCH(MM)                                                              \
    do {                                                                                    \
        if (vec) dsweep_tile_kernel<MM, true, TOPK><<<grid, 256, 0, stream>>>(a);           \
        else dsweep_tile_kernel<MM, false, TOPK><<<grid, 256, 0, stream>>>(a);              \
    } while (0)
    if (metric == GHF_DIST_L1) GHF_DSWEEP_LAUNCH(GHF_DIST_L1);
    else if (metric == GHF_DIST_L2) GHF_DSWEEP_LAUNCH(GHF_DIST_L2);
    else GHF_DSWEEP_LAUNCH(GHF_DIST_COMPLEX);
#undef GHF_DSWEEP_LAUNCH
    GHF_LAUNCH_CHECK();
    return GHF_OK;
}

// what both launches open with; M = the candidates the sweep runs over
static int dsweep_open(const char* op, bool geom_ok, const DsGeom& g, size_t need, const float* q, const float* c, const int64_t* iq,
                       int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d, const int64_t* ic, int64_t C, size_t ws_bytes,
                       DsweepArgs* a) {
    GHF_REQUIRE(d > 0 && rows_q > 0 && N > 0 && B > 0 && nnz >= 0, "%s: bad shape", op);
    if (d > RK_MAX_D) return set_err(GHF_EUNSUPPORTED, "%s: d = %d exceeds %d", op, d, RK_MAX_D);
    GHF_REQUIRE(N < (int64_t)1 << 31, "%s: N = %lld rows, the sweep keeps row ids in 32 bits", op, (long long)N);
    // the tile kernel keeps a query's row number in one SGPR (qrow[]): a table of 2^31 rows or more is refused here
    GHF_REQUIRE(rows_q < (int64_t)1 << 31, "%s: rows_q = %lld rows of q, the sweep keeps row ids in 32 bits", op, (long long)rows_q);
    GHF_REQUIRE(ic ? (C > 0 && C <= N) : C == N, "%s: need 1 <= C <= N candidates, C == N without ic", op);
    GHF_REQUIRE(geom_ok, "%s: B or C out of range", op);
    GHF_REQUIRE(iq || B <= rows_q, "%s: B exceeds the rows of q", op);
    GHF_REQUIRE(need > 0 && ws_bytes >= need, "%s: workspace of %zu bytes, need %zu", op, ws_bytes, need);
    *a = DsweepArgs{};
    a->q = q; a->c = c; a->iq = iq; a->ic = ic; a->rows_q = rows_q; a->Nn = N; a->C = C; a->B = B; a->d = d;
    a->qtiles = g.qtiles; a->slab_tiles = g.slab_tiles; a->slabs = g.slabs;
    return GHF_OK;
}

static int launch_dsweep_rank(int metric, const float* q, const float* c, const int64_t* iq, const int64_t* target,
                              const int64_t* filt_ptr, const int64_t* filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B,
                              int d, const int64_t* ic, int64_t C, void* ws, size_t ws_bytes, int64_t* greater, int64_t* equal,
                              hipStream_t stream) {
    DsweepArgs a;
    DsGeom g = {};
    const bool geom_ok = dsweep_geom_rank(B, C, &g);
    const size_t need = d > 0 && d <= RK_MAX_D ? dsweep_rank_workspace_bytes(B, C, d, nnz) : 0;
    int rc = dsweep_open("dist_sweep_rank", geom_ok, g, need, q, c, iq, nnz, rows_q, N, B, d, ic, C, ws_bytes, &a);
    if (rc != GHF_OK) return rc;
    const size_t base = rk_align((size_t)B * 4) * 2;
    float* t = (float*)ws;
    int* valid = (int*)((char*)ws + rk_align((size_t)B * 4));
    const unsigned qb = (unsigned)cdiv(B, 256);
    const int64_t* tpos = target;                    // all nodes: a node's position is its id
    if (ic) {
        CandMap m = {};
        rc = launch_cand_map(q, c, iq, target, false, filt_ptr, filt_idx, nnz, ic, C, rows_q, N, B, d, nullptr, nullptr, valid, greater,
                             equal, (char*)ws + base, need - base, &m, stream);
        if (rc != GHF_OK) return rc;
        tpos = m.tpos; filt_ptr = m.ptr; filt_idx = m.idx;
    } else {
        score_prep_kernel<<<qb, 256, 0, stream>>>(q, c, iq, target, rows_q, N, B, d, nullptr, valid, (long long*)greater, (long long*)equal);
        GHF_LAUNCH_CHECK();
    }
    dist_target_kernel<<<qb, 256, 0, stream>>>(metric, q, c, iq, target, valid, B, d, t);
    GHF_LAUNCH_CHECK();
    a.t = t; a.greater = (unsigned long long*)greater; a.equal = (unsigned long long*)equal;
    rc = launch_dsweep_tiles<false>(metric, a, stream);
    if (rc != GHF_OK) return rc;
    if (nnz > 0) {
        dsweep_filter_kernel<<<(unsigned)cdiv(nnz, 256), 256, 0, stream>>>(metric, q, c, iq, tpos, filt_ptr, filt_idx, nnz, C, B, d, t,
                                                                          valid, a.greater, a.equal, ic);
        GHF_LAUNCH_CHECK();
    }
    dsweep_finish_kernel<<<qb, 256, 0, stream>>>(t, valid, B, (long long*)greater, (long long*)equal, ic ? tpos : nullptr);
    GHF_LAUNCH_CHECK();
    return GHF_OK;
}

static int launch_dsweep_topk(int metric, const float* q, const float* c, const int64_t* iq, const int64_t* filt_ptr,
                              const int64_t* filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d, int k,
                              const int64_t* ic, int64_t C, void* ws, size_t ws_bytes, float* scores, int64_t* ids,
                              hipStream_t stream) {
    DsweepArgs a;
    DsGeom g = {};
    GHF_REQUIRE(k >= 1 && k <= TOPK_MAX_K, "dist_sweep_topk: k = %d outside 1..%d", k, TOPK_MAX_K);
    const bool geom_ok = dsweep_geom_topk(B, C, &g);
    const size_t need = d > 0 && d <= RK_MAX_D ? dsweep_topk_workspace_bytes(B, C, d, k, nnz) : 0;
    int rc = dsweep_open("dist_sweep_topk", geom_ok, g, need, q, c, iq, nnz, rows_q, N, B, d, ic, C, ws_bytes, &a);
    if (rc != GHF_OK) return rc;
    const size_t base = rk_align((size_t)B * 4) + rk_align((size_t)B * (size_t)g.slabs * (size_t)dsweep_cap(k) * 8);
    int* valid = (int*)ws;
    a.k = k; a.cap = dsweep_cap(k); a.ws_key = (uint64_t*)((char*)ws + rk_align((size_t)B * 4));
    a.filt_ptr = nnz > 0 ? filt_ptr : nullptr; a.filt_idx = filt_idx; a.nnz = nnz;
    if (ic) {
        CandMap m = {};
        rc = launch_cand_map(q, c, iq, nullptr, false, filt_ptr, filt_idx, nnz, ic, C, rows_q, N, B, d, nullptr, nullptr, valid, nullptr,
                             nullptr, (char*)ws + base, need - base, &m, stream);
        if (rc != GHF_OK) return rc;
        a.filt_ptr = m.ptr; a.filt_idx = m.idx;
    } else {
        score_prep_kernel<<<(unsigned)cdiv(B, 256), 256, 0, stream>>>(q, c, iq, nullptr, rows_q, N, B, d, nullptr, valid, nullptr, nullptr);
        GHF_LAUNCH_CHECK();
        if (nnz > 0) {
            list_range_kernel<<<(unsigned)cdiv(nnz, 256), 256, 0, stream>>>(filt_ptr, filt_idx, nnz, N, B, valid);
            GHF_LAUNCH_CHECK();
        }
    }
    rc = launch_dsweep_tiles<true>(metric, a, stream);
    if (rc != GHF_OK) return rc;
    dsweep_merge_kernel<<<(unsigned)cdiv(B, 4), 256, 0, stream>>>(a.ws_key, valid, B, a.slabs, a.cap, k, scores, (long long*)ids, ic);
    GHF_LAUNCH_CHECK();
    return GHF_OK;
}

}  // namespace ghf

// ---- the C ABI (include/ghf_distance_sweep.h) -------------------------------------------------------------------------------
using namespace ghf;

extern "C" {

#define GHF_DSWEEP_METRIC(op, dd)                                                                                            \
    do {                                                                                                                     \
        GHF_REQUIRE(metric == GHF_DIST_L1 || metric == GHF_DIST_L2 || metric == GHF_DIST_COMPLEX,                            \
                    op ": metric must be GHF_DIST_L1, GHF_DIST_L2 or GHF_DIST_COMPLEX");                                     \
        GHF_REQUIRE(metric != GHF_DIST_COMPLEX || ((dd) & 1) == 0, op ": GHF_DIST_COMPLEX needs an even d (re / im interleaved)"); \
    } while (0)

#define GHF_DSWEEP_ENTRY(op, ptrs)                                                                                           \
    do {                                                                                                                     \
        GHF_REQUIRE((ptrs) && workspace, op ": null pointer argument");                                                      \
        GHF_REQUIRE(nnz <= 0 || (filt_ptr && filt_idx), op ": null filter list with nnz > 0");                               \
        GHF_REQUIRE(((uintptr_t)workspace & 255) == 0, op ": workspace not 256-byte aligned");                               \
    } while (0)

size_t ghf_dist_sweep_rank_workspace_bytes(int64_t B, int64_t C, int d, int64_t nnz) {
    return dsweep_rank_workspace_bytes(B, C, d, nnz);
}

int ghf_dist_sweep_rank(int metric, const float* q, const float* c, const int64_t* iq, const int64_t* target,
                        const int64_t* filt_ptr, const int64_t* filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d,
                        const int64_t* ic, int64_t C, void* workspace, size_t workspace_bytes, int64_t* greater, int64_t* equal,
                        void* stream) {
    GHF_DSWEEP_METRIC("dist_sweep_rank", d);
    GHF_DSWEEP_ENTRY("dist_sweep_rank", q && c && target && greater && equal);
    return launch_dsweep_rank(metric, q, c, iq, target, filt_ptr, filt_idx, nnz, rows_q, N, B, d, ic, C, workspace, workspace_bytes,
                              greater, equal, (hipStream_t)stream);
}

size_t ghf_dist_sweep_topk_workspace_bytes(int64_t B, int64_t C, int d, int k, int64_t nnz) {
    return dsweep_topk_workspace_bytes(B, C, d, k, nnz);
}

int ghf_dist_sweep_topk(int metric, const float* q, const float* c, const int64_t* iq, const int64_t* filt_ptr,
                        const int64_t* filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d, int k, const int64_t* ic,
                        int64_t C, void* workspace, size_t workspace_bytes, float* scores, int64_t* ids, void* stream) {
    GHF_DSWEEP_METRIC("dist_sweep_topk", d);
    GHF_DSWEEP_ENTRY("dist_sweep_topk", q && c && scores && ids);
    return launch_dsweep_topk(metric, q, c, iq, filt_ptr, filt_idx, nnz, rows_q, N, B, d, k, ic, C, workspace, workspace_bytes, scores,
                              ids, (hipStream_t)stream);
}

#undef GHF_DSWEEP_ENTRY
#undef GHF_DSWEEP_METRIC

}  // extern "C"
