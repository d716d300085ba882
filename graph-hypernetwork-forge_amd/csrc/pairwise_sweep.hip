// pairwise_sweep.hip — the pairwise ranking losses (hinge, logistic) under a DISTANCE score against every node or a shared
// candidate subset, forward and backward, the B x C distances, ids and coefficients never stored
// (include/ghf_pairwise_sweep.h).
//
// Forward: distance_loss.hip's tile loop, its geometry unchanged (the lane owns 4 candidates, the wave owns 16 queries,
//   candidate rows through two LDS buffers, query rows through scalar loads; distance_sweep_dev.h's chain; the LDS cursor that
//   lets an unlisted full tile touch no memory; slabs from C alone), with a pairwise epilogue.  The target's z_it is known
//   before the tiles start (psweep_target_kernel, the tile's chain) and sits in LDS beside the targets' positions, so a
//   finished tile turns the lane's four z of a query into u = (z - z_it) + margin at once and adds phi(u), phi'(u), 1 and
//   [u > 0] into the lane's four running values — a pair outside J_i adds +0.f and 0.  At the slab's end the lanes merge by
//   the fixed xor butterfly and lane 0 writes one 16-byte partial per (query, slab); psweep_finish_kernel adds the slabs in
//   slab order.
//
// Backward: distance_loss.hip's two passes, their structure unchanged — psweep_bwd_kernel<M, VEC, DQ, HINGE>: the lane OWNS a
//   row in its own LDS row, the other side is STREAMED four wave-uniform rows at a time, phase 1 runs the full chain (the
//   forward's D, bit for bit), phase 2 adds G g_k into 128 static accumulators, d > 128 runs as two column halves, slabs and
//   then launch_ordered_sum.  The coefficient is new: G_ij = w_i phi'(u_ij) on J_i and G_it = -w_i dsum_i on the target pair,
//   which needs no second sweep because dsum_i = sum_j phi'(u_ij) is the forward's (for the hinge the integer `active`).
//   psweep_saved_kernel forms z_it, w_i and G_it once per query for both passes.
//
// The kernel texts restate distance_loss.hip's with another epilogue / coefficient; that file is untouched (folding the two
// into one text is DESIGN.md §27's follow-up, as §23 folded the per-query family).  The public `kind` becomes the template
// parameter HINGE on the host, once, and nothing else: it shares no argument with a kernel selector (§23's trap).
#include "common.h"
#include "rank_sweep.h"
#include "distance_sweep_dev.h"
#include "../../include/ghf_pairwise_sweep.h"

#include <cmath>

namespace ghf {

// ---- geometry: distance_loss.hip's, number for number -----------------------------------------------------------------------
constexpr int PS_SLABS = 128;                // candidate slabs of the forward, at the most: from C alone
constexpr int PS_RS = 4;                     // streamed rows per group of the backward
constexpr int PS_OT = 64;                    // owner rows per workgroup of the backward (one wave)
constexpr int PS_ACC = 128;                  // accumulators a lane (columns per half)
constexpr int PS_ST = 256;                   // streamed rows per slab, at the least
constexpr int PS_BWD_WGS = 1024;             // workgroups a backward pass aims at

struct PsGeom { int64_t qtiles, ctiles, slab_tiles, slabs; };

static inline bool psweep_geom(int64_t B, int64_t C, PsGeom* g) {
    if (B <= 0 || C <= 0 || C >= (int64_t)1 << 31 || B >= (int64_t)1 << 31) return false;
    g->qtiles = cdiv(B, DS_TQ);
    g->ctiles = cdiv(C, DS_CT);
    g->slab_tiles = cdiv(g->ctiles, PS_SLABS);
    g->slabs = cdiv(g->ctiles, g->slab_tiles);
    return g->qtiles * g->slabs < (int64_t)1 << 31;
}

struct PsBwdGeom { int64_t otiles, slab_rows, slabs; };

static inline void psweep_bwd_geom(int64_t nO, int64_t nS, PsBwdGeom* g) {
    g->otiles = cdiv(nO, PS_OT);
    const int64_t st = cdiv(nS, PS_ST);
    int64_t slabs = cdiv(PS_BWD_WGS, g->otiles);
    if (slabs > st) slabs = st;
    if (slabs < 1) slabs = 1;
    const int64_t slab_tiles = cdiv(st, slabs);
    g->slabs = cdiv(st, slab_tiles);
    g->slab_rows = slab_tiles * PS_ST;
}

// one (sum phi, sum phi', n, active) per (query, slab)
struct __attribute__((aligned(16))) PsPart { float f, g; int n, a; };

static size_t psweep_fwd_workspace_bytes(int64_t B, int64_t C, int d, int64_t nnz) {
    PsGeom g;
    if (d <= 0 || d > RK_MAX_D || nnz < 0 || !psweep_geom(B, C, &g)) return 0;
    const size_t map = cand_workspace_bytes(B, nnz);
    if (!map) return 0;
    // t [B] float, valid [B] int32, the partials [B, slabs], the id map's
    return 2 * rk_align((size_t)B * 4) + rk_align((size_t)B * (size_t)g.slabs * sizeof(PsPart)) + map;
}

static size_t psweep_bwd_part_bytes(int64_t nO, int64_t nS, int d) {
    PsBwdGeom g;
    psweep_bwd_geom(nO, nS, &g);
    return g.slabs > 1 ? rk_align((size_t)g.slabs * (size_t)nO * (size_t)d * 4) : 0;
}

static size_t psweep_bwd_workspace_bytes(int64_t B, int64_t C, int d, int64_t nnz) {
    PsGeom g;
    if (d <= 0 || d > RK_MAX_D || nnz < 0 || !psweep_geom(B, C, &g)) return 0;
    const size_t map = cand_workspace_bytes(B, nnz);
    if (!map) return 0;
    // t -> z_it [B], valid [B] int32, w [B], G_it [B], the slabs' partials of dq and of dc, the id map's
    return 4 * rk_align((size_t)B * 4) + psweep_bwd_part_bytes(B, C, d) + psweep_bwd_part_bytes(C, B, d) + map;
}

// sigmoid(u), as negatives_dev.h's pairwise arm forms it
__device__ __forceinline__ float psweep_sigmoid(float u) {
#pragma clang fp contract(off)
    const float e = __expf(-fabsf(u)), rcp = __builtin_amdgcn_rcpf(1.f + e);
    return u >= 0.f ? rcp : e * rcp;
}

// ---- the forward sweep ------------------------------------------------------------------------------------------------------
struct PsweepArgs {
    const float* q; const float* c; const int64_t* iq; const int64_t* ic;
    int64_t rows_q, Nn, C, B;                // Nn rows of c; C candidates (the sweep's positions 0 .. C - 1)
    int d;
    int64_t qtiles, slab_tiles, slabs;
    const int64_t* tpos; const int* valid;   // the targets as positions; a query that is not valid has no target here
    const float* t;                          // -D of the target pair by the tile's chain (NaN: the query is not valid)
    const int64_t* filt_ptr; const int64_t* filt_idx; int64_t nnz;      // lists in position space
    float scale, margin;
    PsPart* part;                            // [B, slabs]
};

template <int M, bool VEC, bool HINGE>
__global__ __launch_bounds__(256) void psweep_tile_kernel(const PsweepArgs a) {
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(16))) float Cs[2 * DS_CT * DS_LDC];
    __shared__ int64_t tposS[DS_TQ], nxtS[DS_TQ], curS[DS_TQ], endS[DS_TQ];
    __shared__ float ztS[DS_TQ];
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

    // the wave's query rows, as the rank sweep's: a query past B or with an id out of range reads row 0, results never used
    ds_cfloat* qc = (ds_cfloat*)a.q;
    int qrow[DS_RQ];
#pragma unroll
    for (int rq = 0; rq < DS_RQ; ++rq) {
        const int64_t qi = q0 + rq;
        int64_t r = 0;
        if (qi < a.B) {
            r = a.iq ? a.iq[qi] : qi;
            if ((uint64_t)r >= (uint64_t)a.rows_q) r = 0;
        }
        qrow[rq] = __builtin_amdgcn_readfirstlane((int)r);
    }
    // per query of the tile: its target's position and z, and the cursor into its list, which starts at the slab's first
    // position
    if (tid < DS_TQ) {
        const int64_t qi = qt * DS_TQ + tid;
        int64_t tp = -1, cur = 0, end = 0, nxt = INT64_MAX;
        float zt = 0.f;
        if (qi < a.B) {
            if (a.valid[qi]) tp = a.tpos[qi];
            zt = a.scale * a.t[qi];
            if (a.filt_ptr) {
                int64_t lo = a.filt_ptr[qi], hi = a.filt_ptr[qi + 1];
                lo = lo < 0 ? 0 : (lo > a.nnz ? a.nnz : lo);
                hi = hi < lo ? lo : (hi > a.nnz ? a.nnz : hi);
                cur = filter_lower_bound(a.filt_idx, lo, hi, tile0 * DS_CT);
                end = hi;
                if (cur < hi) nxt = a.filt_idx[cur];
            }
        }
        tposS[tid] = tp; curS[tid] = cur; endS[tid] = end; nxtS[tid] = nxt; ztS[tid] = zt;
    }

    const int nch = (dpad + DS_BK - 1) / DS_BK;
    const int64_t total = (tile1 - tile0) * nch;

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
    float rf[DS_RQ], rg[DS_RQ];                              // the lane's sums of phi and of phi' per query
    int rn[DS_RQ], ra[DS_RQ];                                // its pairs of J_i and those with u > 0
#pragma unroll
    for (int rq = 0; rq < DS_RQ; ++rq) {
        rf[rq] = 0.f;
        rg[rq] = 0.f;
        rn[rq] = 0;
        ra[rq] = 0;
#pragma unroll
        for (int rc = 0; rc < DS_RC; ++rc) acc[rq][rc] = 0.f;
    }

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

        if (kc == nch - 1) {
            const int64_t tile_lo = tile * DS_CT, tile_end = tile_lo + DS_CT;
            const int64_t base = tile_lo + lane;                // + 64 rc: the accumulator's candidate
            const bool full = tile_end <= a.C;
#pragma unroll
            for (int rq = 0; rq < DS_RQ; ++rq) {
                const int qcol = wave * DS_RQ + rq;
                const int64_t nxt = nxtS[qcol], tp = tposS[qcol];
                const float zt = ztS[qcol];
                float z[DS_RC];
                bool out[DS_RC];
#pragma unroll
                for (int rc = 0; rc < DS_RC; ++rc) {
                    z[rc] = a.scale * -dist_finish<M>(acc[rq][rc]);
                    out[rc] = false;
                    acc[rq][rc] = 0.f;
                }
                const bool tin = tp >= tile_lo && tp < tile_end;
                if (!(full && nxt >= tile_end && !tin)) {       // the same answer in every lane of the wave
                    const bool look = nxt < tile_end;
                    const int64_t f0 = curS[qcol], f1 = endS[qcol];
#pragma unroll
                    for (int rc = 0; rc < DS_RC; ++rc) {
                        const int64_t cand = base + 64 * rc;
                        bool o = cand >= a.C || cand == tp;
                        if (look && !o) o = in_filter(a.filt_idx, f0, f1, cand);
                        out[rc] = o;
                    }
                    if (look) {                                 // the cursor moves behind this tile
                        const int64_t nf = filter_lower_bound(a.filt_idx, f0, f1, tile_end);
                        const int64_t nn = nf < f1 ? a.filt_idx[nf] : INT64_MAX;
                        if (lane == 0) {
                            curS[qcol] = nf;
                            nxtS[qcol] = nn;
                        }
                    }
                }
                // The pairs of the tile, rc ascending, each added without a branch: a pair outside J_i adds +0.f and 0.  The
                // one branch around a query's four pairs skips nothing that counts (all four outside J_i: four times +0.f, and
                // the sums are never -0.f) and is there for the compiler.  Nothing else orders the sixteen epilogues of a tile,
                // and scheduled side by side their temporaries take 290 to 305 registers: one wave per SIMD.  Behind a branch
                // a lane they run one query at a time, as negsamp's do behind its test of the maximum.
                float f = rf[rq], g = rg[rq];
                int n = rn[rq], ac = ra[rq];
                if (!(out[0] && out[1] && out[2] && out[3])) {
#pragma unroll
                    for (int rc = 0; rc < DS_RC; ++rc) {
                        const float u = (z[rc] - zt) + a.margin;
                        float phi;
                        if constexpr (HINGE) phi = u <= 0.f ? 0.f : u;      // not fmaxf: a NaN stays a NaN
                        else phi = softplus(u);
                        f += out[rc] ? 0.f : phi;
                        if constexpr (!HINGE) g += out[rc] ? 0.f : psweep_sigmoid(u);
                        n += out[rc] ? 0 : 1;
                        ac += !out[rc] && u > 0.f ? 1 : 0;
                    }
                }
                rf[rq] = f; rg[rq] = g; rn[rq] = n; ra[rq] = ac;
            }
        }

        if (more) stash(buf ^ 1);
        __syncthreads();
        tile = ntile;
        kc = nkc;
        buf ^= 1;
    }

    // the lanes' partials of a query, merged by a fixed butterfly; lane 0 writes the slab's partial
#pragma unroll
    for (int rq = 0; rq < DS_RQ; ++rq) {
        float f = rf[rq], g = rg[rq];
        int n = rn[rq], ac = ra[rq];
#pragma unroll
        for (int w = 1; w < 64; w *= 2) {
            f += __shfl_xor(f, w, 64);
            if constexpr (!HINGE) g += __shfl_xor(g, w, 64);
            n += __shfl_xor(n, w, 64);
            ac += __shfl_xor(ac, w, 64);
        }
        if (lane == 0 && q0 + rq < a.B) a.part[(size_t)(q0 + rq) * a.slabs + slab] = PsPart{f, g, n, ac};
    }
}

// ---- the small kernels around the sweeps ------------------------------------------------------------------------------------
// one thread per query, behind the pass that validated the ids: the target's score by the tile's chain, from its own row of c
// (node id); NaN for a query that is not valid
__global__ __launch_bounds__(256) void psweep_target_kernel(int metric, const float* __restrict__ q, const float* __restrict__ c,
                                                            const int64_t* __restrict__ iq, const int64_t* __restrict__ target,
                                                            const int* __restrict__ valid, int64_t B, int d, float* __restrict__ t) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= B) return;
    float v = __int_as_float(0x7FC00000);
    if (valid[i]) {
        const int64_t r = iq ? iq[i] : i;
        v = -dist_chain(metric, q + (size_t)r * d, c + (size_t)target[i] * d, d, rows_vec(q, d) && rows_vec(c, d));
    }
    t[i] = v;
}

// one thread per query: the slabs' partials in slab order, then the outputs
__global__ __launch_bounds__(256) void psweep_finish_kernel(const PsPart* __restrict__ part, const int* __restrict__ valid, int64_t B,
                                                            int64_t slabs, int hinge, int normalize, float* __restrict__ loss,
                                                            float* __restrict__ dsum, int* __restrict__ count,
                                                            int* __restrict__ active) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= B) return;
    const PsPart* p = part + (size_t)i * slabs;
    PsPart m = p[0];
    for (int64_t s = 1; s < slabs; ++s) {
        m.f += p[s].f;
        m.g += p[s].g;
        m.n += p[s].n;
        m.a += p[s].a;
    }
    float l = m.f;
    if (normalize) l = m.n > 0 ? m.f * (1.f / (float)m.n) : 0.f;
    const bool ok = valid[i] != 0;
    loss[i] = ok ? l : __int_as_float(0x7FC00000);
    dsum[i] = ok ? (hinge ? (float)m.a : m.g) : __int_as_float(0x7FC00000);
    count[i] = ok ? m.n : -1;
    active[i] = ok ? m.a : -1;
}

// one thread per query, behind psweep_target_kernel: what both passes of the backward read of a query — z_it in place of t
// (NaN: the query takes no part: not valid, or count <= 0), w_i and G_it
__global__ __launch_bounds__(256) void psweep_saved_kernel(const int* __restrict__ valid, const float* __restrict__ dsum,
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
    zt[i] = part ? scale * zt[i] : __int_as_float(0x7FC00000);
    w[i] = part ? wi : 0.f;
    gt[i] = part ? -(wi * dsum[i]) : 0.f;
}

// ---- the backward -----------------------------------------------------------------------------------------------------------
struct PsBwdArgs {
    const float* q; const float* c; const int64_t* iq; const int64_t* ic;
    int64_t rows_q, Nn, C, B;
    int d;
    const int64_t* tpos; const float* zt; const float* w; const float* gt;     // zt: NaN = the query takes no part
    const int64_t* filt_ptr; const int64_t* filt_idx; int64_t nnz;              // lists in position space
    float scale, margin;
    int64_t otiles, slab_rows, slabs;
    float* out;                                                                 // [slabs, owners, d]
};

// G of one pair: d loss / d s with s = -D.  The target's is the query's G_it, listed or not
template <bool HINGE>
__device__ __forceinline__ float psweep_coef(float z, float zt, float w, float gt, float margin, bool is_target, bool listed) {
#pragma clang fp contract(off)
    const float u = (z - zt) + margin;
    float g;
    if constexpr (HINGE) g = u > 0.f ? w : 0.f;
    else g = w * psweep_sigmoid(u);
    return is_target ? gt : (listed ? 0.f : g);
}

template <int M, bool VEC, bool DQ, bool HINGE>
__global__ __launch_bounds__(64) void psweep_bwd_kernel(const PsBwdArgs a) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) float Os[];
    const int lane = threadIdx.x;
    const int d = a.d, dpad = (d + 3) & ~3;
    const int ldo = (d <= PS_ACC ? PS_ACC : 2 * PS_ACC) + 4;
    const int64_t ot = blockIdx.x % a.otiles, slab = blockIdx.x / a.otiles;
    const int kb = blockIdx.y * PS_ACC;                      // the first column of this half
    const int64_t nO = DQ ? a.B : a.C, nS = DQ ? a.C : a.B;
    const int64_t o = ot * PS_OT + lane;                     // the lane's owner row (a query, or a candidate position)

    // the owner's row into the lane's own LDS row (zeros past d and for an absent row); only this lane reads it back
    int64_t orow = -1;
    if (o < nO) {
        if (DQ) {
            const int64_t r = a.iq ? a.iq[o] : o;
            if ((uint64_t)r < (uint64_t)a.rows_q) orow = r;
        } else {
            const int64_t id = a.ic ? a.ic[o] : o;
            if ((uint64_t)id < (uint64_t)a.Nn) orow = id;
        }
    }
    float* mine = Os + lane * ldo;
    {
        const float* ob = DQ ? a.q : a.c;
        const bool vo = rows_vec(ob, d);
        const float* src = orow >= 0 ? ob + (size_t)orow * d : nullptr;
        for (int k = 0; k < dpad; k += 4) *(f32x4*)(mine + k) = load_k4(src, k, d, vo);
    }

    // the owner's own state
    float o_zt = __int_as_float(0x7FC00000), o_w = 0.f, o_gt = 0.f;
    int64_t o_tp = -1, cur = 0, end = 0, nxt = INT64_MAX;
    bool o_live = orow >= 0;
    const int64_t s0 = slab * a.slab_rows;
    const int64_t s1 = s0 + a.slab_rows < nS ? s0 + a.slab_rows : nS;
    if (DQ && o < nO) {
        o_zt = a.zt[o];
        o_w = a.w[o];
        o_gt = a.gt[o];
        o_tp = a.tpos[o];
        o_live = o_live && o_zt == o_zt;
        if (a.filt_ptr) {                                    // the lane's cursor: candidates arrive in ascending position
            int64_t lo = a.filt_ptr[o], hi = a.filt_ptr[o + 1];
            lo = lo < 0 ? 0 : (lo > a.nnz ? a.nnz : lo);
            hi = hi < lo ? lo : (hi > a.nnz ? a.nnz : hi);
            cur = filter_lower_bound(a.filt_idx, lo, hi, s0);
            end = hi;
            if (cur < hi) nxt = a.filt_idx[cur];
        }
    }

    float out[PS_ACC];
#pragma unroll
    for (int k = 0; k < PS_ACC; ++k) out[k] = 0.f;

    ds_cfloat* sc = (ds_cfloat*)(DQ ? a.c : a.q);
    for (int64_t sg = s0; sg < s1; sg += PS_RS) {
        // the group's rows: wave-uniform row numbers (an absent row reads row 0 and its pairs count with G = 0)
        int srow[PS_RS];
        bool s_ok[PS_RS];
        float s_zt[PS_RS], s_w[PS_RS], s_gt[PS_RS];
        int64_t s_tp[PS_RS], s_lo[PS_RS], s_hi[PS_RS];
#pragma unroll
        for (int u = 0; u < PS_RS; ++u) {
            const int64_t sj = sg + u;
            bool ok = sj < s1;
            int64_t r = 0;
            s_zt[u] = 0.f; s_w[u] = 0.f; s_gt[u] = 0.f; s_tp[u] = -1; s_lo[u] = 0; s_hi[u] = 0;
            if (ok) {
                if (DQ) {
                    r = a.ic ? a.ic[sj] : sj;
                    ok = (uint64_t)r < (uint64_t)a.Nn;
                } else {
                    r = a.iq ? a.iq[sj] : sj;
                    ok = (uint64_t)r < (uint64_t)a.rows_q;
                    const float v = a.zt[sj];
                    ok = ok && v == v;
                    s_zt[u] = v;
                    s_w[u] = a.w[sj];
                    s_gt[u] = a.gt[sj];
                    s_tp[u] = a.tpos[sj];
                    if (a.filt_ptr) {
                        int64_t lo = a.filt_ptr[sj], hi = a.filt_ptr[sj + 1];
                        lo = lo < 0 ? 0 : (lo > a.nnz ? a.nnz : lo);
                        hi = hi < lo ? lo : (hi > a.nnz ? a.nnz : hi);
                        s_lo[u] = lo;
                        s_hi[u] = hi;
                    }
                }
            }
            s_ok[u] = ok;
            srow[u] = __builtin_amdgcn_readfirstlane(ok ? (int)r : 0);
        }
        auto streamed = [&](int u, int k) -> f32x4 {
            const size_t off = (size_t)srow[u] * d + k;
            f32x4 v;
            if constexpr (VEC) {
                v = *(ds_cf32x4*)(sc + off);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = k + e < d ? sc[off + e] : 0.f;
            }
            return v;
        };

        // phase 1: the chain over the whole row — the forward's D of the pair, bit for bit
        float D[PS_RS];
#pragma unroll
        for (int u = 0; u < PS_RS; ++u) D[u] = 0.f;
#pragma unroll 1
        for (int k = 0; k < dpad; k += 4) {
            const f32x4 ov = *(const f32x4*)(mine + k);
#pragma unroll
            for (int u = 0; u < PS_RS; ++u) {
                const f32x4 sv4 = streamed(u, k);
                D[u] = DQ ? dist_step4<M>(D[u], ov, sv4) : dist_step4<M>(D[u], sv4, ov);
            }
        }
        // the pairs' coefficients: + G g for a candidate's row, - G g for a query's
        float cf[PS_RS], rD[PS_RS];
        bool any = false;
#pragma unroll
        for (int u = 0; u < PS_RS; ++u) {
            D[u] = dist_finish<M>(D[u]);
            const float z = a.scale * -D[u];
            float G;
            if (DQ) {
                const int64_t j = sg + u;
                G = psweep_coef<HINGE>(z, o_zt, o_w, o_gt, a.margin, j == o_tp, nxt == j);
                if (nxt <= j) {
                    do {
                        ++cur;
                        nxt = cur < end ? a.filt_idx[cur] : INT64_MAX;
                    } while (nxt <= j);
                }
            } else {
                bool listed = false;
                if (s_hi[u] > s_lo[u]) {                     // wave-uniform: does the tile's range hold a listed position at all
                    const int64_t lb = filter_lower_bound(a.filt_idx, s_lo[u], s_hi[u], ot * PS_OT);
                    if (lb < s_hi[u] && a.filt_idx[lb] < ot * PS_OT + PS_OT) listed = in_filter(a.filt_idx, lb, s_hi[u], o);
                }
                G = psweep_coef<HINGE>(z, s_zt[u], s_w[u], s_gt[u], a.margin, o == s_tp[u], listed);
            }
            G = o_live && s_ok[u] ? G : 0.f;
            any |= G != 0.f;
            cf[u] = DQ ? -G : G;
            rD[u] = D[u] > 0.f ? __builtin_amdgcn_rcpf(D[u]) : 0.f;
        }
        if (__ballot(any) == 0) continue;                    // the whole wave

        // phase 2: out[k] += G g_k over this half's columns, statically indexed
#pragma unroll
        for (int k4 = 0; k4 < PS_ACC / 4; ++k4) {
            const int k = kb + 4 * k4;
            if (k < dpad) {
                const f32x4 ov = *(const f32x4*)(mine + k);
#pragma unroll
                for (int u = 0; u < PS_RS; ++u) {
                    const f32x4 sv4 = streamed(u, k);
                    const f32x4 dl = DQ ? ov - sv4 : sv4 - ov;
                    f32x4 g;
                    if constexpr (M == GHF_DIST_L1) {
                        // sign(delta), 0 at 0, without a compare: two factors of 2^100 take the smallest subnormal past 1 in
                        // magnitude (an overflow is +-inf), then a clamp to [-1, 1]
                        const f32x4 big = (dl * 0x1p100f) * 0x1p100f;
#pragma unroll
                        for (int e = 0; e < 4; ++e) g[e] = __builtin_amdgcn_fmed3f(big[e], -1.f, 1.f);
                    } else if constexpr (M == GHF_DIST_L2) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) g[e] = dl[e] * rD[u];
                    } else {
                        const float p0 = dsweep_sqrt(fmaf(dl[1], dl[1], dl[0] * dl[0])), p1 = dsweep_sqrt(fmaf(dl[3], dl[3], dl[2] * dl[2]));
                        const float r0 = p0 > 0.f ? __builtin_amdgcn_rcpf(p0) : 0.f, r1 = p1 > 0.f ? __builtin_amdgcn_rcpf(p1) : 0.f;
                        g = f32x4{dl[0] * r0, dl[1] * r0, dl[2] * r1, dl[3] * r1};
                    }
#pragma unroll
                    for (int e = 0; e < 4; ++e) out[4 * k4 + e] = fmaf(cf[u], g[e], out[4 * k4 + e]);
                }
            }
        }
    }

    // the lane's row of the slab's partial: every row of the pass is written, zeros included
    if (o < nO) {
        float* dst = a.out + ((size_t)slab * (size_t)nO + (size_t)o) * d;
        const bool vd = (d & 3) == 0 && ((uintptr_t)a.out & 15) == 0;
#pragma unroll
        for (int k4 = 0; k4 < PS_ACC / 4; ++k4) {
            const int k = kb + 4 * k4;
            if (k < d) {
                if (vd) {
                    *(f32x4*)(dst + k) = f32x4{out[4 * k4], out[4 * k4 + 1], out[4 * k4 + 2], out[4 * k4 + 3]};
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (k + e < d) dst[k + e] = out[4 * k4 + e];
                }
            }
        }
    }
}

// ---- launches ---------------------------------------------------------------------------------------------------------------
template <bool HINGE>
static int launch_psweep_tiles(int metric, const PsweepArgs& a, hipStream_t stream) {
    const unsigned grid = (unsigned)(a.qtiles * a.slabs);
    const bool vec = (a.d & 3) == 0 && ((uintptr_t)a.q & 15) == 0;
#define GHF_PSWEEP_LAUNCH(MM)                                                              \
    do {                                                                                   \
        if (vec) psweep_tile_kernel<MM, true, HINGE><<<grid, 256, 0, stream>>>(a);         \
        else psweep_tile_kernel<MM, false, HINGE><<<grid, 256, 0, stream>>>(a);            \
    } while (0)
    if (metric == GHF_DIST_L1) GHF_PSWEEP_LAUNCH(GHF_DIST_L1);
    else if (metric == GHF_DIST_L2) GHF_PSWEEP_LAUNCH(GHF_DIST_L2);
    else GHF_PSWEEP_LAUNCH(GHF_DIST_COMPLEX);
#undef GHF_PSWEEP_LAUNCH
    GHF_LAUNCH_CHECK();
    return GHF_OK;
}

template <int M, bool DQ, bool HINGE>
static int launch_psweep_bwd_pass(const PsBwdArgs& a, hipStream_t stream) {
    const float* streamed = DQ ? a.c : a.q;
    const bool vec = (a.d & 3) == 0 && ((uintptr_t)streamed & 15) == 0;
    const size_t lds = (size_t)PS_OT * ((a.d <= PS_ACC ? PS_ACC : 2 * PS_ACC) + 4) * 4;
    const dim3 grid((unsigned)(a.otiles * a.slabs), a.d <= PS_ACC ? 1u : 2u);
    if (vec) {
        GHF_SET_MAX_LDS((psweep_bwd_kernel<M, true, DQ, HINGE>), lds);
        psweep_bwd_kernel<M, true, DQ, HINGE><<<grid, 64, lds, stream>>>(a);
    } else {
        GHF_SET_MAX_LDS((psweep_bwd_kernel<M, false, DQ, HINGE>), lds);
        psweep_bwd_kernel<M, false, DQ, HINGE><<<grid, 64, lds, stream>>>(a);
    }
    GHF_LAUNCH_CHECK();
    return GHF_OK;
}

// one pass: the slabs' partials into `part` and their ordered sum into `result`, or straight into `result` with one slab
template <bool DQ, bool HINGE>
static int launch_psweep_bwd(int metric, PsBwdArgs a, float* part, float* result, hipStream_t stream) {
    const int64_t nO = DQ ? a.B : a.C, nS = DQ ? a.C : a.B;
    PsBwdGeom g;
    psweep_bwd_geom(nO, nS, &g);
    GHF_REQUIRE(g.otiles * g.slabs < (int64_t)1 << 31, "dist_pair_bwd: B or C out of range");
    a.otiles = g.otiles; a.slab_rows = g.slab_rows; a.slabs = g.slabs;
    a.out = g.slabs > 1 ? part : result;
    int rc;
    if (metric == GHF_DIST_L1) rc = launch_psweep_bwd_pass<GHF_DIST_L1, DQ, HINGE>(a, stream);
    else if (metric == GHF_DIST_L2) rc = launch_psweep_bwd_pass<GHF_DIST_L2, DQ, HINGE>(a, stream);
    else rc = launch_psweep_bwd_pass<GHF_DIST_COMPLEX, DQ, HINGE>(a, stream);
    if (rc != GHF_OK || g.slabs == 1) return rc;
    return launch_ordered_sum(part, g.slabs, nO * (int64_t)a.d, result, stream);
}

// what both launches open with: the checks past the entry points' own, in the header's order
static int psweep_open(const char* op, size_t need, const int64_t* iq, int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d,
                       const int64_t* ic, int64_t C, size_t ws_bytes) {
    PsGeom g;
    GHF_REQUIRE(d > 0 && rows_q > 0 && N > 0 && B > 0 && nnz >= 0, "%s: bad shape", op);
    GHF_REQUIRE(ic ? (C > 0 && C <= N) : C == N, "%s: need 1 <= C <= N candidates, C == N without ic", op);
    GHF_REQUIRE(iq || B <= rows_q, "%s: B exceeds the rows of q", op);
    GHF_REQUIRE(N < (int64_t)1 << 31, "%s: N = %lld rows, the sweep keeps row ids in 32 bits", op, (long long)N);
    GHF_REQUIRE(rows_q < (int64_t)1 << 31, "%s: rows_q = %lld rows of q, the sweep keeps row ids in 32 bits", op, (long long)rows_q);
    GHF_REQUIRE(psweep_geom(B, C, &g), "%s: B or C out of range", op);
    if (d > RK_MAX_D) return set_err(GHF_EUNSUPPORTED, "%s: d = %d exceeds %d", op, d, RK_MAX_D);
    GHF_REQUIRE(need > 0 && ws_bytes >= need, "%s: workspace of %zu bytes, need %zu", op, ws_bytes, need);
    return GHF_OK;
}

// valid [B], and the targets and lists in position space (with ic: through the id map at `map_ws`)
static int psweep_validate(const float* q, const float* c, const int64_t* iq, const int64_t* target, const int64_t** filt_ptr,
                           const int64_t** filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d, const int64_t* ic,
                           int64_t C, int* valid, void* map_ws, size_t map_bytes, const int64_t** tpos, hipStream_t stream) {
    *tpos = target;                                  // all nodes: a node's position is its id
    if (nnz <= 0) { *filt_ptr = nullptr; *filt_idx = nullptr; }
    if (ic) {                                        // a target that is no candidate: the query is not valid
        CandMap m = {};
        const int rc = launch_cand_map(q, c, iq, target, true, *filt_ptr, *filt_idx, nnz, ic, C, rows_q, N, B, d, nullptr, nullptr,
                                       valid, nullptr, nullptr, map_ws, map_bytes, &m, stream);
        if (rc != GHF_OK) return rc;
        *tpos = m.tpos; *filt_ptr = m.ptr; *filt_idx = m.idx;
    } else {
        score_prep_kernel<<<(unsigned)cdiv(B, 256), 256, 0, stream>>>(q, c, iq, target, rows_q, N, B, d, nullptr, valid, nullptr, nullptr);
        GHF_LAUNCH_CHECK();
        if (nnz > 0) {
            list_range_kernel<<<(unsigned)cdiv(nnz, 256), 256, 0, stream>>>(*filt_ptr, *filt_idx, nnz, N, B, valid);
            GHF_LAUNCH_CHECK();
        }
    }
    return GHF_OK;
}

template <bool HINGE>
static int launch_psweep_fwd(int metric, const float* q, const float* c, const int64_t* iq, const int64_t* target,
                             const int64_t* filt_ptr, const int64_t* filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B,
                             int d, float scale, float margin, int normalize, const int64_t* ic, int64_t C, void* ws, size_t ws_bytes,
                             float* loss, float* dsum, int* count, int* active, hipStream_t stream) {
    const size_t need = d > 0 && d <= RK_MAX_D ? psweep_fwd_workspace_bytes(B, C, d, nnz) : 0;
    int rc = psweep_open("dist_pair_fwd", need, iq, nnz, rows_q, N, B, d, ic, C, ws_bytes);
    if (rc != GHF_OK) return rc;
    PsGeom g;
    psweep_geom(B, C, &g);
    const size_t base = 2 * rk_align((size_t)B * 4) + rk_align((size_t)B * (size_t)g.slabs * sizeof(PsPart));
    float* t = (float*)ws;
    int* valid = (int*)((char*)ws + rk_align((size_t)B * 4));
    PsPart* part = (PsPart*)((char*)ws + 2 * rk_align((size_t)B * 4));
    const int64_t* tpos;
    rc = psweep_validate(q, c, iq, target, &filt_ptr, &filt_idx, nnz, rows_q, N, B, d, ic, C, valid, (char*)ws + base, need - base, &tpos,
                         stream);
    if (rc != GHF_OK) return rc;
    const unsigned qb = (unsigned)cdiv(B, 256);
    psweep_target_kernel<<<qb, 256, 0, stream>>>(metric, q, c, iq, target, valid, B, d, t);
    GHF_LAUNCH_CHECK();
    PsweepArgs a = {};
    a.q = q; a.c = c; a.iq = iq; a.ic = ic; a.rows_q = rows_q; a.Nn = N; a.C = C; a.B = B; a.d = d;
    a.qtiles = g.qtiles; a.slab_tiles = g.slab_tiles; a.slabs = g.slabs;
    a.tpos = tpos; a.valid = valid; a.t = t; a.filt_ptr = filt_ptr; a.filt_idx = filt_idx; a.nnz = nnz;
    a.scale = scale; a.margin = margin; a.part = part;
    rc = launch_psweep_tiles<HINGE>(metric, a, stream);
    if (rc != GHF_OK) return rc;
    psweep_finish_kernel<<<qb, 256, 0, stream>>>(part, valid, B, g.slabs, HINGE ? 1 : 0, normalize, loss, dsum, count, active);
    GHF_LAUNCH_CHECK();
    return GHF_OK;
}

template <bool HINGE>
static int launch_psweep_backward(int metric, const float* q, const float* c, const int64_t* iq, const int64_t* target,
                                  const int64_t* filt_ptr, const int64_t* filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B,
                                  int d, float scale, float margin, int normalize, const int64_t* ic, int64_t C, const float* dsum,
                                  const int* count, const float* grad, void* ws, size_t ws_bytes, float* dq, float* dc,
                                  hipStream_t stream) {
    const size_t need = d > 0 && d <= RK_MAX_D ? psweep_bwd_workspace_bytes(B, C, d, nnz) : 0;
    int rc = psweep_open("dist_pair_bwd", need, iq, nnz, rows_q, N, B, d, ic, C, ws_bytes);
    if (rc != GHF_OK) return rc;
    const size_t pq = psweep_bwd_part_bytes(B, C, d), pc = psweep_bwd_part_bytes(C, B, d);
    const size_t qbytes = rk_align((size_t)B * 4);
    const size_t base = 4 * qbytes + pq + pc;
    float* zt = (float*)ws;
    int* valid = (int*)((char*)ws + qbytes);
    float* w = (float*)((char*)ws + 2 * qbytes);
    float* gt = (float*)((char*)ws + 3 * qbytes);
    float* part_q = (float*)((char*)ws + 4 * qbytes);
    float* part_c = (float*)((char*)part_q + pq);
    const int64_t* tpos;
    rc = psweep_validate(q, c, iq, target, &filt_ptr, &filt_idx, nnz, rows_q, N, B, d, ic, C, valid, (char*)ws + base, need - base, &tpos,
                         stream);
    if (rc != GHF_OK) return rc;
    const unsigned qb = (unsigned)cdiv(B, 256);
    psweep_target_kernel<<<qb, 256, 0, stream>>>(metric, q, c, iq, target, valid, B, d, zt);
    GHF_LAUNCH_CHECK();
    psweep_saved_kernel<<<qb, 256, 0, stream>>>(valid, dsum, count, grad, B, scale, normalize, zt, w, gt);
    GHF_LAUNCH_CHECK();
    PsBwdArgs a = {};
    a.q = q; a.c = c; a.iq = iq; a.ic = ic; a.rows_q = rows_q; a.Nn = N; a.C = C; a.B = B; a.d = d;
    a.tpos = tpos; a.zt = zt; a.w = w; a.gt = gt; a.filt_ptr = filt_ptr; a.filt_idx = filt_idx; a.nnz = nnz;
    a.scale = scale; a.margin = margin;
    rc = launch_psweep_bwd<true, HINGE>(metric, a, part_q, dq, stream);
    if (rc != GHF_OK) return rc;
    return launch_psweep_bwd<false, HINGE>(metric, a, part_c, dc, stream);
}

}  // namespace ghf

// ---- the C ABI (include/ghf_pairwise_sweep.h) -------------------------------------------------------------------------------
using namespace ghf;

extern "C" {

// the refusals that stand ahead of the sweep's own, in the header's order
#define GHF_PSWEEP_ENTRY(op, ptrs)                                                                                           \
    do {                                                                                                                     \
        GHF_REQUIRE(metric == GHF_DIST_L1 || metric == GHF_DIST_L2 || metric == GHF_DIST_COMPLEX,                            \
                    op ": metric must be GHF_DIST_L1, GHF_DIST_L2 or GHF_DIST_COMPLEX");                                     \
        GHF_REQUIRE(metric != GHF_DIST_COMPLEX || (d & 1) == 0, op ": GHF_DIST_COMPLEX needs an even d (re / im interleaved)"); \
        GHF_REQUIRE(kind == GHF_PAIR_HINGE || kind == GHF_PAIR_LOGISTIC, op ": kind must be GHF_PAIR_HINGE or GHF_PAIR_LOGISTIC"); \
        GHF_REQUIRE(std::isfinite(scale) && scale > 0.f, op ": scale must be finite and positive");                          \
        GHF_REQUIRE(std::isfinite(margin), op ": margin must be finite");                                                    \
        GHF_REQUIRE(normalize == 0 || normalize == 1, op ": normalize must be 0 or 1");                                      \
        GHF_REQUIRE((ptrs) && workspace, op ": null pointer argument");                                                      \
        GHF_REQUIRE(nnz <= 0 || (filt_ptr && filt_idx), op ": null filter list with nnz > 0");                               \
        GHF_REQUIRE(((uintptr_t)workspace & 255) == 0, op ": workspace not 256-byte aligned");                               \
    } while (0)

size_t ghf_dist_pair_fwd_workspace_bytes(int64_t B, int64_t C, int d, int64_t nnz) { return psweep_fwd_workspace_bytes(B, C, d, nnz); }

int ghf_dist_pair_fwd(int metric, int kind, const float* q, const float* c, const int64_t* iq, const int64_t* target,
                      const int64_t* filt_ptr, const int64_t* filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d,
                      float scale, float margin, int normalize, const int64_t* ic, int64_t C, void* workspace,
                      size_t workspace_bytes, float* loss, float* dsum, int32_t* count, int32_t* active, void* stream) {
    GHF_PSWEEP_ENTRY("dist_pair_fwd", q && c && target && loss && dsum && count && active);
    if (kind == GHF_PAIR_HINGE)
        return launch_psweep_fwd<true>(metric, q, c, iq, target, filt_ptr, filt_idx, nnz, rows_q, N, B, d, scale, margin, normalize, ic,
                                       C, workspace, workspace_bytes, loss, dsum, count, active, (hipStream_t)stream);
    return launch_psweep_fwd<false>(metric, q, c, iq, target, filt_ptr, filt_idx, nnz, rows_q, N, B, d, scale, margin, normalize, ic, C,
                                    workspace, workspace_bytes, loss, dsum, count, active, (hipStream_t)stream);
}

size_t ghf_dist_pair_bwd_workspace_bytes(int64_t B, int64_t C, int d, int64_t nnz) { return psweep_bwd_workspace_bytes(B, C, d, nnz); }

int ghf_dist_pair_bwd(int metric, int kind, const float* q, const float* c, const int64_t* iq, const int64_t* target,
                      const int64_t* filt_ptr, const int64_t* filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d,
                      float scale, float margin, int normalize, const int64_t* ic, int64_t C, const float* dsum,
                      const int32_t* count, const float* grad_loss, void* workspace, size_t workspace_bytes, float* dq, float* dc,
                      void* stream) {
    GHF_PSWEEP_ENTRY("dist_pair_bwd", q && c && target && dsum && count && grad_loss && dq && dc);
    if (kind == GHF_PAIR_HINGE)
        return launch_psweep_backward<true>(metric, q, c, iq, target, filt_ptr, filt_idx, nnz, rows_q, N, B, d, scale, margin, normalize,
                                            ic, C, dsum, count, grad_loss, workspace, workspace_bytes, dq, dc, (hipStream_t)stream);
    return launch_psweep_backward<false>(metric, q, c, iq, target, filt_ptr, filt_idx, nnz, rows_q, N, B, d, scale, margin, normalize, ic,
                                         C, dsum, count, grad_loss, workspace, workspace_bytes, dq, dc, (hipStream_t)stream);
}

#undef GHF_PSWEEP_ENTRY

}  // extern "C"
