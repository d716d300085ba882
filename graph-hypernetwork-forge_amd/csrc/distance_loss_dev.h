// distance_loss_dev.h — the ONE text of the shared-set distance losses: what distance_loss.hip (softmax,
// negsamp; §25) and pairwise_sweep.hip (hinge, logistic; §27) share, each a translation unit of its own that instantiates only
// its own kernels, as negatives.hip, distance.hip and pairwise.hip do over negatives_dev.h.
//
//   geometry        the constants, the forward's slabs (from C alone), a backward pass's owner tiles and slabs
//   dl_tile_kernel  <M, VEC, E>: the forward sweep; the front end, the step loop and the masking block once, an
//                   `if constexpr` arm per epilogue E and per end-of-slab merge
//   dl_bwd_kernel   <M, VEC, DQ, K>: one pass of a backward; the owner row, the streamed group, phase 1, phase 2 and the
//                   store once, the per-query state and the coefficient in the policy K (which the unit defines)
//   launches        the two ladders (metric x load path), a pass (slab partials, then launch_ordered_sum), dl_validate,
//                   dl_sweep (validate, targets, tiles) and dl_backward (validate, the unit's saved kernels, two passes)
//
// Each unit keeps its extern "C" functions, its argument structs (their layouts are the kernels' kernarg offsets), its finish
// and saved kernels, its workspace layouts and its own open check: the two refuse in different orders (the public headers).
#pragma once
#include "common.h"
#include "rank_sweep.h"
#include "distance_sweep_dev.h"
#include "../../include/ghf_pairwise.h"

#include <type_traits>

namespace ghf {

// The epilogue of a forward sweep.  NOTHING below the extern "C" functions takes a public `mode` or `kind` (§23's trap: two
// public constant sets share their numbers): each set is translated here, once, the entry points alone call the
// translations, and a value outside its set never gets this far (the entry point refuses it by its own message).
enum class DlEpi { Softmax, Negsamp, Hinge, Logistic };
constexpr DlEpi dl_of_dist_mode(int mode) { return mode == GHF_DIST_NEGSAMP ? DlEpi::Negsamp : DlEpi::Softmax; }
constexpr DlEpi dl_of_pair_kind(int kind) { return kind == GHF_PAIR_HINGE ? DlEpi::Hinge : DlEpi::Logistic; }
static_assert(dl_of_dist_mode(GHF_DIST_SOFTMAX) == DlEpi::Softmax && dl_of_dist_mode(GHF_DIST_NEGSAMP) == DlEpi::Negsamp, "ghf_distance.h");
static_assert(dl_of_pair_kind(GHF_PAIR_HINGE) == DlEpi::Hinge && dl_of_pair_kind(GHF_PAIR_LOGISTIC) == DlEpi::Logistic, "ghf_pairwise.h");
constexpr bool dl_is_pair(DlEpi e) { return e == DlEpi::Hinge || e == DlEpi::Logistic; }

// ---- geometry ---------------------------------------------------------------------------------------------------------------
constexpr int DL_SLABS = 128;                // candidate slabs of the forward, at the most: from C alone
constexpr int DL_RS = 4;                     // streamed rows per group of the backward
constexpr int DL_OT = 64;                    // owner rows per workgroup of the backward (one wave)
constexpr int DL_ACC = 128;                  // accumulators a lane (columns per half)
constexpr int DL_ST = 256;                   // streamed rows per slab, at the least
constexpr int DL_BWD_WGS = 1024;             // workgroups a backward pass aims at

struct DlGeom { int64_t qtiles, ctiles, slab_tiles, slabs; };

static inline bool dloss_geom(int64_t B, int64_t C, DlGeom* g) {
    if (B <= 0 || C <= 0 || C >= (int64_t)1 << 31 || B >= (int64_t)1 << 31) return false;
    g->qtiles = cdiv(B, DS_TQ);
    g->ctiles = cdiv(C, DS_CT);
    g->slab_tiles = cdiv(g->ctiles, DL_SLABS);
    g->slabs = cdiv(g->ctiles, g->slab_tiles);
    return g->qtiles * g->slabs < (int64_t)1 << 31;
}

// a backward pass over nO owner rows and nS streamed rows
struct DlBwdGeom { int64_t otiles, slab_rows, slabs; };

static inline void dloss_bwd_geom(int64_t nO, int64_t nS, DlBwdGeom* g) {
    g->otiles = cdiv(nO, DL_OT);
    const int64_t st = cdiv(nS, DL_ST);
    int64_t slabs = cdiv(DL_BWD_WGS, g->otiles);
    if (slabs > st) slabs = st;
    if (slabs < 1) slabs = 1;
    const int64_t slab_tiles = cdiv(st, slabs);
    g->slabs = cdiv(st, slab_tiles);
    g->slab_rows = slab_tiles * DL_ST;
}

static inline size_t dloss_bwd_part_bytes(int64_t nO, int64_t nS, int d) {
    DlBwdGeom g;
    dloss_bwd_geom(nO, nS, &g);
    return g.slabs > 1 ? rk_align((size_t)g.slabs * (size_t)nO * (size_t)d * 4) : 0;
}

// ---- the forward sweep ------------------------------------------------------------------------------------------------------
// The argument block of an epilogue's sweep: the unit's own struct.  Every block names q, c, iq, ic, rows_q, Nn, C, B, d,
// qtiles, slab_tiles, slabs, tpos, valid, filt_ptr, filt_idx, nnz, scale, margin and part; DlossArgs adds alpha, PsweepArgs t.
struct DlossArgs;                            // distance_loss.hip
struct PsweepArgs;                           // pairwise_sweep.hip
template <DlEpi E>
using DlTileArgs = std::conditional_t<dl_is_pair(E), PsweepArgs, DlossArgs>;

// one (sum phi, sum phi', n, active) per (query, slab) of a pairwise sweep; the set losses write a NegTriple's three floats
struct __attribute__((aligned(16))) PsPart { float f, g; int n, a; };

// sigmoid(u), as negatives_dev.h's pairwise arm forms it
__device__ __forceinline__ float psweep_sigmoid(float u) {
#pragma clang fp contract(off)
    const float e = __expf(-fabsf(u)), rcp = __builtin_amdgcn_rcpf(1.f + e);
    return u >= 0.f ? rcp : e * rcp;
}

template <int M, bool VEC, DlEpi E>
__global__ __launch_bounds__(256) void dl_tile_kernel(const DlTileArgs<E> a) {
#pragma clang fp contract(off)
    constexpr bool PAIR = dl_is_pair(E);
    constexpr bool EXCL = E != DlEpi::Softmax;               // the target is no term of the sum (softmax: exempt from the lists)
    __shared__ __attribute__((aligned(16))) float Cs[2 * DS_CT * DS_LDC];
    __shared__ int64_t tposS[DS_TQ], nxtS[DS_TQ], curS[DS_TQ], endS[DS_TQ];
    __shared__ float ztS[DS_TQ];                             // pairwise alone: an instance that never names it holds no LDS for it
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
    // per query of the tile: its target's position (pairwise: and z, known before the tiles start) and the cursor into its
    // list, which starts at the slab's first position
    if (tid < DS_TQ) {
        const int64_t qi = qt * DS_TQ + tid;
        int64_t tp = -1, cur = 0, end = 0, nxt = INT64_MAX;
        [[maybe_unused]] float zt = 0.f;
        if (qi < a.B) {
            if (a.valid[qi]) tp = a.tpos[qi];
            if constexpr (PAIR) zt = a.scale * a.t[qi];
            if (a.filt_ptr) {
                int64_t lo = a.filt_ptr[qi], hi = a.filt_ptr[qi + 1];
                lo = lo < 0 ? 0 : (lo > a.nnz ? a.nnz : lo);
                hi = hi < lo ? lo : (hi > a.nnz ? a.nnz : hi);
                cur = filter_lower_bound(a.filt_idx, lo, hi, tile0 * DS_CT);
                end = hi;
                if (cur < hi) nxt = a.filt_idx[cur];
            }
        }
        tposS[tid] = tp; curS[tid] = cur; endS[tid] = end; nxtS[tid] = nxt;
        if constexpr (PAIR) ztS[tid] = zt;
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
    [[maybe_unused]] float rm[DS_RQ], rs[DS_RQ], rt[DS_RQ];  // the set losses: the lane's online triple per query
    [[maybe_unused]] float rf[DS_RQ], rg[DS_RQ];             // pairwise: the lane's sums of phi and of phi' per query
    [[maybe_unused]] int rn[DS_RQ], ra[DS_RQ];               //           its pairs of J_i and those with u > 0
#pragma unroll
    for (int rq = 0; rq < DS_RQ; ++rq) {
        if constexpr (PAIR) {
            rf[rq] = 0.f;
            rg[rq] = 0.f;
            rn[rq] = 0;
            ra[rq] = 0;
        } else {
            rm[rq] = -INFINITY;
            rs[rq] = 0.f;
            rt[rq] = 0.f;
        }
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
                [[maybe_unused]] float zt;
                if constexpr (PAIR) zt = ztS[qcol];
                float z[DS_RC];
                bool out[DS_RC];
#pragma unroll
                for (int rc = 0; rc < DS_RC; ++rc) {
                    z[rc] = a.scale * -dist_finish<M>(acc[rq][rc]);
                    out[rc] = false;
                    acc[rq][rc] = 0.f;
                }
                const bool tin = EXCL && tp >= tile_lo && tp < tile_end;    // matters only where the target is excluded
                if (!(full && nxt >= tile_end && !tin)) {       // the same answer in every lane of the wave
                    const bool look = nxt < tile_end;
                    const int64_t f0 = curS[qcol], f1 = endS[qcol];
#pragma unroll
                    for (int rc = 0; rc < DS_RC; ++rc) {
                        const int64_t cand = base + 64 * rc;
                        bool o = cand >= a.C || (EXCL && cand == tp);
                        if (look && !o && (EXCL || cand != tp)) o = in_filter(a.filt_idx, f0, f1, cand);
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
                if constexpr (E == DlEpi::Softmax) {
                    float mx = rm[rq];
#pragma unroll
                    for (int rc = 0; rc < DS_RC; ++rc) mx = out[rc] ? mx : fmaxf(mx, z[rc]);
                    if (mx > -INFINITY) {
                        float s = rs[rq] * __expf(rm[rq] - mx);
#pragma unroll
                        for (int rc = 0; rc < DS_RC; ++rc) s += out[rc] ? 0.f : __expf(z[rc] - mx);
                        rs[rq] = s;
                        rm[rq] = mx;
                    }
                } else if constexpr (E == DlEpi::Negsamp) {
                    float mx = rm[rq];
#pragma unroll
                    for (int rc = 0; rc < DS_RC; ++rc) mx = out[rc] ? mx : fmaxf(mx, a.alpha * z[rc]);
                    if (mx > -INFINITY) {
                        const float r = __expf(rm[rq] - mx);
                        float s = rs[rq] * r, t = rt[rq] * r;
#pragma unroll
                        for (int rc = 0; rc < DS_RC; ++rc) {
                            const float w = __expf(fmaf(a.alpha, z[rc], -mx));
                            const float nt = fmaf(w, softplus(z[rc] + a.margin), t);
                            s += out[rc] ? 0.f : w;
                            t = out[rc] ? t : nt;
                        }
                        rs[rq] = s;
                        rt[rq] = t;
                        rm[rq] = mx;
                    }
                } else {
                    // The pairs of the tile, rc ascending, each added without a branch: a pair outside J_i adds +0.f and 0.  The
                    // one branch around a query's four pairs skips nothing that counts (all four outside J_i: four times +0.f, and
                    // the sums are never -0.f) and is there for the compiler.  Nothing else orders the sixteen epilogues of a tile,
                    // and scheduled side by side their temporaries take 290 to 305 registers: one wave per SIMD.  Behind a branch
                    // a lane they run one query at a time, as negsamp's do behind its test of the maximum.
                    constexpr bool HINGE = E == DlEpi::Hinge;
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
        if constexpr (PAIR) {
            float f = rf[rq], g = rg[rq];
            int n = rn[rq], ac = ra[rq];
#pragma unroll
            for (int w = 1; w < 64; w *= 2) {
                f += __shfl_xor(f, w, 64);
                if constexpr (E != DlEpi::Hinge) g += __shfl_xor(g, w, 64);
                n += __shfl_xor(n, w, 64);
                ac += __shfl_xor(ac, w, 64);
            }
            if (lane == 0 && q0 + rq < a.B) a.part[(size_t)(q0 + rq) * a.slabs + slab] = PsPart{f, g, n, ac};
        } else {
            NegTriple p = {rm[rq], rs[rq], rt[rq]};
#pragma unroll
            for (int w = 1; w < 64; w *= 2) {
                const NegTriple o = {__shfl_xor(p.m, w, 64), __shfl_xor(p.s, w, 64), __shfl_xor(p.t, w, 64)};
                p = neg_merge(p, o);
            }
            if (lane == 0 && q0 + rq < a.B) {
                float* w = a.part + ((size_t)(q0 + rq) * a.slabs + slab) * 3;
                w[0] = p.m;
                w[1] = p.s;
                w[2] = p.t;
            }
        }
    }
}

// ---- the backward -----------------------------------------------------------------------------------------------------------
// One pass, dl_bwd_kernel<M, VEC, DQ, K>.  Lane l of a one-wave workgroup OWNS a row (DQ: query l of the tile; otherwise
// candidate l) in its own LDS row; the other side is STREAMED, four wave-uniform rows at a time through scalar loads, in
// ascending order.  The coefficient policy K is the unit's and has static functions over floats only (the form that keeps
// hipcc's instruction streams, §23; what a query carries as a struct returned by value did not, §29):
//   K::Args                                  the pass's argument block: q, c, iq, ic, rows_q, Nn, C, B, d, tpos, filt_ptr,
//                                            filt_idx, nnz, scale, otiles, slab_rows, slabs, out, and what K reads
//   K::carry<S>(a, i), S = 0, 1, 2           what query i carries into a pair, three floats at the most, loaded alike for an
//                                            owner lane and for a streamed row.  carry<0> is the key: its NaN means "the query
//                                            takes no part".  A slot the policy does not use returns 0.f and costs nothing
//   K::G(a, z, c0, c1, c2, is_target, listed)  d loss / d s of the pair, from the three carried floats
//   K::inputs(a)                             host: are the per-query inputs of the block there
template <int M, bool VEC, bool DQ, class K>
__global__ __launch_bounds__(64) void dl_bwd_kernel(const typename K::Args a) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) float Os[];
    const int lane = threadIdx.x;
    const int d = a.d, dpad = (d + 3) & ~3;
    const int ldo = (d <= DL_ACC ? DL_ACC : 2 * DL_ACC) + 4;
    const int64_t ot = blockIdx.x % a.otiles, slab = blockIdx.x / a.otiles;
    const int kb = blockIdx.y * DL_ACC;                      // the first column of this half
    const int64_t nO = DQ ? a.B : a.C, nS = DQ ? a.C : a.B;
    const int64_t o = ot * DL_OT + lane;                     // the lane's owner row (a query, or a candidate position)

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
    float o_c0 = __int_as_float(0x7FC00000), o_c1 = 0.f, o_c2 = 0.f;
    int64_t o_tp = -1, cur = 0, end = 0, nxt = INT64_MAX;
    bool o_live = orow >= 0;
    const int64_t s0 = slab * a.slab_rows;
    const int64_t s1 = s0 + a.slab_rows < nS ? s0 + a.slab_rows : nS;
    if (DQ && o < nO) {
        o_c0 = K::template carry<0>(a, o);
        o_c1 = K::template carry<1>(a, o);
        o_c2 = K::template carry<2>(a, o);
        o_tp = a.tpos[o];
        o_live = o_live && o_c0 == o_c0;
        if (a.filt_ptr) {                                    // the lane's cursor: candidates arrive in ascending position
            int64_t lo = a.filt_ptr[o], hi = a.filt_ptr[o + 1];
            lo = lo < 0 ? 0 : (lo > a.nnz ? a.nnz : lo);
            hi = hi < lo ? lo : (hi > a.nnz ? a.nnz : hi);
            cur = filter_lower_bound(a.filt_idx, lo, hi, s0);
            end = hi;
            if (cur < hi) nxt = a.filt_idx[cur];
        }
    }

    float out[DL_ACC];
#pragma unroll
    for (int k = 0; k < DL_ACC; ++k) out[k] = 0.f;

    ds_cfloat* sc = (ds_cfloat*)(DQ ? a.c : a.q);
    for (int64_t sg = s0; sg < s1; sg += DL_RS) {
        // the group's rows: wave-uniform row numbers (an absent row reads row 0 and its pairs count with G = 0)
        int srow[DL_RS];
        bool s_ok[DL_RS];
        float s_c0[DL_RS], s_c1[DL_RS], s_c2[DL_RS];
        int64_t s_tp[DL_RS], s_lo[DL_RS], s_hi[DL_RS];
#pragma unroll
        for (int u = 0; u < DL_RS; ++u) {
            const int64_t sj = sg + u;
            bool ok = sj < s1;
            int64_t r = 0;
            s_c0[u] = 0.f; s_c1[u] = 0.f; s_c2[u] = 0.f; s_tp[u] = -1; s_lo[u] = 0; s_hi[u] = 0;
            if (ok) {
                if (DQ) {
                    r = a.ic ? a.ic[sj] : sj;
                    ok = (uint64_t)r < (uint64_t)a.Nn;
                } else {
                    r = a.iq ? a.iq[sj] : sj;
                    ok = (uint64_t)r < (uint64_t)a.rows_q;
                    const float v = K::template carry<0>(a, sj);
                    ok = ok && v == v;
                    s_c0[u] = v;
                    s_c1[u] = K::template carry<1>(a, sj);
                    s_c2[u] = K::template carry<2>(a, sj);
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
        float D[DL_RS];
#pragma unroll
        for (int u = 0; u < DL_RS; ++u) D[u] = 0.f;
#pragma unroll 1
        for (int k = 0; k < dpad; k += 4) {
            const f32x4 ov = *(const f32x4*)(mine + k);
#pragma unroll
            for (int u = 0; u < DL_RS; ++u) {
                const f32x4 sv4 = streamed(u, k);
                D[u] = DQ ? dist_step4<M>(D[u], ov, sv4) : dist_step4<M>(D[u], sv4, ov);
            }
        }
        // the pairs' coefficients: + G g for a candidate's row, - G g for a query's
        float cf[DL_RS], rD[DL_RS];
        bool any = false;
#pragma unroll
        for (int u = 0; u < DL_RS; ++u) {
            D[u] = dist_finish<M>(D[u]);
            const float z = a.scale * -D[u];
            float G;
            if (DQ) {
                const int64_t j = sg + u;
                G = K::G(a, z, o_c0, o_c1, o_c2, j == o_tp, nxt == j);
                if (nxt <= j) {
                    do {
                        ++cur;
                        nxt = cur < end ? a.filt_idx[cur] : INT64_MAX;
                    } while (nxt <= j);
                }
            } else {
                bool listed = false;
                if (s_hi[u] > s_lo[u]) {                     // wave-uniform: does the tile's range hold a listed position at all
                    const int64_t lb = filter_lower_bound(a.filt_idx, s_lo[u], s_hi[u], ot * DL_OT);
                    if (lb < s_hi[u] && a.filt_idx[lb] < ot * DL_OT + DL_OT) listed = in_filter(a.filt_idx, lb, s_hi[u], o);
                }
                G = K::G(a, z, s_c0[u], s_c1[u], s_c2[u], o == s_tp[u], listed);
            }
            G = o_live && s_ok[u] ? G : 0.f;
            any |= G != 0.f;
            cf[u] = DQ ? -G : G;
            rD[u] = D[u] > 0.f ? __builtin_amdgcn_rcpf(D[u]) : 0.f;
        }
        if (__ballot(any) == 0) continue;                    // the whole wave

        // phase 2: out[k] += G g_k over this half's columns, statically indexed
#pragma unroll
        for (int k4 = 0; k4 < DL_ACC / 4; ++k4) {
            const int k = kb + 4 * k4;
            if (k < dpad) {
                const f32x4 ov = *(const f32x4*)(mine + k);
#pragma unroll
                for (int u = 0; u < DL_RS; ++u) {
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
        for (int k4 = 0; k4 < DL_ACC / 4; ++k4) {
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
// valid [B], and the targets and lists in position space (with ic: through the id map at `map_ws`)
static int dl_validate(const float* q, const float* c, const int64_t* iq, const int64_t* target, const int64_t** filt_ptr,
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

// what a forward's finish kernel writes: loss and aux (lse, lw) for the set losses; loss, dsum, count and active for pairwise
struct DlOut { float* loss; float* aux; float* dsum; int* count; int* active; };

// A forward up to its finish kernel: validation, the targets' scores into `t`, the tiles into a.part.  `a` comes with
// everything but tpos and valid, and with the caller's lists (validation puts targets and lists into position space).  Before the first launch an
// argument block whose outputs for its epilogue are null is refused: a wrong dispatch ends as a message, not a memory fault.
template <DlEpi E>
static int dl_sweep(const char* op, int metric, DlTileArgs<E> a, const int64_t* target, int* valid, float* t, void* map_ws,
                    size_t map_bytes, const DlOut& out, hipStream_t stream) {
    GHF_REQUIRE(a.part && valid && t && out.loss && (dl_is_pair(E) ? out.dsum && out.count && out.active : out.aux != nullptr),
                "%s: null output for its epilogue", op);
    int rc = dl_validate(a.q, a.c, a.iq, target, &a.filt_ptr, &a.filt_idx, a.nnz, a.rows_q, a.Nn, a.B, a.d, a.ic, a.C, valid, map_ws,
                         map_bytes, &a.tpos, stream);
    if (rc != GHF_OK) return rc;
    a.valid = valid;
    dist_target_kernel<<<(unsigned)cdiv(a.B, 256), 256, 0, stream>>>(metric, a.q, a.c, a.iq, target, valid, a.B, a.d, t);
    GHF_LAUNCH_CHECK();
    const unsigned grid = (unsigned)(a.qtiles * a.slabs);
    const bool vec = (a.d & 3) == 0 && ((uintptr_t)a.q & 15) == 0;
#define GHF_DL_LAUNCH(MM)                                                          \
    do {                                                                           \
        if (vec) dl_tile_kernel<MM, true, E><<<grid, 256, 0, stream>>>(a);         \
        else dl_tile_kernel<MM, false, E><<<grid, 256, 0, stream>>>(a);            \
    } while (0)
    if (metric == GHF_DIST_L1) GHF_DL_LAUNCH(GHF_DIST_L1);
    else if (metric == GHF_DIST_L2) GHF_DL_LAUNCH(GHF_DIST_L2);
    else GHF_DL_LAUNCH(GHF_DIST_COMPLEX);
#undef GHF_DL_LAUNCH
    GHF_LAUNCH_CHECK();
    return GHF_OK;
}

template <int M, bool DQ, class K>
static int dl_launch_bwd_pass(const typename K::Args& a, hipStream_t stream) {
    const float* streamed = DQ ? a.c : a.q;
    const bool vec = (a.d & 3) == 0 && ((uintptr_t)streamed & 15) == 0;
    const size_t lds = (size_t)DL_OT * ((a.d <= DL_ACC ? DL_ACC : 2 * DL_ACC) + 4) * 4;
    const dim3 grid((unsigned)(a.otiles * a.slabs), a.d <= DL_ACC ? 1u : 2u);
    if (vec) {
        GHF_SET_MAX_LDS((dl_bwd_kernel<M, true, DQ, K>), lds);
        dl_bwd_kernel<M, true, DQ, K><<<grid, 64, lds, stream>>>(a);
    } else {
        GHF_SET_MAX_LDS((dl_bwd_kernel<M, false, DQ, K>), lds);
        dl_bwd_kernel<M, false, DQ, K><<<grid, 64, lds, stream>>>(a);
    }
    GHF_LAUNCH_CHECK();
    return GHF_OK;
}

// one pass: the slabs' partials into `part` and their ordered sum into `result`, or straight into `result` with one slab
template <bool DQ, class K>
static int dl_launch_bwd(const char* op, int metric, typename K::Args a, float* part, float* result, hipStream_t stream) {
    const int64_t nO = DQ ? a.B : a.C, nS = DQ ? a.C : a.B;
    DlBwdGeom g;
    dloss_bwd_geom(nO, nS, &g);
    GHF_REQUIRE(g.otiles * g.slabs < (int64_t)1 << 31, "%s: B or C out of range", op);
    a.otiles = g.otiles; a.slab_rows = g.slab_rows; a.slabs = g.slabs;
    a.out = g.slabs > 1 ? part : result;
    int rc;
    if (metric == GHF_DIST_L1) rc = dl_launch_bwd_pass<GHF_DIST_L1, DQ, K>(a, stream);
    else if (metric == GHF_DIST_L2) rc = dl_launch_bwd_pass<GHF_DIST_L2, DQ, K>(a, stream);
    else rc = dl_launch_bwd_pass<GHF_DIST_COMPLEX, DQ, K>(a, stream);
    if (rc != GHF_OK || g.slabs == 1) return rc;
    return launch_ordered_sum(part, g.slabs, nO * (int64_t)a.d, result, stream);
}

// A backward: validation, the unit's kernels that form what a query carries (`saved()`, behind the validation because they
// read `valid`), then the pass that owns the queries and the pass that owns the candidates.  Refuses, before the first
// launch, a block without its results or its per-query inputs.
template <class K, class Saved>
static int dl_backward(const char* op, int metric, typename K::Args a, const int64_t* target, int* valid, void* map_ws,
                       size_t map_bytes, float* part_q, float* part_c, float* dq, float* dc, Saved saved, hipStream_t stream) {
    GHF_REQUIRE(dq && dc && valid && K::inputs(a), "%s: null result or saved input", op);
    int rc = dl_validate(a.q, a.c, a.iq, target, &a.filt_ptr, &a.filt_idx, a.nnz, a.rows_q, a.Nn, a.B, a.d, a.ic, a.C, valid, map_ws,
                         map_bytes, &a.tpos, stream);
    if (rc != GHF_OK) return rc;
    rc = saved();
    if (rc != GHF_OK) return rc;
    rc = dl_launch_bwd<true, K>(op, metric, a, part_q, dq, stream);
    if (rc != GHF_OK) return rc;
    return dl_launch_bwd<false, K>(op, metric, a, part_c, dc, stream);
}

}  // namespace ghf
