// distance_loss.hip — the softmax and the negative-sampling loss under a DISTANCE score against every node or a shared candidate
// subset, forward and backward, the B x C distances never stored (include/ghf_distance_loss.h).
//
// Forward: distance_sweep.hip's tile loop (the lane owns 4 candidates, the wave owns 16 queries, candidate rows through two LDS
//   buffers, query rows through scalar loads; distance_sweep_dev.h's chain) with a loss epilogue.  Once per finished tile the
//   lane's four z = -scale D of a query fold into the lane's online (max, S) — softmax — or (max of alpha z, S, T) —
//   negsamp, rank_sweep.h's RK_NEGSAMP triple.  The lists are in position space and sorted and tiles arrive in ascending
//   position: a per-query cursor in LDS says "this tile's range holds no listed position", and such a tile touches no memory;
//   only the others call in_filter.  A listed candidate is masked before it enters a sum.  At the slab's end the lanes'
//   partials merge across the wave by a fixed butterfly and lane 0 writes one triple per (query, slab); dloss_finish_kernel
//   merges the slabs in slab order and forms loss and lse / lw from z_it, which dloss_target_kernel formed by the tile's chain.
//   The slabs depend on C alone (dloss_geom), so a query's bits do not depend on its batch.
//
// Backward: ONE kernel text for two passes, dloss_bwd_kernel<M, VEC, DQ>.  Lane l of a one-wave workgroup OWNS a row (DQ: query
//   l of the tile; otherwise candidate l), kept in its own LDS row (stride 132 or 260 floats: the lanes of a ds_read_b128 step 4
//   banks); the other side is STREAMED, four wave-uniform rows at a time through scalar loads, in ascending order.  Per group:
//   phase 1 runs the full-d chain to D, z and G of the lane's four pairs; phase 2 walks k again and adds G g_k into 128
//   statically indexed accumulators.  d > 128 runs as two column halves (blockIdx.y), phase 1 paid twice.  A workgroup owns
//   (owner tile, slab of the streamed side) and writes one partial; launch_ordered_sum adds the slabs in slab order.  No
//   floating-point atomics anywhere.
//   The public `mode` of ghf_dist_loss_bwd becomes the boolean DlBwdArgs::negsamp on the host and nothing else: it shares no
//   argument and no template parameter with a kernel selector (DESIGN.md §23's trap).
#include "common.h"
#include "rank_sweep.h"
#include "distance_sweep_dev.h"
#include "../../include/ghf_distance_loss.h"

#include <cmath>

namespace ghf {

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

static size_t dloss_fwd_workspace_bytes(int64_t B, int64_t C, int d, int64_t nnz) {
    DlGeom g;
    if (d <= 0 || d > RK_MAX_D || nnz < 0 || !dloss_geom(B, C, &g)) return 0;
    const size_t map = cand_workspace_bytes(B, nnz);
    if (!map) return 0;
    // t [B] float, valid [B] int32, (max, S, T) [B, slabs], the id map's
    return 2 * rk_align((size_t)B * 4) + rk_align((size_t)B * (size_t)g.slabs * 12) + map;
}

static size_t dloss_bwd_part_bytes(int64_t nO, int64_t nS, int d) {
    DlBwdGeom g;
    dloss_bwd_geom(nO, nS, &g);
    return g.slabs > 1 ? rk_align((size_t)g.slabs * (size_t)nO * (size_t)d * 4) : 0;
}

static size_t dloss_bwd_workspace_bytes(int64_t B, int64_t C, int d, int64_t nnz) {
    DlGeom g;
    if (d <= 0 || d > RK_MAX_D || nnz < 0 || !dloss_geom(B, C, &g)) return 0;
    const size_t map = cand_workspace_bytes(B, nnz);
    if (!map) return 0;
    // sv [B] float, valid [B] int32, the slabs' partials of dq and of dc, the id map's
    return 2 * rk_align((size_t)B * 4) + dloss_bwd_part_bytes(B, C, d) + dloss_bwd_part_bytes(C, B, d) + map;
}

// ---- the forward sweep ------------------------------------------------------------------------------------------------------
struct DlossArgs {
    const float* q; const float* c; const int64_t* iq; const int64_t* ic;
    int64_t rows_q, Nn, C, B;                // Nn rows of c; C candidates (the sweep's positions 0 .. C - 1)
    int d;
    int64_t qtiles, slab_tiles, slabs;
    const int64_t* tpos; const int* valid;   // the targets as positions; a query that is not valid has no target here
    const int64_t* filt_ptr; const int64_t* filt_idx; int64_t nnz;      // lists in position space
    float scale, margin, alpha;
    float* part;                             // (max, S, T) [B, slabs]
};

template <int M, bool VEC, bool NEGSAMP>
__global__ __launch_bounds__(256) void dloss_tile_kernel(const DlossArgs a) {
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(16))) float Cs[2 * DS_CT * DS_LDC];
    __shared__ int64_t tposS[DS_TQ], nxtS[DS_TQ], curS[DS_TQ], endS[DS_TQ];
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
    // per query of the tile: its target's position and the cursor into its list, which starts at the slab's first position
    if (tid < DS_TQ) {
        const int64_t qi = qt * DS_TQ + tid;
        int64_t tp = -1, cur = 0, end = 0, nxt = INT64_MAX;
        if (qi < a.B) {
            if (a.valid[qi]) tp = a.tpos[qi];
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
    float rm[DS_RQ], rs[DS_RQ], rt[DS_RQ];                   // the lane's online triple per query
#pragma unroll
    for (int rq = 0; rq < DS_RQ; ++rq) {
        rm[rq] = -INFINITY;
        rs[rq] = 0.f;
        rt[rq] = 0.f;
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
                float z[DS_RC];
                bool out[DS_RC];
#pragma unroll
                for (int rc = 0; rc < DS_RC; ++rc) {
                    z[rc] = a.scale * -dist_finish<M>(acc[rq][rc]);
                    out[rc] = false;
                    acc[rq][rc] = 0.f;
                }
                const bool tin = NEGSAMP && tp >= tile_lo && tp < tile_end;
                if (!(full && nxt >= tile_end && !tin)) {       // the same answer in every lane of the wave
                    const bool look = nxt < tile_end;
                    const int64_t f0 = curS[qcol], f1 = endS[qcol];
#pragma unroll
                    for (int rc = 0; rc < DS_RC; ++rc) {
                        const int64_t cand = base + 64 * rc;
                        bool o = cand >= a.C || (NEGSAMP && cand == tp);
                        if (look && !o && cand != tp) o = in_filter(a.filt_idx, f0, f1, cand);
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
                if constexpr (!NEGSAMP) {
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
                } else {
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
                }
            }
        }

        if (more) stash(buf ^ 1);
        __syncthreads();
        tile = ntile;
        kc = nkc;
        buf ^= 1;
    }

    // the lanes' partials of a query, merged by a fixed butterfly; lane 0 writes the slab's triple
#pragma unroll
    for (int rq = 0; rq < DS_RQ; ++rq) {
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

// ---- the small kernels around the sweeps ------------------------------------------------------------------------------------
// one thread per query, behind the pass that validated the ids: the target's score by the tile's chain, from its own row of c
// (node id); NaN for a query that is not valid
__global__ __launch_bounds__(256) void dloss_target_kernel(int metric, const float* __restrict__ q, const float* __restrict__ c,
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

// one thread per query: the slabs' triples in slab order, then the loss from z_it
__global__ __launch_bounds__(256) void dloss_finish_kernel(const float* __restrict__ part, const float* __restrict__ t,
                                                           const int* __restrict__ valid, int64_t B, int64_t slabs, float scale,
                                                           float margin, int negsamp, float* __restrict__ loss,
                                                           float* __restrict__ aux) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= B) return;
    const float* p = part + (size_t)i * slabs * 3;
    NegTriple m = {p[0], p[1], p[2]};
    for (int64_t s = 1; s < slabs; ++s) m = neg_merge(m, NegTriple{p[3 * s], p[3 * s + 1], p[3 * s + 2]});
    float l = __int_as_float(0x7FC00000), w = l;
    if (valid[i]) {
        const float zt = scale * t[i];
        if (negsamp) {
            const bool any = m.s > 0.f;                  // no negatives: the positive term alone, lw = -inf
            w = any ? m.m + logf(m.s) : -INFINITY;
            l = softplus(-(zt + margin)) + (any ? m.t / m.s : 0.f);
        } else {
            w = m.m + logf(m.s);                         // the target is in the sum: the tile that holds it put it there
            l = w - zt;
        }
    }
    loss[i] = l;
    aux[i] = w;
}

// one thread per query: what the backward reads in place of lse_or_lw — NaN for a query that is not valid
__global__ __launch_bounds__(256) void dloss_saved_kernel(const float* __restrict__ saved, const int* __restrict__ valid, int64_t B,
                                                          float* __restrict__ sv) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= B) return;
    sv[i] = valid[i] ? saved[i] : __int_as_float(0x7FC00000);
}

// ---- the backward -----------------------------------------------------------------------------------------------------------
struct DlBwdArgs {
    const float* q; const float* c; const int64_t* iq; const int64_t* ic;
    int64_t rows_q, Nn, C, B;
    int d;
    const int64_t* tpos; const float* sv; const float* grad;            // sv: NaN = the query takes no part
    const int64_t* filt_ptr; const int64_t* filt_idx; int64_t nnz;      // lists in position space
    float scale, margin, alpha;
    int negsamp;                                                        // which loss: set by the host from the public mode
    int64_t otiles, slab_rows, slabs;
    float* out;                                                         // [slabs, owners, d]
};

// G of one pair: d loss / d s, ghf_neg_bwd's per loss.  sv = lse (softmax) or lw (negsamp)
__device__ __forceinline__ float dloss_coef(bool negsamp, float z, float sv, float gs, float margin, float alpha, bool is_target,
                                            bool listed) {
#pragma clang fp contract(off)
    if (!negsamp) {
        const float e = __expf(z - sv);
        return is_target ? gs * (e - 1.f) : (listed ? 0.f : gs * e);
    }
    const float y = z + margin;
    const float e = __expf(-fabsf(y)), rcp = __builtin_amdgcn_rcpf(1.f + e);
    if (is_target) return -gs * (y >= 0.f ? e * rcp : rcp);
    const float w = sv > -INFINITY ? __expf(fmaf(alpha, z, -sv)) : 0.f;
    return listed ? 0.f : gs * (w * (y >= 0.f ? rcp : e * rcp));
}

template <int M, bool VEC, bool DQ>
__global__ __launch_bounds__(64) void dloss_bwd_kernel(const DlBwdArgs a) {
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
    float o_sv = __int_as_float(0x7FC00000), o_gs = 0.f;
    int64_t o_tp = -1, cur = 0, end = 0, nxt = INT64_MAX;
    bool o_live = orow >= 0;
    const int64_t s0 = slab * a.slab_rows;
    const int64_t s1 = s0 + a.slab_rows < nS ? s0 + a.slab_rows : nS;
    if (DQ && o < nO) {
        o_sv = a.sv[o];
        o_gs = a.grad[o] * a.scale;
        o_tp = a.tpos[o];
        o_live = o_live && o_sv == o_sv;
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
        float s_sv[DL_RS], s_gs[DL_RS];
        int64_t s_tp[DL_RS], s_lo[DL_RS], s_hi[DL_RS];
#pragma unroll
        for (int u = 0; u < DL_RS; ++u) {
            const int64_t sj = sg + u;
            bool ok = sj < s1;
            int64_t r = 0;
            s_sv[u] = 0.f; s_gs[u] = 0.f; s_tp[u] = -1; s_lo[u] = 0; s_hi[u] = 0;
            if (ok) {
                if (DQ) {
                    r = a.ic ? a.ic[sj] : sj;
                    ok = (uint64_t)r < (uint64_t)a.Nn;
                } else {
                    r = a.iq ? a.iq[sj] : sj;
                    ok = (uint64_t)r < (uint64_t)a.rows_q;
                    const float v = a.sv[sj];
                    ok = ok && v == v;
                    s_sv[u] = v;
                    s_gs[u] = a.grad[sj] * a.scale;
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
                G = dloss_coef(a.negsamp != 0, z, o_sv, o_gs, a.margin, a.alpha, j == o_tp, nxt == j);
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
                G = dloss_coef(a.negsamp != 0, z, s_sv[u], s_gs[u], a.margin, a.alpha, o == s_tp[u], listed);
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
template <bool NEGSAMP>
static int launch_dloss_tiles(int metric, const DlossArgs& a, hipStream_t stream) {
    const unsigned grid = (unsigned)(a.qtiles * a.slabs);
    const bool vec = (a.d & 3) == 0 && ((uintptr_t)a.q & 15) == 0;
#define GHF_DLOSS_LAUNCH(MM)                                                                \
    do {                                                                                    \
        if (vec) dloss_tile_kernel<MM, true, NEGSAMP><<<grid, 256, 0, stream>>>(a);         \
        else dloss_tile_kernel<MM, false, NEGSAMP><<<grid, 256, 0, stream>>>(a);            \
    } while (0)
    if (metric == GHF_DIST_L1) GHF_DLOSS_LAUNCH(GHF_DIST_L1);
    else if (metric == GHF_DIST_L2) GHF_DLOSS_LAUNCH(GHF_DIST_L2);
    else GHF_DLOSS_LAUNCH(GHF_DIST_COMPLEX);
#undef GHF_DLOSS_LAUNCH
    GHF_LAUNCH_CHECK();
    return GHF_OK;
}

template <int M, bool DQ>
static int launch_dloss_bwd_pass(const DlBwdArgs& a, hipStream_t stream) {
    const float* streamed = DQ ? a.c : a.q;
    const bool vec = (a.d & 3) == 0 && ((uintptr_t)streamed & 15) == 0;
    const size_t lds = (size_t)DL_OT * ((a.d <= DL_ACC ? DL_ACC : 2 * DL_ACC) + 4) * 4;
    const dim3 grid((unsigned)(a.otiles * a.slabs), a.d <= DL_ACC ? 1u : 2u);
    if (vec) {
        GHF_SET_MAX_LDS((dloss_bwd_kernel<M, true, DQ>), lds);
        dloss_bwd_kernel<M, true, DQ><<<grid, 64, lds, stream>>>(a);
    } else {
        GHF_SET_MAX_LDS((dloss_bwd_kernel<M, false, DQ>), lds);
        dloss_bwd_kernel<M, false, DQ><<<grid, 64, lds, stream>>>(a);
    }
    GHF_LAUNCH_CHECK();
    return GHF_OK;
}

// one pass: the slabs' partials into `part` and their ordered sum into `result`, or straight into `result` with one slab
template <bool DQ>
static int launch_dloss_bwd(int metric, DlBwdArgs a, float* part, float* result, hipStream_t stream) {
    const int64_t nO = DQ ? a.B : a.C, nS = DQ ? a.C : a.B;
    DlBwdGeom g;
    dloss_bwd_geom(nO, nS, &g);
    GHF_REQUIRE(g.otiles * g.slabs < (int64_t)1 << 31, "dist_loss_bwd: B or C out of range");
    a.otiles = g.otiles; a.slab_rows = g.slab_rows; a.slabs = g.slabs;
    a.out = g.slabs > 1 ? part : result;
    int rc;
    if (metric == GHF_DIST_L1) rc = launch_dloss_bwd_pass<GHF_DIST_L1, DQ>(a, stream);
    else if (metric == GHF_DIST_L2) rc = launch_dloss_bwd_pass<GHF_DIST_L2, DQ>(a, stream);
    else rc = launch_dloss_bwd_pass<GHF_DIST_COMPLEX, DQ>(a, stream);
    if (rc != GHF_OK || g.slabs == 1) return rc;
    return launch_ordered_sum(part, g.slabs, nO * (int64_t)a.d, result, stream);
}

// what the three launches open with: the checks past the entry points' own, in ghf_distance_sweep.h's order
static int dloss_open(const char* op, size_t need, const int64_t* iq, int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d,
                      const int64_t* ic, int64_t C, size_t ws_bytes) {
    DlGeom g;
    GHF_REQUIRE(d > 0 && rows_q > 0 && N > 0 && B > 0 && nnz >= 0, "%s: bad shape", op);
    if (d > RK_MAX_D) return set_err(GHF_EUNSUPPORTED, "%s: d = %d exceeds %d", op, d, RK_MAX_D);
    GHF_REQUIRE(N < (int64_t)1 << 31, "%s: N = %lld rows, the sweep keeps row ids in 32 bits", op, (long long)N);
    GHF_REQUIRE(rows_q < (int64_t)1 << 31, "%s: rows_q = %lld rows of q, the sweep keeps row ids in 32 bits", op, (long long)rows_q);
    GHF_REQUIRE(ic ? (C > 0 && C <= N) : C == N, "%s: need 1 <= C <= N candidates, C == N without ic", op);
    GHF_REQUIRE(dloss_geom(B, C, &g), "%s: B or C out of range", op);
    GHF_REQUIRE(iq || B <= rows_q, "%s: B exceeds the rows of q", op);
    GHF_REQUIRE(need > 0 && ws_bytes >= need, "%s: workspace of %zu bytes, need %zu", op, ws_bytes, need);
    return GHF_OK;
}

// valid [B], and the targets and lists in position space (with ic: through the id map at `map_ws`)
static int dloss_validate(const float* q, const float* c, const int64_t* iq, const int64_t* target, const int64_t** filt_ptr,
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

static int launch_dloss_fwd(int metric, bool negsamp, const char* op, const float* q, const float* c, const int64_t* iq,
                            const int64_t* target, const int64_t* filt_ptr, const int64_t* filt_idx, int64_t nnz, int64_t rows_q,
                            int64_t N, int64_t B, int d, float scale, float margin, float alpha, const int64_t* ic, int64_t C,
                            void* ws, size_t ws_bytes, float* loss, float* aux, hipStream_t stream) {
    const size_t need = d > 0 && d <= RK_MAX_D ? dloss_fwd_workspace_bytes(B, C, d, nnz) : 0;
    int rc = dloss_open(op, need, iq, nnz, rows_q, N, B, d, ic, C, ws_bytes);
    if (rc != GHF_OK) return rc;
    DlGeom g;
    dloss_geom(B, C, &g);
    const size_t base = 2 * rk_align((size_t)B * 4) + rk_align((size_t)B * (size_t)g.slabs * 12);
    float* t = (float*)ws;
    int* valid = (int*)((char*)ws + rk_align((size_t)B * 4));
    float* part = (float*)((char*)ws + 2 * rk_align((size_t)B * 4));
    const int64_t* tpos;
    rc = dloss_validate(q, c, iq, target, &filt_ptr, &filt_idx, nnz, rows_q, N, B, d, ic, C, valid, (char*)ws + base, need - base, &tpos,
                        stream);
    if (rc != GHF_OK) return rc;
    const unsigned qb = (unsigned)cdiv(B, 256);
    dloss_target_kernel<<<qb, 256, 0, stream>>>(metric, q, c, iq, target, valid, B, d, t);
    GHF_LAUNCH_CHECK();
    DlossArgs a = {};
    a.q = q; a.c = c; a.iq = iq; a.ic = ic; a.rows_q = rows_q; a.Nn = N; a.C = C; a.B = B; a.d = d;
    a.qtiles = g.qtiles; a.slab_tiles = g.slab_tiles; a.slabs = g.slabs;
    a.tpos = tpos; a.valid = valid; a.filt_ptr = filt_ptr; a.filt_idx = filt_idx; a.nnz = nnz;
    a.scale = scale; a.margin = margin; a.alpha = alpha; a.part = part;
    rc = negsamp ? launch_dloss_tiles<true>(metric, a, stream) : launch_dloss_tiles<false>(metric, a, stream);
    if (rc != GHF_OK) return rc;
    dloss_finish_kernel<<<qb, 256, 0, stream>>>(part, t, valid, B, g.slabs, scale, margin, negsamp ? 1 : 0, loss, aux);
    GHF_LAUNCH_CHECK();
    return GHF_OK;
}

static int launch_dloss_backward(int metric, bool negsamp, const float* q, const float* c, const int64_t* iq, const int64_t* target,
                                 const int64_t* filt_ptr, const int64_t* filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B,
                                 int d, float scale, float margin, float alpha, const int64_t* ic, int64_t C, const float* saved,
                                 const float* grad, void* ws, size_t ws_bytes, float* dq, float* dc, hipStream_t stream) {
    const size_t need = d > 0 && d <= RK_MAX_D ? dloss_bwd_workspace_bytes(B, C, d, nnz) : 0;
    int rc = dloss_open("dist_loss_bwd", need, iq, nnz, rows_q, N, B, d, ic, C, ws_bytes);
    if (rc != GHF_OK) return rc;
    const size_t pq = dloss_bwd_part_bytes(B, C, d), pc = dloss_bwd_part_bytes(C, B, d);
    const size_t base = 2 * rk_align((size_t)B * 4) + pq + pc;
    float* sv = (float*)ws;
    int* valid = (int*)((char*)ws + rk_align((size_t)B * 4));
    float* part_q = (float*)((char*)ws + 2 * rk_align((size_t)B * 4));
    float* part_c = (float*)((char*)part_q + pq);
    const int64_t* tpos;
    rc = dloss_validate(q, c, iq, target, &filt_ptr, &filt_idx, nnz, rows_q, N, B, d, ic, C, valid, (char*)ws + base, need - base, &tpos,
                        stream);
    if (rc != GHF_OK) return rc;
    dloss_saved_kernel<<<(unsigned)cdiv(B, 256), 256, 0, stream>>>(saved, valid, B, sv);
    GHF_LAUNCH_CHECK();
    DlBwdArgs a = {};
    a.q = q; a.c = c; a.iq = iq; a.ic = ic; a.rows_q = rows_q; a.Nn = N; a.C = C; a.B = B; a.d = d;
    a.tpos = tpos; a.sv = sv; a.grad = grad; a.filt_ptr = filt_ptr; a.filt_idx = filt_idx; a.nnz = nnz;
    a.scale = scale; a.margin = margin; a.alpha = alpha; a.negsamp = negsamp ? 1 : 0;
    rc = launch_dloss_bwd<true>(metric, a, part_q, dq, stream);
    if (rc != GHF_OK) return rc;
    return launch_dloss_bwd<false>(metric, a, part_c, dc, stream);
}

}  // namespace ghf

// ---- the C ABI (include/ghf_distance_loss.h) --------------------------------------------------------------------------------
using namespace ghf;

extern "C" {

#define GHF_DLOSS_METRIC(op, dd)                                                                                             \
    do {                                                                                                                     \
        GHF_REQUIRE(metric == GHF_DIST_L1 || metric == GHF_DIST_L2 || metric == GHF_DIST_COMPLEX,                            \
                    op ": metric must be GHF_DIST_L1, GHF_DIST_L2 or GHF_DIST_COMPLEX");                                     \
        GHF_REQUIRE(metric != GHF_DIST_COMPLEX || ((dd) & 1) == 0, op ": GHF_DIST_COMPLEX needs an even d (re / im interleaved)"); \
    } while (0)

#define GHF_DLOSS_ENTRY(op, ptrs)                                                                                            \
    do {                                                                                                                     \
        GHF_REQUIRE((ptrs) && workspace, op ": null pointer argument");                                                      \
        GHF_REQUIRE(nnz <= 0 || (filt_ptr && filt_idx), op ": null filter list with nnz > 0");                               \
        GHF_REQUIRE(((uintptr_t)workspace & 255) == 0, op ": workspace not 256-byte aligned");                               \
    } while (0)

size_t ghf_dist_loss_fwd_workspace_bytes(int64_t B, int64_t C, int d, int64_t nnz) { return dloss_fwd_workspace_bytes(B, C, d, nnz); }

int ghf_dist_loss_softmax_fwd(int metric, const float* q, const float* c, const int64_t* iq, const int64_t* target,
                              const int64_t* filt_ptr, const int64_t* filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B,
                              int d, float scale, const int64_t* ic, int64_t C, void* workspace, size_t workspace_bytes, float* loss,
                              float* lse, void* stream) {
    GHF_DLOSS_METRIC("dist_loss_softmax_fwd", d);
    GHF_REQUIRE(std::isfinite(scale) && scale > 0.f, "dist_loss_softmax_fwd: scale must be finite and positive");
    GHF_DLOSS_ENTRY("dist_loss_softmax_fwd", q && c && target && loss && lse);
    return launch_dloss_fwd(metric, false, "dist_loss_softmax_fwd", q, c, iq, target, filt_ptr, filt_idx, nnz, rows_q, N, B, d, scale,
                            0.f, 0.f, ic, C, workspace, workspace_bytes, loss, lse, (hipStream_t)stream);
}

int ghf_dist_loss_negsamp_fwd(int metric, const float* q, const float* c, const int64_t* iq, const int64_t* target,
                              const int64_t* filt_ptr, const int64_t* filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B,
                              int d, float scale, float margin, float adv_temperature, const int64_t* ic, int64_t C,
                              void* workspace, size_t workspace_bytes, float* loss, float* lw, void* stream) {
    GHF_DLOSS_METRIC("dist_loss_negsamp_fwd", d);
    GHF_REQUIRE(std::isfinite(scale) && scale > 0.f, "dist_loss_negsamp_fwd: scale must be finite and positive");
    GHF_REQUIRE(std::isfinite(margin), "dist_loss_negsamp_fwd: margin must be finite");
    GHF_REQUIRE(std::isfinite(adv_temperature) && adv_temperature >= 0.f,
                "dist_loss_negsamp_fwd: adv_temperature must be finite and >= 0");
    GHF_DLOSS_ENTRY("dist_loss_negsamp_fwd", q && c && target && loss && lw);
    return launch_dloss_fwd(metric, true, "dist_loss_negsamp_fwd", q, c, iq, target, filt_ptr, filt_idx, nnz, rows_q, N, B, d, scale,
                            margin, adv_temperature, ic, C, workspace, workspace_bytes, loss, lw, (hipStream_t)stream);
}

size_t ghf_dist_loss_bwd_workspace_bytes(int64_t B, int64_t C, int d, int64_t nnz) { return dloss_bwd_workspace_bytes(B, C, d, nnz); }

int ghf_dist_loss_bwd(int metric, int mode, const float* q, const float* c, const int64_t* iq, const int64_t* target,
                      const int64_t* filt_ptr, const int64_t* filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d,
                      float scale, float margin, float adv_temperature, const int64_t* ic, int64_t C, const float* lse_or_lw,
                      const float* grad_loss, void* workspace, size_t workspace_bytes, float* dq, float* dc, void* stream) {
    GHF_DLOSS_METRIC("dist_loss_bwd", d);
    GHF_REQUIRE(mode == GHF_DIST_SOFTMAX || mode == GHF_DIST_NEGSAMP, "dist_loss_bwd: mode must be GHF_DIST_SOFTMAX or GHF_DIST_NEGSAMP");
    GHF_REQUIRE(std::isfinite(scale) && scale > 0.f, "dist_loss_bwd: scale must be finite and positive");
    GHF_REQUIRE(std::isfinite(margin), "dist_loss_bwd: margin must be finite");
    GHF_REQUIRE(std::isfinite(adv_temperature) && adv_temperature >= 0.f, "dist_loss_bwd: adv_temperature must be finite and >= 0");
    GHF_DLOSS_ENTRY("dist_loss_bwd", q && c && target && lse_or_lw && grad_loss && dq && dc);
    return launch_dloss_backward(metric, mode == GHF_DIST_NEGSAMP, q, c, iq, target, filt_ptr, filt_idx, nnz, rows_q, N, B, d, scale,
                                 margin, adv_temperature, ic, C, lse_or_lw, grad_loss, workspace, workspace_bytes, dq, dc,
                                 (hipStream_t)stream);
}

#undef GHF_DLOSS_ENTRY
#undef GHF_DLOSS_METRIC

}  // extern "C"
