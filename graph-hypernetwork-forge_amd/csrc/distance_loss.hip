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
//   merges the slabs in slab order and forms loss and lse / lw from z_it, which dist_target_kernel formed by the tile's chain.
//   The slabs depend on C alone (dloss_geom), so a query's bits do not depend on its batch.
//
// Backward: ONE kernel text for two passes, dl_bwd_kernel<M, VEC, DQ, DlossCoef>.  Lane l of a one-wave workgroup OWNS a row (DQ: query
//   l of the tile; otherwise candidate l), kept in its own LDS row (stride 132 or 260 floats: the lanes of a ds_read_b128 step 4
//   banks); the other side is STREAMED, four wave-uniform rows at a time through scalar loads, in ascending order.  Per group:
//   phase 1 runs the full-d chain to D, z and G of the lane's four pairs; phase 2 walks k again and adds G g_k into 128
//   statically indexed accumulators.  d > 128 runs as two column halves (blockIdx.y), phase 1 paid twice.  A workgroup owns
//   (owner tile, slab of the streamed side) and writes one partial; launch_ordered_sum adds the slabs in slab order.  No
//   floating-point atomics anywhere.
//
// The kernel texts, the geometry, the launch ladders and the validation are distance_loss_dev.h's, shared with
// pairwise_sweep.hip; this unit instantiates the softmax and negsamp sweeps and the backward under DlossCoef, and keeps its
// argument blocks, its finish and saved kernels, its workspace layouts, its open check and its entry points.  The public
// `mode` of ghf_dist_loss_bwd becomes a DlEpi in the entry point and the boolean DlBwdArgs::negsamp on the host, and nothing
// else: it shares no argument and no template parameter with a kernel selector (§23's trap).
#include "distance_loss_dev.h"
#include "../../include/ghf_distance_loss.h"

#include <cmath>

namespace ghf {

static size_t dloss_fwd_workspace_bytes(int64_t B, int64_t C, int d, int64_t nnz) {
    DlGeom g;
    if (d <= 0 || d > RK_MAX_D || nnz < 0 || !dloss_geom(B, C, &g)) return 0;
    const size_t map = cand_workspace_bytes(B, nnz);
    if (!map) return 0;
    // t [B] float, valid [B] int32, (max, S, T) [B, slabs], the id map's
    return 2 * rk_align((size_t)B * 4) + rk_align((size_t)B * (size_t)g.slabs * 12) + map;
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

// ---- the small kernels around the sweeps ------------------------------------------------------------------------------------
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

// The set losses' coefficient policy (distance_loss_dev.h): a query carries sv = lse (softmax) or lw (negsamp) and
// gs = grad * scale; which loss is the run-time boolean a.negsamp, one instantiation for both
struct DlossCoef {
    using Args = DlBwdArgs;
    template <int S>
    static __device__ __forceinline__ float carry(const Args& a, int64_t i) {
        if constexpr (S == 0) return a.sv[i];
        else if constexpr (S == 1) return a.grad[i] * a.scale;
        else return 0.f;
    }
    // G of one pair: d loss / d s, ghf_neg_bwd's per loss
    static __device__ __forceinline__ float G(const Args& a, float z, float sv, float gs, float, bool is_target, bool listed) {
#pragma clang fp contract(off)
        if (!a.negsamp) {
            const float e = __expf(z - sv);
            return is_target ? gs * (e - 1.f) : (listed ? 0.f : gs * e);
        }
        const float y = z + a.margin;
        const float e = __expf(-fabsf(y)), rcp = __builtin_amdgcn_rcpf(1.f + e);
        if (is_target) return -gs * (y >= 0.f ? e * rcp : rcp);
        const float w = sv > -INFINITY ? __expf(fmaf(a.alpha, z, -sv)) : 0.f;
        return listed ? 0.f : gs * (w * (y >= 0.f ? rcp : e * rcp));
    }
    static bool inputs(const Args& a) { return a.sv && a.grad; }
};

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

template <DlEpi E>
static int launch_dloss_fwd(int metric, const char* op, const float* q, const float* c, const int64_t* iq, const int64_t* target,
                            const int64_t* filt_ptr, const int64_t* filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B,
                            int d, float scale, float margin, float alpha, const int64_t* ic, int64_t C, void* ws, size_t ws_bytes,
                            float* loss, float* aux, hipStream_t stream) {
    const size_t need = d > 0 && d <= RK_MAX_D ? dloss_fwd_workspace_bytes(B, C, d, nnz) : 0;
    int rc = dloss_open(op, need, iq, nnz, rows_q, N, B, d, ic, C, ws_bytes);
    if (rc != GHF_OK) return rc;
    DlGeom g;
    dloss_geom(B, C, &g);
    const size_t base = 2 * rk_align((size_t)B * 4) + rk_align((size_t)B * (size_t)g.slabs * 12);
    float* t = (float*)ws;
    int* valid = (int*)((char*)ws + rk_align((size_t)B * 4));
    float* part = (float*)((char*)ws + 2 * rk_align((size_t)B * 4));
    DlossArgs a = {};
    a.q = q; a.c = c; a.iq = iq; a.ic = ic; a.rows_q = rows_q; a.Nn = N; a.C = C; a.B = B; a.d = d;
    a.qtiles = g.qtiles; a.slab_tiles = g.slab_tiles; a.slabs = g.slabs;
    a.filt_ptr = filt_ptr; a.filt_idx = filt_idx; a.nnz = nnz;
    a.scale = scale; a.margin = margin; a.alpha = alpha; a.part = part;
    rc = dl_sweep<E>(op, metric, a, target, valid, t, (char*)ws + base, need - base, DlOut{loss, aux, nullptr, nullptr, nullptr}, stream);
    if (rc != GHF_OK) return rc;
    dloss_finish_kernel<<<(unsigned)cdiv(B, 256), 256, 0, stream>>>(part, t, valid, B, g.slabs, scale, margin,
                                                                    E == DlEpi::Negsamp ? 1 : 0, loss, aux);
    GHF_LAUNCH_CHECK();
    return GHF_OK;
}

static int launch_dloss_backward(int metric, DlEpi e, const float* q, const float* c, const int64_t* iq, const int64_t* target,
                                 const int64_t* filt_ptr, const int64_t* filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B,
                                 int d, float scale, float margin, float alpha, const int64_t* ic, int64_t C, const float* saved,
                                 const float* grad, void* ws, size_t ws_bytes, float* dq, float* dc, hipStream_t stream) {
    GHF_REQUIRE(!dl_is_pair(e), "dist_loss_bwd: this unit holds no pairwise backward");
    const size_t need = d > 0 && d <= RK_MAX_D ? dloss_bwd_workspace_bytes(B, C, d, nnz) : 0;
    int rc = dloss_open("dist_loss_bwd", need, iq, nnz, rows_q, N, B, d, ic, C, ws_bytes);
    if (rc != GHF_OK) return rc;
    const size_t pq = dloss_bwd_part_bytes(B, C, d), pc = dloss_bwd_part_bytes(C, B, d);
    const size_t base = 2 * rk_align((size_t)B * 4) + pq + pc;
    float* sv = (float*)ws;
    int* valid = (int*)((char*)ws + rk_align((size_t)B * 4));
    float* part_q = (float*)((char*)ws + 2 * rk_align((size_t)B * 4));
    float* part_c = (float*)((char*)part_q + pq);
    DlBwdArgs a = {};
    a.q = q; a.c = c; a.iq = iq; a.ic = ic; a.rows_q = rows_q; a.Nn = N; a.C = C; a.B = B; a.d = d;
    a.sv = sv; a.grad = grad; a.filt_ptr = filt_ptr; a.filt_idx = filt_idx; a.nnz = nnz;
    a.scale = scale; a.margin = margin; a.alpha = alpha; a.negsamp = e == DlEpi::Negsamp ? 1 : 0;
    const auto saved_pass = [&]() -> int {
        dloss_saved_kernel<<<(unsigned)cdiv(B, 256), 256, 0, stream>>>(saved, valid, B, sv);
        GHF_LAUNCH_CHECK();
        return GHF_OK;
    };
    return dl_backward<DlossCoef>("dist_loss_bwd", metric, a, target, valid, (char*)ws + base, need - base, part_q, part_c, dq, dc,
                                  saved_pass, stream);
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
    return launch_dloss_fwd<DlEpi::Softmax>(metric, "dist_loss_softmax_fwd", q, c, iq, target, filt_ptr, filt_idx, nnz, rows_q, N, B, d, scale,
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
    return launch_dloss_fwd<DlEpi::Negsamp>(metric, "dist_loss_negsamp_fwd", q, c, iq, target, filt_ptr, filt_idx, nnz, rows_q, N, B, d, scale,
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
    return launch_dloss_backward(metric, dl_of_dist_mode(mode), q, c, iq, target, filt_ptr, filt_idx, nnz, rows_q, N, B, d, scale,
                                 margin, adv_temperature, ic, C, lse_or_lw, grad_loss, workspace, workspace_bytes, dq, dc,
                                 (hipStream_t)stream);
}

#undef GHF_DLOSS_ENTRY
#undef GHF_DLOSS_METRIC

}  // extern "C"
