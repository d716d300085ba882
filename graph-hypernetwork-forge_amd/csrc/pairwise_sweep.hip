// pairwise_sweep.hip — the pairwise ranking losses (hinge, logistic) under a DISTANCE score against every node or a shared
// candidate subset, forward and backward, the B x C distances, ids and coefficients never stored
// (include/ghf_pairwise_sweep.h).
//
// Forward: distance_loss.hip's tile loop, its geometry unchanged (the lane owns 4 candidates, the wave owns 16 queries,
//   candidate rows through two LDS buffers, query rows through scalar loads; distance_sweep_dev.h's chain; the LDS cursor that
//   lets an unlisted full tile touch no memory; slabs from C alone), with a pairwise epilogue.  The target's z_it is known
//   before the tiles start (dist_target_kernel, the tile's chain) and sits in LDS beside the targets' positions, so a
//   finished tile turns the lane's four z of a query into u = (z - z_it) + margin at once and adds phi(u), phi'(u), 1 and
//   [u > 0] into the lane's four running values — a pair outside J_i adds +0.f and 0.  At the slab's end the lanes merge by
//   the fixed xor butterfly and lane 0 writes one 16-byte partial per (query, slab); psweep_finish_kernel adds the slabs in
//   slab order.
//
// Backward: distance_loss.hip's two passes, their structure unchanged — dl_bwd_kernel<M, VEC, DQ, PsweepCoef<HINGE>>: the lane OWNS a
//   row in its own LDS row, the other side is STREAMED four wave-uniform rows at a time, phase 1 runs the full chain (the
//   forward's D, bit for bit), phase 2 adds G g_k into 128 static accumulators, d > 128 runs as two column halves, slabs and
//   then launch_ordered_sum.  The coefficient is new: G_ij = w_i phi'(u_ij) on J_i and G_it = -w_i dsum_i on the target pair,
//   which needs no second sweep because dsum_i = sum_j phi'(u_ij) is the forward's (for the hinge the integer `active`).
//   psweep_saved_kernel forms z_it, w_i and G_it once per query for both passes.
//
// The kernel texts, the geometry, the launch ladders and the validation are distance_loss_dev.h's, shared with
// distance_loss.hip; this unit instantiates the hinge and logistic sweeps and the backward under PsweepCoef<HINGE>, and keeps
// its argument blocks, its finish and saved kernels, its workspace layouts, its open check and its entry points.  The public
// `kind` becomes a DlEpi in the entry point, once, and nothing else: it shares no argument with a kernel selector (§23's trap).
#include "distance_loss_dev.h"
#include "../../include/ghf_pairwise_sweep.h"

#include <cmath>

namespace ghf {

static size_t psweep_fwd_workspace_bytes(int64_t B, int64_t C, int d, int64_t nnz) {
    DlGeom g;
    if (d <= 0 || d > RK_MAX_D || nnz < 0 || !dloss_geom(B, C, &g)) return 0;
    const size_t map = cand_workspace_bytes(B, nnz);
    if (!map) return 0;
    // t [B] float, valid [B] int32, the partials [B, slabs], the id map's
    return 2 * rk_align((size_t)B * 4) + rk_align((size_t)B * (size_t)g.slabs * sizeof(PsPart)) + map;
}

static size_t psweep_bwd_workspace_bytes(int64_t B, int64_t C, int d, int64_t nnz) {
    DlGeom g;
    if (d <= 0 || d > RK_MAX_D || nnz < 0 || !dloss_geom(B, C, &g)) return 0;
    const size_t map = cand_workspace_bytes(B, nnz);
    if (!map) return 0;
    // t -> z_it [B], valid [B] int32, w [B], G_it [B], the slabs' partials of dq and of dc, the id map's
    return 4 * rk_align((size_t)B * 4) + dloss_bwd_part_bytes(B, C, d) + dloss_bwd_part_bytes(C, B, d) + map;
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

// ---- the small kernels around the sweeps ------------------------------------------------------------------------------------
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

// The pairwise coefficient policy (distance_loss_dev.h): a query carries z_it, w_i and G_it, as psweep_saved_kernel left them
template <bool HINGE>
struct PsweepCoef {
    using Args = PsBwdArgs;
    template <int S>
    static __device__ __forceinline__ float carry(const Args& a, int64_t i) {
        if constexpr (S == 0) return a.zt[i];
        else if constexpr (S == 1) return a.w[i];
        else return a.gt[i];
    }
    // G of one pair: d loss / d s with s = -D.  The target's is the query's G_it, listed or not
    static __device__ __forceinline__ float G(const Args& a, float z, float zt, float w, float gt, bool is_target, bool listed) {
#pragma clang fp contract(off)
        const float u = (z - zt) + a.margin;
        float g;
        if constexpr (HINGE) g = u > 0.f ? w : 0.f;
        else g = w * psweep_sigmoid(u);
        return is_target ? gt : (listed ? 0.f : g);
    }
    static bool inputs(const Args& a) { return a.zt && a.w && a.gt; }
};

// what both launches open with: the checks past the entry points' own, in the header's order
static int psweep_open(const char* op, size_t need, const int64_t* iq, int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d,
                       const int64_t* ic, int64_t C, size_t ws_bytes) {
    DlGeom g;
    GHF_REQUIRE(d > 0 && rows_q > 0 && N > 0 && B > 0 && nnz >= 0, "%s: bad shape", op);
    GHF_REQUIRE(ic ? (C > 0 && C <= N) : C == N, "%s: need 1 <= C <= N candidates, C == N without ic", op);
    GHF_REQUIRE(iq || B <= rows_q, "%s: B exceeds the rows of q", op);
    GHF_REQUIRE(N < (int64_t)1 << 31, "%s: N = %lld rows, the sweep keeps row ids in 32 bits", op, (long long)N);
    GHF_REQUIRE(rows_q < (int64_t)1 << 31, "%s: rows_q = %lld rows of q, the sweep keeps row ids in 32 bits", op, (long long)rows_q);
    GHF_REQUIRE(dloss_geom(B, C, &g), "%s: B or C out of range", op);
    if (d > RK_MAX_D) return set_err(GHF_EUNSUPPORTED, "%s: d = %d exceeds %d", op, d, RK_MAX_D);
    GHF_REQUIRE(need > 0 && ws_bytes >= need, "%s: workspace of %zu bytes, need %zu", op, ws_bytes, need);
    return GHF_OK;
}

template <DlEpi E>
static int launch_psweep_fwd(int metric, const float* q, const float* c, const int64_t* iq, const int64_t* target,
                             const int64_t* filt_ptr, const int64_t* filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B,
                             int d, float scale, float margin, int normalize, const int64_t* ic, int64_t C, void* ws, size_t ws_bytes,
                             float* loss, float* dsum, int* count, int* active, hipStream_t stream) {
    const size_t need = d > 0 && d <= RK_MAX_D ? psweep_fwd_workspace_bytes(B, C, d, nnz) : 0;
    int rc = psweep_open("dist_pair_fwd", need, iq, nnz, rows_q, N, B, d, ic, C, ws_bytes);
    if (rc != GHF_OK) return rc;
    DlGeom g;
    dloss_geom(B, C, &g);
    const size_t base = 2 * rk_align((size_t)B * 4) + rk_align((size_t)B * (size_t)g.slabs * sizeof(PsPart));
    float* t = (float*)ws;
    int* valid = (int*)((char*)ws + rk_align((size_t)B * 4));
    PsPart* part = (PsPart*)((char*)ws + 2 * rk_align((size_t)B * 4));
    PsweepArgs a = {};
    a.q = q; a.c = c; a.iq = iq; a.ic = ic; a.rows_q = rows_q; a.Nn = N; a.C = C; a.B = B; a.d = d;
    a.qtiles = g.qtiles; a.slab_tiles = g.slab_tiles; a.slabs = g.slabs;
    a.t = t; a.filt_ptr = filt_ptr; a.filt_idx = filt_idx; a.nnz = nnz;
    a.scale = scale; a.margin = margin; a.part = part;
    rc = dl_sweep<E>("dist_pair_fwd", metric, a, target, valid, t, (char*)ws + base, need - base, DlOut{loss, nullptr, dsum, count, active},
                     stream);
    if (rc != GHF_OK) return rc;
    psweep_finish_kernel<<<(unsigned)cdiv(B, 256), 256, 0, stream>>>(part, valid, B, g.slabs, E == DlEpi::Hinge ? 1 : 0, normalize, loss,
                                                                     dsum, count, active);
    GHF_LAUNCH_CHECK();
    return GHF_OK;
}

template <DlEpi E>
static int launch_psweep_backward(int metric, const float* q, const float* c, const int64_t* iq, const int64_t* target,
                                  const int64_t* filt_ptr, const int64_t* filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B,
                                  int d, float scale, float margin, int normalize, const int64_t* ic, int64_t C, const float* dsum,
                                  const int* count, const float* grad, void* ws, size_t ws_bytes, float* dq, float* dc,
                                  hipStream_t stream) {
    const size_t need = d > 0 && d <= RK_MAX_D ? psweep_bwd_workspace_bytes(B, C, d, nnz) : 0;
    int rc = psweep_open("dist_pair_bwd", need, iq, nnz, rows_q, N, B, d, ic, C, ws_bytes);
    if (rc != GHF_OK) return rc;
    const size_t pq = dloss_bwd_part_bytes(B, C, d), pc = dloss_bwd_part_bytes(C, B, d);
    const size_t qbytes = rk_align((size_t)B * 4);
    const size_t base = 4 * qbytes + pq + pc;
    float* zt = (float*)ws;
    int* valid = (int*)((char*)ws + qbytes);
    float* w = (float*)((char*)ws + 2 * qbytes);
    float* gt = (float*)((char*)ws + 3 * qbytes);
    float* part_q = (float*)((char*)ws + 4 * qbytes);
    float* part_c = (float*)((char*)part_q + pq);
    PsBwdArgs a = {};
    a.q = q; a.c = c; a.iq = iq; a.ic = ic; a.rows_q = rows_q; a.Nn = N; a.C = C; a.B = B; a.d = d;
    a.zt = zt; a.w = w; a.gt = gt; a.filt_ptr = filt_ptr; a.filt_idx = filt_idx; a.nnz = nnz;
    a.scale = scale; a.margin = margin;
    const auto saved_pass = [&]() -> int {
        const unsigned qb = (unsigned)cdiv(B, 256);
        dist_target_kernel<<<qb, 256, 0, stream>>>(metric, q, c, iq, target, valid, B, d, zt);
        GHF_LAUNCH_CHECK();
        psweep_saved_kernel<<<qb, 256, 0, stream>>>(valid, dsum, count, grad, B, scale, normalize, zt, w, gt);
        GHF_LAUNCH_CHECK();
        return GHF_OK;
    };
    return dl_backward<PsweepCoef<E == DlEpi::Hinge>>("dist_pair_bwd", metric, a, target, valid, (char*)ws + base, need - base, part_q,
                                                      part_c, dq, dc, saved_pass, stream);
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
    const DlEpi e = dl_of_pair_kind(kind);
    if (e == DlEpi::Hinge)
        return launch_psweep_fwd<DlEpi::Hinge>(metric, q, c, iq, target, filt_ptr, filt_idx, nnz, rows_q, N, B, d, scale, margin,
                                               normalize, ic, C, workspace, workspace_bytes, loss, dsum, count, active,
                                               (hipStream_t)stream);
    GHF_REQUIRE(e == DlEpi::Logistic, "dist_pair_fwd: this unit holds the hinge and the logistic sweep only");
    return launch_psweep_fwd<DlEpi::Logistic>(metric, q, c, iq, target, filt_ptr, filt_idx, nnz, rows_q, N, B, d, scale, margin,
                                              normalize, ic, C, workspace, workspace_bytes, loss, dsum, count, active,
                                              (hipStream_t)stream);
}

size_t ghf_dist_pair_bwd_workspace_bytes(int64_t B, int64_t C, int d, int64_t nnz) { return psweep_bwd_workspace_bytes(B, C, d, nnz); }

int ghf_dist_pair_bwd(int metric, int kind, const float* q, const float* c, const int64_t* iq, const int64_t* target,
                      const int64_t* filt_ptr, const int64_t* filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d,
                      float scale, float margin, int normalize, const int64_t* ic, int64_t C, const float* dsum,
                      const int32_t* count, const float* grad_loss, void* workspace, size_t workspace_bytes, float* dq, float* dc,
                      void* stream) {
    GHF_PSWEEP_ENTRY("dist_pair_bwd", q && c && target && dsum && count && grad_loss && dq && dc);
    const DlEpi e = dl_of_pair_kind(kind);
    if (e == DlEpi::Hinge)
        return launch_psweep_backward<DlEpi::Hinge>(metric, q, c, iq, target, filt_ptr, filt_idx, nnz, rows_q, N, B, d, scale, margin,
                                                    normalize, ic, C, dsum, count, grad_loss, workspace, workspace_bytes, dq, dc,
                                                    (hipStream_t)stream);
    GHF_REQUIRE(e == DlEpi::Logistic, "dist_pair_bwd: this unit holds the hinge and the logistic backward only");
    return launch_psweep_backward<DlEpi::Logistic>(metric, q, c, iq, target, filt_ptr, filt_idx, nnz, rows_q, N, B, d, scale, margin,
                                                   normalize, ic, C, dsum, count, grad_loss, workspace, workspace_bytes, dq, dc,
                                                   (hipStream_t)stream);
}

#undef GHF_PSWEEP_ENTRY

}  // extern "C"
