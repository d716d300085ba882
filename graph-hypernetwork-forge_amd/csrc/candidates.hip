// candidates.hip — a candidate subset for the four all-node operations (rank, top-k, softmax loss, BCE loss; include/ghf.h:
// the ghf_score_*_sub calls).  The caller names the candidates as node ids ic [C], strictly ascending; the
// result is that of the all-node call on the table c[ic], every id going in or coming out still a node id.
//
// No copy of the candidate rows is made: the sweeps (rank_sweep.h, softmax.hip) run in POSITION space — candidate j of the
// sweep is row ic[j] of c, one index load per row — with N := C, so the cursors, the top-k key order (score descending,
// position ascending = id ascending) and the slab geometry are the all-node ones.  What has to change space is small and is
// done here, ahead of the sweep:
//   targets   a binary search in ic per query: the position, or -1 for a node that is not a candidate
//   lists     a binary search per entry, then a stable compaction (one exclusive scan over the keep flags): entries that are
//             no candidates leave, the others become positions; ic is ascending, so every list stays ascending, and a new CSR
//             pointer array goes with them.  Entries behind the last kept one are set to -1 (no position).
//   ic        checked by the same pass: strictly ascending and inside [0, N).  A bad ic makes every query invalid; the
//             sweeps themselves read no row outside c whatever ic holds (sub_row).
#include "common.h"
#include "rank_sweep.h"

#include <hipcub/hipcub.hpp>

namespace ghf {

static size_t cand_scan_bytes(int64_t n) {
    size_t tb = 0;
    hipcub::DeviceScan::ExclusiveSum(nullptr, tb, (const int32_t*)nullptr, (int32_t*)nullptr, (int)n, (hipStream_t)0);
    return tb;
}

size_t cand_workspace_bytes(int64_t B, int64_t nnz) {
    if (B <= 0 || nnz < 0 || nnz >= ((int64_t)1 << 31) - 1) return 0;
    // bad flag, valid [B] int32, tpos [B], lse [B] float, then for the lists: ptr [B + 1], idx [nnz], pos [nnz], keep and
    // off [nnz + 1] int32, the scan's own
    size_t b = 256 + rk_align((size_t)B * 4) + rk_align((size_t)B * 8) + rk_align((size_t)B * 4);
    if (nnz > 0)
        b += rk_align((size_t)(B + 1) * 8) + 2 * rk_align((size_t)nnz * 8) + 2 * rk_align((size_t)(nnz + 1) * 4) +
             rk_align(cand_scan_bytes(nnz + 1));
    return b;
}

// position of node id `id` in the ascending ic [C], -1 when it is not there
__device__ __forceinline__ int64_t cand_position(const int64_t* __restrict__ ic, int64_t C, int64_t id) {
    int64_t lo = 0, hi = C;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (ic[mid] < id) lo = mid + 1; else hi = mid;
    }
    return lo < C && ic[lo] == id ? lo : -1;
}

// one thread per candidate
__global__ __launch_bounds__(256) void cand_check_kernel(const int64_t* __restrict__ ic, int64_t C, int64_t N, int* bad) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= C) return;
    const int64_t id = ic[j];
    if (id < 0 || id >= N || (j > 0 && ic[j - 1] >= id)) *bad = 1;
}

// one thread per query: score_prep_kernel's work for a sweep over a subset
__global__ __launch_bounds__(256) void cand_prep_kernel(const float* __restrict__ q, const float* __restrict__ c,
                                                        const int64_t* __restrict__ iq, const int64_t* __restrict__ target,
                                                        int target_in, const int64_t* __restrict__ ic, int64_t C, int64_t rows_q,
                                                        int64_t N, int64_t B, int d, const int* __restrict__ bad,
                                                        const float* __restrict__ lse_in, float* __restrict__ t,
                                                        int* __restrict__ valid, int64_t* __restrict__ tpos,
                                                        float* __restrict__ lse_out, long long* __restrict__ greater,
                                                        long long* __restrict__ equal) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= B) return;
    const int64_t r = iq ? iq[i] : i;
    bool ok = !*bad && r >= 0 && r < rows_q;
    int64_t tp = -1;
    if (target) {
        const int64_t tg = target[i];
        ok = ok && tg >= 0 && tg < N;
        if (ok) tp = cand_position(ic, C, tg);
        if (target_in) ok = ok && tp >= 0;
        if (t) t[i] = ok ? dot_chain(q + (size_t)r * d, c + (size_t)tg * d, d, rows_vec(q, d) && rows_vec(c, d)) : __int_as_float(0x7FC00000);
    }
    tpos[i] = ok ? tp : -1;
    if (lse_out) lse_out[i] = ok ? lse_in[i] : __int_as_float(0x7FC00000);
    if (greater) {
        greater[i] = 0;
        equal[i] = 0;
    }
    valid[i] = ok ? 1 : 0;
}

// one thread per list entry (and one behind the last, whose flag closes the scan): where the entry is in ic.  An id outside
// [0, N) marks the query whose list holds it, as list_range_kernel does.
__global__ __launch_bounds__(256) void cand_find_kernel(const int64_t* __restrict__ list_ptr, const int64_t* __restrict__ list_idx,
                                                        int64_t nnz, const int64_t* __restrict__ ic, int64_t C, int64_t N, int64_t B,
                                                        int64_t* __restrict__ pos, int32_t* __restrict__ keep, int* valid) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e > nnz) return;
    if (e == nnz) {
        keep[e] = 0;
        return;
    }
    const int64_t j = list_idx[e];
    int64_t p = -1;
    if (j >= 0 && j < N) {
        p = cand_position(ic, C, j);
    } else {
        int64_t i;
        if (list_owner(list_ptr, B, e, &i)) valid[i] = 0;
    }
    pos[e] = p;
    keep[e] = p >= 0 ? 1 : 0;
}

// the compaction: thread e moves its entry (kept entries keep their order: off is the exclusive scan of keep), clears slot e
// where it lies behind the last kept entry, and, for e <= B, writes the new list pointer
__global__ __launch_bounds__(256) void cand_compact_kernel(const int64_t* __restrict__ list_ptr, const int64_t* __restrict__ pos,
                                                           const int32_t* __restrict__ off, int64_t nnz, int64_t B,
                                                           int64_t* __restrict__ ptr, int64_t* __restrict__ idx) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e < nnz) {
        if (pos[e] >= 0) idx[off[e]] = pos[e];
        if (e >= off[nnz]) idx[e] = -1;
    }
    if (e <= B) {
        int64_t p = list_ptr[e];
        p = p < 0 ? 0 : (p > nnz ? nnz : p);
        ptr[e] = off[p];
    }
}

// one thread per candidate: the bias of node ic[j] at position j, where the BIAS sweeps read it; an id outside
// the table reads nothing (cand_check_kernel reports such a list, and every query is then invalid)
__global__ __launch_bounds__(256) void cand_bias_kernel(const float* __restrict__ bias, const int64_t* __restrict__ ic, int64_t C,
                                                        int64_t N, float* __restrict__ out) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= C) return;
    const int64_t id = ic[j];
    out[j] = id >= 0 && id < N ? bias[id] : 0.f;
}

int launch_cand_bias(const float* bias, const int64_t* ic, int64_t C, int64_t N, float* out, hipStream_t stream) {
    GHF_REQUIRE(bias && ic && out && C > 0 && C <= N, "candidates: bias gather needs 1 <= C <= N ids");
    cand_bias_kernel<<<(unsigned)cdiv(C, 256), 256, 0, stream>>>(bias, ic, C, N, out);
    GHF_LAUNCH_CHECK();
    return GHF_OK;
}

int launch_cand_map(const float* q, const float* c, const int64_t* iq, const int64_t* target, bool target_in,
                    const int64_t* list_ptr, const int64_t* list_idx, int64_t nnz, const int64_t* ic, int64_t C, int64_t rows_q,
                    int64_t N, int64_t B, int d, const float* lse, float* t, int* valid, int64_t* greater, int64_t* equal, void* ws,
                    size_t ws_bytes, CandMap* m, hipStream_t stream) {
    GHF_REQUIRE(ic && C > 0 && C <= N, "candidates: need 1 <= C <= N ids, got C = %lld of N = %lld", (long long)C, (long long)N);
    GHF_REQUIRE(N < (int64_t)1 << 31, "candidates: N = %lld rows, the sweep keeps row ids in 32 bits", (long long)N);
    // ws_bytes: the caller's cand_workspace_bytes(B, nnz), asked once per launch — the scan's own size is what the fixed
    // part of the layout leaves of it
    GHF_REQUIRE(ws_bytes > 0, "candidates: B or nnz out of range");
    char* p = (char*)ws;
    int* bad = (int*)p;                          p += 256;
    int* own_valid = (int*)p;                    p += rk_align((size_t)B * 4);
    int64_t* tpos = (int64_t*)p;                 p += rk_align((size_t)B * 8);
    float* lse_out = (float*)p;                  p += rk_align((size_t)B * 4);
    if (!valid) valid = own_valid;
    GHF_HIP_CHECK(hipMemsetAsync(bad, 0, 4, stream));
    cand_check_kernel<<<(unsigned)cdiv(C, 256), 256, 0, stream>>>(ic, C, N, bad);
    GHF_LAUNCH_CHECK();
    cand_prep_kernel<<<(unsigned)cdiv(B, 256), 256, 0, stream>>>(q, c, iq, target, target_in ? 1 : 0, ic, C, rows_q, N, B, d, bad, lse,
                                                                 t, valid, tpos, lse ? lse_out : nullptr, (long long*)greater,
                                                                 (long long*)equal);
    GHF_LAUNCH_CHECK();
    *m = CandMap{tpos, nullptr, nullptr, lse ? lse_out : nullptr};
    if (nnz > 0) {
        int64_t* ptr = (int64_t*)p;              p += rk_align((size_t)(B + 1) * 8);
        int64_t* idx = (int64_t*)p;              p += rk_align((size_t)nnz * 8);
        int64_t* pos = (int64_t*)p;              p += rk_align((size_t)nnz * 8);
        int32_t* keep = (int32_t*)p;             p += rk_align((size_t)(nnz + 1) * 4);
        int32_t* off = (int32_t*)p;              p += rk_align((size_t)(nnz + 1) * 4);
        size_t scan_bytes = ws_bytes - (size_t)(p - (char*)ws);
        cand_find_kernel<<<(unsigned)cdiv(nnz + 1, 256), 256, 0, stream>>>(list_ptr, list_idx, nnz, ic, C, N, B, pos, keep, valid);
        GHF_LAUNCH_CHECK();
        GHF_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum((void*)p, scan_bytes, (const int32_t*)keep, off, (int)(nnz + 1), stream));
        const int64_t n = nnz > B + 1 ? nnz : B + 1;
        cand_compact_kernel<<<(unsigned)cdiv(n, 256), 256, 0, stream>>>(list_ptr, pos, off, nnz, B, ptr, idx);
        GHF_LAUNCH_CHECK();
        m->ptr = ptr;
        m->idx = idx;
    }
    return GHF_OK;
}

}  // namespace ghf
