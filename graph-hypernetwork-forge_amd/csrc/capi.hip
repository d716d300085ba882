// capi.hip — the extern "C" surface declared in include/ghf.h.
#include "common.h"
#include "negatives.h"
#include "distance.h"
#include "pairwise.h"
#include "../../include/ghf_pairwise_dot_sweep.h"
#include <vector>
#include <thread>
#include <algorithm>

#include <stdlib.h>
#include <string.h>

namespace ghf {

char* err_buf() {
    static thread_local char buf[512] = {0};
    return buf;
}

int set_err(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(err_buf(), 512, fmt, ap);
    va_end(ap);
    return code;
}

}  // namespace ghf

namespace ghf {
static std::atomic<int32_t*> g_range_flag{nullptr};
int32_t* range_flag_ptr() { return g_range_flag.load(std::memory_order_acquire); }
}  // namespace ghf

using namespace ghf;

extern "C" {

int ghf_set_range_flag(int32_t* device_word) {
    g_range_flag.store(device_word, std::memory_order_release);
    return GHF_OK;
}

int ghf_abi_version(void) { return GHF_ABI_VERSION; }

unsigned long long ghf_host_checksum64(const void* p, size_t nbytes, unsigned long long seed) {
    // four independent multiply-xor lanes over 32-byte strides (memory-bound from ~2 lanes on), folded with their positions
    const unsigned long long K0 = 0x9E3779B97F4A7C15ull, K1 = 0xC2B2AE3D27D4EB4Full, K2 = 0x165667B19E3779F9ull, K3 = 0x27D4EB2F165667C5ull;
    const unsigned long long* w = (const unsigned long long*)p;
    const size_t n = nbytes / 8;
    unsigned long long h0 = seed ^ K0, h1 = seed ^ K1, h2 = seed ^ K2, h3 = seed ^ K3;
    size_t i = 0;
    for (; i + 4 <= n; i += 4) {
        h0 = (h0 ^ w[i]) * K1;      h0 ^= h0 >> 29;
        h1 = (h1 ^ w[i + 1]) * K2;  h1 ^= h1 >> 31;
        h2 = (h2 ^ w[i + 2]) * K3;  h2 ^= h2 >> 27;
        h3 = (h3 ^ w[i + 3]) * K0;  h3 ^= h3 >> 33;
    }
    for (; i < n; ++i) { h0 = (h0 ^ w[i]) * K1; h0 ^= h0 >> 29; }
    unsigned long long h = (h0 * K0) ^ (h1 * K1 + 1) ^ (h2 * K2 + 2) ^ (h3 * K3 + 3) ^ (unsigned long long)n;
    h ^= h >> 32; h *= K2; h ^= h >> 29;
    return h;
}

const char* ghf_last_error(void) { return err_buf(); }

int ghf_message_config(int d, int* block_nodes, int* wlayout, int* chunk_rows, int* split_chunks) {
    if (!block_nodes || !wlayout || !chunk_rows || !split_chunks) return set_err(GHF_EINVAL, "message_config: null output pointer");
    int bn = 1, cr = 0, sc = 0;
    // GHF_KERNEL selects the d = 128 kernel for A/B runs: "bx" (default) = two fp16 pieces, three products, block sums in
    // registers (message_bx.hip; round 1's LDS-sum variant message_hx.hip was removed in round 3); "pp" = exact fp32,
    // v_mfma_f32_16x16x4_f32 (message_pp.hip: also what the range guard falls back to)
    // "rs" / "rs32" / "generic": a CSR plan also where a destination-block kernel exists (A/B of the relation-stationary
    // layer at d = 128)
    const char* kv = getenv("GHF_KERNEL");
    if (kv && (!strcmp(kv, "rs") || !strcmp(kv, "rs32") || !strcmp(kv, "generic"))) {
        *block_nodes = 1;
        *wlayout = GHF_WLAYOUT_NATURAL;
        *chunk_rows = 0;
        *split_chunks = 0;
    } else if ((!kv || !strcmp(kv, "bx")) && message_bx_config(d, &bn, &cr, &sc)) {
        *block_nodes = bn;
        *wlayout = GHF_WLAYOUT_SPLIT2H;
        *chunk_rows = cr;
        *split_chunks = sc;
    } else if (message_pp_config(d, &bn, &cr, &sc)) {
        *block_nodes = bn;
        *wlayout = GHF_WLAYOUT_FRAG16;
        *chunk_rows = cr;
        *split_chunks = sc;
    } else {
        *block_nodes = 1;
        *wlayout = GHF_WLAYOUT_NATURAL;
        *chunk_rows = 0;
        *split_chunks = 0;
    }
    return GHF_OK;
}

int64_t ghf_plan_max_items(int64_t N, int64_t E, int R, int block_nodes, int chunk_rows, int split_chunks) {
    return plan_max_items(N, E, R, block_nodes, chunk_rows, split_chunks);
}

size_t ghf_plan_workspace_bytes(int64_t N, int64_t E, int R, int block_nodes, int chunk_rows) {
    return plan_workspace_bytes(N, E, R, block_nodes, chunk_rows);
}

int64_t ghf_plan_max_chunks(int64_t N, int64_t E, int R, int block_nodes, int chunk_rows) {
    return plan_max_chunks(N, E, R, block_nodes, chunk_rows);
}

int ghf_plan_build(const int64_t* edge_index, const int64_t* rel_id, int64_t N, int64_t E, int R, int block_nodes,
                   int chunk_rows, int split_chunks, void* workspace, size_t workspace_bytes, uint32_t* sorted_key,
                   int32_t* sorted_src, int32_t* seg_off, int32_t* indeg, int32_t* chunk_tab, int32_t* blk_chunk_off,
                   int32_t* item_tab, int32_t* blk_item_off, int32_t* status, void* stream) {
    GHF_REQUIRE(edge_index && rel_id && workspace && sorted_key && sorted_src && seg_off && indeg && status,
                "plan_build: null pointer argument");
    GHF_REQUIRE(block_nodes == 1 || (chunk_tab && blk_chunk_off && chunk_rows > 0),
                "plan_build: block plans need chunk_tab, blk_chunk_off and chunk_rows");
    return launch_plan_build(edge_index, rel_id, N, E, R, block_nodes, chunk_rows, split_chunks, workspace, workspace_bytes,
                             sorted_key, sorted_src, seg_off, indeg, chunk_tab, blk_chunk_off, item_tab, blk_item_off, status,
                             (hipStream_t)stream);
}

int ghf_weightgen_fwd(const float* text_emb, const float* const* head_params, const float* const* log_scales,
                      int R, int T, int Hh, int num_hidden, int d_in, int d_out, int layout, float* hidden_ws,
                      float* W_msg, float* W_self, float* bias, const float* hidden_drop, float* acts, void* stream) {
    GHF_REQUIRE(text_emb && head_params && log_scales && log_scales[0] && log_scales[1] && log_scales[2] && hidden_ws && W_msg && bias,
                "weightgen_fwd: null pointer argument");
    return launch_weightgen(text_emb, head_params, log_scales, R, T, Hh, num_hidden, d_in, d_out, layout,
                            hidden_ws, W_msg, W_self, bias, hidden_drop, (hipStream_t)stream, acts);
}

int ghf_weightgen_fwd_batched(int L, const float* text_emb, const float* const* head_params, const float* const* log_scales,
                              int R, int T, int Hh, int num_hidden, int d_in, int d_out, int layout, float* hidden_ws,
                              float* const* W_msg, float* const* W_self, float* const* bias, void* stream) {
    GHF_REQUIRE(text_emb && head_params && log_scales && hidden_ws && W_msg && bias, "weightgen_fwd_batched: null pointer argument");
    return launch_weightgen_batched(L, text_emb, head_params, log_scales, R, T, Hh, num_hidden, d_in, d_out, layout, hidden_ws,
                                    W_msg, W_self, bias, nullptr, (hipStream_t)stream);
}

int ghf_text_encode_fwd(const int32_t* ids, const int32_t* lens, int U, int Lmax, const float* char_emb, int V, int C,
                        const float* W, const float* b, int T, float* out, void* stream) {
    GHF_REQUIRE(ids && lens && char_emb && W && b && out, "text_encode_fwd: null pointer argument");
    return launch_text_encode(ids, lens, U, Lmax, char_emb, V, C, W, b, T, out, (hipStream_t)stream);
}

int ghf_input_proj_fwd(const float* x, const float* W_in, const float* b_in, int64_t N, int F, int d,
                       float* h0, void* h_split, int split_layout, void* stream) {
    GHF_REQUIRE(x && W_in && b_in && h0, "input_proj_fwd: null pointer argument");
    return launch_input_proj(x, W_in, b_in, N, F, d, h0, h_split, split_layout, (hipStream_t)stream);
}

size_t ghf_split_rows_bytes(int64_t N, int d, int wlayout) {
    if (wlayout == GHF_WLAYOUT_SPLIT2H) return (size_t)N * d * 4 + (size_t)N * 4;
    return 0;
}

size_t ghf_weights_bytes(int R, int d_in, int d_out, int wlayout) {
    const size_t n = (size_t)R * d_in * d_out;
    switch (wlayout) {
        case GHF_WLAYOUT_FRAG16:  return 2 * n * 4;
        case GHF_WLAYOUT_SPLIT2H: return 2 * n * 4 + (size_t)R * 4;
        default:                  return n * 4;
    }
}

int ghf_split_rows(const float* h, int64_t N, int d, int64_t row0, int64_t rows, int wlayout, void* h_split, void* stream) {
    GHF_REQUIRE(h && h_split, "split_rows: null pointer argument");
    GHF_REQUIRE(N > 0 && d > 0 && d % 4 == 0 && row0 >= 0 && rows >= 0 && row0 + rows <= N, "split_rows: bad shape or row range");
    if (wlayout == GHF_WLAYOUT_SPLIT2H) return launch_split2h_rows(h, N, d, row0, rows, h_split, (hipStream_t)stream);
    return set_err(GHF_EINVAL, "split_rows: layout %d gathers h itself", wlayout);
}

namespace {
// open-addressing table of machine words -> dense ids (0 is not a valid object address)
struct WordTable {
    std::vector<unsigned long long> key;
    std::vector<long long> val;
    size_t mask;
    explicit WordTable(size_t max_uniq) {
        size_t cap = 64;
        while (cap < max_uniq * 4) cap <<= 1;
        key.assign(cap, 0ull);
        val.assign(cap, -1);
        mask = cap - 1;
    }
    // id of x, or -1 (then *slot is where it belongs)
    long long find(unsigned long long x, size_t* slot) const {
        size_t h = (size_t)((x >> 4) * 0x9E3779B97F4A7C15ull >> 20) & mask;
        for (;;) {
            if (key[h] == x) return val[h];
            if (val[h] < 0) { *slot = h; return -1; }
            h = (h + 1) & mask;
        }
    }
    void put(size_t slot, unsigned long long x, long long id) { key[slot] = x; val[slot] = id; }
};
}  // namespace

long long ghf_host_word_ids(const void* words, long long n, long long* ids, void** uniq, long long max_uniq, int threads) {
    if (!words || !ids || !uniq || n < 0 || max_uniq <= 0) return -1;
    const unsigned long long* w = (const unsigned long long*)words;
    // One pass in order over a prefix finds (nearly always all of) the distinct words; the rest of the array is mapped by
    // `threads` threads against a copy of that table.  A word a thread meets that the prefix did not hold gets a provisional id
    // (>= PROV, per thread, in the thread's order); those are ranked afterwards — thread by thread, i.e. in array order — and the
    // few entries that carry one rewritten.  The result equals the sequential pass: ids by first appearance.
    const long long PROV = 1ll << 40;
    WordTable tab((size_t)max_uniq);
    long long k = 0;
    auto seq = [&](long long a, long long b) -> bool {
        unsigned long long last = 0;
        long long last_id = -1;
        for (long long i = a; i < b; ++i) {
            const unsigned long long x = w[i];
            if (x == last && last_id >= 0) { ids[i] = last_id; continue; }
            size_t slot;
            long long id = tab.find(x, &slot);
            if (id < 0) {
                if (k >= max_uniq) return false;
                id = k;
                tab.put(slot, x, id);
                uniq[k++] = (void*)x;
            }
            last = x;
            last_id = id;
            ids[i] = id;
        }
        return true;
    };
    const long long prefix = n < (1ll << 18) || threads <= 1 ? n : (1ll << 16);
    if (!seq(0, prefix)) return -1;
    if (prefix == n) return k;
    const int T = (int)std::min<long long>(threads, (n - prefix + (1ll << 18) - 1) >> 18);
    std::vector<std::vector<unsigned long long>> fresh(T);             // a thread's new words, in its order
    std::vector<int> bad(T, 0);
    const long long per = (n - prefix + T - 1) / T;
    auto work = [&](int t) {
        WordTable mine = tab;                                          // (a few KB .. MB: max_uniq * 4 slots)
        const long long a = prefix + t * per, b = std::min(n, a + per);
        unsigned long long last = 0;
        long long last_id = -1;
        for (long long i = a; i < b; ++i) {
            const unsigned long long x = w[i];
            if (x == last && last_id >= 0) { ids[i] = last_id; continue; }
            size_t slot;
            long long id = mine.find(x, &slot);
            if (id < 0) {
                if ((long long)fresh[t].size() + k >= max_uniq) { bad[t] = 1; return; }
                id = PROV + (long long)fresh[t].size();
                mine.put(slot, x, id);
                fresh[t].push_back(x);
            }
            last = x;
            last_id = id;
            ids[i] = id;
        }
    };
    {
        std::vector<std::thread> pool;
        for (int t = 1; t < T; ++t) pool.emplace_back(work, t);
        work(0);
        for (auto& th : pool) th.join();
    }
    for (int t = 0; t < T; ++t)
        if (bad[t]) return -1;
    bool any = false;
    std::vector<std::vector<long long>> rank(T);
    for (int t = 0; t < T; ++t) {                                      // threads in array order: first appearance
        rank[t].resize(fresh[t].size());
        for (size_t j = 0; j < fresh[t].size(); ++j) {
            any = true;
            size_t slot;
            long long id = tab.find(fresh[t][j], &slot);
            if (id < 0) {
                if (k >= max_uniq) return -1;
                id = k;
                tab.put(slot, fresh[t][j], id);
                uniq[k++] = (void*)fresh[t][j];
            }
            rank[t][j] = id;
        }
    }
    if (any) {
        auto fix = [&](int t) {
            if (fresh[t].empty()) return;
            const long long a = prefix + t * per, b = std::min(n, a + per);
            for (long long i = a; i < b; ++i)
                if (ids[i] >= PROV) ids[i] = rank[t][(size_t)(ids[i] - PROV)];
        };
        std::vector<std::thread> pool;
        for (int t = 1; t < T; ++t) pool.emplace_back(fix, t);
        fix(0);
        for (auto& th : pool) th.join();
    }
    return k;
}

int ghf_message_side_output_supported(int d, int block_nodes, int wlayout) {
    return wlayout == GHF_WLAYOUT_SPLIT2H && message_bx_owns(d, block_nodes) ? 1 : 0;
}

int ghf_message_layer_fwd(const float* h, const void* h_split, int64_t N, int d, const uint32_t* sorted_key, const int32_t* sorted_src,
                          const int32_t* seg_off, const int32_t* indeg, const int32_t* chunk_tab,
                          const int32_t* blk_chunk_off, const int32_t* item_tab, const int32_t* blk_item_off,
                          int64_t item0, int64_t n_items, float* partial, int64_t E, int R, int block_nodes,
                          const float* W_msg, const float* W_self, const float* bias, int wlayout,
                          const float* ln_gamma, const float* ln_beta, float ln_eps, int64_t row0, int64_t rows,
                          float* h_out, void* h_split_out, float* agg_out, int flags, void* stream) {
    GHF_REQUIRE(h && sorted_key && sorted_src && seg_off && indeg && W_msg && bias && h_out,
                "message_layer_fwd: null pointer argument");
    if (flags & GHF_FLAG_RAW_SUM) flags |= GHF_FLAG_NO_TAIL;
    GHF_REQUIRE((flags & GHF_FLAG_NO_TAIL) || (ln_gamma && ln_beta), "message_layer_fwd: LayerNorm parameters missing");
    GHF_REQUIRE(h != h_out, "message_layer_fwd: h_out must not alias h");
    GHF_REQUIRE(N > 0 && d > 0 && R > 0 && block_nodes > 0, "message_layer_fwd: N, d, R, block_nodes must be positive");
    GHF_REQUIRE(row0 >= 0 && rows >= 0 && row0 + rows <= N, "message_layer_fwd: row range [%lld,+%lld) outside [0,%lld)",
                (long long)row0, (long long)rows, (long long)N);
    GHF_REQUIRE(row0 % block_nodes == 0, "message_layer_fwd: row0 must be a multiple of block_nodes");
    GHF_REQUIRE(block_nodes == 1 || (chunk_tab && blk_chunk_off && item_tab && blk_item_off && item0 >= 0 && n_items >= 0),
                "message_layer_fwd: block plans need the chunk and item tables");
    const bool split = wlayout == GHF_WLAYOUT_SPLIT2H;
    GHF_REQUIRE(!split || h_split, "message_layer_fwd: SPLIT2H weights need h_split (ghf_split_rows)");
    GHF_REQUIRE(!h_split_out || (split && !(flags & GHF_FLAG_NO_TAIL) && h_split_out != h_split),
                "message_layer_fwd: h_split_out needs split weights and the fused tail, and must not alias h_split");
    MsgArgs a{h, h_split, N, d, sorted_key, sorted_src, seg_off, indeg, chunk_tab, blk_chunk_off, item_tab, blk_item_off, item0, n_items,
              partial, E, R, block_nodes, W_msg, W_self, bias, wlayout,
              ln_gamma, ln_beta, ln_eps, row0, rows, h_out, h_split_out, flags, agg_out};
    GHF_REQUIRE((flags & (GHF_FLAG_ZERO_SRC | GHF_FLAG_ZERO_DST)) != (GHF_FLAG_ZERO_SRC | GHF_FLAG_ZERO_DST),
                "message_layer_fwd: GHF_FLAG_ZERO_SRC and GHF_FLAG_ZERO_DST together leave nothing to compute");
    GHF_REQUIRE(!agg_out || (!(flags & GHF_FLAG_NO_TAIL) && agg_out != h_out), "message_layer_fwd: agg_out goes with the fused tail and must not alias h_out");
    GHF_REQUIRE(!(flags & GHF_FLAG_ADD_H) || (flags & (GHF_FLAG_NO_TAIL | GHF_FLAG_RAW_SUM)), "message_layer_fwd: GHF_FLAG_ADD_H goes with NO_TAIL / RAW_SUM");
    if ((flags & GHF_FLAG_ADD_H) && !ghf_message_side_output_supported(d, block_nodes, wlayout))
        return set_err(GHF_EUNSUPPORTED, "message_layer_fwd: GHF_FLAG_ADD_H is not implemented by the kernel for d=%d, block_nodes=%d, layout %d", d, block_nodes, wlayout);
    if ((flags & (GHF_FLAG_ZERO_SRC | GHF_FLAG_ZERO_DST)) && !ghf_message_side_output_supported(d, block_nodes, wlayout))
        return set_err(GHF_EUNSUPPORTED, "message_layer_fwd: GHF_FLAG_ZERO_SRC / ZERO_DST (a half of the weights that must not be read) is "
                       "not implemented by the kernel for d=%d, block_nodes=%d, layout %d: pack that half as zeros instead", d, block_nodes, wlayout);
    if (agg_out && !ghf_message_side_output_supported(d, block_nodes, wlayout))
        return set_err(GHF_EUNSUPPORTED, "message_layer_fwd: no side output from the kernel for d=%d, block_nodes=%d, layout %d", d, block_nodes, wlayout);
    if (block_nodes == 1) return launch_message_generic(a, (hipStream_t)stream);
    if (wlayout == GHF_WLAYOUT_SPLIT2H) {
        GHF_REQUIRE(message_bx_owns(d, block_nodes), "message_layer_fwd: no SPLIT2H kernel for d=%d with blocks of %d nodes", d, block_nodes);
        return launch_message_bx(a, (hipStream_t)stream);
    }
    GHF_REQUIRE(wlayout == GHF_WLAYOUT_FRAG16, "message_layer_fwd: unknown weight layout %d", wlayout);
    return launch_message_pp(a, (hipStream_t)stream);
}

size_t ghf_group_workspace_bytes(int64_t E) { return group_workspace_bytes(E); }

int ghf_group_edges(const int64_t* rel_id, int64_t E, int R, void* workspace, size_t workspace_bytes, int64_t* perm,
                    int64_t* goff, void* stream) {
    GHF_REQUIRE(rel_id && workspace && perm && goff, "group_edges: null pointer argument");
    return launch_group_edges(rel_id, E, R, workspace, workspace_bytes, perm, goff, (hipStream_t)stream);
}

size_t ghf_tail_bwd_workspace_floats(int64_t N, int d) { return (N >= 0 && d > 0) ? tail_bwd_workspace_floats(N, d) : 0; }

int ghf_tail_bwd(const float* grad_out, const float* agg, const float* h, const float* ln_gamma, float ln_eps,
                 const int32_t* indeg, int64_t N, int d, float* dpre, float* G, void* G_split, float* dgamma_dbeta,
                 float* workspace, const float* drop, void* stream) {
    GHF_REQUIRE(grad_out && agg && h && ln_gamma && indeg && dpre && G && dgamma_dbeta && workspace, "tail_bwd: null pointer argument");
    return launch_tail_bwd(grad_out, agg, h, ln_gamma, ln_eps, indeg, N, d, dpre, G, G_split, dgamma_dbeta, workspace, drop,
                           (hipStream_t)stream);
}

size_t ghf_colsum_workspace_floats(int64_t N, int d) { return colsum_workspace_floats(N, d); }

int ghf_colsum(const float* X, const float* mask, int64_t N, int d, float* workspace, float* out, int accumulate, void* stream) {
    GHF_REQUIRE(X && workspace && out, "colsum: null pointer argument");
    return launch_colsum(X, mask, N, d, workspace, out, accumulate, (hipStream_t)stream);
}

int ghf_relu_mask(const float* X, const float* ref, int64_t n, float* out, void* stream) {
    GHF_REQUIRE(X && ref && out, "relu_mask: null pointer argument");
    return launch_relu_mask(X, ref, n, out, (hipStream_t)stream);
}

int ghf_group_outer(const float* A, const int64_t* ia, int da, const float* B, const int64_t* ib, int db,
                    const int64_t* gstart, const int64_t* gend, int ngroups, float* C, int accumulate, void* stream) {
    GHF_REQUIRE((A || da == 0) && B && gstart && gend && C, "group_outer: null pointer argument");
    return launch_group_outer(A, ia, da, B, ib, db, gstart, gend, ngroups, C, accumulate, (hipStream_t)stream);
}

int ghf_message_rs_supported(int d) { return message_rs_supported(d); }

int ghf_edge_transform_fwd(const float* h, int64_t N, int d, const int64_t* src, const int64_t* dst, const int64_t* ypos,
                           const int64_t* slice_tab, int64_t nslices, const float* WmT, const float* WsT, const float* bias,
                           float* Y, void* stream) {
    GHF_REQUIRE(h && src && dst && ypos && slice_tab && WmT && WsT && bias && Y, "edge_transform_fwd: null pointer argument");
    return launch_edge_transform(h, N, d, src, dst, ypos, slice_tab, nslices, WmT, WsT, bias, Y, (hipStream_t)stream);
}

size_t ghf_weights_rs_bytes(int R, int d) { return weights_rs_bytes(R, d); }

int ghf_weights_pack_rs(const float* W_msg, const float* W_self, int R, int d, void* w2h, int* shift_ws, void* stream) {
    GHF_REQUIRE(W_msg && W_self && w2h && shift_ws, "weights_pack_rs: null pointer argument");
    return launch_weights_pack_rs(W_msg, W_self, R, d, w2h, shift_ws, (hipStream_t)stream);
}

int ghf_edge_transform_h_fwd(const void* h_split, int64_t N, int d, const int64_t* src, const int64_t* dst, const int64_t* ypos,
                             const int64_t* slice_tab, int64_t nslices, const void* w2h, int R, const float* bias,
                             const void* x_split, int64_t NX, const float* row_cnt, float* Y, void* stream) {
    GHF_REQUIRE(h_split && src && dst && ypos && slice_tab && w2h && bias && Y, "edge_transform_h_fwd: null pointer argument");
    GHF_REQUIRE((x_split != nullptr) == (NX > 0), "edge_transform_h_fwd: x_split and its row count go together");
    return launch_edge_transform_h(h_split, N, d, src, dst, ypos, slice_tab, nslices, w2h, R, bias, x_split, NX, row_cnt, Y,
                                   (hipStream_t)stream);
}

int ghf_run_rows_fwd(const float* h, int64_t N, int d, const int64_t* run_src, const int64_t* run_start, int64_t nruns,
                     void* x_split, void* stream) {
    GHF_REQUIRE((h && run_src && run_start && x_split) || nruns == 0, "run_rows_fwd: null pointer argument");
    return launch_run_rows(h, N, d, run_src, run_start, nruns, x_split, (hipStream_t)stream);
}

int ghf_segment_partial_fwd(const float* Y, const int64_t* hub_chunks, int64_t nchunks, int d, float* P, void* stream) {
    GHF_REQUIRE((Y && hub_chunks && P) || nchunks == 0, "segment_partial_fwd: null pointer argument");
    return launch_segment_partial(Y, hub_chunks, nchunks, d, P, (hipStream_t)stream);
}

int ghf_segment_tail_fwd(const float* Y, const int64_t* off, const int32_t* deg_of, const int32_t* hub_of, const int64_t* hub_tab, const float* P,
                         const float* h, const float* ln_gamma, const float* ln_beta, float ln_eps, int64_t row0,
                         int64_t rows, int d, float* h_out, void* h_split_out, int64_t n_split, int flags, void* stream) {
    GHF_REQUIRE(Y && off && h_out, "segment_tail_fwd: null pointer argument");
    GHF_REQUIRE(!hub_of || (hub_tab && P), "segment_tail_fwd: hub_of without hub_tab / P");
    GHF_REQUIRE((flags & (GHF_FLAG_NO_TAIL | GHF_FLAG_RAW_SUM)) || (h && ln_gamma && ln_beta), "segment_tail_fwd: tail inputs missing");
    GHF_REQUIRE(!h_split_out || n_split >= row0 + rows, "segment_tail_fwd: h_split_out has fewer rows than the range written");
    return launch_segment_tail(Y, off, deg_of, hub_of, hub_tab, P, h, ln_gamma, ln_beta, ln_eps, row0, rows, d, h_out, h_split_out,
                               n_split, flags, (hipStream_t)stream);
}

int ghf_edge_outer_supported(int d) { return edge_outer_supported(d); }

int ghf_edge_outer(const float* h, const float* G, const int64_t* src, const int64_t* dst, const int64_t* slice_tab,
                   const int64_t* slice_off, const int32_t* order, int64_t nslices, int R, int d, int64_t N, float* workspace,
                   float* dW, float* db, void* stream) {
    GHF_REQUIRE(h && G && src && dst && slice_tab && slice_off && workspace && dW && db, "edge_outer: null pointer argument");
    return launch_edge_outer(h, G, src, dst, slice_tab, slice_off, nslices, R, d, N, workspace, dW, db, (hipStream_t)stream, nullptr,
                             nullptr, order);
}

int ghf_edge_outer_scaled(const float* h, const float* G, const float* h_rowscale, const float* G_rowscale, const int64_t* src,
                          const int64_t* dst, const int64_t* slice_tab, const int64_t* slice_off, const int32_t* order,
                          int64_t nslices, int R, int d, int64_t N, float* workspace, float* dW, float* db, void* stream) {
    GHF_REQUIRE(h && G && h_rowscale && G_rowscale && src && dst && slice_tab && slice_off && workspace && dW && db,
                "edge_outer_scaled: null pointer argument");
    GHF_REQUIRE(N > 0, "edge_outer_scaled: N = %lld (the exact chain has no use for row scales: ghf_edge_outer with N <= 0)", (long long)N);
    return launch_edge_outer(h, G, src, dst, slice_tab, slice_off, nslices, R, d, N, workspace, dW, db, (hipStream_t)stream,
                             h_rowscale, G_rowscale, order);
}

int ghf_scale_exp(const float* X, int64_t n, const float* log_scale, float* out, void* stream) {
    GHF_REQUIRE((X && log_scale && out) || n == 0, "scale_exp: null pointer argument");
    return n > 0 ? launch_scale_exp(X, n, log_scale, out, (hipStream_t)stream) : GHF_OK;
}

int ghf_add3(const float* a, const float* b, const float* c, int64_t n, float* out, void* stream) {
    GHF_REQUIRE((a && b && out) || n == 0, "add3: null pointer argument");
    return n > 0 ? launch_add3(a, b, c, n, out, (hipStream_t)stream) : GHF_OK;
}

int ghf_rowscale(const float* X, const float* g, int64_t n, int d, float* out, void* stream) {
    GHF_REQUIRE((X && g && out) || n == 0, "rowscale: null pointer argument");
    return n > 0 ? launch_rowscale(X, g, n, d, out, (hipStream_t)stream) : GHF_OK;
}

int ghf_segment_axpy(const float* w, const int64_t* iw, const float* X, const int64_t* ix, const int64_t* off, int64_t nseg,
                     int64_t nx, int d, float* out, void* stream) {
    GHF_REQUIRE((w && iw && X && ix && off && out) || nseg == 0, "segment_axpy: null pointer argument");
    return launch_segment_axpy(w, iw, X, ix, off, nseg, nx, d, out, (hipStream_t)stream);
}

int ghf_dot(const float* X, const float* Y, int64_t n, float* workspace, float* out, void* stream) {
    GHF_REQUIRE(X && Y && workspace && out, "dot: null pointer argument");
    return launch_dot(X, Y, n, workspace, out, (hipStream_t)stream);
}

int ghf_weightgen_acts(const float* text_emb, const float* const* head_params, int R, int T, int Hh, int num_hidden,
                       float* acts, const float* hidden_drop, void* stream) {
    GHF_REQUIRE(text_emb && head_params && (acts || num_hidden == 0), "weightgen_acts: null pointer argument");
    return launch_weightgen_acts(text_emb, head_params, R, T, Hh, num_hidden, acts, hidden_drop, (hipStream_t)stream);
}

int ghf_weightgen_bwd_supported(int T, int Hh, int num_hidden) { return weightgen_bwd_supported(T, Hh, num_hidden); }

size_t ghf_weightgen_bwd_workspace_floats(int R, int T, int Hh, int num_hidden, int d_in, int d_out) {
    return weightgen_bwd_workspace_floats(R, T, Hh, num_hidden, d_in, d_out);
}

int ghf_weightgen_bwd(const float* text_emb, const float* const* head_params, const float* acts, const float* const* outs,
                      const float* const* grads, const float* const* log_scales, int R, int T, int Hh, int num_hidden, int d_in,
                      int d_out, const float* log_keep, float* const* dparams, float* const* dls, float* d_text_emb,
                      float* workspace, void* stream) {
    GHF_REQUIRE(text_emb && head_params && outs && grads && log_scales && dparams && dls && workspace,
                "weightgen_bwd: null pointer argument");
    return launch_weightgen_bwd(text_emb, head_params, acts, outs, grads, log_scales, R, T, Hh, num_hidden, d_in, d_out, log_keep,
                                dparams, dls, d_text_emb, workspace, (hipStream_t)stream);
}

int ghf_text_encode_bwd(const int32_t* ids, const int32_t* lens, int U, int Lmax, const float* char_emb, int V, int C,
                        const float* W, int T, const float* te, const float* dte, float* workspace, float* d_char_emb,
                        float* dW, float* db, void* stream) {
    GHF_REQUIRE(ids && lens && char_emb && W && te && dte && workspace && d_char_emb && dW && db, "text_encode_bwd: null pointer argument");
    return launch_text_encode_bwd(ids, lens, U, Lmax, char_emb, V, C, W, T, te, dte, workspace, d_char_emb, dW, db,
                                  (hipStream_t)stream);
}

int ghf_transpose_batched(const float* in, int batch, int rows, int cols, float* out, void* stream) {
    GHF_REQUIRE(in && out && in != out, "transpose_batched: null or aliased pointers");
    return launch_transpose_batched(in, batch, rows, cols, out, (hipStream_t)stream);
}

int ghf_weights_pack(const float* top, const float* bottom, int transpose, int R, int d, int wlayout, float* out, void* stream) {
    return launch_weights_pack(top, bottom, transpose, R, d, wlayout, out, (hipStream_t)stream);
}

int ghf_rows_pack(const void* rows, int64_t row_bytes, const void* extra, int64_t extra_bytes, const int64_t* idx, int64_t n,
                  int64_t nrows, void* packed, void* stream) {
    GHF_REQUIRE(rows && ((idx && packed) || n == 0), "rows_pack: null pointer argument");   // (an empty message has no address)
    return launch_rows_pack(false, (void*)rows, row_bytes, (void*)extra, extra_bytes, idx, n, nrows, packed, (hipStream_t)stream);
}

int ghf_rows_unpack(const void* packed, const int64_t* idx, int64_t n, int64_t nrows, void* rows, int64_t row_bytes, void* extra,
                    int64_t extra_bytes, void* stream) {
    GHF_REQUIRE(rows && ((idx && packed) || n == 0), "rows_unpack: null pointer argument");
    return launch_rows_pack(true, rows, row_bytes, extra, extra_bytes, idx, n, nrows, (void*)packed, (hipStream_t)stream);
}

int ghf_rows_accumulate(const float* packed, const int64_t* idx, int64_t n, int64_t nrows, float* rows, int d, void* stream) {
    GHF_REQUIRE(rows && (packed || n == 0), "rows_accumulate: null pointer argument");
    return launch_rows_accumulate(packed, idx, n, nrows, rows, d, (hipStream_t)stream);
}

int ghf_rows_accumulate_any(const float* packed, const int64_t* idx, int64_t n, int64_t nrows, float* rows, int d, void* stream) {
    GHF_REQUIRE(rows && (packed || n == 0), "rows_accumulate_any: null pointer argument");
    return launch_rows_accumulate(packed, idx, n, nrows, rows, d, (hipStream_t)stream, true);
}

size_t ghf_subgraph_workspace_bytes(int64_t N, int64_t E, int k) { return subgraph_workspace_bytes(N, E, k); }

int ghf_subgraph_hops(const uint32_t* sorted_key, const int32_t* sorted_src, int64_t N, int64_t E, int R, int block_nodes,
                      const int64_t* seeds, int64_t S, int k, void* workspace, size_t workspace_bytes, int32_t* dist, void* stream) {
    GHF_REQUIRE(workspace && dist && (seeds || S == 0) && ((sorted_key && sorted_src) || E == 0),
                "subgraph_hops: null pointer argument");
    return launch_subgraph_hops(sorted_key, sorted_src, N, E, R, block_nodes, seeds, S, k, workspace, workspace_bytes, dist,
                                nullptr, 0, 0, (hipStream_t)stream);
}

int ghf_subgraph_nodes(const int32_t* dist, int64_t N, int k, void* workspace, size_t workspace_bytes, int64_t* node_list,
                       int64_t* new_id, int64_t* m, void* stream) {
    GHF_REQUIRE(dist && workspace && node_list && new_id && m, "subgraph_nodes: null pointer argument");
    return launch_subgraph_nodes(dist, N, k, workspace, workspace_bytes, node_list, new_id, m, (hipStream_t)stream);
}

int ghf_subgraph_edges(const uint32_t* sorted_key, const int32_t* sorted_src, int64_t N, int64_t E, int R, int block_nodes,
                       const int32_t* dist, const int64_t* new_id, int k, void* workspace, size_t workspace_bytes,
                       int64_t* edge_out, int64_t* rel_out, int64_t* num_edges, void* stream) {
    GHF_REQUIRE(dist && new_id && workspace && num_edges && ((sorted_key && sorted_src && edge_out && rel_out) || E == 0),
                "subgraph_edges: null pointer argument");
    return launch_subgraph_edges(sorted_key, sorted_src, N, E, R, block_nodes, dist, new_id, k, workspace, workspace_bytes,
                                 edge_out, rel_out, num_edges, nullptr, 0, 0, (hipStream_t)stream);
}

size_t ghf_subgraph_sample_workspace_bytes(int64_t N, int64_t E, int k) { return subgraph_sample_workspace_bytes(N, E, k); }

int ghf_subgraph_sample_hops(const uint32_t* sorted_key, const int32_t* sorted_src, int64_t N, int64_t E, int R, int block_nodes,
                             const int64_t* seeds, int64_t S, int k, const int* fanout, uint64_t seed, void* workspace,
                             size_t workspace_bytes, int32_t* dist, int32_t* keep, int64_t* host_reads, void* stream) {
    GHF_REQUIRE(workspace && dist && fanout && (seeds || S == 0) && ((sorted_key && sorted_src && keep) || E == 0),
                "subgraph_sample_hops: null pointer argument");
    GHF_REQUIRE(k >= 1, "subgraph_sample_hops: k must be positive");
    return launch_subgraph_sample_hops(sorted_key, sorted_src, N, E, R, block_nodes, seeds, S, k, fanout, seed, workspace,
                                       workspace_bytes, dist, keep, host_reads, nullptr, 0, 0, (hipStream_t)stream);
}

int ghf_subgraph_sample_edges(const uint32_t* sorted_key, const int32_t* sorted_src, int64_t N, int64_t E, int R, int block_nodes,
                              const int32_t* keep, const int64_t* new_id, void* workspace, size_t workspace_bytes,
                              int64_t* edge_out, int64_t* rel_out, int64_t* num_edges, void* stream) {
    GHF_REQUIRE(new_id && workspace && num_edges && ((sorted_key && sorted_src && keep && edge_out && rel_out) || E == 0),
                "subgraph_sample_edges: null pointer argument");
    return launch_subgraph_sample_edges(sorted_key, sorted_src, N, E, R, block_nodes, keep, new_id, workspace, workspace_bytes,
                                        edge_out, rel_out, num_edges, (hipStream_t)stream);
}

// the exclusion list of the *_excl calls, checked on the host before anything else is looked at
static int excl_check(const uint64_t* excl, int64_t n_excl, int typed, const char* what) {
    GHF_REQUIRE(n_excl >= 0, "%s: negative exclusion count", what);
    GHF_REQUIRE(excl || n_excl == 0, "%s: null exclusion list with n_excl = %lld", what, (long long)n_excl);
    GHF_REQUIRE(typed == 0 || typed == 1, "%s: typed = %d (needs 0 or 1)", what, typed);
    return GHF_OK;
}

int ghf_subgraph_hops_excl(const uint32_t* sorted_key, const int32_t* sorted_src, int64_t N, int64_t E, int R, int block_nodes,
                           const int64_t* seeds, int64_t S, int k, void* workspace, size_t workspace_bytes, int32_t* dist,
                           void* stream, const uint64_t* excl, int64_t n_excl, int typed) {
    const int rc = excl_check(excl, n_excl, typed, "subgraph_hops_excl");
    if (rc) return rc;
    GHF_REQUIRE(workspace && dist && (seeds || S == 0) && ((sorted_key && sorted_src) || E == 0),
                "subgraph_hops_excl: null pointer argument");
    return launch_subgraph_hops(sorted_key, sorted_src, N, E, R, block_nodes, seeds, S, k, workspace, workspace_bytes, dist,
                                excl, n_excl, typed, (hipStream_t)stream);
}

int ghf_subgraph_edges_excl(const uint32_t* sorted_key, const int32_t* sorted_src, int64_t N, int64_t E, int R, int block_nodes,
                            const int32_t* dist, const int64_t* new_id, int k, void* workspace, size_t workspace_bytes,
                            int64_t* edge_out, int64_t* rel_out, int64_t* num_edges, void* stream, const uint64_t* excl,
                            int64_t n_excl, int typed) {
    const int rc = excl_check(excl, n_excl, typed, "subgraph_edges_excl");
    if (rc) return rc;
    GHF_REQUIRE(dist && new_id && workspace && num_edges && ((sorted_key && sorted_src && edge_out && rel_out) || E == 0),
                "subgraph_edges_excl: null pointer argument");
    return launch_subgraph_edges(sorted_key, sorted_src, N, E, R, block_nodes, dist, new_id, k, workspace, workspace_bytes,
                                 edge_out, rel_out, num_edges, excl, n_excl, typed, (hipStream_t)stream);
}

int ghf_subgraph_sample_hops_excl(const uint32_t* sorted_key, const int32_t* sorted_src, int64_t N, int64_t E, int R,
                                  int block_nodes, const int64_t* seeds, int64_t S, int k, const int* fanout, uint64_t seed,
                                  void* workspace, size_t workspace_bytes, int32_t* dist, int32_t* keep, int64_t* host_reads,
                                  void* stream, const uint64_t* excl, int64_t n_excl, int typed) {
    const int rc = excl_check(excl, n_excl, typed, "subgraph_sample_hops_excl");
    if (rc) return rc;
    GHF_REQUIRE(workspace && dist && fanout && (seeds || S == 0) && ((sorted_key && sorted_src && keep) || E == 0),
                "subgraph_sample_hops_excl: null pointer argument");
    GHF_REQUIRE(k >= 1, "subgraph_sample_hops_excl: k must be positive");
    return launch_subgraph_sample_hops(sorted_key, sorted_src, N, E, R, block_nodes, seeds, S, k, fanout, seed, workspace,
                                       workspace_bytes, dist, keep, host_reads, excl, n_excl, typed, (hipStream_t)stream);
}

int ghf_score_pairs_fwd(const float* a, const float* b, const int64_t* ia, const int64_t* ib, int64_t rows_a, int64_t rows_b,
                        int64_t n, int d, float* scores, void* stream) {
    GHF_REQUIRE(a && b && (scores || n == 0), "score_pairs_fwd: null pointer argument");
    return launch_score_pairs(a, b, ia, ib, rows_a, rows_b, n, d, scores, (hipStream_t)stream);
}

// What the six ghf_score_* calls check before they launch, in this order.  `ptrs`: every pointer the call needs is there;
// `noun`: what its lists are ("filter" or "positive"); an operation without a scale or smoothing passes 1 and 0.
static int score_entry_check(const char* op, const char* noun, bool ptrs, const int64_t* list_ptr, const int64_t* list_idx,
                             int64_t nnz, float scale, float smoothing, const void* workspace) {
    GHF_REQUIRE(ptrs && workspace, "%s: null pointer argument", op);
    GHF_REQUIRE(nnz <= 0 || (list_ptr && list_idx), "%s: null %s list with nnz > 0", op, noun);
    GHF_REQUIRE(scale > 0.f && scale <= 3.402823466e38f, "%s: scale must be finite and positive", op);
    GHF_REQUIRE(smoothing >= 0.f && smoothing < 1.f, "%s: smoothing must be in [0, 1)", op);
    GHF_REQUIRE(((uintptr_t)workspace & 255) == 0, "%s: workspace not 256-byte aligned", op);
    return GHF_OK;
}

size_t ghf_score_rank_workspace_bytes(int64_t B, int64_t N, int d) { return score_rank_workspace_bytes(B, N, d); }

int ghf_score_rank(const float* q, const float* c, const int64_t* iq, const int64_t* target, const int64_t* filt_ptr,
                   const int64_t* filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d, void* workspace,
                   size_t workspace_bytes, int64_t* greater, int64_t* equal, void* stream) {
    const int rc = score_entry_check("score_rank", "filter", q && c && target && greater && equal, filt_ptr, filt_idx, nnz, 1.f, 0.f,
                                     workspace);
    if (rc != GHF_OK) return rc;
    return launch_score_rank(q, c, iq, target, filt_ptr, filt_idx, nnz, rows_q, N, B, d, workspace, workspace_bytes, greater, equal,
                             (hipStream_t)stream);
}

size_t ghf_score_topk_workspace_bytes(int64_t B, int64_t N, int d, int k) { return score_topk_workspace_bytes(B, N, d, k); }

int ghf_score_topk(const float* q, const float* c, const int64_t* iq, const int64_t* filt_ptr, const int64_t* filt_idx,
                   int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d, int k, void* workspace, size_t workspace_bytes,
                   float* scores, int64_t* ids, void* stream) {
    const int rc = score_entry_check("score_topk", "filter", q && c && scores && ids, filt_ptr, filt_idx, nnz, 1.f, 0.f, workspace);
    if (rc != GHF_OK) return rc;
    return launch_score_topk(q, c, iq, filt_ptr, filt_idx, nnz, rows_q, N, B, d, k, workspace, workspace_bytes, scores, ids,
                             (hipStream_t)stream);
}

size_t ghf_score_softmax_workspace_bytes(int64_t B, int64_t N, int d) { return score_softmax_workspace_bytes(B, N, d); }

int ghf_score_softmax_fwd(const float* q, const float* c, const int64_t* iq, const int64_t* target, const int64_t* filt_ptr,
                          const int64_t* filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d, float scale,
                          void* workspace, size_t workspace_bytes, float* loss, float* lse, void* stream) {
    const int rc = score_entry_check("score_softmax_fwd", "filter", q && c && target && loss && lse, filt_ptr, filt_idx, nnz, scale, 0.f,
                                     workspace);
    if (rc != GHF_OK) return rc;
    return launch_score_softmax_fwd(q, c, iq, target, filt_ptr, filt_idx, nnz, rows_q, N, B, d, scale, workspace, workspace_bytes,
                                    loss, lse, (hipStream_t)stream);
}

size_t ghf_score_softmax_bwd_workspace_bytes(int64_t B, int64_t N, int d) { return score_softmax_bwd_workspace_bytes(B, N, d); }

int ghf_score_softmax_bwd(const float* q, const float* c, const int64_t* iq, const int64_t* target, const int64_t* filt_ptr,
                          const int64_t* filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d, float scale,
                          const float* lse, const float* grad_loss, void* workspace, size_t workspace_bytes, float* dq, float* dc,
                          void* stream) {
    const int rc = score_entry_check("score_softmax_bwd", "filter", q && c && target && lse && grad_loss && dq && dc, filt_ptr, filt_idx,
                                     nnz, scale, 0.f, workspace);
    if (rc != GHF_OK) return rc;
    return launch_score_softmax_bwd(q, c, iq, target, filt_ptr, filt_idx, nnz, rows_q, N, B, d, scale, lse, grad_loss, workspace,
                                    workspace_bytes, dq, dc, (hipStream_t)stream);
}

size_t ghf_score_bce_workspace_bytes(int64_t B, int64_t N, int d) { return score_bce_workspace_bytes(B, N, d); }

int ghf_score_bce_fwd(const float* q, const float* c, const int64_t* iq, const int64_t* pos_ptr, const int64_t* pos_idx, int64_t nnz,
                      int64_t rows_q, int64_t N, int64_t B, int d, float scale, float smoothing, void* workspace,
                      size_t workspace_bytes, float* loss, void* stream) {
    const int rc = score_entry_check("score_bce_fwd", "positive", q && c && loss, pos_ptr, pos_idx, nnz, scale, smoothing, workspace);
    if (rc != GHF_OK) return rc;
    return launch_score_bce_fwd(q, c, iq, pos_ptr, pos_idx, nnz, rows_q, N, B, d, scale, smoothing, workspace, workspace_bytes, loss,
                                (hipStream_t)stream);
}

size_t ghf_score_bce_bwd_workspace_bytes(int64_t B, int64_t N, int d) { return score_bce_bwd_workspace_bytes(B, N, d); }

int ghf_score_bce_bwd(const float* q, const float* c, const int64_t* iq, const int64_t* pos_ptr, const int64_t* pos_idx, int64_t nnz,
                      int64_t rows_q, int64_t N, int64_t B, int d, float scale, float smoothing, const float* loss,
                      const float* grad_loss, void* workspace, size_t workspace_bytes, float* dq, float* dc, void* stream) {
    const int rc = score_entry_check("score_bce_bwd", "positive", q && c && loss && grad_loss && dq && dc, pos_ptr, pos_idx, nnz, scale,
                                     smoothing, workspace);
    if (rc != GHF_OK) return rc;
    return launch_score_bce_bwd(q, c, iq, pos_ptr, pos_idx, nnz, rows_q, N, B, d, scale, smoothing, loss, grad_loss, workspace,
                                workspace_bytes, dq, dc, (hipStream_t)stream);
}

// the same six against a candidate subset (candidates.hip): score_entry_check, then the list itself
#define GHF_SUB_CHECK(op) GHF_REQUIRE(ic && C > 0 && C <= N, op ": need ic and 1 <= C <= N")

size_t ghf_score_rank_sub_workspace_bytes(int64_t B, int64_t C, int d, int64_t nnz) {
    return score_rank_sub_workspace_bytes(B, C, d, nnz);
}

int ghf_score_rank_sub(const float* q, const float* c, const int64_t* iq, const int64_t* target, const int64_t* filt_ptr,
                       const int64_t* filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d, const int64_t* ic,
                       int64_t C, void* workspace, size_t workspace_bytes, int64_t* greater, int64_t* equal, void* stream) {
    const int rc = score_entry_check("score_rank_sub", "filter", q && c && target && greater && equal, filt_ptr, filt_idx, nnz, 1.f,
                                     0.f, workspace);
    if (rc != GHF_OK) return rc;
    GHF_SUB_CHECK("score_rank_sub");
    return launch_score_rank(q, c, iq, target, filt_ptr, filt_idx, nnz, rows_q, N, B, d, workspace, workspace_bytes, greater, equal,
                             (hipStream_t)stream, ic, C);
}

size_t ghf_score_topk_sub_workspace_bytes(int64_t B, int64_t C, int d, int k, int64_t nnz) {
    return score_topk_sub_workspace_bytes(B, C, d, k, nnz);
}

int ghf_score_topk_sub(const float* q, const float* c, const int64_t* iq, const int64_t* filt_ptr, const int64_t* filt_idx,
                       int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d, int k, const int64_t* ic, int64_t C,
                       void* workspace, size_t workspace_bytes, float* scores, int64_t* ids, void* stream) {
    const int rc = score_entry_check("score_topk_sub", "filter", q && c && scores && ids, filt_ptr, filt_idx, nnz, 1.f, 0.f, workspace);
    if (rc != GHF_OK) return rc;
    GHF_SUB_CHECK("score_topk_sub");
    return launch_score_topk(q, c, iq, filt_ptr, filt_idx, nnz, rows_q, N, B, d, k, workspace, workspace_bytes, scores, ids,
                             (hipStream_t)stream, ic, C);
}

size_t ghf_score_softmax_sub_workspace_bytes(int64_t B, int64_t C, int d, int64_t nnz) {
    return score_softmax_sub_workspace_bytes(B, C, d, nnz);
}

int ghf_score_softmax_fwd_sub(const float* q, const float* c, const int64_t* iq, const int64_t* target, const int64_t* filt_ptr,
                              const int64_t* filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d, float scale,
                              const int64_t* ic, int64_t C, void* workspace, size_t workspace_bytes, float* loss, float* lse,
                              void* stream) {
    const int rc = score_entry_check("score_softmax_fwd_sub", "filter", q && c && target && loss && lse, filt_ptr, filt_idx, nnz, scale,
                                     0.f, workspace);
    if (rc != GHF_OK) return rc;
    GHF_SUB_CHECK("score_softmax_fwd_sub");
    return launch_score_softmax_fwd(q, c, iq, target, filt_ptr, filt_idx, nnz, rows_q, N, B, d, scale, workspace, workspace_bytes,
                                    loss, lse, (hipStream_t)stream, ic, C);
}

size_t ghf_score_softmax_bwd_sub_workspace_bytes(int64_t B, int64_t C, int d, int64_t nnz) {
    return score_softmax_bwd_sub_workspace_bytes(B, C, d, nnz);
}

int ghf_score_softmax_bwd_sub(const float* q, const float* c, const int64_t* iq, const int64_t* target, const int64_t* filt_ptr,
                              const int64_t* filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d, float scale,
                              const float* lse, const float* grad_loss, const int64_t* ic, int64_t C, void* workspace,
                              size_t workspace_bytes, float* dq, float* dc, void* stream) {
    const int rc = score_entry_check("score_softmax_bwd_sub", "filter", q && c && target && lse && grad_loss && dq && dc, filt_ptr,
                                     filt_idx, nnz, scale, 0.f, workspace);
    if (rc != GHF_OK) return rc;
    GHF_SUB_CHECK("score_softmax_bwd_sub");
    return launch_score_softmax_bwd(q, c, iq, target, filt_ptr, filt_idx, nnz, rows_q, N, B, d, scale, lse, grad_loss, workspace,
                                    workspace_bytes, dq, dc, (hipStream_t)stream, ic, C);
}

size_t ghf_score_bce_sub_workspace_bytes(int64_t B, int64_t C, int d, int64_t nnz) {
    return score_bce_sub_workspace_bytes(B, C, d, nnz);
}

int ghf_score_bce_fwd_sub(const float* q, const float* c, const int64_t* iq, const int64_t* pos_ptr, const int64_t* pos_idx,
                          int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d, float scale, float smoothing, const int64_t* ic,
                          int64_t C, void* workspace, size_t workspace_bytes, float* loss, void* stream) {
    const int rc = score_entry_check("score_bce_fwd_sub", "positive", q && c && loss, pos_ptr, pos_idx, nnz, scale, smoothing,
                                     workspace);
    if (rc != GHF_OK) return rc;
    GHF_SUB_CHECK("score_bce_fwd_sub");
    return launch_score_bce_fwd(q, c, iq, pos_ptr, pos_idx, nnz, rows_q, N, B, d, scale, smoothing, workspace, workspace_bytes, loss,
                                (hipStream_t)stream, ic, C);
}

size_t ghf_score_bce_bwd_sub_workspace_bytes(int64_t B, int64_t C, int d, int64_t nnz) {
    return score_bce_bwd_sub_workspace_bytes(B, C, d, nnz);
}

int ghf_score_bce_bwd_sub(const float* q, const float* c, const int64_t* iq, const int64_t* pos_ptr, const int64_t* pos_idx,
                          int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d, float scale, float smoothing, const float* loss,
                          const float* grad_loss, const int64_t* ic, int64_t C, void* workspace, size_t workspace_bytes, float* dq,
                          float* dc, void* stream) {
    const int rc = score_entry_check("score_bce_bwd_sub", "positive", q && c && loss && grad_loss && dq && dc, pos_ptr, pos_idx, nnz,
                                     scale, smoothing, workspace);
    if (rc != GHF_OK) return rc;
    GHF_SUB_CHECK("score_bce_bwd_sub");
    return launch_score_bce_bwd(q, c, iq, pos_ptr, pos_idx, nnz, rows_q, N, B, d, scale, smoothing, loss, grad_loss, workspace,
                                workspace_bytes, dq, dc, (hipStream_t)stream, ic, C);
}

#undef GHF_SUB_CHECK

// the same six with a per-candidate bias (include/ghf.h): ic = NULL with C = 0 is every node, otherwise the
// subset's rules; the bias itself is required
#define GHF_BIAS_CHECK(op)                                                                              \
    do {                                                                                                \
        GHF_REQUIRE(bias, op ": null bias");                                                            \
        GHF_REQUIRE(ic ? (C > 0 && C <= N) : C == 0, op ": need ic and 1 <= C <= N, or ic = NULL and C = 0"); \
    } while (0)

size_t ghf_score_rank_b_workspace_bytes(int64_t B, int64_t N, int64_t C, int d, int64_t nnz) {
    return score_rank_b_workspace_bytes(B, N, C, d, nnz);
}

int ghf_score_rank_b(const float* q, const float* c, const int64_t* iq, const int64_t* target, const int64_t* filt_ptr,
                     const int64_t* filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d, const int64_t* ic,
                     int64_t C, const float* bias, void* workspace, size_t workspace_bytes, int64_t* greater, int64_t* equal,
                     void* stream) {
    const int rc = score_entry_check("score_rank_b", "filter", q && c && target && greater && equal, filt_ptr, filt_idx, nnz, 1.f,
                                     0.f, workspace);
    if (rc != GHF_OK) return rc;
    GHF_BIAS_CHECK("score_rank_b");
    return launch_score_rank(q, c, iq, target, filt_ptr, filt_idx, nnz, rows_q, N, B, d, workspace, workspace_bytes, greater, equal,
                             (hipStream_t)stream, ic, C, bias);
}

size_t ghf_score_topk_b_workspace_bytes(int64_t B, int64_t N, int64_t C, int d, int k, int64_t nnz) {
    return score_topk_b_workspace_bytes(B, N, C, d, k, nnz);
}

int ghf_score_topk_b(const float* q, const float* c, const int64_t* iq, const int64_t* filt_ptr, const int64_t* filt_idx,
                     int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d, int k, const int64_t* ic, int64_t C,
                     const float* bias, void* workspace, size_t workspace_bytes, float* scores, int64_t* ids, void* stream) {
    const int rc = score_entry_check("score_topk_b", "filter", q && c && scores && ids, filt_ptr, filt_idx, nnz, 1.f, 0.f, workspace);
    if (rc != GHF_OK) return rc;
    GHF_BIAS_CHECK("score_topk_b");
    return launch_score_topk(q, c, iq, filt_ptr, filt_idx, nnz, rows_q, N, B, d, k, workspace, workspace_bytes, scores, ids,
                             (hipStream_t)stream, ic, C, bias);
}

size_t ghf_score_softmax_b_workspace_bytes(int64_t B, int64_t N, int64_t C, int d, int64_t nnz) {
    return score_softmax_b_workspace_bytes(B, N, C, d, nnz);
}

int ghf_score_softmax_fwd_b(const float* q, const float* c, const int64_t* iq, const int64_t* target, const int64_t* filt_ptr,
                            const int64_t* filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d, float scale,
                            const int64_t* ic, int64_t C, const float* bias, void* workspace, size_t workspace_bytes, float* loss,
                            float* lse, void* stream) {
    const int rc = score_entry_check("score_softmax_fwd_b", "filter", q && c && target && loss && lse, filt_ptr, filt_idx, nnz, scale,
                                     0.f, workspace);
    if (rc != GHF_OK) return rc;
    GHF_BIAS_CHECK("score_softmax_fwd_b");
    return launch_score_softmax_fwd(q, c, iq, target, filt_ptr, filt_idx, nnz, rows_q, N, B, d, scale, workspace, workspace_bytes,
                                    loss, lse, (hipStream_t)stream, ic, C, bias);
}

size_t ghf_score_softmax_bwd_b_workspace_bytes(int64_t B, int64_t N, int64_t C, int d, int64_t nnz) {
    return score_softmax_bwd_b_workspace_bytes(B, N, C, d, nnz);
}

int ghf_score_softmax_bwd_b(const float* q, const float* c, const int64_t* iq, const int64_t* target, const int64_t* filt_ptr,
                            const int64_t* filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d, float scale,
                            const float* lse, const float* grad_loss, const int64_t* ic, int64_t C, const float* bias,
                            void* workspace, size_t workspace_bytes, float* dq, float* dc, float* db, void* stream) {
    const int rc = score_entry_check("score_softmax_bwd_b", "filter", q && c && target && lse && grad_loss && dq && dc, filt_ptr,
                                     filt_idx, nnz, scale, 0.f, workspace);
    if (rc != GHF_OK) return rc;
    GHF_BIAS_CHECK("score_softmax_bwd_b");
    return launch_score_softmax_bwd(q, c, iq, target, filt_ptr, filt_idx, nnz, rows_q, N, B, d, scale, lse, grad_loss, workspace,
                                    workspace_bytes, dq, dc, (hipStream_t)stream, ic, C, bias, db);
}

size_t ghf_score_bce_b_workspace_bytes(int64_t B, int64_t N, int64_t C, int d, int64_t nnz) {
    return score_bce_b_workspace_bytes(B, N, C, d, nnz);
}

int ghf_score_bce_fwd_b(const float* q, const float* c, const int64_t* iq, const int64_t* pos_ptr, const int64_t* pos_idx,
                        int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d, float scale, float smoothing, const int64_t* ic,
                        int64_t C, const float* bias, void* workspace, size_t workspace_bytes, float* loss, void* stream) {
    const int rc = score_entry_check("score_bce_fwd_b", "positive", q && c && loss, pos_ptr, pos_idx, nnz, scale, smoothing, workspace);
    if (rc != GHF_OK) return rc;
    GHF_BIAS_CHECK("score_bce_fwd_b");
    return launch_score_bce_fwd(q, c, iq, pos_ptr, pos_idx, nnz, rows_q, N, B, d, scale, smoothing, workspace, workspace_bytes, loss,
                                (hipStream_t)stream, ic, C, bias);
}

size_t ghf_score_bce_bwd_b_workspace_bytes(int64_t B, int64_t N, int64_t C, int d, int64_t nnz) {
    return score_bce_bwd_b_workspace_bytes(B, N, C, d, nnz);
}

int ghf_score_bce_bwd_b(const float* q, const float* c, const int64_t* iq, const int64_t* pos_ptr, const int64_t* pos_idx,
                        int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d, float scale, float smoothing, const float* loss,
                        const float* grad_loss, const int64_t* ic, int64_t C, const float* bias, void* workspace,
                        size_t workspace_bytes, float* dq, float* dc, float* db, void* stream) {
    const int rc = score_entry_check("score_bce_bwd_b", "positive", q && c && loss && grad_loss && dq && dc, pos_ptr, pos_idx, nnz,
                                     scale, smoothing, workspace);
    if (rc != GHF_OK) return rc;
    GHF_BIAS_CHECK("score_bce_bwd_b");
    return launch_score_bce_bwd(q, c, iq, pos_ptr, pos_idx, nnz, rows_q, N, B, d, scale, smoothing, loss, grad_loss, workspace,
                                workspace_bytes, dq, dc, (hipStream_t)stream, ic, C, bias, db);
}

#undef GHF_BIAS_CHECK

// the negative-sampling loss (include/ghf.h): one general form per call — ic = NULL with C = 0 is every node,
// bias = NULL none.  score_entry_check, then its own two floats and the pairing of ic and C.
#define GHF_NEGSAMP_CHECK(op)                                                                                       \
    do {                                                                                                            \
        GHF_REQUIRE(margin >= -3.402823466e38f && margin <= 3.402823466e38f, op ": margin must be finite");         \
        GHF_REQUIRE(adv_temperature >= 0.f && adv_temperature <= 3.402823466e38f,                                    \
                    op ": adv_temperature must be finite and not negative");                                        \
        GHF_REQUIRE(ic ? (C > 0 && C <= N) : C == 0, op ": need ic and 1 <= C <= N, or ic = NULL and C = 0");        \
    } while (0)

size_t ghf_score_negsamp_workspace_bytes(int64_t B, int64_t N, int64_t C, int d, int64_t nnz) {
    return score_negsamp_workspace_bytes(B, N, C, d, nnz);
}

int ghf_score_negsamp_fwd(const float* q, const float* c, const int64_t* iq, const int64_t* target, const int64_t* filt_ptr,
                          const int64_t* filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d, float scale,
                          float margin, float adv_temperature, const int64_t* ic, int64_t C, const float* bias, void* workspace,
                          size_t workspace_bytes, float* loss, float* lw, void* stream) {
    const int rc = score_entry_check("score_negsamp_fwd", "filter", q && c && target && loss && lw, filt_ptr, filt_idx, nnz, scale, 0.f,
                                     workspace);
    if (rc != GHF_OK) return rc;
    GHF_NEGSAMP_CHECK("score_negsamp_fwd");
    return launch_score_negsamp_fwd(q, c, iq, target, filt_ptr, filt_idx, nnz, rows_q, N, B, d, scale, margin, adv_temperature, ic, C,
                                    bias, workspace, workspace_bytes, loss, lw, (hipStream_t)stream);
}

size_t ghf_score_negsamp_bwd_workspace_bytes(int64_t B, int64_t N, int64_t C, int d, int64_t nnz) {
    return score_negsamp_bwd_workspace_bytes(B, N, C, d, nnz);
}

int ghf_score_negsamp_bwd(const float* q, const float* c, const int64_t* iq, const int64_t* target, const int64_t* filt_ptr,
                          const int64_t* filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d, float scale,
                          float margin, float adv_temperature, const float* lw, const float* grad_loss, const int64_t* ic,
                          int64_t C, const float* bias, void* workspace, size_t workspace_bytes, float* dq, float* dc, float* db,
                          void* stream) {
    const int rc = score_entry_check("score_negsamp_bwd", "filter", q && c && target && lw && grad_loss && dq && dc, filt_ptr,
                                     filt_idx, nnz, scale, 0.f, workspace);
    if (rc != GHF_OK) return rc;
    GHF_NEGSAMP_CHECK("score_negsamp_bwd");
    return launch_score_negsamp_bwd(q, c, iq, target, filt_ptr, filt_idx, nnz, rows_q, N, B, d, scale, margin, adv_temperature, lw,
                                    grad_loss, ic, C, bias, workspace, workspace_bytes, dq, dc, bias ? db : nullptr, (hipStream_t)stream);
}

#undef GHF_NEGSAMP_CHECK

// the pairwise ranking losses by dot product against every node or a shared candidate set (include/ghf_pairwise_dot_sweep.h;
// DESIGN.md §28): the refusals that stand ahead of the launches' own (score_pair_open), in the header's order.  The public
// kind becomes the launches' `hinge` here, once.
#define GHF_SCORE_PAIR_ENTRY(op, ptrs)                                                                                         \
    do {                                                                                                                       \
        GHF_REQUIRE(kind == GHF_PAIR_HINGE || kind == GHF_PAIR_LOGISTIC, op ": kind must be GHF_PAIR_HINGE or GHF_PAIR_LOGISTIC"); \
        GHF_REQUIRE(scale > 0.f && scale <= 3.402823466e38f, op ": scale must be finite and positive");                        \
        GHF_REQUIRE(margin >= -3.402823466e38f && margin <= 3.402823466e38f, op ": margin must be finite");                    \
        GHF_REQUIRE(normalize == 0 || normalize == 1, op ": normalize must be 0 or 1");                                        \
        GHF_REQUIRE((ptrs) && workspace, op ": null pointer argument");                                                        \
        GHF_REQUIRE(nnz <= 0 || (filt_ptr && filt_idx), op ": null filter list with nnz > 0");                                 \
        GHF_REQUIRE(((uintptr_t)workspace & 255) == 0, op ": workspace not 256-byte aligned");                                 \
    } while (0)

size_t ghf_score_pair_fwd_workspace_bytes(int64_t B, int64_t N, int64_t C, int d, int64_t nnz) {
    return score_pair_workspace_bytes(B, N, C, d, nnz);
}

int ghf_score_pair_fwd(int kind, const float* q, const float* c, const int64_t* iq, const int64_t* target, const int64_t* filt_ptr,
                       const int64_t* filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d, float scale, float margin,
                       int normalize, const int64_t* ic, int64_t C, const float* bias, void* workspace, size_t workspace_bytes,
                       float* loss, float* dsum, int32_t* count, int32_t* active, void* stream) {
    GHF_SCORE_PAIR_ENTRY("score_pair_fwd", q && c && target && loss && dsum && count && active);
    return launch_score_pair_fwd(kind == GHF_PAIR_HINGE, q, c, iq, target, filt_ptr, filt_idx, nnz, rows_q, N, B, d, scale, margin,
                                 normalize, ic, C, bias, workspace, workspace_bytes, loss, dsum, count, active, (hipStream_t)stream);
}

size_t ghf_score_pair_bwd_workspace_bytes(int64_t B, int64_t N, int64_t C, int d, int64_t nnz) {
    return score_pair_bwd_workspace_bytes(B, N, C, d, nnz);
}

int ghf_score_pair_bwd(int kind, const float* q, const float* c, const int64_t* iq, const int64_t* target, const int64_t* filt_ptr,
                       const int64_t* filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d, float scale, float margin,
                       int normalize, const int64_t* ic, int64_t C, const float* bias, const float* dsum, const int32_t* count,
                       const float* grad_loss, void* workspace, size_t workspace_bytes, float* dq, float* dc, float* db,
                       void* stream) {
    GHF_SCORE_PAIR_ENTRY("score_pair_bwd", q && c && target && dsum && count && grad_loss && dq && dc);
    return launch_score_pair_bwd(kind == GHF_PAIR_HINGE, q, c, iq, target, filt_ptr, filt_idx, nnz, rows_q, N, B, d, scale, margin,
                                 normalize, ic, C, bias, dsum, count, grad_loss, workspace, workspace_bytes, dq, dc, db,
                                 (hipStream_t)stream);
}

#undef GHF_SCORE_PAIR_ENTRY

// ---- the per-query family: negatives= [B, K] (the fold: §23) -----------------------------------------
// include/ghf_negatives.h (dot product), ghf_distance.h (a distance) and ghf_pairwise.h (the pairwise losses) share one entry
// helper.  Each extern "C" function below is its null-pointer expression, the translation of its public mode or kind into
// the kernels' epilogue (negatives.h: nothing past this file takes a public mode) and one call.
enum PqFamily { PQ_NEG, PQ_DIST, PQ_PAIR };

// the metric of a distance call; with `dot`, GHF_PAIR_DOT as well
static int pq_metric_check(const char* op, int metric, int d, bool dot) {
    if (dot)
        GHF_REQUIRE(metric == GHF_PAIR_DOT || metric == GHF_DIST_L1 || metric == GHF_DIST_L2 || metric == GHF_DIST_COMPLEX,
                    "%s: metric must be GHF_PAIR_DOT, GHF_DIST_L1, GHF_DIST_L2 or GHF_DIST_COMPLEX", op);
    else
        GHF_REQUIRE(metric == GHF_DIST_L1 || metric == GHF_DIST_L2 || metric == GHF_DIST_COMPLEX,
                    "%s: metric must be GHF_DIST_L1, GHF_DIST_L2 or GHF_DIST_COMPLEX", op);
    GHF_REQUIRE(metric != GHF_DIST_COMPLEX || (d & 1) == 0, "%s: GHF_DIST_COMPLEX needs an even d (re / im interleaved)", op);
    return GHF_OK;
}

// what every call of the family hands over but its outputs
static NegArgs pq_args(const float* q, const float* c, const int64_t* iq, const int64_t* target, const int64_t* filt_ptr,
                       const int64_t* filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d, float scale, float margin,
                       float alpha, const int64_t* neg, int64_t K, const float* bias) {
    NegArgs a{};
    a.q = q; a.c = c; a.iq = iq; a.target = target; a.filt_ptr = filt_ptr; a.filt_idx = filt_idx; a.nnz = nnz;
    a.neg = neg; a.K = K; a.rows_q = rows_q; a.N = N; a.B = B; a.d = d; a.bias = bias;
    a.scale = scale; a.margin = margin; a.alpha = alpha;
    return a;
}

// The refusals, in each header's order.  ghf_neg_* : score_entry_check, the mode (a backward), margin and adv_temperature (the
// negative-sampling loss), the set.  ghf_dist_*: the metric first — an unknown one is refused whatever else the call holds —
// then the same.  ghf_pair_*: the two selectors, the three scalars, the bias, and only then what the others check.
// `sel_err`: the message for a mode or kind outside its set, NULL for one inside; `ptrs`: every pointer the call needs is there.
static int pq_entry(PqFamily fam, const char* op, int metric, PqEpi e, bool bwd, const char* sel_err, bool ptrs, NegArgs a,
                    void* workspace, size_t workspace_bytes, void* stream) {
    const bool margin_ok = a.margin >= -3.402823466e38f && a.margin <= 3.402823466e38f;
    if (fam != PQ_NEG) {
        const int rc = pq_metric_check(op, metric, a.d, fam == PQ_PAIR);
        if (rc != GHF_OK) return rc;
    }
    if (fam == PQ_PAIR) {
        GHF_REQUIRE(!sel_err, "%s", sel_err);
        GHF_REQUIRE(a.scale > 0.f && a.scale <= 3.402823466e38f, "%s: scale must be finite and positive", op);
        GHF_REQUIRE(margin_ok, "%s: margin must be finite", op);
        GHF_REQUIRE(a.normalize == 0 || a.normalize == 1, "%s: normalize must be 0 or 1", op);
        GHF_REQUIRE(metric == GHF_PAIR_DOT || !a.bias, "%s: no per-candidate bias under a distance", op);
    }
    const int rc = score_entry_check(op, "filter", ptrs, a.filt_ptr, a.filt_idx, a.nnz, a.scale, 0.f, workspace);
    if (rc != GHF_OK) return rc;
    if (fam != PQ_PAIR) {
        GHF_REQUIRE(!sel_err, "%s", sel_err);
        if (e == PqEpi::Negsamp) {
            GHF_REQUIRE(margin_ok, "%s: margin must be finite", op);
            GHF_REQUIRE(a.alpha >= 0.f && a.alpha <= 3.402823466e38f, "%s: adv_temperature must be finite and not negative", op);
        }
    }
    GHF_REQUIRE(a.neg && a.K > 0, "%s: need neg [B, K] with K >= 1", op);
    if (a.nnz <= 0) a.filt_ptr = nullptr;                // the kernels read `no lists` from the pointer
    switch (fam) {
        case PQ_NEG: return launch_neg(e, bwd, op, a, workspace_bytes, (hipStream_t)stream);
        case PQ_DIST: return launch_dist(metric, e, bwd, op, a, workspace_bytes, (hipStream_t)stream);
        default: return launch_pair(metric, e, bwd, op, a, workspace_bytes, (hipStream_t)stream);
    }
}

size_t ghf_neg_workspace_bytes(int64_t B, int64_t K, int d, int64_t nnz) { return neg_workspace_bytes(B, K, d, nnz); }

int ghf_neg_rank(const float* q, const float* c, const int64_t* iq, const int64_t* target, const int64_t* filt_ptr,
                 const int64_t* filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d, const int64_t* neg, int64_t K,
                 const float* bias, void* workspace, size_t workspace_bytes, int64_t* greater, int64_t* equal, void* stream) {
    NegArgs a = pq_args(q, c, iq, target, filt_ptr, filt_idx, nnz, rows_q, N, B, d, 1.f, 0.f, 0.f, neg, K, bias);
    a.greater = (long long*)greater; a.equal = (long long*)equal;
    return pq_entry(PQ_NEG, "neg_rank", 0, PqEpi::Rank, false, nullptr, q && c && target && greater && equal, a, workspace,
                    workspace_bytes, stream);
}

int ghf_neg_softmax_fwd(const float* q, const float* c, const int64_t* iq, const int64_t* target, const int64_t* filt_ptr,
                        const int64_t* filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d, float scale,
                        const int64_t* neg, int64_t K, const float* bias, void* workspace, size_t workspace_bytes, float* loss,
                        float* lse, void* stream) {
    NegArgs a = pq_args(q, c, iq, target, filt_ptr, filt_idx, nnz, rows_q, N, B, d, scale, 0.f, 0.f, neg, K, bias);
    a.loss = loss; a.aux = lse;
    return pq_entry(PQ_NEG, "neg_softmax_fwd", 0, pq_of_neg_mode(GHF_NEG_SOFTMAX), false, nullptr, q && c && target && loss && lse, a,
                    workspace, workspace_bytes, stream);
}

int ghf_neg_negsamp_fwd(const float* q, const float* c, const int64_t* iq, const int64_t* target, const int64_t* filt_ptr,
                        const int64_t* filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d, float scale,
                        float margin, float adv_temperature, const int64_t* neg, int64_t K, const float* bias, void* workspace,
                        size_t workspace_bytes, float* loss, float* lw, void* stream) {
    NegArgs a = pq_args(q, c, iq, target, filt_ptr, filt_idx, nnz, rows_q, N, B, d, scale, margin, adv_temperature, neg, K, bias);
    a.loss = loss; a.aux = lw;
    return pq_entry(PQ_NEG, "neg_negsamp_fwd", 0, pq_of_neg_mode(GHF_NEG_NEGSAMP), false, nullptr, q && c && target && loss && lw, a,
                    workspace, workspace_bytes, stream);
}

int ghf_neg_bwd(int mode, const float* q, const float* c, const int64_t* iq, const int64_t* target, const int64_t* filt_ptr,
                const int64_t* filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d, float scale, float margin,
                float adv_temperature, const int64_t* neg, int64_t K, const float* bias, const float* lse_or_lw,
                const float* grad_loss, void* workspace, size_t workspace_bytes, float* dq, float* coef, void* stream) {
    NegArgs a = pq_args(q, c, iq, target, filt_ptr, filt_idx, nnz, rows_q, N, B, d, scale, margin, adv_temperature, neg, K, bias);
    a.saved = lse_or_lw; a.grad = grad_loss; a.dq = dq; a.coef = coef;
    const bool known = mode == GHF_NEG_SOFTMAX || mode == GHF_NEG_NEGSAMP;
    return pq_entry(PQ_NEG, "neg_bwd", 0, pq_of_neg_mode(mode), true,
                    known ? nullptr : "neg_bwd: mode must be GHF_NEG_SOFTMAX or GHF_NEG_NEGSAMP",
                    q && c && target && lse_or_lw && grad_loss && dq && coef, a, workspace, workspace_bytes, stream);
}

size_t ghf_dist_workspace_bytes(int64_t B, int64_t K, int d, int64_t nnz) { return dist_workspace_bytes(B, K, d, nnz); }

int ghf_dist_rank(int metric, const float* q, const float* c, const int64_t* iq, const int64_t* target, const int64_t* filt_ptr,
                  const int64_t* filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d, const int64_t* neg, int64_t K,
                  void* workspace, size_t workspace_bytes, int64_t* greater, int64_t* equal, void* stream) {
    NegArgs a = pq_args(q, c, iq, target, filt_ptr, filt_idx, nnz, rows_q, N, B, d, 1.f, 0.f, 0.f, neg, K, nullptr);
    a.greater = (long long*)greater; a.equal = (long long*)equal;
    return pq_entry(PQ_DIST, "dist_rank", metric, PqEpi::Rank, false, nullptr, q && c && target && greater && equal, a, workspace,
                    workspace_bytes, stream);
}

int ghf_dist_softmax_fwd(int metric, const float* q, const float* c, const int64_t* iq, const int64_t* target,
                         const int64_t* filt_ptr, const int64_t* filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d,
                         float scale, const int64_t* neg, int64_t K, void* workspace, size_t workspace_bytes, float* loss,
                         float* lse, void* stream) {
    NegArgs a = pq_args(q, c, iq, target, filt_ptr, filt_idx, nnz, rows_q, N, B, d, scale, 0.f, 0.f, neg, K, nullptr);
    a.loss = loss; a.aux = lse;
    return pq_entry(PQ_DIST, "dist_softmax_fwd", metric, pq_of_dist_mode(GHF_DIST_SOFTMAX), false, nullptr,
                    q && c && target && loss && lse, a, workspace, workspace_bytes, stream);
}

int ghf_dist_negsamp_fwd(int metric, const float* q, const float* c, const int64_t* iq, const int64_t* target,
                         const int64_t* filt_ptr, const int64_t* filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d,
                         float scale, float margin, float adv_temperature, const int64_t* neg, int64_t K, void* workspace,
                         size_t workspace_bytes, float* loss, float* lw, void* stream) {
    NegArgs a = pq_args(q, c, iq, target, filt_ptr, filt_idx, nnz, rows_q, N, B, d, scale, margin, adv_temperature, neg, K, nullptr);
    a.loss = loss; a.aux = lw;
    return pq_entry(PQ_DIST, "dist_negsamp_fwd", metric, pq_of_dist_mode(GHF_DIST_NEGSAMP), false, nullptr,
                    q && c && target && loss && lw, a, workspace, workspace_bytes, stream);
}

int ghf_dist_bwd(int metric, int mode, const float* q, const float* c, const int64_t* iq, const int64_t* target,
                 const int64_t* filt_ptr, const int64_t* filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d,
                 float scale, float margin, float adv_temperature, const int64_t* neg, int64_t K, const float* lse_or_lw,
                 const float* grad_loss, void* workspace, size_t workspace_bytes, float* dq, float* coef, void* stream) {
    NegArgs a = pq_args(q, c, iq, target, filt_ptr, filt_idx, nnz, rows_q, N, B, d, scale, margin, adv_temperature, neg, K, nullptr);
    a.saved = lse_or_lw; a.grad = grad_loss; a.dq = dq; a.coef = coef;
    const bool known = mode == GHF_DIST_SOFTMAX || mode == GHF_DIST_NEGSAMP;
    return pq_entry(PQ_DIST, "dist_bwd", metric, pq_of_dist_mode(mode), true,
                    known ? nullptr : "dist_bwd: mode must be GHF_DIST_SOFTMAX or GHF_DIST_NEGSAMP",
                    q && c && target && lse_or_lw && grad_loss && dq && coef, a, workspace, workspace_bytes, stream);
}

int ghf_dist_rows_grad(int metric, const float* q, const float* c, const int64_t* iq, int64_t rows_q, int64_t N, int64_t B, int d,
                       int64_t K, const float* coef, const int64_t* perm, const int64_t* off, float* dc, void* stream) {
    const int rc = pq_metric_check("dist_rows_grad", metric, d, false);
    if (rc != GHF_OK) return rc;
    GHF_REQUIRE(q && c && coef && perm && off && dc, "dist_rows_grad: null pointer argument");
    return launch_dist_rows_grad(metric, q, c, iq, rows_q, N, B, d, K, coef, perm, off, dc, (hipStream_t)stream);
}

size_t ghf_pair_workspace_bytes(int64_t B, int64_t K, int d, int64_t nnz) { return pair_workspace_bytes(B, K, d, nnz); }

int ghf_pair_fwd(int metric, int kind, const float* q, const float* c, const int64_t* iq, const int64_t* target,
                 const int64_t* filt_ptr, const int64_t* filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d,
                 float scale, float margin, int normalize, const int64_t* neg, int64_t K, const float* bias, void* workspace,
                 size_t workspace_bytes, float* loss, int32_t* count, int32_t* active, void* stream) {
    NegArgs a = pq_args(q, c, iq, target, filt_ptr, filt_idx, nnz, rows_q, N, B, d, scale, margin, 0.f, neg, K, bias);
    a.loss = loss; a.count = count; a.active = active; a.normalize = normalize;
    const bool known = kind == GHF_PAIR_HINGE || kind == GHF_PAIR_LOGISTIC;
    return pq_entry(PQ_PAIR, "pair_fwd", metric, pq_of_pair_kind(kind), false,
                    known ? nullptr : "pair_fwd: kind must be GHF_PAIR_HINGE or GHF_PAIR_LOGISTIC",
                    q && c && target && loss && count && active, a, workspace, workspace_bytes, stream);
}

int ghf_pair_bwd(int metric, int kind, const float* q, const float* c, const int64_t* iq, const int64_t* target,
                 const int64_t* filt_ptr, const int64_t* filt_idx, int64_t nnz, int64_t rows_q, int64_t N, int64_t B, int d,
                 float scale, float margin, int normalize, const int64_t* neg, int64_t K, const float* bias, const int32_t* count,
                 const float* grad_loss, void* workspace, size_t workspace_bytes, float* dq, float* coef, void* stream) {
    NegArgs a = pq_args(q, c, iq, target, filt_ptr, filt_idx, nnz, rows_q, N, B, d, scale, margin, 0.f, neg, K, bias);
    a.saved_n = count; a.grad = grad_loss; a.dq = dq; a.coef = coef; a.normalize = normalize;
    const bool known = kind == GHF_PAIR_HINGE || kind == GHF_PAIR_LOGISTIC;
    return pq_entry(PQ_PAIR, "pair_bwd", metric, pq_of_pair_kind(kind), true,
                    known ? nullptr : "pair_bwd: kind must be GHF_PAIR_HINGE or GHF_PAIR_LOGISTIC",
                    q && c && target && count && grad_loss && dq && coef, a, workspace, workspace_bytes, stream);
}

size_t ghf_relation_rows_workspace_bytes(int64_t B, int R) { return relation_rows_workspace_bytes(B, R); }

int ghf_relation_rows(const float* x, const int64_t* ix, const int64_t* rel, const float* W, const float* bias,
                      const int64_t* perm, const int64_t* goff, int64_t rows_x, int64_t B, int R, int d, int flags,
                      void* workspace, size_t workspace_bytes, float* out, void* stream) {
    GHF_REQUIRE(x && rel && W && perm && goff && workspace && out, "relation_rows: null pointer argument");
    GHF_REQUIRE(((uintptr_t)workspace & 255) == 0, "relation_rows: workspace not 256-byte aligned");
    return launch_relation_rows(x, ix, rel, W, bias, perm, goff, rows_x, B, R, d, flags, workspace, workspace_bytes, out,
                                (hipStream_t)stream);
}

int ghf_relation_scores(const float* x, const int64_t* ia, const int64_t* ib, const float* W, const float* bias, int64_t rows_x,
                        int64_t B, int64_t U, int d, int flags, float* out, void* stream) {
    GHF_REQUIRE(x && ia && ib && W && out, "relation_scores: null pointer argument");
    return launch_relation_scores(x, ia, ib, W, bias, rows_x, B, U, d, flags, out, (hipStream_t)stream);
}

size_t ghf_relation_scores_bwd_rows_workspace_bytes(int64_t B, int64_t U, int d) {
    return U >= ((int64_t)1 << 23) ? 0 : relation_scores_bwd_rows_workspace_bytes(B, (int)U, d);
}

int ghf_relation_scores_bwd_rows(const float* x, const int64_t* ia, const float* G, const float* W, const float* bias,
                                 int64_t rows_x, int64_t B, int64_t U, int d, int flags, void* workspace, size_t workspace_bytes,
                                 float* out, void* stream) {
    GHF_REQUIRE(x && ia && G && W && workspace && out, "relation_scores_bwd_rows: null pointer argument");
    GHF_REQUIRE(((uintptr_t)workspace & 255) == 0, "relation_scores_bwd_rows: workspace not 256-byte aligned");
    return launch_relation_scores_bwd_rows(x, ia, G, W, bias, rows_x, B, U, d, flags, workspace, workspace_bytes, out,
                                           (hipStream_t)stream);
}

size_t ghf_relation_scores_bwd_weights_workspace_bytes(int64_t B, int64_t U, int d) {
    return U >= ((int64_t)1 << 23) ? 0 : relation_scores_bwd_weights_workspace_bytes(B, (int)U, d);
}

int ghf_relation_scores_bwd_weights(const float* x, const int64_t* ia, const int64_t* ib, const float* G, int64_t rows_x, int64_t B,
                                    int64_t U, int d, int flags, void* workspace, size_t workspace_bytes, float* dW, float* dbias,
                                    void* stream) {
    GHF_REQUIRE(x && ia && ib && G && workspace && dW, "relation_scores_bwd_weights: null pointer argument");
    GHF_REQUIRE(((uintptr_t)workspace & 255) == 0, "relation_scores_bwd_weights: workspace not 256-byte aligned");
    return launch_relation_scores_bwd_weights(x, ia, ib, G, rows_x, B, U, d, flags, workspace, workspace_bytes, dW, dbias,
                                              (hipStream_t)stream);
}

int ghf_tail_fwd(const float* agg, const float* h, const float* ln_gamma, const float* ln_beta, float ln_eps,
                 int64_t row0, int64_t rows, int d, float* h_out, const float* drop, void* stream) {
    GHF_REQUIRE(agg && h && ln_gamma && ln_beta && h_out, "tail_fwd: null pointer argument");
    GHF_REQUIRE(row0 >= 0 && rows >= 0, "tail_fwd: bad row range");
    return launch_tail(agg, h, ln_gamma, ln_beta, ln_eps, row0, rows, d, h_out, drop, (hipStream_t)stream);
}

}  // extern "C"
