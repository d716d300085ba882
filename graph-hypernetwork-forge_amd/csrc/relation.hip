// relation.hip — relation-typed query rows: out[i] = [x[ix[i]]] + x[ix[i]] . op(W[rel[i]]) + [bias[rel[i]]]  (ghf.h:
// ghf_relation_rows).  The step between the encoder and the rank / top-k / softmax sweeps of a (head, relation, ?) query:
// every query row is multiplied by ITS relation's d x d matrix without gathering one matrix per query.
//
//   The caller groups the queries by relation (ghf_group_edges: perm, goff).  rr_tiles_kernel cuts every relation's range
//   into tiles of <= 64 grouped rows on the device: a table of at most ceil(B/64) + R (relation, first position) pairs in
//   the workspace; the launch has that many workgroups and the ones past the table's end return at once (no host read).
//   relation_rows_kernel: one workgroup per (relation, tile).  The tile's x rows are gathered through perm -> ix, W[r] is
//   streamed and multiplied as relation_sweep.h describes (tile, LDS layout, numerics).  The epilogue adds residual and bias
//   into the wave's own rows of the LDS tile (no other wave reads them), and the workgroup writes whole rows back through
//   perm.
//
// Every id (a tile's relation and position, perm, rel, ix) is tested against its range before an address is formed from it.
#include "relation_sweep.h"

namespace ghf {

static inline int64_t rr_max_tiles(int64_t B, int R) { return cdiv(B, REL_ROWS) + R; }

size_t relation_rows_workspace_bytes(int64_t B, int R) {
    if (B <= 0 || B >= (int64_t)1 << 31 || R <= 0 || R >= 1 << 23) return 0;
    return align_up((size_t)rr_max_tiles(B, R) * sizeof(int2), 256);
}

__device__ __forceinline__ int64_t rr_clamp(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

// One workgroup: tab[t] = (relation, first grouped position) of tile t, relations ascending, (-1, 0) past the last tile.
// goff comes from the caller: every offset is clamped into [0, B] and nothing is written past max_tiles.
__global__ __launch_bounds__(256) void rr_tiles_kernel(const int64_t* __restrict__ goff, int64_t B, int R, int64_t max_tiles,
                                                       int2* __restrict__ tab) {
    __shared__ int64_t sc[256];
    __shared__ int64_t run;
    const int tid = threadIdx.x;
    if (tid == 0) run = 0;
    __syncthreads();
    for (int base = 0; base < R; base += 256) {
        const int r = base + tid;
        int64_t lo = 0, n = 0;
        if (r < R) {
            lo = rr_clamp(goff[r], 0, B);
            const int64_t hi = rr_clamp(goff[r + 1], lo, B);
            n = (hi - lo + REL_ROWS - 1) / REL_ROWS;
        }
        sc[tid] = n;
        __syncthreads();
        for (int off = 1; off < 256; off <<= 1) {
            const int64_t v = tid >= off ? sc[tid - off] : 0;
            __syncthreads();
            sc[tid] += v;
            __syncthreads();
        }
        const int64_t first = run + sc[tid] - n;
        for (int64_t j = 0; j < n; ++j)
            if (first + j < max_tiles) tab[first + j] = make_int2(r, (int)(lo + REL_ROWS * j));
        __syncthreads();
        if (tid == 255) run += sc[255];
        __syncthreads();
    }
    for (int64_t t = run + tid; t < max_tiles; t += 256) tab[t] = make_int2(-1, 0);
}

struct RelArgs {
    const float* x; const int64_t* ix; const int64_t* rel; const float* W; const float* bias;
    const int64_t* perm; const int64_t* goff; const int2* tab;
    int64_t rows_x, B;
    int R, d, add_x;
    float* out;
};

template <int NCT, bool TR>
__global__ __launch_bounds__(REL_NT) void relation_rows_kernel(const RelArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    using G = RelGeom<NCT>;
    float* Xs = lds;
    float* Ws = Xs + G::XS;
    int64_t* rowx = (int64_t*)(Ws + G::WS);                  // the row of x, -1: none (a row of zeros)
    int* rowi = (int*)(rowx + REL_ROWS);                     // the query (row of out), -1: none
    int* rowbad = rowi + REL_ROWS;                           // an id out of range: the row of out is NaN
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int d = a.d;

    const int2 te = a.tab[blockIdx.x];
    const int r = te.x;
    if (r < 0 || r >= a.R) return;                          // past the table's end (the whole workgroup)
    const int64_t p0 = rr_clamp(te.y, 0, a.B);
    const int64_t p1 = rr_clamp(a.goff[r + 1], p0, p0 + REL_ROWS < a.B ? p0 + REL_ROWS : a.B);
    const int nrows = (int)(p1 - p0);

    if (tid < REL_ROWS) {
        int di = -1, bad = 0;
        int64_t xr = -1;
        if (tid < nrows) {
            const int64_t i = a.perm[p0 + tid];
            if (i >= 0 && i < a.B) {
                di = (int)i;
                const int64_t xi = a.ix ? a.ix[i] : i;
                bad = (a.rel[i] != r || xi < 0 || xi >= a.rows_x) ? 1 : 0;   // (ghf_group_edges files a bad relation id under R - 1)
                if (!bad) xr = xi;
            }
        }
        rowx[tid] = xr;
        rowi[tid] = di;
        rowbad[tid] = bad;
    }
    __syncthreads();

    const bool vx = rows_vec(a.x, d), vw = rows_vec(a.W, d), vo = rows_vec(a.out, d);
    rel_gather<NCT>(Xs, rowx, a.x, d, vx, tid);

    const float* Wr = a.W + (size_t)r * d * d;
    f32x4 pre[G::NL], acc[NCT];
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) acc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int nsl = (d + REL_BK - 1) / REL_BK;
    rel_fetch<NCT, TR>(pre, Wr, 0, d, vw, tid);
    rel_stash<NCT, TR>(pre, Ws, 0, tid);
    __syncthreads();
    int buf = 0;
    for (int s = 0; s < nsl; ++s) {
        const bool more = s + 1 < nsl;
        if (more) rel_fetch<NCT, TR>(pre, Wr, s + 1, d, vw, tid);
        rel_multiply<NCT>(acc, Xs, Ws, buf, s, lane, wave);
        if (more) rel_stash<NCT, TR>(pre, Ws, buf ^ 1, tid);
        __syncthreads();
        buf ^= 1;
    }

    // residual and bias, into the wave's own rows of the tile
    const float* br = a.bias ? a.bias + (size_t)r * d : nullptr;
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) {
        const int col = rel_dcol(ct, lane);
        const float bv = rel_bias(br, col, d);
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            float* px = Xs + rel_drow(wave, lane, reg) * G::LDX + col;
            *px = rel_value(acc[ct][reg], px, a.add_x, br, bv);
        }
    }
    __syncthreads();

    rel_store_rows<NCT>(Xs, rowbad, nrows, d, a.out, vo, tid, [&](int row) { return rowi[row]; });
}

template <int NCT, bool TR>
static int launch_rr(const RelArgs& a, unsigned grid, hipStream_t stream) {
    const size_t lds = (size_t)(RelGeom<NCT>::XS + RelGeom<NCT>::WS) * 4 + REL_ROWS * (8 + 4 + 4);     // + rowx, rowi, rowbad
    GHF_SET_MAX_LDS((relation_rows_kernel<NCT, TR>), lds);
    relation_rows_kernel<NCT, TR><<<grid, REL_NT, lds, stream>>>(a);
    GHF_LAUNCH_CHECK();
    return GHF_OK;
}

int launch_relation_rows(const float* x, const int64_t* ix, const int64_t* rel, const float* W, const float* bias,
                         const int64_t* perm, const int64_t* goff, int64_t rows_x, int64_t B, int R, int d, int flags,
                         void* ws, size_t ws_bytes, float* out, hipStream_t stream) {
    if (int rc = rel_check("relation_rows", rows_x, B, R, d, flags, GHF_REL_ADD_X | GHF_REL_TRANSPOSE)) return rc;
    const size_t need = relation_rows_workspace_bytes(B, R);
    GHF_REQUIRE(need > 0, "relation_rows: B or R out of range");
    GHF_REQUIRE(ix || B <= rows_x, "relation_rows: B exceeds the rows of x");
    GHF_REQUIRE(ws_bytes >= need, "relation_rows: workspace of %zu bytes, need %zu", ws_bytes, need);
    const int64_t max_tiles = rr_max_tiles(B, R);
    int2* tab = (int2*)ws;
    rr_tiles_kernel<<<1, 256, 0, stream>>>(goff, B, R, max_tiles, tab);
    GHF_LAUNCH_CHECK();
    RelArgs a = {};
    a.x = x; a.ix = ix; a.rel = rel; a.W = W; a.bias = bias; a.perm = perm; a.goff = goff; a.tab = tab;
    a.rows_x = rows_x; a.B = B; a.R = R; a.d = d; a.add_x = (flags & GHF_REL_ADD_X) ? 1 : 0; a.out = out;
    return rel_dispatch(d, (flags & GHF_REL_TRANSPOSE) != 0, [&](auto nct, auto tr) {
        return launch_rr<decltype(nct)::value, decltype(tr)::value>(a, (unsigned)max_tiles, stream);
    });
}

}  // namespace ghf
