// relation.hip — relation-typed query rows: out[i] = [x[ix[i]]] + x[ix[i]] . op(W[rel[i]]) + [bias[rel[i]]]  (ghf.h:
// ghf_relation_rows).  The step between the encoder and the rank / top-k / softmax sweeps of a (head, relation, ?) query:
// every query row is multiplied by ITS relation's d x d matrix without gathering one matrix per query.
//
//   The caller groups the queries by relation (ghf_group_edges: perm, goff).  rr_tiles_kernel cuts every relation's range
//   into tiles of <= 64 grouped rows on the device: a table of at most ceil(B/64) + R (relation, first position) pairs in
//   the workspace; the launch has that many workgroups and the ones past the table's end return at once (no host read).
//   workgroup = 256 threads = 4 waves, one (relation, tile).  The tile's x rows are gathered through perm -> ix into LDS
//   once; W[r] streams through two LDS buffers of 16 rows of k (all d columns), fetched into registers one slice ahead of
//   the slice being multiplied: one barrier per slice.  Wave w owns rows 16 w .. 16 w + 15 of the tile and all d columns:
//   DC / 16 accumulators of v_mfma_f32_16x16x4_f32 (A: lane l = x[row l & 15][k = l >> 4]; B: W[k = l >> 4][col l & 15];
//   D: row 4 (l >> 4) + reg, col l & 15).  The transposed form reads the same slice of k out of W's COLUMNS and stores it
//   transposed, so the multiply loop is the same.
//   The epilogue adds residual and bias into the wave's own rows of the LDS tile (no other wave reads them), and the
//   workgroup writes whole rows back through perm with 16-byte stores.
//
// LDS: the x tile has a row stride of DC + 4 floats, a weight slice one of DC + 16 (DC = the padded width, 64 / 128 / 192 / 256):
// the B operand's reads (ds_read_b32: 32 banks, half a wave per cycle: k = l >> 4 in {0, 1} x 16 columns) touch 32 distinct
// banks; the A operand's four reads per slice are 2-way conflicted (rows r and r + 8), against 4 DC / 16 of B's.  The
// transposed stash writes scalars 4-way conflicted: 4 DC / 64 writes per thread and slice next to DC / 4 matrix
// instructions of 32 cycles each.
//
// Numerics: an output element is bit for bit the chain s = fmaf(x[k], W[k][l], s), k = 0 .. d-1 from s = 0 (the padded k
// add fma(0, 0, s) = s), then (x[l] + s) + bias[l].  It depends on the row's own x, W[r] and bias[r] only: not on the tile
// it shares, its position in it or the other queries of the call.
#include "common.h"
#include "rank_sweep.h"

namespace ghf {

constexpr int RR_ROWS = 64;                  // grouped query rows per workgroup
constexpr int RR_BK = 16;                    // rows of k per weight slice
constexpr int RR_NT = 256;
constexpr int RR_MAX_D = 256;

static inline int64_t rr_max_tiles(int64_t B, int R) { return cdiv(B, RR_ROWS) + R; }

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
            n = (hi - lo + RR_ROWS - 1) / RR_ROWS;
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
            if (first + j < max_tiles) tab[first + j] = make_int2(r, (int)(lo + RR_ROWS * j));
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

static inline size_t rr_lds_bytes(int NCT) {
    const int DC = NCT * 16;
    return ((size_t)RR_ROWS * (DC + 4) + 2 * (size_t)RR_BK * (DC + 16)) * 4 + RR_ROWS * (8 + 4 + 4);
}

template <int NCT, bool TR>
__global__ __launch_bounds__(RR_NT) void relation_rows_kernel(const RelArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int DC = NCT * 16, LDX = DC + 4, LDW = DC + 16, F4 = DC / 4, NL = RR_BK * F4 / RR_NT;
    float* Xs = lds;
    float* Ws = Xs + RR_ROWS * LDX;
    int64_t* rowx = (int64_t*)(Ws + 2 * RR_BK * LDW);       // the row of x, -1: none (a row of zeros)
    int* rowi = (int*)(rowx + RR_ROWS);                     // the query (row of out), -1: none
    int* rowbad = rowi + RR_ROWS;                           // an id out of range: the row of out is NaN
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int d = a.d;

    const int2 te = a.tab[blockIdx.x];
    const int r = te.x;
    if (r < 0 || r >= a.R) return;                          // past the table's end (the whole workgroup)
    const int64_t p0 = rr_clamp(te.y, 0, a.B);
    const int64_t p1 = rr_clamp(a.goff[r + 1], p0, p0 + RR_ROWS < a.B ? p0 + RR_ROWS : a.B);
    const int nrows = (int)(p1 - p0);

    if (tid < RR_ROWS) {
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
    for (int idx = tid; idx < RR_ROWS * F4; idx += RR_NT) {
        const int row = idx / F4, c4 = idx - row * F4;
        const int64_t xr = rowx[row];
        *(f32x4*)(Xs + row * LDX + c4 * 4) = load_k4(xr >= 0 ? a.x + (size_t)xr * d : nullptr, c4 * 4, d, vx);
    }

    const float* Wr = a.W + (size_t)r * d * d;
    f32x4 pre[NL];
    // slice s holds k = 16 s .. 16 s + 15 of op(W[r]) as [k][column], zeros past d either way
    auto fetch = [&](int s) {
#pragma unroll
        for (int i = 0; i < NL; ++i) {
            const int idx = tid + RR_NT * i;
            if (TR) {
                const int l = idx >> 2, c4 = idx & 3;
                pre[i] = load_k4(l < d ? Wr + (size_t)l * d : nullptr, s * RR_BK + c4 * 4, d, vw);
            } else {
                const int kk = idx / F4, c4 = idx - kk * F4, k = s * RR_BK + kk;
                pre[i] = load_k4(k < d ? Wr + (size_t)k * d : nullptr, c4 * 4, d, vw);
            }
        }
    };
    auto stash = [&](int buf) {
        float* w = Ws + buf * RR_BK * LDW;
#pragma unroll
        for (int i = 0; i < NL; ++i) {
            const int idx = tid + RR_NT * i;
            if (TR) {
                const int l = idx >> 2, c4 = idx & 3;
#pragma unroll
                for (int e = 0; e < 4; ++e) w[(c4 * 4 + e) * LDW + l] = pre[i][e];
            } else {
                const int kk = idx / F4, c4 = idx - kk * F4;
                *(f32x4*)(w + kk * LDW + c4 * 4) = pre[i];
            }
        }
    };

    f32x4 acc[NCT];
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) acc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int nsl = (d + RR_BK - 1) / RR_BK;
    fetch(0);
    stash(0);
    __syncthreads();
    int buf = 0;
    for (int s = 0; s < nsl; ++s) {
        const bool more = s + 1 < nsl;
        if (more) fetch(s + 1);
        const float* xa = Xs + (wave * 16 + (lane & 15)) * LDX + s * RR_BK + (lane >> 4);
        const float* wb = Ws + buf * RR_BK * LDW + (lane >> 4) * LDW + (lane & 15);
#pragma unroll
        for (int kq = 0; kq < RR_BK / 4; ++kq) {
            const float av = xa[4 * kq];
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct)      // every tile, also the ones past d (zeros): a test here costs the accumulators their registers
                acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, wb[4 * kq * LDW + ct * 16], acc[ct], 0, 0, 0);
        }
        if (more) stash(buf ^ 1);
        __syncthreads();
        buf ^= 1;
    }

    // residual and bias, into the wave's own rows of the tile
    const float* br = a.bias ? a.bias + (size_t)r * d : nullptr;
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) {
        const int col = ct * 16 + (lane & 15);
        const float bv = (br && col < d) ? br[col] : 0.f;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            float* px = Xs + (wave * 16 + 4 * (lane >> 4) + reg) * LDX + col;
            float v = acc[ct][reg];
            if (a.add_x) v = *px + v;
            if (br) v += bv;
            *px = v;
        }
    }
    __syncthreads();

    const float nan = __int_as_float(0x7FC00000);
    const int nf4 = (d + 3) >> 2;
    for (int idx = tid; idx < nrows * nf4; idx += RR_NT) {
        const int row = idx / nf4, c4 = idx - row * nf4;
        const int di = rowi[row];
        if (di < 0) continue;
        f32x4 v = *(const f32x4*)(Xs + row * LDX + c4 * 4);
        if (rowbad[row]) v = f32x4{nan, nan, nan, nan};
        float* o = a.out + (size_t)di * d + c4 * 4;
        if (vo) {
            *(f32x4*)o = v;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (c4 * 4 + e < d) o[e] = v[e];
        }
    }
}

template <int NCT, bool TR>
static int launch_rr(const RelArgs& a, unsigned grid, hipStream_t stream) {
    const size_t lds = rr_lds_bytes(NCT);
    GHF_SET_MAX_LDS((relation_rows_kernel<NCT, TR>), lds);
    relation_rows_kernel<NCT, TR><<<grid, RR_NT, lds, stream>>>(a);
    GHF_LAUNCH_CHECK();
    return GHF_OK;
}

int launch_relation_rows(const float* x, const int64_t* ix, const int64_t* rel, const float* W, const float* bias,
                         const int64_t* perm, const int64_t* goff, int64_t rows_x, int64_t B, int R, int d, int flags,
                         void* ws, size_t ws_bytes, float* out, hipStream_t stream) {
    GHF_REQUIRE(d > 0 && rows_x > 0 && B > 0 && R > 0, "relation_rows: bad shape");
    if (d > RR_MAX_D) return set_err(GHF_EUNSUPPORTED, "relation_rows: d = %d exceeds %d", d, RR_MAX_D);
    GHF_REQUIRE((flags & ~(GHF_REL_ADD_X | GHF_REL_TRANSPOSE)) == 0, "relation_rows: unknown flags %d", flags);
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
    const unsigned grid = (unsigned)max_tiles;
    const bool tr = (flags & GHF_REL_TRANSPOSE) != 0;
    if (d <= 64) return tr ? launch_rr<4, true>(a, grid, stream) : launch_rr<4, false>(a, grid, stream);
    if (d <= 128) return tr ? launch_rr<8, true>(a, grid, stream) : launch_rr<8, false>(a, grid, stream);
    if (d <= 192) return tr ? launch_rr<12, true>(a, grid, stream) : launch_rr<12, false>(a, grid, stream);
    return tr ? launch_rr<16, true>(a, grid, stream) : launch_rr<16, false>(a, grid, stream);
}

}  // namespace ghf
