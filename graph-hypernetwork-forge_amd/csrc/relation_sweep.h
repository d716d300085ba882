// relation_sweep.h — the streamed-weight sweep that relation.hip (relation_rows_kernel: the rows of a (head, relation, ?)
// query) and relation_predict.hip (rp_sweep_kernel: the [B, U] table of a (head, ?, tail) query and its row gradients) share:
//
//   q = [x] + x . op(W[u]) + [bias[u]]      for a tile of 64 rows x and one d x d matrix W[u] at a time
//
// Each kernel keeps its own control flow (what a workgroup owns, which relations it walks) and its own epilogue; the tile,
// the slice pipeline and the chain are written here once, so that a row of q is the same bits wherever it is built.
//
// Tile: workgroup = 256 threads = 4 waves and 64 rows.  The rows of x are gathered into LDS once, through a per-row table of
// ids that the kernel has already tested against their range (-1: a row of zeros, nothing is read).  op(W[u]) streams
// through two LDS buffers of 16 rows of k (all d columns), fetched into registers one slice ahead of the slice being
// multiplied: one barrier per slice.  Wave w owns rows 16 w .. 16 w + 15 of the tile and all d columns: DC / 16 accumulators
// of v_mfma_f32_16x16x4_f32 (A: lane l = x[row l & 15][k = l >> 4]; B: W[k = l >> 4][col l & 15]; D: row 4 (l >> 4) + reg,
// col l & 15).  The transposed form reads the same slice of k out of W's COLUMNS and stores it transposed, so the multiply
// is the same.  The padded columns and the padded tail of k are multiplied as zeros: a test around the matrix instruction
// costs the accumulators their registers.
//
// LDS: the x tile has a row stride of DC + 4 floats, a weight slice one of DC + 16 (DC = the padded width, 64 / 128 / 192 /
// 256): the B operand's reads (ds_read_b32: 32 banks, half a wave per cycle: k = l >> 4 in {0, 1} x 16 columns) touch 32
// distinct banks; the A operand's four reads per slice are 2-way conflicted (rows r and r + 8), against 4 DC / 16 of B's.
// The transposed stash writes scalars 4-way conflicted: 4 DC / 64 writes per thread and slice next to DC / 4 matrix
// instructions of 32 cycles each.
//
// Numerics: an element of q is bit for bit the chain s = fmaf(x[k], W[k][l], s), k = 0 .. d-1 from s = 0 (the padded k add
// fma(0, 0, s) = s), then (x[l] + s) + bias[l].  It depends on the row's own x, W[u] and bias[u] only: not on the tile it
// shares, its position in it or the other rows of the call.
#pragma once
#include <type_traits>

#include "common.h"
#include "rank_sweep.h"

namespace ghf {

constexpr int REL_ROWS = 64;                 // rows per workgroup
constexpr int REL_BK = 16;                   // rows of k per weight slice
constexpr int REL_NT = 256;
constexpr int REL_MAX_D = 256;

template <int NCT>                           // NCT column tiles of 16: the widths 64 / 128 / 192 / 256
struct RelGeom {
    static constexpr int DC = NCT * 16, LDX = DC + 4, LDW = DC + 16, F4 = DC / 4, NL = REL_BK * F4 / REL_NT;
    static constexpr int XS = REL_ROWS * LDX, WS = 2 * REL_BK * LDW;      // floats of the x tile and of the two W buffers
};

// the D layout: register reg of accumulator ct holds (row, column) of the tile
__device__ __forceinline__ int rel_drow(int wave, int lane, int reg) { return wave * 16 + 4 * (lane >> 4) + reg; }
__device__ __forceinline__ int rel_dcol(int ct, int lane) { return ct * 16 + (lane & 15); }

template <int NCT>
__device__ __forceinline__ void rel_gather(float* Xs, const int64_t* rowx, const float* x, int d, bool vx, int tid) {
    using G = RelGeom<NCT>;
    for (int idx = tid; idx < REL_ROWS * G::F4; idx += REL_NT) {
        const int row = idx / G::F4, c4 = idx - row * G::F4;
        const int64_t xr = rowx[row];
        *(f32x4*)(Xs + row * G::LDX + c4 * 4) = load_k4(xr >= 0 ? x + (size_t)xr * d : nullptr, c4 * 4, d, vx);
    }
}

// slice s of Wu holds k = 16 s .. 16 s + 15 of op(Wu) as [k][column], zeros past d either way
template <int NCT, bool TR>
__device__ __forceinline__ void rel_fetch(f32x4 (&pre)[RelGeom<NCT>::NL], const float* Wu, int s, int d, bool vw, int tid) {
    using G = RelGeom<NCT>;
#pragma unroll
    for (int i = 0; i < G::NL; ++i) {
        const int idx = tid + REL_NT * i;
        if (TR) {
            const int l = idx >> 2, c4 = idx & 3;
            pre[i] = load_k4(l < d ? Wu + (size_t)l * d : nullptr, s * REL_BK + c4 * 4, d, vw);
        } else {
            const int kk = idx / G::F4, c4 = idx - kk * G::F4, k = s * REL_BK + kk;
            pre[i] = load_k4(k < d ? Wu + (size_t)k * d : nullptr, c4 * 4, d, vw);
        }
    }
}

template <int NCT, bool TR>
__device__ __forceinline__ void rel_stash(const f32x4 (&pre)[RelGeom<NCT>::NL], float* Ws, int buf, int tid) {
    using G = RelGeom<NCT>;
    float* w = Ws + buf * REL_BK * G::LDW;
#pragma unroll
    for (int i = 0; i < G::NL; ++i) {
        const int idx = tid + REL_NT * i;
        if (TR) {
            const int l = idx >> 2, c4 = idx & 3;
#pragma unroll
            for (int e = 0; e < 4; ++e) w[(c4 * 4 + e) * G::LDW + l] = pre[i][e];
        } else {
            const int kk = idx / G::F4, c4 = idx - kk * G::F4;
            *(f32x4*)(w + kk * G::LDW + c4 * 4) = pre[i];
        }
    }
}

// acc += x[:, 16 s .. 16 s + 15] . (the slice in buffer buf): every column tile, also the ones past d (zeros)
template <int NCT>
__device__ __forceinline__ void rel_multiply(f32x4 (&acc)[NCT], const float* Xs, const float* Ws, int buf, int s, int lane, int wave) {
    using G = RelGeom<NCT>;
    const float* xa = Xs + (wave * 16 + (lane & 15)) * G::LDX + s * REL_BK + (lane >> 4);
    const float* wb = Ws + buf * REL_BK * G::LDW + (lane >> 4) * G::LDW + (lane & 15);
#pragma unroll
    for (int kq = 0; kq < REL_BK / 4; ++kq) {
        const float av = xa[4 * kq];
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct)
            acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, wb[4 * kq * G::LDW + ct * 16], acc[ct], 0, 0, 0);
    }
}

// bias[u][col] of a lane's column (bu = bias + u d, or nullptr)
__device__ __forceinline__ float rel_bias(const float* bu, int col, int d) { return (bu && col < d) ? bu[col] : 0.f; }

// (x + s) + bias of an element in the D layout, in this order; px: the element's x in the LDS tile
__device__ __forceinline__ float rel_value(float s, const float* px, bool add_x, bool add_bias, float bv) {
    float v = s;
    if (add_x) v = *px + v;
    if (add_bias) v += bv;
    return v;
}

// Whole rows of the LDS tile to rows row_of(row) of out (negative: the row is not written): 16-byte stores where the output
// allows (vo), and NaN for a row whose id was out of range.
template <int NCT, class RowOf>
__device__ __forceinline__ void rel_store_rows(const float* Xs, const int* rowbad, int nrows, int d, float* out, bool vo, int tid,
                                               RowOf row_of) {
    const float nan = __int_as_float(0x7FC00000);
    const int nf4 = (d + 3) >> 2;
    for (int idx = tid; idx < nrows * nf4; idx += REL_NT) {
        const int row = idx / nf4, c4 = idx - row * nf4;
        const auto r = row_of(row);
        if (r < 0) continue;
        f32x4 v = *(const f32x4*)(Xs + row * RelGeom<NCT>::LDX + c4 * 4);
        if (rowbad[row]) v = f32x4{nan, nan, nan, nan};
        float* o = out + (size_t)r * d + c4 * 4;
        if (vo) {
            *(f32x4*)o = v;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (c4 * 4 + e < d) o[e] = v[e];
        }
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------
// d -> the NCT instantiation: f(std::integral_constant<int, NCT>); with the transpose: f(.., std::bool_constant<TR>)
template <class F>
static inline int rel_dispatch(int d, F&& f) {
    if (d <= 64) return f(std::integral_constant<int, 4>{});
    if (d <= 128) return f(std::integral_constant<int, 8>{});
    if (d <= 192) return f(std::integral_constant<int, 12>{});
    return f(std::integral_constant<int, 16>{});
}
template <class F>
static inline int rel_dispatch(int d, bool tr, F&& f) {
    return rel_dispatch(d, [&](auto nct) { return tr ? f(nct, std::true_type{}) : f(nct, std::false_type{}); });
}

// what every relation entry point tests first (n_rel: R or U)
static inline int rel_check(const char* what, int64_t rows_x, int64_t B, int64_t n_rel, int d, int flags, int allowed) {
    GHF_REQUIRE(d > 0 && rows_x > 0 && B > 0 && n_rel > 0, "%s: bad shape", what);
    if (d > REL_MAX_D) return set_err(GHF_EUNSUPPORTED, "%s: d = %d exceeds %d", what, d, REL_MAX_D);
    GHF_REQUIRE((flags & ~allowed) == 0, "%s: unknown flags %d", what, flags);
    return GHF_OK;
}

}  // namespace ghf
