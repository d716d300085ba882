// negatives_dev.h — the device helpers that negatives.hip (dot-product scores) and distance.hip (distance
// scores; §22) share: the geometry of a query against ITS OWN rows of c — the lane's slice of a row, the branch-free id and
// row loads of the loops, the butterfly over a group of L lanes, and what a kernel knows of its query before the first
// negative.  Moved here from negatives.hip unchanged.
#pragma once
#include "common.h"
#include "rank_sweep.h"

namespace ghf {

constexpr int NG_U = 8;                          // row loads a lane keeps in flight
constexpr int NG_RANK = 0, NG_SOFTMAX = 1, NG_NEGSAMP = 2;
constexpr int NG_SPLIT_K = 256;                  // above it a query's positions are dealt to the four waves of a workgroup
static inline int neg_waves(int64_t K) { return K > NG_SPLIT_K ? 4 : 1; }

struct NegArgs {
    const float* q; const float* c; const int64_t* iq; const int64_t* target;
    const int64_t* filt_ptr; const int64_t* filt_idx; int64_t nnz;
    const int64_t* neg; int64_t K, rows_q, N, B;
    int d;
    const float* bias; float scale, margin, alpha;
    long long* greater; long long* equal; float* loss; float* aux;             // forward: counts, or loss and lse / lw
    const float* saved; const float* grad; float* dq; float* coef;             // backward
};

// the lane's four floats of a row: floats 4 gl .. 4 gl + 3 (VEC) or gl, gl + 64, gl + 128, gl + 192 (the scalar path, L = 64);
// zeros past d and for an absent row
template <bool VEC>
__device__ __forceinline__ f32x4 neg_slice(const float* __restrict__ row, int gl, int d) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (row) {
        if constexpr (VEC) {
            if (4 * gl < d) v = *(const f32x4*)(row + 4 * gl);
        } else {
#pragma unroll
            for (int m = 0; m < 4; ++m)
                if (gl + 64 * m < d) v[m] = row[gl + 64 * m];
        }
    }
    return v;
}

// An entry of neg as the loops keep it, 32 bits (N < 2^31: the launch says so): the node id, -1 for the padding, -2 for
// anything else — the query is then invalid.  Compared against the range before it addresses anything.
__device__ __forceinline__ int neg_id32(int64_t v, int64_t N) {
    return (uint64_t)v < (uint64_t)N ? (int)v : (v == -1 ? -1 : -2);
}

// The same four floats of row `id` of c for the loops: a load WITHOUT a branch around it.  An entry that names no row (id < 0)
// reads row 0 and a lane past d reads the row's first floats — both inside c, which has N >= 1 rows — and the value is dropped
// by a select.  A load under a branch gets a wait for all outstanding loads at the branch's end: the rows of a step then
// arrive one after the other instead of together.
template <bool VEC>
__device__ __forceinline__ f32x4 neg_row(const float* __restrict__ c, int id, int gl, int d) {
    const bool in = id >= 0;
    const float* __restrict__ row = c + (size_t)(in ? id : 0) * d;
    f32x4 v;
    if constexpr (VEC) {
        const bool has = 4 * gl < d;
        const f32x4 x = *(const f32x4*)(row + (has ? 4 * gl : 0));
#pragma unroll
        for (int m = 0; m < 4; ++m) v[m] = in && has ? x[m] : 0.f;
    } else {
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const bool has = gl + 64 * m < d;
            const float x = row[has ? gl + 64 * m : 0];
            v[m] = in && has ? x : 0.f;
        }
    }
    return v;
}
// entry j of a row of neg in the loops' form, -1 past K: the load is of an entry inside the row in every case
__device__ __forceinline__ int neg_entry(const int64_t* __restrict__ nrow, int64_t j, int64_t K, int64_t N) {
    const int v = neg_id32(nrow[j < K ? j : K - 1], N);
    return j < K ? v : -1;
}

__device__ __forceinline__ float neg_xor(float v, int mask) { return __shfl_xor(v, mask, 64); }

// sum over the group of L lanes that holds the lane, in every lane of it; all 64 lanes take part
template <int L>
__device__ __forceinline__ float group_sum(float v) {
    v += dpp_take<0xB1, 0xF>(v);                          // quad_perm [1,0,3,2]
    v += dpp_take<0x4E, 0xF>(v);                          // quad_perm [2,3,0,1]
    v += dpp_take<0x141, 0xF>(v);                         // row_half_mirror: 8 lanes
    if constexpr (L >= 16) v += dpp_take<0x140, 0xF>(v);  // row_mirror: 16 lanes
    if constexpr (L >= 32) v += neg_xor(v, 16);
    if constexpr (L >= 64) v += neg_xor(v, 32);
    return v;
}

// what both kernels know of their query before the first negative
struct NegQuery {
    int64_t tg, lo, hi;          // target; the query's list [lo, hi) of filt_idx
    bool ok;                     // row id, target and list bounds in range
    f32x4 qv, tv;                // the lane's floats of q_i and of the target's row (zeros when !ok)
    float tb;                    // bias[target] (0 without a bias)
};

template <bool VEC, bool BIAS>
__device__ __forceinline__ NegQuery neg_open(const NegArgs& a, int64_t i, int gl) {
    NegQuery s;
    const int64_t r = a.iq ? a.iq[i] : i;
    s.tg = a.target[i];
    s.ok = (uint64_t)r < (uint64_t)a.rows_q && (uint64_t)s.tg < (uint64_t)a.N;
    s.lo = s.hi = 0;
    if (a.filt_ptr) {
        s.lo = a.filt_ptr[i];
        s.hi = a.filt_ptr[i + 1];
        if (s.lo < 0 || s.hi > a.nnz || s.lo > s.hi) { s.ok = false; s.lo = s.hi = 0; }
    }
    s.qv = neg_slice<VEC>(s.ok ? a.q + (size_t)r * a.d : nullptr, gl, a.d);
    s.tv = neg_slice<VEC>(s.ok ? a.c + (size_t)s.tg * a.d : nullptr, gl, a.d);
    s.tb = 0.f;
    if constexpr (BIAS) s.tb = s.ok ? a.bias[s.tg] : 0.f;
    return s;
}

}  // namespace ghf
