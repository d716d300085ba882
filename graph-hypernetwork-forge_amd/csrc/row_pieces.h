// row_pieces.h — the one place a row is cut into its GHF_WLAYOUT_SPLIT2H pieces and counted for the range guard.
//
// Every kernel that writes a row in the two-fp16-piece form follows the same protocol (common.h has its arithmetic): the
// row's largest magnitude picks the power of two, every element is cut into hi + lo, the row's 2^-s scale goes behind the
// pieces, and the row's far-down and nonzero elements are counted for GHF_RANGE_ROWS.  The kernels differ in which lanes
// hold a row (a lane group, below) and in how they store the pieces (their own vector width: the stores stay with them).
#pragma once

#include "common.h"

namespace ghf {

// ---- lane groups: the lanes that hold one row; sum / max leave the same bits in every lane of a group -----------------
// G consecutive lanes, G a power of two: a butterfly (data-parallel moves inside a row of 16 lanes, exchanges above; the
// whole wave: common.h's wave_sum, the same tree up to the order of each addition's two operands)
template <int G>
struct LaneGroup {
    static_assert(G >= 2 && G <= 64 && (G & (G - 1)) == 0, "a power of two of lanes");
    static __device__ __forceinline__ bool leader(int lane) { return lane % G == 0; }
    static __device__ __forceinline__ float sum(float v) {
        if constexpr (G == 64) return wave_sum(v);
        if constexpr (G >= 2) v += dpp_take<0xB1, 0xF>(v);       // quad_perm [1,0,3,2]
        if constexpr (G >= 4) v += dpp_take<0x4E, 0xF>(v);       // quad_perm [2,3,0,1]
        if constexpr (G >= 8) v += dpp_take<0x141, 0xF>(v);      // row_half_mirror
        if constexpr (G >= 16) v += dpp_take<0x140, 0xF>(v);     // row_mirror
        if constexpr (G >= 32) v += __shfl_xor(v, 16);
        return v;
    }
    static __device__ __forceinline__ float absmax(float v) {    // of non-negative values
        if constexpr (G == 64) return wave_absmax(v);
        if constexpr (G >= 2) v = fmaxf(v, dpp_take<0xB1, 0xF>(v));
        if constexpr (G >= 4) v = fmaxf(v, dpp_take<0x4E, 0xF>(v));
        if constexpr (G >= 8) v = fmaxf(v, dpp_take<0x141, 0xF>(v));
        if constexpr (G >= 16) v = fmaxf(v, dpp_take<0x140, 0xF>(v));
        if constexpr (G >= 32) v = fmaxf(v, __shfl_xor(v, 16));
        return v;
    }
};
// the four lanes {c, c + 16, c + 32, c + 48} that hold row c of a 16x16 MFMA result
struct MfmaRowGroup {
    static __device__ __forceinline__ bool leader(int lane) { return lane < 16; }
    static __device__ __forceinline__ float sum(float v) { v += __shfl_xor(v, 16); return v + __shfl_xor(v, 32); }
    static __device__ __forceinline__ float absmax(float v) { v = fmaxf(v, __shfl_xor(v, 16)); return fmaxf(v, __shfl_xor(v, 32)); }
};

// ---- the cut ------------------------------------------------------------------------------------------------------------
// RowCut<Group> cut(mx) with mx the largest magnitude among the lane's elements; cut.piece(x, hi, lo) for each of them (the
// caller stores hi and lo); cut.finish(...) once (without `scale` where the pieces stay in registers).  Every lane of the
// wave calls all three (the reductions span the wave).
template <class Group>
struct RowCut {
    int sh, tiny = 0, nz = 0;
    float up;
    __device__ __forceinline__ explicit RowCut(float lane_absmax) : sh(split2h_shift(Group::absmax(lane_absmax))), up(pow2f(sh)) {}
    __device__ __forceinline__ void piece(float x, _Float16& hi, _Float16& lo) {
        const float xs = x * up;
        split2h(xs, hi, lo);
        tiny += range_tiny(xs);
        nz += xs != 0.f;
    }
    // `writes`: this lane is the leader of a group whose row is stored.  The counts are summed only when some row of the
    // wave has a far-down element (without one no row can raise the guard).
    __device__ __forceinline__ void finish(bool writes, int32_t* range_flag) {
        if (__ballot(tiny != 0)) {
            const int t = (int)Group::sum((float)tiny), n = (int)Group::sum((float)nz);      // (at most 1024: exact)
            if (writes) range_raise(range_flag, GHF_RANGE_ROWS, t, n);
        }
    }
    __device__ __forceinline__ void finish(bool writes, float* scale, int32_t* range_flag) {
        if (writes) *scale = pow2f(-sh);
        finish(writes, range_flag);
    }
};

// ---- LayerNorm statistics of a held row ---------------------------------------------------------------------------------
// mean and 1 / sqrt(variance + eps) of a row of D elements, n of them in this lane (x(i), i < n, in the order they are added)
// PAIRWISE (n a power of two): the lane's squared deviations are added as a tree, not one by one.  A row with one large
// entry otherwise takes n - 1 small terms onto the large one, each addition rounded at the large one's ulp — for dyadic
// data every one a tie that rounds the same way (n = 16: rstd 4.5 ulps off, which the backward's dx magnifies 60-fold).
template <class Group, int D, int n, bool PAIRWISE = false, class X>
__device__ __forceinline__ void row_mean_rstd(X x, float eps, float& mean, float& rstd) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < n; ++i) s += x(i);
    mean = Group::sum(s) * (1.0f / D);
    float var = 0.f;
    if constexpr (PAIRWISE) {
        static_assert((n & (n - 1)) == 0, "a power of two of elements");
        float q[n];
#pragma unroll
        for (int i = 0; i < n; ++i) { const float t = x(i) - mean; q[i] = t * t; }
#pragma unroll
        for (int m = n; m > 1; m >>= 1)
#pragma unroll
            for (int i = 0; i < m / 2; ++i) q[i] = q[2 * i] + q[2 * i + 1];
        var = q[0];
    } else {
#pragma unroll
        for (int i = 0; i < n; ++i) { const float t = x(i) - mean; var += t * t; }
    }
    rstd = 1.0f / sqrtf(Group::sum(var) * (1.0f / D) + eps);
}

}  // namespace ghf
