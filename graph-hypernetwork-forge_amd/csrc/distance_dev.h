// distance_dev.h — the distance chain that distance.hip and pairwise.hip (§26) share: D(x, y) of a group's
// row pair with what its gradient needs (dist_eval), g = dD / dx (dist_grad) and, over the two, the score policy DistScore<M>
// of the per-query kernel, under GHF_DIST_L1 / L2 / COMPLEX.  The geometry and the kernel are negatives_dev.h's.
#pragma once
#include "common.h"
#include "negatives_dev.h"
#include "../../include/ghf_distance.h"

namespace ghf {

__device__ __forceinline__ float dist_sqrt(float v) { return __builtin_amdgcn_sqrtf(v); }

// D(x, y) in every lane of the group, delta = x - y of the lane's four floats in dl and (COMPLEX) the modulus of each
// float's pair in rho.  All 64 lanes take part.
template <int M, int L, bool VEC>
__device__ __forceinline__ float dist_eval(const f32x4 x, const f32x4 y, int gl, f32x4& dl, f32x4& rho) {
#pragma clang fp contract(off)
#pragma unroll
    for (int m = 0; m < 4; ++m) dl[m] = x[m] - y[m];
    rho = f32x4{0.f, 0.f, 0.f, 0.f};
    if constexpr (M == GHF_DIST_L1) {
        return group_sum<L>(((fabsf(dl[0]) + fabsf(dl[1])) + fabsf(dl[2])) + fabsf(dl[3]));
    } else if constexpr (M == GHF_DIST_L2) {
        return dist_sqrt(group_sum<L>(fmaf(dl[3], dl[3], fmaf(dl[2], dl[2], fmaf(dl[1], dl[1], dl[0] * dl[0])))));
    } else if constexpr (VEC) {                                  // floats 4 gl .. 4 gl + 3: two pairs of the lane's own
        const float r0 = dist_sqrt(fmaf(dl[1], dl[1], dl[0] * dl[0])), r1 = dist_sqrt(fmaf(dl[3], dl[3], dl[2] * dl[2]));
        rho = f32x4{r0, r0, r1, r1};
        return group_sum<L>(r0 + r1);
    } else {                                                     // floats gl + 64 m: the pair's other half is the lane gl ^ 1
        float part = 0.f;
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const float sq = dl[m] * dl[m];
            rho[m] = dist_sqrt(sq + dpp_take<0xB1, 0xF>(sq));    // quad_perm [1,0,3,2]; a + b = b + a: the same bits in both
            part += (gl & 1) == 0 ? rho[m] : 0.f;
        }
        return group_sum<L>(part);
    }
}

// g = dD / dx of the lane's four floats, from what dist_eval left
template <int M>
__device__ __forceinline__ f32x4 dist_grad(const f32x4 dl, const f32x4 rho, float D) {
    f32x4 g;
    if constexpr (M == GHF_DIST_L1) {
#pragma unroll
        for (int m = 0; m < 4; ++m) g[m] = dl[m] > 0.f ? 1.f : (dl[m] < 0.f ? -1.f : 0.f);
    } else if constexpr (M == GHF_DIST_L2) {
        const float r = D > 0.f ? __builtin_amdgcn_rcpf(D) : 0.f;
#pragma unroll
        for (int m = 0; m < 4; ++m) g[m] = dl[m] * r;
    } else {
        const float r0 = rho[0] > 0.f ? __builtin_amdgcn_rcpf(rho[0]) : 0.f, r1 = rho[1] > 0.f ? __builtin_amdgcn_rcpf(rho[1]) : 0.f;
        const float r2 = rho[2] > 0.f ? __builtin_amdgcn_rcpf(rho[2]) : 0.f, r3 = rho[3] > 0.f ? __builtin_amdgcn_rcpf(rho[3]) : 0.f;
        g = f32x4{dl[0] * r0, dl[1] * r1, dl[2] * r2, dl[3] * r3};
    }
    return g;
}

// the score policy of pq_kernel (negatives_dev.h): s = -D, and ds / dx = -g with the sign left to the kernel
template <int M>
struct DistScore {
    static constexpr bool NEG = true, BIAS = false;
    struct Saved { f32x4 dl, rho; };
    template <int L, bool VEC>
    static __device__ __forceinline__ float eval(const f32x4 x, const f32x4 y, int gl, Saved& k) {
        return -dist_eval<M, L, VEC>(x, y, gl, k.dl, k.rho);
    }
    static __device__ __forceinline__ f32x4 grad(const Saved& k, const f32x4, float s) { return dist_grad<M>(k.dl, k.rho, -s); }
};

}  // namespace ghf
