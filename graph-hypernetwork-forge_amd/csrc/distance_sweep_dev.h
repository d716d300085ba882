// distance_sweep_dev.h — what distance_sweep.hip (rank, top-k), distance_loss.hip (the two losses and their
// backward; §25) and pairwise_sweep.hip (§27) share: the tile constants, the one chain every distance of a pair equals bit for
// bit, the types through which a wave-uniform row is read from the constant address space (scalar loads), and the kernel that
// forms the targets' scores by that chain.
#pragma once
#include "common.h"
#include "rank_sweep.h"
#include "../../include/ghf_distance.h"

namespace ghf {

constexpr int DS_TQ = 64;                    // queries per workgroup
constexpr int DS_RQ = 16;                    // queries per wave
constexpr int DS_RC = 4;                     // candidates per lane
constexpr int DS_CT = 64 * DS_RC;            // candidates per step
constexpr int DS_BK = 16;                    // columns per step
constexpr int DS_LDC = DS_BK + 4;            // LDS row stride in floats
constexpr int DS_NL = DS_CT * (DS_BK / 4) / 256;    // 16-byte pieces a thread fetches per step
constexpr int DS_MIN_TILES = 4;              // tiles per slab, at the least

// ---- the chain --------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float dsweep_sqrt(float v) { return __builtin_amdgcn_sqrtf(v); }

// four consecutive k of one pair's chain: x the query's floats, y the candidate's
template <int M>
__device__ __forceinline__ float dist_step4(float acc, const f32x4 x, const f32x4 y) {
#pragma clang fp contract(off)
    const float d0 = x[0] - y[0], d1 = x[1] - y[1], d2 = x[2] - y[2], d3 = x[3] - y[3];
    if constexpr (M == GHF_DIST_L1) {
        acc = acc + fabsf(d0);
        acc = acc + fabsf(d1);
        acc = acc + fabsf(d2);
        acc = acc + fabsf(d3);
    } else if constexpr (M == GHF_DIST_L2) {
        acc = fmaf(d0, d0, acc);
        acc = fmaf(d1, d1, acc);
        acc = fmaf(d2, d2, acc);
        acc = fmaf(d3, d3, acc);
    } else {
        const float r0 = dsweep_sqrt(fmaf(d1, d1, d0 * d0));
        acc = acc + r0;
        const float r1 = dsweep_sqrt(fmaf(d3, d3, d2 * d2));
        acc = acc + r1;
    }
    return acc;
}

template <int M>
__device__ __forceinline__ float dist_finish(float acc) { return M == GHF_DIST_L2 ? dsweep_sqrt(acc) : acc; }

template <int M>
__device__ __forceinline__ float dist_chain_m(const float* __restrict__ x, const float* __restrict__ y, int d, bool vec) {
    float acc = 0.f;
    for (int k = 0; k < d; k += 4) acc = dist_step4<M>(acc, load_k4(x, k, d, vec), load_k4(y, k, d, vec));
    return dist_finish<M>(acc);
}

// D(x, y) under `metric`: the chain every accumulator of the tile equals
__device__ __forceinline__ float dist_chain(int metric, const float* __restrict__ x, const float* __restrict__ y, int d, bool vec) {
    if (metric == GHF_DIST_L1) return dist_chain_m<GHF_DIST_L1>(x, y, d, vec);
    if (metric == GHF_DIST_L2) return dist_chain_m<GHF_DIST_L2>(x, y, d, vec);
    return dist_chain_m<GHF_DIST_COMPLEX>(x, y, d, vec);
}

typedef const float __attribute__((address_space(4))) ds_cfloat;
typedef const f32x4 __attribute__((address_space(4))) ds_cf32x4;

// one thread per query, behind the pass that validated the ids: the target's score by the tile's chain, from its own row of c
// (node id; the target need not be a candidate); NaN for a query that is not valid
static __global__ __launch_bounds__(256) void dist_target_kernel(int metric, const float* __restrict__ q, const float* __restrict__ c,
                                                                 const int64_t* __restrict__ iq, const int64_t* __restrict__ target,
                                                                 const int* __restrict__ valid, int64_t B, int d,
                                                                 float* __restrict__ t) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= B) return;
    float v = __int_as_float(0x7FC00000);
    if (valid[i]) {
        const int64_t r = iq ? iq[i] : i;
        v = -dist_chain(metric, q + (size_t)r * d, c + (size_t)target[i] * d, d, rows_vec(q, d) && rows_vec(c, d));
    }
    t[i] = v;
}

}  // namespace ghf
