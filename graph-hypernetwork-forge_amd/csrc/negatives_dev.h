// negatives_dev.h — the per-query family's device code (the fold: §23): the geometry of a query
// against ITS OWN rows of c — the lane's slice of a row, the branch-free id and row loads of the loops, the butterfly over a
// group of L lanes, what a kernel knows of its query before the first negative — and, over them, the ONE kernel template
// (pq_kernel: a score policy, an epilogue, forward or backward), its launch ladder and its open check.  negatives.hip,
// distance.hip and pairwise.hip each turn their public selectors into its template parameters and instantiate their own kernels.
#pragma once
#include "common.h"
#include "rank_sweep.h"
#include "negatives.h"

namespace ghf {

constexpr int NG_U = 8;                          // row loads a lane keeps in flight
constexpr int NG_SPLIT_K = 256;                  // above it a query's positions are dealt to the four waves of a workgroup
static inline int neg_waves(int64_t K) { return K > NG_SPLIT_K ? 4 : 1; }

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

// what a kernel knows of its query before the first negative
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

// ---- the score, as a policy ------------------------------------------------------------------------------------------------
// eval<L, VEC>(x, y, gl, k): s(x, y) in every lane of the group, and in k what grad needs of it; grad(k, y, s): the lane's four
// floats of ds / dx up to the sign NEG, which the kernel puts on the coefficient (fmaf(-G, g, acc) stays one instruction).
// BIAS: whether a per-candidate bias may join the score.  The distance policies are distance_dev.h's.
__device__ __forceinline__ float neg_dot(f32x4 x, f32x4 y) {
    return fmaf(x[3], y[3], fmaf(x[2], y[2], fmaf(x[1], y[1], x[0] * y[0])));
}

struct DotScore {
    static constexpr bool NEG = false, BIAS = true;
    struct Saved {};
    template <int L, bool VEC>
    static __device__ __forceinline__ float eval(const f32x4 x, const f32x4 y, int, Saved&) { return group_sum<L>(neg_dot(x, y)); }
    static __device__ __forceinline__ f32x4 grad(const Saved&, const f32x4 y, float) { return y; }
};

// ---- the epilogue's partial, by value --------------------------------------------------------------------------------------
// rank: c0, c1 = greater, equal.  softmax: ms = (max, sum).  negsamp: (ms, t) = §19's triple.  pairwise: ms[1] = the sum of
// phi, c0, c1 = n_i, the violated pairs.  Every merge is symmetric in its two arguments.
struct PqPart { f32x2 ms; float t; int c0, c1; };

template <PqEpi E>
__device__ __forceinline__ PqPart pq_merge(PqPart x, const PqPart y) {
    if constexpr (E == PqEpi::Softmax) {
        x.ms = lse_merge(x.ms, y.ms);
    } else if constexpr (E == PqEpi::Negsamp) {
        const NegTriple r = neg_merge(NegTriple{x.ms[0], x.ms[1], x.t}, NegTriple{y.ms[0], y.ms[1], y.t});
        x.ms = f32x2{r.m, r.s};
        x.t = r.t;
    } else {
        if constexpr (pq_is_pair(E)) x.ms[1] += y.ms[1];
        x.c0 += y.c0;
        x.c1 += y.c1;
    }
    return x;
}
// the partial of the lane `w` away (the two losses with a maximum; the sums and counts are added in the kernel)
template <PqEpi E>
__device__ __forceinline__ PqPart pq_xor(PqPart p, int w) {
    if constexpr (E == PqEpi::Softmax || E == PqEpi::Negsamp) p.ms = f32x2{neg_xor(p.ms[0], w), neg_xor(p.ms[1], w)};
    if constexpr (E == PqEpi::Negsamp) p.t = neg_xor(p.t, w);
    return p;
}
// a wave's partial into its LDS slots and back
template <PqEpi E>
__device__ __forceinline__ void pq_put(float* f, int* n, const PqPart p) {
    if constexpr (E == PqEpi::Softmax || E == PqEpi::Negsamp) { f[0] = p.ms[0]; f[1] = p.ms[1]; }
    if constexpr (E == PqEpi::Negsamp) f[2] = p.t;
    if constexpr (pq_is_pair(E)) f[0] = p.ms[1];
    if constexpr (E == PqEpi::Rank || pq_is_pair(E)) { n[0] = p.c0; n[1] = p.c1; }
}
template <PqEpi E>
__device__ __forceinline__ PqPart pq_get(const float* f, const int* n) {
    PqPart p = {f32x2{0.f, 0.f}, 0.f, 0, 0};
    if constexpr (E == PqEpi::Softmax || E == PqEpi::Negsamp) p.ms = f32x2{f[0], f[1]};
    if constexpr (E == PqEpi::Negsamp) p.t = f[2];
    if constexpr (pq_is_pair(E)) p.ms[1] = f[0];
    if constexpr (E == PqEpi::Rank || pq_is_pair(E)) { p.c0 = n[0]; p.c1 = n[1]; }
    return p;
}

// ---- the kernel ------------------------------------------------------------------------------------------------------------
// One text for every member: the score policy P, the epilogue E and the direction choose its arms.  The id walk, the row and
// bias loads and the filter searches are written once.  The walk's state stays in plain locals, `bad` never leaves the
// body, and the W > 1 hand-off's barrier and early return stand here, not in a helper: each of those forms changed what the
// compiler made of every kernel (§23).
template <class P, int L, bool VEC, PqEpi E, bool BWD, bool BIAS, int W>
__global__ __launch_bounds__(256) void pq_kernel(const NegArgs a) {
#pragma clang fp contract(off)                           // z is rounded before the margin is added, as in negsamp.hip
    static_assert(!(BWD && E == PqEpi::Rank), "the rank has no backward");
    static_assert(P::BIAS || !BIAS, "no bias under this score");
    constexpr bool PAIR = pq_is_pair(E);
    constexpr int G = 64 / L;                            // rows per wave instruction
    constexpr int STEP = NG_U * G;                       // positions per step of a wave
    const int lane = threadIdx.x & 63, gl = lane & (L - 1), g = lane / L, wv = threadIdx.x >> 6;
    const int64_t i = W == 1 ? (int64_t)blockIdx.x * 4 + wv : (int64_t)blockIdx.x;
    const int sub = W == 1 ? 0 : wv;                     // the wave's place among the query's W
    if (W == 1 && i >= a.B) return;                      // the whole wave, and no barrier on this path
    const int d = a.d;
    NegQuery s = neg_open<VEC, BIAS>(a, i, gl);
    bool bad = false;                                    // forward: a listed id or a negative outside its range
    if constexpr (!BWD)
        for (int64_t e = s.lo + lane; e < s.hi; e += 64) bad |= (uint64_t)a.filt_idx[e] >= (uint64_t)a.N;
    // backward: what the forward saved says whether the query takes part — lse or lw (NaN: it does not), or the pair count
    // (-1: it does not; 0: no pair, an all-zero row).  Constants, each formed once: as variables assigned in an `if constexpr`
    // they changed the compiler's output (§23).
    const int n = BWD && PAIR ? a.saved_n[i] : 0;
    const float sv = BWD && !PAIR ? a.saved[i] : 0.f;
    const bool part = !BWD || (s.ok && (PAIR ? n >= 0 : sv == sv));
    const float gs = BWD ? a.grad[i] * a.scale : 0.f;
    const float wi = PAIR && a.normalize ? gs * (n > 0 ? 1.f / (float)n : 0.f) : gs;
    typename P::Saved tk;
    const float t = P::template eval<L, VEC>(s.qv, s.tv, gl, tk);
    const float tb = BIAS ? t + s.tb : t;                // rank: the target's score with its bias entry
    float zt = 0.f;                                      // pairwise: every term needs z_it; the others form it after the merge
    if constexpr (PAIR) {
        if constexpr (BIAS) zt = fmaf(a.scale, t, s.tb);
        else zt = a.scale * t;
    }
    float* __restrict__ crow = BWD ? a.coef + (size_t)i * (a.K + 1) : nullptr;

    float F = 0.f;                                       // pairwise: sum of phi(u) over the group's positions, in order
    int c0 = 0, c1 = 0;                                  // rank: greater, equal; pairwise: n_i, violated (K < 2^31)
    float m = -INFINITY, S = 0.f, T = 0.f;               // softmax: (m, S); negsamp: (m, S, T) of alpha z
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};                    // backward: dq of the lane's floats
    float Gs = 0.f;                                      // pairwise backward: sum of G_ij over the group's positions, in order

    const int64_t* __restrict__ nrow = a.neg + (size_t)i * a.K;
    int idn[NG_U];
#pragma unroll
    for (int u = 0; u < NG_U; ++u) idn[u] = neg_entry(nrow, sub * STEP + u * G + g, a.K, a.N);
    for (int64_t base = (int64_t)sub * STEP; base < a.K; base += W * STEP) {
        int id[NG_U];
        f32x4 row[NG_U];
        float b[NG_U];
        bool live[NG_U];
#pragma unroll
        for (int u = 0; u < NG_U; ++u) id[u] = idn[u];
#pragma unroll
        for (int u = 0; u < NG_U; ++u) {
            const int64_t j = base + W * STEP + u * G + g;
            idn[u] = neg_entry(nrow, j, a.K, a.N);
        }
#pragma unroll
        for (int u = 0; u < NG_U; ++u) {
            const bool in = part && id[u] >= 0;
            if constexpr (!BWD) bad |= id[u] == -2;
            row[u] = neg_row<VEC>(a.c, BWD ? (in ? id[u] : -1) : id[u], gl, d);
            b[u] = 0.f;
            if constexpr (BIAS) { const float x = a.bias[in ? id[u] : 0]; b[u] = in ? x : 0.f; }
            live[u] = in;
        }
#pragma unroll
        for (int u = 0; u < NG_U; ++u)
            live[u] = live[u] && (int64_t)id[u] != s.tg && !(s.hi > s.lo && in_filter(a.filt_idx, s.lo, s.hi, (int64_t)id[u]));
#pragma unroll
        for (int u = 0; u < NG_U; ++u) {
            if constexpr (!BWD && (E == PqEpi::Rank || PAIR)) {
                // One row at a time, as the losses' running sums force it.  Nothing else orders the eight scores of a step in
                // these two branch-free arms, and computed side by side they cost 30 VGPRs and with them the fourth wave per
                // SIMD: the empty statement makes row u wait for the count (rank) or the sum (pairwise) of row u - 1.
                float r0 = row[u][0];
                if constexpr (PAIR) asm volatile("" : "+v"(r0), "+v"(F));
                else asm volatile("" : "+v"(r0), "+v"(c0));
                row[u][0] = r0;
            }
            typename P::Saved k;
            const float sc = P::template eval<L, VEC>(s.qv, row[u], gl, k);
            float z;
            if constexpr (BIAS) z = fmaf(a.scale, sc, b[u]);
            else z = a.scale * sc;
            if constexpr (!BWD && E == PqEpi::Rank) {
                const float sb = BIAS ? sc + b[u] : sc;
                c0 += live[u] && sb > tb ? 1 : 0;
                c1 += live[u] && sb == tb ? 1 : 0;
            } else if constexpr (!BWD && PAIR) {         // no branch: a position outside J_i adds 0.f and 0
                const float y = (z - zt) + a.margin;
                float phi;
                if constexpr (E == PqEpi::Hinge) phi = y <= 0.f ? 0.f : y;     // not fmaxf: a NaN stays a NaN
                else phi = softplus(y);
                F += live[u] ? phi : 0.f;
                c0 += live[u] ? 1 : 0;
                c1 += live[u] && y > 0.f ? 1 : 0;
            } else if constexpr (!BWD) {
                if (live[u]) {
                    const float x = E == PqEpi::Negsamp ? a.alpha * z : z;
                    float sp = 0.f;
                    if constexpr (E == PqEpi::Negsamp) sp = softplus(z + a.margin);
                    if (x > m) {                          // the max rises: rescale what is there (exp(-inf) = 0 at the first)
                        const float e = __expf(m - x);
                        S = fmaf(S, e, 1.f);
                        T = fmaf(T, e, sp);
                        m = x;
                    } else if (x > -INFINITY) {
                        const float w = __expf(x - m);
                        S += w;
                        T = fmaf(w, sp, T);
                    } else if (x != x) {                  // a NaN on its way out
                        m = S = T = x;
                    }
                }
            } else {
                float gv;
                if constexpr (E == PqEpi::Softmax) {
                    gv = gs * __expf(z - sv);
                } else if constexpr (E == PqEpi::Negsamp) {
                    const float y = z + a.margin;
                    const float e = __expf(-fabsf(y)), rcp = __builtin_amdgcn_rcpf(1.f + e);
                    const float w = sv > -INFINITY ? __expf(fmaf(a.alpha, z, -sv)) : 0.f;
                    gv = gs * (w * (y >= 0.f ? rcp : e * rcp));
                } else {
                    const float y = (z - zt) + a.margin;
                    if constexpr (E == PqEpi::Hinge) {
                        gv = y > 0.f ? wi : 0.f;
                    } else {                             // sigmoid(y), as the negsamp arm forms it
                        const float e = __expf(-fabsf(y)), rcp = __builtin_amdgcn_rcpf(1.f + e);
                        gv = wi * (y >= 0.f ? rcp : e * rcp);
                    }
                }
                gv = live[u] ? gv : 0.f;
                const int64_t j = base + u * G + g;
                if (gl == 0 && j < a.K) crow[j] = gv;
                if constexpr (PAIR) Gs += gv;
                // positions in order within the group; a zero coefficient adds nothing, whatever the row holds
                const f32x4 gr = P::grad(k, row[u], sc);
                const float cg = P::NEG ? -gv : gv;
                const f32x4 nx = {fmaf(cg, gr[0], acc[0]), fmaf(cg, gr[1], acc[1]), fmaf(cg, gr[2], acc[2]), fmaf(cg, gr[3], acc[3])};
                acc = gv != 0.f ? nx : acc;
            }
        }
    }

    if constexpr (!BWD) {
        bad = __any(bad);
        // the groups' partials, merged in a fixed tree; then the waves' (W > 1), in wave order, by wave 0
        if constexpr (E == PqEpi::Rank || PAIR) {        // sums and counts one by one, on the loop's own variables (§23)
#pragma unroll
            for (int w = L; w < 64; w *= 2) {
                if constexpr (PAIR) F += neg_xor(F, w);
                c0 += __shfl_xor(c0, w, 64);
                c1 += __shfl_xor(c1, w, 64);
            }
        }
        PqPart p = {f32x2{m, PAIR ? F : S}, T, c0, c1};
        if constexpr (E == PqEpi::Softmax || E == PqEpi::Negsamp) {
#pragma unroll
            for (int w = L; w < 64; w *= 2) p = pq_merge<E>(p, pq_xor<E>(p, w));
        }
        if constexpr (W > 1) {
            __shared__ float shf[W][PAIR ? 1 : 4];
            __shared__ int shi[W][4];
            if (lane == 0) { pq_put<E>(shf[wv], shi[wv], p); shi[wv][2] = bad; }
            __syncthreads();
            if (wv != 0) return;
            for (int w = 1; w < W; ++w) { p = pq_merge<E>(p, pq_get<E>(shf[w], shi[w])); bad |= shi[w][2] != 0; }
        }
        s.ok = s.ok && !bad;
        if constexpr (!PAIR) {
            if constexpr (BIAS) zt = fmaf(a.scale, t, s.tb);
            else zt = a.scale * t;
        }
        if constexpr (E == PqEpi::Rank) {
            if (lane == 0) {
                a.greater[i] = s.ok ? p.c0 : -1;
                a.equal[i] = s.ok ? p.c1 : -1;
            }
        } else if constexpr (E == PqEpi::Softmax) {
            p.ms = lse_merge(p.ms, f32x2{zt, 1.f});      // the target enters exactly once
            const float lse = p.ms[0] + logf(p.ms[1]);
            if (lane == 0) {
                a.loss[i] = s.ok ? lse - zt : __int_as_float(0x7FC00000);
                a.aux[i] = s.ok ? lse : __int_as_float(0x7FC00000);
            }
        } else if constexpr (E == PqEpi::Negsamp) {
            const bool any = p.ms[1] > 0.f;              // no negatives: the positive term alone, lw = -inf
            const float lw = any ? p.ms[0] + logf(p.ms[1]) : -INFINITY;
            const float l = softplus(-(zt + a.margin)) + (any ? p.t / p.ms[1] : 0.f);
            if (lane == 0) {
                a.loss[i] = s.ok ? l : __int_as_float(0x7FC00000);
                a.aux[i] = s.ok ? lw : __int_as_float(0x7FC00000);
            }
        } else {
            float l = p.ms[1];
            if (a.normalize) l = p.c0 > 0 ? p.ms[1] * (1.f / (float)p.c0) : 0.f;
            if (lane == 0) {
                a.loss[i] = s.ok ? l : __int_as_float(0x7FC00000);
                a.count[i] = s.ok ? p.c0 : -1;
                a.active[i] = s.ok ? p.c1 : -1;
            }
        }
    } else {
#pragma unroll
        for (int w = L; w < 64; w *= 2) {
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] += neg_xor(acc[e], w);
            if constexpr (PAIR) Gs += neg_xor(Gs, w);
        }
        if constexpr (W > 1) {                           // the waves' sums, in wave order, by wave 0
            __shared__ f32x4 shq[W][64];
            __shared__ float shg[W];
            shq[wv][lane] = acc;
            if constexpr (PAIR)
                if (lane == 0) shg[wv] = Gs;
            __syncthreads();
            if (wv != 0) return;
            for (int w = 1; w < W; ++w) {
                const f32x4 o = shq[w][lane];
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[e] += o[e];
                if constexpr (PAIR) Gs += shg[w];
            }
        }
        // the target's entry, last; pairwise: minus the row's sum
        float gt;
        if constexpr (!PAIR) {
            if constexpr (BIAS) zt = fmaf(a.scale, t, s.tb);
            else zt = a.scale * t;
        }
        if constexpr (E == PqEpi::Softmax) {
            gt = gs * (__expf(zt - sv) - 1.f);
        } else if constexpr (E == PqEpi::Negsamp) {
            const float y = zt + a.margin;
            const float e = __expf(-fabsf(y)), rcp = __builtin_amdgcn_rcpf(1.f + e);
            gt = -gs * (y >= 0.f ? e * rcp : rcp);
        } else {
            gt = 0.f - Gs;
        }
        gt = part ? gt : 0.f;
        if (gt != 0.f) {
            const f32x4 gr = P::grad(tk, s.tv, t);
            const float cg = P::NEG ? -gt : gt;
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] = fmaf(cg, gr[e], acc[e]);
        }
        if (lane == 0) crow[a.K] = gt;
        if (g == 0) {
            float* __restrict__ out = a.dq + (size_t)i * d;
            if constexpr (VEC) {                         // (a dq that is not 16-byte aligned takes four stores: the path, and with
                if (4 * gl < d) {                        // it the order of every sum, is the forward's — q, c and d choose it)
                    if (((uintptr_t)out & 15) == 0) {
                        *(f32x4*)(out + 4 * gl) = acc;
                    } else {
#pragma unroll
                        for (int m = 0; m < 4; ++m) out[4 * gl + m] = acc[m];
                    }
                }
            } else {
#pragma unroll
                for (int m = 0; m < 4; ++m)
                    if (gl + 64 * m < d) out[gl + 64 * m] = acc[m];
            }
        }
    }
}

// ---- launches --------------------------------------------------------------------------------------------------------------
// What every member checks before it launches, and last the guard of the mode trap: an argument block whose outputs for its
// epilogue are missing is refused here, so a wrong dispatch ends as a message and not as a store through a null pointer.
static int pq_open_launch(const char* op, PqEpi e, bool bwd, const NegArgs& a, size_t ws_bytes) {
    GHF_REQUIRE(a.d > 0 && a.rows_q > 0 && a.N > 0 && a.B > 0 && a.K > 0 && a.nnz >= 0, "%s: bad shape", op);
    if (a.d > RK_MAX_D) return set_err(GHF_EUNSUPPORTED, "%s: d = %d exceeds %d", op, a.d, RK_MAX_D);
    GHF_REQUIRE(a.N < (int64_t)1 << 31, "%s: N out of range", op);            // the loops keep ids in 32 bits (neg_id32)
    const size_t need = neg_workspace_bytes(a.B, a.K, a.d, a.nnz);
    GHF_REQUIRE(need > 0, "%s: B (K + 1) out of range", op);
    GHF_REQUIRE(a.iq || a.B <= a.rows_q, "%s: B exceeds the rows of q", op);
    GHF_REQUIRE(ws_bytes >= need, "%s: workspace of %zu bytes, need %zu", op, ws_bytes, need);
    bool outs;
    if (bwd) outs = e != PqEpi::Rank && (pq_is_pair(e) ? a.saved_n != nullptr : a.saved != nullptr) && a.grad && a.dq && a.coef;
    else if (e == PqEpi::Rank) outs = a.greater && a.equal;
    else if (pq_is_pair(e)) outs = a.loss && a.count && a.active;
    else outs = a.loss && a.aux;
    GHF_REQUIRE(outs, "%s: the argument block lacks the outputs of its epilogue", op);
    return GHF_OK;
}

// the one ladder: vec from d and the alignment of q | c (forward and backward alike), L from d, W from neg_waves(K), BIAS
template <class P, PqEpi E, bool BWD, bool BIAS, int W>
static int pq_launch_path(const NegArgs& a, hipStream_t stream) {
    const unsigned grid = (unsigned)(W == 1 ? cdiv(a.B, 4) : a.B);
    const bool vec = (a.d & 3) == 0 && (((uintptr_t)a.q | (uintptr_t)a.c) & 15) == 0;
    if (!vec) pq_kernel<P, 64, false, E, BWD, BIAS, W><<<grid, 256, 0, stream>>>(a);
    else if (a.d <= 32) pq_kernel<P, 8, true, E, BWD, BIAS, W><<<grid, 256, 0, stream>>>(a);
    else if (a.d <= 64) pq_kernel<P, 16, true, E, BWD, BIAS, W><<<grid, 256, 0, stream>>>(a);
    else if (a.d <= 128) pq_kernel<P, 32, true, E, BWD, BIAS, W><<<grid, 256, 0, stream>>>(a);
    else pq_kernel<P, 64, true, E, BWD, BIAS, W><<<grid, 256, 0, stream>>>(a);
    GHF_LAUNCH_CHECK();
    return GHF_OK;
}

template <class P, PqEpi E, bool BWD>
static int pq_launch(const NegArgs& a, hipStream_t stream) {
    const bool one = neg_waves(a.K) == 1;
    if constexpr (P::BIAS) {
        if (a.bias) return one ? pq_launch_path<P, E, BWD, true, 1>(a, stream) : pq_launch_path<P, E, BWD, true, 4>(a, stream);
    }
    return one ? pq_launch_path<P, E, BWD, false, 1>(a, stream) : pq_launch_path<P, E, BWD, false, 4>(a, stream);
}

// rank and the two set losses under the score P (negatives.hip, distance.hip); pq_open_launch has refused a rank backward
template <class P>
static int pq_launch_set(PqEpi e, bool bwd, const NegArgs& a, hipStream_t stream) {
    if (e == PqEpi::Rank) return pq_launch<P, PqEpi::Rank, false>(a, stream);
    if (e == PqEpi::Softmax) return bwd ? pq_launch<P, PqEpi::Softmax, true>(a, stream) : pq_launch<P, PqEpi::Softmax, false>(a, stream);
    if (e == PqEpi::Negsamp) return bwd ? pq_launch<P, PqEpi::Negsamp, true>(a, stream) : pq_launch<P, PqEpi::Negsamp, false>(a, stream);
    return set_err(GHF_EINVAL, "per-query launch: a pairwise epilogue outside pairwise.hip");
}

}  // namespace ghf
