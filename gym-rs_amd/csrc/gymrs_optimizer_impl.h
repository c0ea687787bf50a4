// gymrs_optimizer_impl.h -- the kernel of gymrs_apply_gradient (include/gymrs_amd.h, "Optimizer"): every set of one head in ONE
// launch, from the fixed-point table straight into the engine's weight buffers.  gfx950.
//
// The work split.  A group of G lanes owns one set; G is the power of two from 8 to 64 that holds S (G = 64 from S = 33 on), so
// 64 / G sets share a wave and four waves a block: a population of nine-float policies spends eight lanes per set, not a wave.  Lane l
// of the group holds the parameters s = l + G*j, j < P, in registers from the load to the store.  P is 1 below G = 64 and 1, 2, 4 or
// 8 at G = 64 (S <= 512; the largest network has 450): a shape between two of them runs the next P with its surplus slots switched
// off, which is also the general path -- no shape needs another kernel.
//
// One pass over memory.  q (8 B), w, m, v and the target of all P slots are loaded before the first arithmetic, coalesced along s, and
// stored once.  A slot that is switched off (s >= S, or a group past the last set) loads element 0 of every table instead, so the
// loads are unconditional and issued back to back; what it loaded is replaced by zeros, and it stores nothing.  The table and the
// Adam state are read once per call: non-temporal, like the record rows of the other learner kernels.  Weights and target stay
// cacheable for the launch that follows.
//
// The norm stays in registers.  A lane adds the squares of its slots in ascending j as f64; its sum IS slot[l] of the rule (for
// G < 64 the slots from G on hold +0.0, and the exchanges with masks >= G add +0.0 to a non-negative sum: exact, so they are left
// out).  Then one __shfl_xor of the double per mask G/2 .. 1: IEEE addition commutes, so both partners of an exchange hold the same
// bits afterwards and every lane of the group ends with slot[0].  No LDS memory, no atomics.
//
// excluded[m] and pw[m] are loaded by lane 0 of the group and broadcast.  A skipped set stores nothing but the zeros of
// GYMRS_OPT_ZERO_GRAD; `skipped` gets one atomic per wave that skipped anything.
//
// Template axes: ADAM and CLIP.  SGD instantiates no state access, clip-off no f64 beyond the conversion of q the rule prescribes.
// Target and zeroing are wave-uniform branches around stores.
#pragma once
#include <hip/hip_runtime.h>

#include "gymrs_kernels.h"
#include "gymrs_optimizer.h"

namespace gymrs {

constexpr int kOptBlock = 256; // four waves

template <class T>
__device__ __forceinline__ T opt_load_once(const T* p)
{
    return __builtin_nontemporal_load(p);
}

template <int G, int P, bool ADAM, bool CLIP>
__global__ __launch_bounds__(kOptBlock) void optimizer_kernel(const OptimizerArgs a)
{
    static_assert(G >= 8 && G <= 64 && (G & (G - 1)) == 0 && (P == 1 || G == 64), "a group is 8 .. 64 lanes; only full waves hold more than one slot per lane");
    constexpr int kSets = kOptBlock / G; // sets per block
    const uint32_t l = threadIdx.x % G;
    const uint64_t set = (uint64_t)blockIdx.x * kSets + threadIdx.x / G;
    const bool live = set < a.n_sets; // the same for every lane of a group
    const bool lead = live && l == 0;
    const uint32_t S = a.S;
    const bool has_target = a.target != nullptr, zero = (a.flags & GYMRS_OPT_ZERO_GRAD) != 0, ascend = (a.flags & GYMRS_OPT_ASCEND) != 0;

    // ---- every load, before any arithmetic ----
    uint64_t at[P];
    bool on[P];
    unsigned long long qbits[P];
    float w[P], mo[P], vo[P], tg[P];
#pragma unroll
    for (int j = 0; j < P; ++j) {
        const uint32_t s = l + (uint32_t)(G * j);
        on[j] = live && s < S;
        at[j] = on[j] ? set * S + s : 0; // (element 0 exists: n_sets >= 1 and S >= 1)
    }
    unsigned long long excl = 0;
    float p1 = 1.0f, p2 = 1.0f;
    if (lead) { // one lane of the group
        excl = opt_load_once(a.excluded + set);
        if constexpr (ADAM) {
            p1 = opt_load_once(a.pw + 2 * set);
            p2 = opt_load_once(a.pw + 2 * set + 1);
        }
    }
#pragma unroll
    for (int j = 0; j < P; ++j) qbits[j] = opt_load_once(a.grad + at[j]);
#pragma unroll
    for (int j = 0; j < P; ++j) w[j] = a.weights[at[j]];
    if constexpr (ADAM) {
#pragma unroll
        for (int j = 0; j < P; ++j) {
            mo[j] = opt_load_once(a.m + at[j]);
            vo[j] = opt_load_once(a.v + at[j]);
        }
    }
    if (has_target) {
#pragma unroll
        for (int j = 0; j < P; ++j) tg[j] = a.target[at[j]];
    }

    // what lane 0 of the group read, for the whole group
    excl = __shfl(excl, 0, G);
    if constexpr (ADAM) {
        p1 = __shfl(p1, 0, G);
        p2 = __shfl(p2, 0, G);
    }
    const bool skip = excl != 0;

    // ---- the rule ----
    float g[P];
#pragma unroll
    for (int j = 0; j < P; ++j) g[j] = opt_gradient(on[j] ? (long long)qbits[j] : 0ll, a.grad_scale);
    if constexpr (CLIP) {
        double sum = 0.0;
#pragma unroll
        for (int j = 0; j < P; ++j) sum = sum + opt_square(g[j]);
#pragma unroll
        for (int mask = G / 2; mask >= 1; mask >>= 1) sum = sum + __shfl_xor(sum, mask, G);
        bool clipped;
        const float cs = opt_clip_scale(sum, a.max_norm, clipped);
#pragma unroll
        for (int j = 0; j < P; ++j) g[j] = clipped ? g[j] * cs : g[j];
    }
    float c1 = 1.0f, c2 = 1.0f;
    if constexpr (ADAM) opt_adam_advance(a.beta1, a.beta2, p1, p2, c1, c2);

    // ---- one store per word ----
#pragma unroll
    for (int j = 0; j < P; ++j) {
        float step;
        if constexpr (ADAM)
            step = opt_adam_step(g[j], a.lr, a.beta1, a.beta2, a.eps, c1, c2, mo[j], vo[j]);
        else
            step = opt_sgd_step(g[j], a.lr);
        const float wn = opt_apply(w[j], step, ascend);
        if (on[j] && !skip) {
            a.weights[at[j]] = wn;
            if constexpr (ADAM) {
                __builtin_nontemporal_store(mo[j], a.m + at[j]);
                __builtin_nontemporal_store(vo[j], a.v + at[j]);
            }
            if (has_target) a.target[at[j]] = opt_target(a.tau, wn, tg[j]);
        }
        if (on[j] && zero) a.grad[at[j]] = 0ull;
    }
    if (lead) {
        if constexpr (ADAM) {
            if (!skip) {
                a.pw[2 * set] = p1;
                a.pw[2 * set + 1] = p2;
            }
        }
        if (zero) a.excluded[set] = 0ull;
    }
    if (a.skipped) { // one atomic per wave that skipped anything
        const unsigned long long who = __ballot(lead && skip);
        if (who != 0 && (threadIdx.x & 63) == 0) atomicAdd(a.skipped, (unsigned long long)__popcll(who));
    }
}

// m = v = +0.0f, pw = 1.0f
__global__ __launch_bounds__(kOptBlock) void optimizer_fresh_kernel(float* m, float* v, float* pw, uint64_t words, uint64_t sets2)
{
    const uint64_t i = (uint64_t)blockIdx.x * kOptBlock + threadIdx.x;
    if (i < words) {
        m[i] = 0.0f;
        v[i] = 0.0f;
    }
    if (i < sets2) pw[i] = 1.0f;
}

template <int G, int P>
static hipError_t apply_gradient_shape(const OptimizerArgs& a, hipStream_t stream)
{
    constexpr uint32_t kSets = kOptBlock / G;
    const dim3 grid((uint32_t)(((uint64_t)a.n_sets + kSets - 1) / kSets)), block(kOptBlock);
    const bool adam = a.kind == GYMRS_OPT_ADAM, clip = a.max_norm < __builtin_inff();
    launch_begin();
    if (adam) {
        if (clip)
            hipLaunchKernelGGL((optimizer_kernel<G, P, true, true>), grid, block, 0, stream, a);
        else
            hipLaunchKernelGGL((optimizer_kernel<G, P, true, false>), grid, block, 0, stream, a);
    } else {
        if (clip)
            hipLaunchKernelGGL((optimizer_kernel<G, P, false, true>), grid, block, 0, stream, a);
        else
            hipLaunchKernelGGL((optimizer_kernel<G, P, false, false>), grid, block, 0, stream, a);
    }
    return hipGetLastError();
}

} // namespace gymrs
