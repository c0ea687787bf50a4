// gymrs_es.h -- the rule of include/gymrs_amd.h, "Evolution strategies": the noise of one (generation, pair, parameter), the two
// members of a pair, the utility of one policy and one term of the gradient.  One text for the kernels (gymrs_es_impl.h) and for the
// host (gymrs_es_noise, gymrs_es_utilities): every operation is a single IEEE operation in the order written there, fmaf rounds once,
// f64 divide and square root are the correctly rounded ones.  Nothing here may be contracted or reordered.  The update itself is the
// optimizer's (gymrs_optimizer.h) and the fixed point is the gradients' (gradient_fixed): neither is restated.
//
// What is NOT here is the order of the sums over policies (the two-level butterfly): the kernel spreads a chunk over a block, the host
// walks it; both follow the header.
#pragma once
#include "gymrs_gradient.h"
#include "gymrs_philox.h"

namespace gymrs {

// 1 / sqrt(8 * (65536^2 - 1) / 12) = 1 / sqrt(2863311530), to the nearest f32: 1.8688124328036793e-05
constexpr float kEsNoiseScale = 0x1.3988e2p-16f;
constexpr uint64_t kEsGenerationMask = (1ull << 39) - 1; // the generation bits that enter the key

// the tick word of the key: generation (39 bits) above the parameter (9 bits)
GYMRS_HD uint64_t es_tick(uint64_t gen, uint32_t s) { return ((gen & kEsGenerationMask) << 9) | (uint64_t)s; }

// the sum of the eight 16-bit halves of a block, centred: exact, symmetric, in [-262140, 262140]
GYMRS_HD int32_t es_halves(const u32x4& b)
{
    uint32_t h = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int i = 0; i < 4; ++i) h += (b.v[i] & 0xffffu) + (b.v[i] >> 16);
    return (int32_t)h - 262140;
}

GYMRS_HD float es_noise(uint64_t seed, uint64_t gen, uint64_t pair, uint32_t s)
{
    return (float)es_halves(draw4(seed, pair, es_tick(gen, s), kStreamEs)) * kEsNoiseScale;
}

// the two members of pair j at parameter s
GYMRS_HD void es_members(float sigma, float eps, float theta, float& plus, float& minus)
{
    plus = fmaf_(sigma, eps, theta);
    minus = fmaf_(-sigma, eps, theta);
}

// F[p] of a valid policy (episodes > 0)
GYMRS_HD double es_fitness(long long return_sum, unsigned long long episodes) { return (double)return_sum / (double)episodes; }

GYMRS_HD double es_sd(double sum2, double n_valid) { return __builtin_sqrt(sum2 / n_valid); }

GYMRS_HD float es_utility(bool valid, double F, double mean, double sd) { return (valid && sd > 0.0) ? (float)((F - mean) / sd) : 0.0f; }

// the centred-rank utility (gymrs_es_ranks): c = rank2 - (n - 1) of a policy among the n valid ones, exact; one f64 division, one cast
GYMRS_HD float es_rank_utility(bool valid, uint32_t n, long long c) { return (valid && n > 1u) ? (float)((double)c / (double)(2ull * (n - 1u))) : 0.0f; }

// one term of G[s]: false = the term is excluded (q = 0)
GYMRS_HD bool es_term(float d, float eps, long long& q) { return gradient_fixed(d * eps, q); }

} // namespace gymrs
