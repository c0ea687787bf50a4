// gymrs_replay.h -- the rules of include/gymrs_amd.h, "Replay": the integer priority of a TD error and the stratified proportional
// draw.  One text for the kernels (gymrs_replay_impl.h) and for the host (gymrs_replay_priority, gymrs_replay_draw).  The priority
// rule is f32, every operation a single IEEE operation in the order written here, built from the two bit-defined functions the
// project already has (entropy_log2, sample_weight); nothing may be contracted or reordered.  The draw is integers alone: a sample
// is a pure function of (priorities, seed, draw counter) and depends neither on scheduling nor on how the store is tiled.
#pragma once
#include "gymrs_entropy.h"

namespace gymrs {

constexpr uint32_t kStreamReplay = 5;              // the Philox stream of the draws (gymrs_philox.h)
constexpr uint32_t kReplayMaxPriority = 1u << 24;  // a priority is in 0 .. 2^24; 0 is never drawn
constexpr uint32_t kReplayNone = 0xffffffffu;      // idx of a draw from a store without mass
constexpr uint64_t kReplayMaxCapacity = 1ull << 26, kReplayMaxSamples = 1ull << 24;

// 2^-126 <= eps <= cap < inf and 0 <= alpha <= 1 (false for a NaN anywhere)
GYMRS_HD bool replay_rule_ok(float alpha, float eps, float cap)
{
    return eps >= 0x1p-126f && eps <= cap && cap <= 0x1.fffffep+127f && alpha >= 0.0f && alpha <= 1.0f;
}

// p = round(2^24 * (min(|td| + eps, cap) / cap)^alpha), at least 1.  NaN and +inf land on cap: an unknown error has the highest priority.
GYMRS_HD uint32_t replay_priority(float td, float alpha, float eps, float cap)
{
    float v = fabsf_(td) + eps;
    v = !(v <= cap) ? cap : v;
    float d = alpha * (entropy_log2(v) - entropy_log2(cap));
    d = d > 0.0f ? 0.0f : d;
    const float w = sample_weight(d);
    const uint32_t p = (uint32_t)__builtin_rintf(w * 16777216.0f);
    return p < 1u ? 1u : p;
}

// floor(r * w / 2^32) as the high half of (r << 32) * w: no division
GYMRS_HD uint64_t replay_scale(uint32_t r, uint64_t w)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi((uint64_t)r << 32, w);
#else
    return (uint64_t)(((unsigned __int128)((uint64_t)r << 32) * w) >> 64);
#endif
}

// The B strata of a total mass T > 0: stratum j is [lo(j), lo(j) + width(j)), the first T % B of them one wider.
struct ReplayStrata {
    uint64_t T, q, rem;
    uint32_t B;
};
GYMRS_HD ReplayStrata replay_strata(uint64_t T, uint32_t B) { return ReplayStrata{T, T / B, T % B, B}; }
GYMRS_HD uint64_t replay_lo(const ReplayStrata& s, uint32_t j) { return (uint64_t)j * s.q + ((uint64_t)j < s.rem ? (uint64_t)j : s.rem); }
GYMRS_HD uint64_t replay_width(const ReplayStrata& s, uint32_t j) { return s.q + ((uint64_t)j < s.rem ? 1u : 0u); }

// The four words of samples 4g .. 4g + 3: sample j uses word j & 3 of block j >> 2 (only the low 48 bits of `draw` reach the counter).
GYMRS_HD u32x4 replay_block(uint64_t seed, uint64_t draw, uint32_t g) { return draw4(seed, (uint64_t)g, draw, kStreamReplay); }

// u_j: the point of sample j in [0, T) from its word r.  An empty stratum (T < B, j >= T) lands on T - 1.
GYMRS_HD uint64_t replay_point(const ReplayStrata& s, uint32_t r, uint32_t j)
{
    const uint64_t u = replay_lo(s, j) + replay_scale(r, replay_width(s, j));
    return u < s.T - 1u ? u : s.T - 1u;
}

// The stratum that holds x < T (lo(j) <= x < lo(j) + width(j)): the closed form, two 64-bit divisions at the most.
GYMRS_HD uint32_t replay_stratum_of(const ReplayStrata& s, uint64_t x)
{
    const uint64_t wide = s.rem * (s.q + 1u); // where the strata of width q begin (q == 0: wide == T, and x is below it)
    return (uint32_t)(x < wide ? x / (s.q + 1u) : s.rem + (x - wide) / s.q);
}

// The draw over host memory: the points ascend with j, so one walk of the prefix sum serves them all.
inline void replay_draw_host(const uint32_t* priority, uint64_t count, uint32_t B, uint64_t seed, uint64_t draw, uint32_t* idx, uint64_t* total)
{
    uint64_t T = 0;
    for (uint64_t e = 0; e < count; ++e) T += priority[e];
    if (total) *total = T;
    if (T == 0) {
        for (uint32_t j = 0; j < B; ++j) idx[j] = kReplayNone;
        return;
    }
    const ReplayStrata s = replay_strata(T, B);
    uint64_t e = 0, P = priority[0]; // P = the inclusive prefix sum at e
    u32x4 words{};
    for (uint32_t j = 0; j < B; ++j) {
        if ((j & 3u) == 0u) words = replay_block(seed, draw, j >> 2);
        const uint64_t u = replay_point(s, words.v[j & 3u], j);
        while (!(P > u)) P += priority[++e]; // (u < T = P[count - 1]: e stays below count)
        idx[j] = (uint32_t)e;
    }
}

} // namespace gymrs
