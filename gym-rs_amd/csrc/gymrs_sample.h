// gymrs_sample.h -- the softmax sampling rule of include/gymrs_amd.h, "sampling": weights, selection and probabilities from the
// logits of one lane.  One text for the kernels (SamplingActions, gymrs_policy.h) and for the host (gymrs_sample_draw): every
// operation is a single IEEE f32 operation in the order written there -- one subtract and one multiply for d, floor, one subtract,
// six fma, an exact ldexp, adds in index order, one divide.  Nothing here may be contracted or reordered; the library is built with
// -ffp-contract=off and without fast-math.  n is the number of actions (a constant after inlining in the kernels: the loops unroll).
#pragma once
#include "gymrs_philox.h"

namespace gymrs {

constexpr uint32_t kMaxSampleActions = 8; // gymrs_sample_draw takes 2 .. 8

// The first maximum; a NaN at a >= 1 never wins (the argmax of "closed-loop rollouts").
GYMRS_HD uint32_t sample_greedy(const float* y, uint32_t n)
{
    uint32_t best = 0;
    float yb = y[0];
    for (uint32_t a = 1; a < n; ++a) {
        if (y[a] > yb) {
            yb = y[a];
            best = a;
        }
    }
    return best;
}

// 2^f on [0, 1] by Horner with fma, c6 down to c0; c0 == 1 makes P(0) == 1 exactly.
GYMRS_HD float sample_exp2_poly(float f)
{
    float acc = 0x1.b4d1e4p-13f;
    acc = fmaf_(acc, f, 0x1.4ca4ccp-10f);
    acc = fmaf_(acc, f, 0x1.3c4a8ap-7f);
    acc = fmaf_(acc, f, 0x1.c69f6ap-5f);
    acc = fmaf_(acc, f, 0x1.ebfc40p-3f);
    acc = fmaf_(acc, f, 0x1.62e430p-1f);
    acc = fmaf_(acc, f, 1.0f);
    return acc;
}

// w = 2^d for d in [-126, 0]; NaN, -inf and the far tail weigh nothing.  floor(d) is in [-126, 0] and P in [1, 2], so the ldexp is
// exact and w is a normal number.
GYMRS_HD float sample_weight(float d)
{
    if (!(d >= -126.0f)) return 0.0f;
    const float fl = __builtin_floorf(d);
    return __builtin_ldexpf(sample_exp2_poly(d - fl), (int)fl);
}

GYMRS_HD void sample_weights(const float* y, uint32_t n, uint32_t greedy, float scale, float* w)
{
    const float m = y[greedy];
    for (uint32_t a = 0; a < n; ++a) w[a] = sample_weight((y[a] - m) * scale);
}

GYMRS_HD float sample_total(const float* w, uint32_t n)
{
    float total = w[0];
    for (uint32_t a = 1; a < n; ++a) total = total + w[a];
    return total;
}

// The first a with thr < w[0] + .. + w[a]; none (all weights 0, or thr rounded up to the total): greedy.
GYMRS_HD uint32_t sample_select(const float* w, uint32_t n, float total, uint32_t word, uint32_t greedy)
{
    const float thr = ((float)(word >> 8) * 0x1p-24f) * total;
    uint32_t action = greedy;
    bool found = false;
    float run = 0.0f;
    for (uint32_t a = 0; a < n; ++a) {
        run = a == 0 ? w[0] : run + w[a];
        if (!found && thr < run) {
            action = a;
            found = true;
        }
    }
    return action;
}

GYMRS_HD float sample_prob(const float* w, float total, uint32_t greedy, uint32_t a)
{
    if (!(total > 0.0f)) return a == greedy ? 1.0f : 0.0f;
    return w[a] / total;
}

// Everything for one lane: the action taken; prob (may be NULL) gets prob[0 .. n).
GYMRS_HD uint32_t sample_action(const float* y, uint32_t n, float scale, uint32_t word, float* prob)
{
    float w[kMaxSampleActions];
    const uint32_t greedy = sample_greedy(y, n);
    sample_weights(y, n, greedy, scale, w);
    const float total = sample_total(w, n);
    if (prob)
        for (uint32_t a = 0; a < n; ++a) prob[a] = sample_prob(w, total, greedy, a);
    return sample_select(w, n, total, word, greedy);
}

} // namespace gymrs
