// gymrs_entropy.h -- the rule of include/gymrs_amd.h, "Entropy": the entropy of the sampling rule's distribution, its gradient with
// respect to the logits, and the k3 estimate of the KL divergence from a recorded policy, over the lane-steps of a transitions
// record.  One text for the kernels (gymrs_entropy_impl.h) and for the host (gymrs_entropy_lane, gymrs_entropy_log2): every operation
// is a single IEEE f32 operation in the order written there, every multiply-add ONE fused multiply-add, every `?:` a select.  Nothing
// here may be contracted or reordered; the library is built with -ffp-contract=off and without fast-math.
//
// The sampling rule works in base 2: w[b] = 2^d[b], so log2 p[b] = d[b] - log2(total) with total in [1, A].  entropy_log2 is the one
// logarithm the library has.  Its maximum absolute error against f64 log2 over all 2^23 f32 values of [1, 2), evaluated with true
// fmaf, is 1.41e-7 (measured: 1.4052e-7, below 1.41e-7; tests/test_entropy_host.py repeats the measurement).  A degree-8 Q leaves
// 7e-9 of that to the polynomial; the rest is the rounding of the Horner steps and of the result (half an ulp of [0.5, 1) is 3e-8):
// degrees 9 to 11 measure 1.65e-7 to 1.77e-7, no better.
//
// Everything is written for the VEC lanes of a caller, lanes innermost (the host has VEC = 1), as in gymrs_gradient.h, whose
// accumulators, backward pass and fixed point take this head's g.
#pragma once
#include "gymrs_gradient.h"

namespace gymrs {

constexpr float kLn2 = 0x1.62e430p-1f; // the constant of beta (gymrs_gradient.h)

// log2(v) for a finite v >= 2^-126: the exponent, and t * Q(t) for the mantissa m = 1 + t in [1, 2).  entropy_log2(1) == +0; near 1
// the result keeps its relative accuracy (r = t * Q(t) is a product, e == 0 adds nothing).  Any other v gives some float and no trap:
// the callers select it away.
GYMRS_HD float entropy_log2(float v)
{
    const uint32_t u = f2u(v);
    const int e = (int)((u >> 23) & 0xffu) - 127;
    const float t = u2f((u & 0x007fffffu) | 0x3f800000u) - 1.0f; // exact
    float q = 0x1.739d30p-8f;
    q = fmaf_(q, t, -0x1.19ef3ap-5f);
    q = fmaf_(q, t, 0x1.925438p-4f);
    q = fmaf_(q, t, -0x1.76f800p-3f);
    q = fmaf_(q, t, 0x1.1255d2p-2f);
    q = fmaf_(q, t, -0x1.6c7e8ep-2f);
    q = fmaf_(q, t, 0x1.ebcb78p-2f);
    q = fmaf_(q, t, -0x1.714ef8p-1f);
    q = fmaf_(q, t, 0x1.715466p+0f);
    return (float)e + t * q;
}

// The entropy head of one lane-step: g[b] = d (coef * Hn) / d y[b], on = total > 0 (a lane-step with on == false leaves every
// accumulator as it is and is not counted), hn = the entropy in nats, pr[b] = p[b] of the sampling rule.
template <int A, int VEC>
GYMRS_HD void entropy_head(const float (&y)[A][VEC], float scale, float coef, float (&g)[A][VEC], bool (&on)[VEC], float (&hn)[VEC], float (&pr)[A][VEC])
{
    const float beta = scale * kLn2;
    const float ck = (coef * beta) * kLn2;
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
        float yl[A], wt[A], l[A];
#pragma unroll
        for (int b = 0; b < A; ++b) yl[b] = y[b][k];
        const uint32_t greedy = sample_greedy(yl, A);
        sample_weights(yl, A, greedy, scale, wt);
        const float total = sample_total(wt, A);
        on[k] = total > 0.0f;
        const float lt = entropy_log2(total);
        float sum = 0.0f;
#pragma unroll
        for (int b = 0; b < A; ++b) {
            const float d = (yl[b] - yl[greedy]) * scale; // d[b] of the sampling rule, the same two operations
            l[b] = d - lt;
            pr[b][k] = sample_prob(wt, total, greedy, (uint32_t)b);
            const float t = wt[b] > 0.0f ? pr[b][k] * l[b] : 0.0f;
            sum = b == 0 ? t : sum + t;
        }
        const float h2 = -sum;
        hn[k] = h2 * kLn2;
#pragma unroll
        for (int b = 0; b < A; ++b) {
            const float u = wt[b] > 0.0f ? pr[b][k] * (l[b] + h2) : 0.0f;
            g[b][k] = -(ck * u);
        }
    }
}

// The k3 estimate of one lane-step from pa = p[a] and the recorded probability: ok = it is accumulated and counted.
GYMRS_HD float entropy_kl(float pa, float po, bool& ok)
{
    const float ratio = pa / po;
    ok = ratio >= 0x1p-126f && ratio <= 0x1.fffffep+127f; // false for NaN, +inf, zero, denormals and negatives
    return (ratio - 1.0f) - entropy_log2(ratio) * kLn2;
}

// p[a] by a select chain; +0.0f where a >= A
template <int A, int VEC>
GYMRS_HD float entropy_pick(const float (&pr)[A][VEC], int k, uint8_t act)
{
    float pa = 0.0f;
#pragma unroll
    for (int b = 0; b < A; ++b) pa = act == (uint8_t)b ? pr[b][k] : pa;
    return pa;
}

// The running sums of a lane: the entropy of its counted lane-steps, the KL estimates of its counted ones, and both counts.
template <int VEC>
struct EntropySums {
    float h[VEC], kl[VEC];
    uint32_t n_h[VEC], n_kl[VEC];
};

// KL: old_prob is there; act and po are read then only.
template <int A, int VEC, bool KL>
GYMRS_HD void entropy_sums_step(const bool (&on)[VEC], const float (&hn)[VEC], const float (&pr)[A][VEC], const uint8_t (&act)[VEC], const float (&po)[VEC],
                                EntropySums<VEC>& s)
{
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
        const float th = s.h[k] + hn[k];
        s.h[k] = on[k] ? th : s.h[k];
        s.n_h[k] += on[k] ? 1u : 0u;
        if constexpr (KL) {
            bool ok;
            const float kl = entropy_kl(entropy_pick<A, VEC>(pr, k, act[k]), po[k], ok);
            const bool take = on[k] && act[k] < (uint8_t)A && ok;
            const float tk = s.kl[k] + kl;
            s.kl[k] = take ? tk : s.kl[k];
            s.n_kl[k] += take ? 1u : 0u;
        }
    }
}

} // namespace gymrs
