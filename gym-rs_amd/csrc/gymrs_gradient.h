// gymrs_gradient.h -- the rule of include/gymrs_amd.h, "gradients": the score-function gradient of a small policy (and the value
// gradient of a critic) over the lane-steps of a transitions record, as exact fixed-point integers.  One text for the kernels
// (gymrs_gradient_impl.h) and for the host (gymrs_gradient_lane): every operation is a single IEEE f32 operation in the order
// written there, every multiply-add ONE fused multiply-add, every `?:` a select.  Nothing here may be contracted or reordered; the
// library is built with -ffp-contract=off and without fast-math.
//
// Everything is written for the VEC lanes of a caller, lanes innermost (the host has VEC = 1); w(k, i) = float i of lane k's
// network: H == 0: W[A][D], b[A]; H > 0: W1[H][D], b1[H], W2[A][H], b2[A] -- the policy layout; the critic is A = 1.  The gradient
// table of one set has the same layout.  The accumulators of a hidden layer do not fit in registers, so its units are taken
// kGradientChunk at a time: a chunk owns the sums of dW1, db1 and dW2 of its units (db2 belongs to chunk 0), and every sum is the
// same sequence of operations whichever chunk size is chosen.
//
// "clipped surrogate" (gymrs_ppo_gradient, gymrs_ppo_lane) is the policy head with its coefficient computed here: ppo_coefficient,
// gradient_ppo_head.
#pragma once
#include "gymrs_sample.h"

namespace gymrs {

constexpr int kGradientChunk = 4; // hidden units per pass over the record; need not divide H

// The logits of "closed-loop rollouts" (the arithmetic of policy_logits, gymrs_policy.h).  UNITS = units per trip of the rolled loop.
template <int D, int A, int VEC, int UNITS, class W>
GYMRS_HD void gradient_logits(const W& w, uint32_t H, const float (&x)[D][VEC], float (&y)[A][VEC])
{
    if (H == 0) {
#pragma unroll
        for (int a = 0; a < A; ++a) {
#pragma unroll
            for (int k = 0; k < VEC; ++k) y[a][k] = w(k, (uint32_t)(A * D + a));
#pragma unroll
            for (int j = 0; j < D; ++j) {
#pragma unroll
                for (int k = 0; k < VEC; ++k) y[a][k] = fmaf_(w(k, (uint32_t)(a * D + j)), x[j][k], y[a][k]);
            }
        }
    } else {
        const uint32_t o_b1 = H * D, o_w2 = o_b1 + H, o_b2 = o_w2 + A * H;
#pragma unroll
        for (int a = 0; a < A; ++a) {
#pragma unroll
            for (int k = 0; k < VEC; ++k) y[a][k] = w(k, o_b2 + a);
        }
#pragma unroll UNITS
        for (uint32_t h = 0; h < H; ++h) {
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                float z = w(k, o_b1 + h);
#pragma unroll
                for (int j = 0; j < D; ++j) z = fmaf_(w(k, h * D + j), x[j][k], z);
                const float r = (z > 0.0f) ? z : 0.0f;
#pragma unroll
                for (int a = 0; a < A; ++a) y[a][k] = fmaf_(w(k, o_w2 + a * H + h), r, y[a][k]);
            }
        }
    }
}

// The policy head: g[b] = (c * beta) * ((b == a ? 1 : 0) - p[b]) under the sampling rule at `scale`; on = the action is one of
// the A (a lane-step with on == false leaves every accumulator as it is); pa = p[a], +0.0f where a >= A.
template <int A, int VEC>
GYMRS_HD void gradient_policy_head(const float (&y)[A][VEC], const uint8_t (&act)[VEC], const float (&c)[VEC], float scale, float (&g)[A][VEC],
                                   bool (&on)[VEC], float (&pa)[VEC])
{
    const float beta = scale * 0x1.62e430p-1f;
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
        float yl[A], wt[A];
#pragma unroll
        for (int b = 0; b < A; ++b) yl[b] = y[b][k];
        const uint32_t greedy = sample_greedy(yl, A);
        sample_weights(yl, A, greedy, scale, wt);
        const float total = sample_total(wt, A);
        const float cb = c[k] * beta;
        pa[k] = 0.0f;
#pragma unroll
        for (int b = 0; b < A; ++b) {
            const float p = sample_prob(wt, total, greedy, (uint32_t)b);
            const bool hit = act[k] == (uint8_t)b;
            g[b][k] = cb * ((hit ? 1.0f : 0.0f) - p);
            pa[k] = hit ? p : pa[k];
        }
        on[k] = act[k] < (uint8_t)A;
    }
}

// The coefficient of "clipped surrogate": one divide, the compares (false on NaN), a select, one multiply.  cut = the lane-step is
// outside the clip range on the side its advantage pushes to: it adds nothing.
GYMRS_HD float ppo_coefficient(float adv, float po, float pa, float clip_low, float clip_high, bool& cut)
{
    const float ratio = pa / po;
    cut = (adv > 0.0f && ratio > clip_high) || (adv < 0.0f && ratio < clip_low);
    return cut ? 0.0f : adv * ratio;
}

// The policy head of "clipped surrogate": gradient_policy_head with c = ppo_coefficient(adv, po, pa), which needs pa before g.
// cut[k] is set for a lane-step with `on` only: one that is not `on` is not counted.
template <int A, int VEC>
GYMRS_HD void gradient_ppo_head(const float (&y)[A][VEC], const uint8_t (&act)[VEC], const float (&adv)[VEC], const float (&po)[VEC], float scale,
                                float clip_low, float clip_high, float (&g)[A][VEC], bool (&on)[VEC], float (&pa)[VEC], bool (&cut)[VEC])
{
    const float beta = scale * 0x1.62e430p-1f;
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
        float yl[A], wt[A], p[A];
#pragma unroll
        for (int b = 0; b < A; ++b) yl[b] = y[b][k];
        const uint32_t greedy = sample_greedy(yl, A);
        sample_weights(yl, A, greedy, scale, wt);
        const float total = sample_total(wt, A);
        pa[k] = 0.0f;
#pragma unroll
        for (int b = 0; b < A; ++b) {
            p[b] = sample_prob(wt, total, greedy, (uint32_t)b);
            pa[k] = (act[k] == (uint8_t)b) ? p[b] : pa[k];
        }
        on[k] = act[k] < (uint8_t)A;
        bool out;
        const float c = ppo_coefficient(adv[k], po[k], pa[k], clip_low, clip_high, out);
        const float cb = c * beta;
#pragma unroll
        for (int b = 0; b < A; ++b) g[b][k] = cb * ((act[k] == (uint8_t)b ? 1.0f : 0.0f) - p[b]);
        cut[k] = on[k] && out;
    }
}

// The per-lane f32 sums.  Every index is a compile-time constant after unrolling: they live in registers.
template <int D, int A, int VEC>
struct GradientAffine {
    float dW[A][D][VEC], db[A][VEC];
};
template <int D, int A, int VEC>
struct GradientChunk {
    float dW1[kGradientChunk][D][VEC], db1[kGradientChunk][VEC], dW2[A][kGradientChunk][VEC];
};

// MASK: the `on` select is compiled in (the policy head); the critic head has no action to be out of range.
template <int D, int A, int VEC, bool MASK>
GYMRS_HD void gradient_affine_step(const float (&x)[D][VEC], const float (&g)[A][VEC], const bool (&on)[VEC], GradientAffine<D, A, VEC>& acc)
{
#pragma unroll
    for (int b = 0; b < A; ++b) {
#pragma unroll
        for (int j = 0; j < D; ++j) {
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                const float t = fmaf_(g[b][k], x[j][k], acc.dW[b][j][k]);
                acc.dW[b][j][k] = (!MASK || on[k]) ? t : acc.dW[b][j][k];
            }
        }
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            const float t = acc.db[b][k] + g[b][k];
            acc.db[b][k] = (!MASK || on[k]) ? t : acc.db[b][k];
        }
    }
}

// db2 of a hidden network (once per lane-step: it does not depend on the unit)
template <int A, int VEC, bool MASK>
GYMRS_HD void gradient_bias_step(const float (&g)[A][VEC], const bool (&on)[VEC], float (&db2)[A][VEC])
{
#pragma unroll
    for (int b = 0; b < A; ++b) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            const float t = db2[b][k] + g[b][k];
            db2[b][k] = (!MASK || on[k]) ? t : db2[b][k];
        }
    }
}

// The units h0 .. h0 + kGradientChunk - 1 that exist (h < H) of one lane-step.
template <int D, int A, int VEC, bool MASK, class W>
GYMRS_HD void gradient_chunk_step(const W& w, uint32_t H, uint32_t h0, const float (&x)[D][VEC], const float (&g)[A][VEC], const bool (&on)[VEC],
                                  GradientChunk<D, A, VEC>& acc)
{
    const uint32_t o_b1 = H * D, o_w2 = o_b1 + H;
#pragma unroll
    for (int u = 0; u < kGradientChunk; ++u) {
        const uint32_t h = h0 + u;
        if (h < H) {
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                const bool keep = MASK && !on[k];
                float z = w(k, o_b1 + h);
#pragma unroll
                for (int j = 0; j < D; ++j) z = fmaf_(w(k, h * D + j), x[j][k], z);
                const float r = (z > 0.0f) ? z : 0.0f;
#pragma unroll
                for (int b = 0; b < A; ++b) {
                    const float t = fmaf_(g[b][k], r, acc.dW2[b][u][k]);
                    acc.dW2[b][u][k] = keep ? acc.dW2[b][u][k] : t;
                }
                float e = g[0][k] * w(k, o_w2 + h);
#pragma unroll
                for (int b = 1; b < A; ++b) e = fmaf_(g[b][k], w(k, o_w2 + b * H + h), e);
                const float dz = (z > 0.0f) ? e : 0.0f;
                const float t1 = acc.db1[u][k] + dz;
                acc.db1[u][k] = keep ? acc.db1[u][k] : t1;
#pragma unroll
                for (int j = 0; j < D; ++j) {
                    const float t = fmaf_(dz, x[j][k], acc.dW1[u][j][k]);
                    acc.dW1[u][j][k] = keep ? acc.dW1[u][j][k] : t;
                }
            }
        }
    }
}

// Where every sum goes: fn(s, L) with s = the parameter's index in the network's layout and L its VEC per-lane sums.
template <int D, int A, int VEC, class Fn>
GYMRS_HD void gradient_affine_each(const GradientAffine<D, A, VEC>& acc, Fn&& fn)
{
#pragma unroll
    for (int b = 0; b < A; ++b) {
#pragma unroll
        for (int j = 0; j < D; ++j) fn((uint32_t)(b * D + j), acc.dW[b][j]);
    }
#pragma unroll
    for (int b = 0; b < A; ++b) fn((uint32_t)(A * D + b), acc.db[b]);
}
template <int D, int A, int VEC, class Fn>
GYMRS_HD void gradient_chunk_each(uint32_t H, uint32_t h0, const GradientChunk<D, A, VEC>& acc, Fn&& fn)
{
    const uint32_t o_b1 = H * D, o_w2 = o_b1 + H;
#pragma unroll
    for (int u = 0; u < kGradientChunk; ++u) {
        const uint32_t h = h0 + u;
        if (h < H) {
#pragma unroll
            for (int j = 0; j < D; ++j) fn(h * D + j, acc.dW1[u][j]);
            fn(o_b1 + h, acc.db1[u]);
#pragma unroll
            for (int b = 0; b < A; ++b) fn(o_w2 + b * H + h, acc.dW2[b][u]);
        }
    }
}
template <int D, int A, int VEC, class Fn>
GYMRS_HD void gradient_bias_each(uint32_t H, const float (&db2)[A][VEC], Fn&& fn)
{
    const uint32_t o_b2 = H * D + H + A * H;
#pragma unroll
    for (int b = 0; b < A; ++b) fn(o_b2 + b, db2[b]);
}

// The fixed point of one (lane, parameter) sum: q = rint(L * 2^24), exact in f64, for a finite |L| < 2^30; else the pair is
// excluded (false) and q = 0.
GYMRS_HD bool gradient_fixed(float L, long long& q)
{
    const bool ok = fabsf_(L) < 0x1p30f; // false for NaN and the infinities
    const double v = ok ? (double)L * 16777216.0 : 0.0;
    q = (long long)__builtin_rint(v);
    return ok;
}

} // namespace gymrs
