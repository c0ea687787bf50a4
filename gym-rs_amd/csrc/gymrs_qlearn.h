// gymrs_qlearn.h -- the rule of include/gymrs_amd.h, "Q-learning": the TD error of a lane-step under an online and a target set, its
// Huber clamp and the one-hot output gradient of the selected logit.  One text for the kernels (gymrs_qlearn_impl.h) and for the host
// (gymrs_q_lane): every operation is a single IEEE f32 operation in the order written there, every multiply-add ONE fused
// multiply-add, every `?:` a select.  Nothing here may be contracted or reordered; the library is built with -ffp-contract=off and
// without fast-math.  The logits are gradient_logits' (the arithmetic of "closed-loop rollouts"), the backward pass, the
// accumulators and the fixed point are gymrs_gradient.h's, unchanged.
//
// Everything is written for the VEC lanes of a caller, lanes innermost (the host has VEC = 1).
#pragma once
#include "gymrs_gradient.h"

namespace gymrs {

// The TD error of one lane-step.  y = the online logits of x, yt = the target logits of the successor x', ysel = the logits that
// choose the bootstrap action (yt; with GYMRS_Q_DOUBLE the online logits of x').  on = the action is one of the A; delta = +0.0f
// where it is not.  A done step bootstraps from +0.0f whatever v is (a select: a NaN v reaches nothing).
template <int A, int VEC>
GYMRS_HD void q_td_step(const float (&y)[A][VEC], const float (&yt)[A][VEC], const float (&ysel)[A][VEC], const uint8_t (&act)[VEC],
                        const float (&rew)[VEC], const bool (&dn)[VEC], float gamma, float (&delta)[VEC], bool (&on)[VEC])
{
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
        // the first maximum; a NaN never wins
        float best = ysel[0][k], v = yt[0][k];
#pragma unroll
        for (int b = 1; b < A; ++b) {
            const bool up = ysel[b][k] > best;
            best = up ? ysel[b][k] : best;
            v = up ? yt[b][k] : v;
        }
        const float boot = dn[k] ? 0.0f : v;
        const float target = fmaf_(gamma, boot, rew[k]);
        float qa = y[0][k];
#pragma unroll
        for (int b = 1; b < A; ++b) qa = (act[k] == (uint8_t)b) ? y[b][k] : qa;
        on[k] = act[k] < (uint8_t)A;
        delta[k] = on[k] ? qa - target : 0.0f;
    }
}

// |delta| > kappa, as two compares (false on NaN): what counts[set][1] counts
GYMRS_HD bool q_clamped(float delta, float kappa) { return delta > kappa || delta < -kappa; }

// The output gradient of sum huber_kappa(delta): d on the selected logit, +0.0f on the others.  A NaN delta passes through.
template <int A, int VEC>
GYMRS_HD void q_head(const float (&delta)[VEC], const uint8_t (&act)[VEC], float kappa, float (&g)[A][VEC], bool (&on)[VEC])
{
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
        const float d = delta[k] > kappa ? kappa : (delta[k] < -kappa ? -kappa : delta[k]);
#pragma unroll
        for (int b = 0; b < A; ++b) g[b][k] = (act[k] == (uint8_t)b) ? d : 0.0f;
        on[k] = act[k] < (uint8_t)A;
    }
}

} // namespace gymrs
