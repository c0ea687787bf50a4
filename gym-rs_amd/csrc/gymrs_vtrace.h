// gymrs_vtrace.h -- the rule of include/gymrs_amd.h, "V-trace": the current policy's probability of the recorded action, the three
// clipped importance ratios and one step of the backward scan.  One text for the kernel (gymrs_vtrace_impl.h) and for the host
// (gymrs_vtrace_lane): every operation is a single IEEE f32 operation in the order written there, every multiply-add ONE fused
// multiply-add, every `?:` a select.  Nothing here may be contracted or reordered; the library is built with -ffp-contract=off and
// without fast-math.  The logits are gradient_logits' (gymrs_gradient.h), the critic is critic_values (gymrs_advantages.h).
#pragma once
#include "gymrs_advantages.h"
#include "gymrs_sample.h"

namespace gymrs {

// pa = p[act] of the sampling rule under `scale` (the bits gymrs_policy_gradient writes to prob); +0.0f where act >= A.
template <int A>
GYMRS_HD float vtrace_prob(const float (&y)[A], uint8_t act, float scale)
{
    float wt[A];
    const uint32_t greedy = sample_greedy(y, A);
    sample_weights(y, A, greedy, scale, wt);
    const float total = sample_total(wt, A);
    float pa = 0.0f;
#pragma unroll
    for (int b = 0; b < A; ++b) {
        const float p = sample_prob(wt, total, greedy, (uint32_t)b);
        pa = (act == (uint8_t)b) ? p : pa;
    }
    return pa;
}

// What the scan needs of one lane-step's importance ratio.  A NaN ratio passes every compare: it is not clipped.
struct VtraceWeights {
    float rho, gc, rho_pg; // the clipped TD weight, gamma * lambda * the clipped trace weight, the clipped policy-gradient weight
    bool over_rho, over_c; // valid && ratio > rho_bar, valid && ratio > c_bar (the counters)
};
GYMRS_HD VtraceWeights vtrace_weights(float pa, float po, bool valid, float gamma, float lambda, float rho_bar, float c_bar, float pg_rho_bar)
{
    const float ratio = valid ? pa / po : 0.0f;
    VtraceWeights w;
    w.rho = (ratio > rho_bar) ? rho_bar : ratio;
    const float cc = lambda * ((ratio > c_bar) ? c_bar : ratio);
    w.rho_pg = (ratio > pg_rho_bar) ? pg_rho_bar : ratio;
    w.gc = gamma * cc;
    w.over_rho = valid && ratio > rho_bar;
    w.over_c = valid && ratio > c_bar;
    return w;
}

// One step of the scan for one lane.  v_succ = V(x_next) as evaluated (not selected where done is set), v_cur = V(x_cur), acc = acc[k + 1]
// on entry (not selected behind an end) and acc[k] on return.
GYMRS_HD void vtrace_step(float gamma, float reward, bool done, bool ended, float v_succ, float v_cur, float rho, float gc, float rho_pg, float& acc,
                          float& vs, float& pg)
{
    const float v_next = done ? 0.0f : v_succ;
    const float td = fmaf_(gamma, v_next, reward) - v_cur;
    const float carry = ended ? 0.0f : acc;
    acc = fmaf_(gc, carry, rho * td);
    vs = acc + v_cur;
    const float vs_next = carry + v_next;
    pg = rho_pg * (fmaf_(gamma, vs_next, reward) - v_cur);
}

} // namespace gymrs
