// gymrs_advantages.h -- the rule of include/gymrs_amd.h, "advantages": the critic (the policy network with one output) and one
// step of the GAE(lambda) backward scan.  One text for the kernels (gymrs_advantages_impl.h) and for the host
// (gymrs_critic_value): every operation is a single IEEE f32 operation in the order written there, every multiply-add ONE fused
// multiply-add, every `?:` a select.  Nothing here may be contracted or reordered; the library is built with -ffp-contract=off and
// without fast-math.
#pragma once
#include "gymrs_math.h"

namespace gymrs {

// S: floats of one critic with D observation components and H hidden units
GYMRS_HD uint64_t critic_floats_of(uint32_t D, uint32_t H) { return H == 0 ? (uint64_t)D + 1 : (uint64_t)H * (D + 2) + 1; }

// v[k] = V(x[.][k]) for the VEC lanes of a caller.  w(k, i) = float i of lane k's critic: H == 0: W[D], b; H > 0: W1[H][D], b1[H],
// W2[H], b2 (the policy layout with one action).  The hidden layer is consumed unit by unit, UNITS units per trip of a loop that
// stays rolled, lanes innermost: one accumulator and one temporary per lane whatever H is (policy_logits, gymrs_policy.h).
template <int D, int VEC, int UNITS, class W>
GYMRS_HD void critic_values(const W& w, uint32_t H, const float (&x)[D][VEC], float (&v)[VEC])
{
    if (H == 0) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) v[k] = w(k, (uint32_t)D);
#pragma unroll
        for (int j = 0; j < D; ++j) {
#pragma unroll
            for (int k = 0; k < VEC; ++k) v[k] = fmaf_(w(k, (uint32_t)j), x[j][k], v[k]);
        }
    } else {
        const uint32_t o_b1 = H * D, o_w2 = o_b1 + H, o_b2 = o_w2 + H;
#pragma unroll
        for (int k = 0; k < VEC; ++k) v[k] = w(k, o_b2);
#pragma unroll UNITS
        for (uint32_t h = 0; h < H; ++h) {
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                float z = w(k, o_b1 + h);
#pragma unroll
                for (int j = 0; j < D; ++j) z = fmaf_(w(k, h * D + j), x[j][k], z);
                const float r = (z > 0.0f) ? z : 0.0f;
                v[k] = fmaf_(w(k, o_w2 + h), r, v[k]);
            }
        }
    }
}

// One step of the scan for one lane.  v_succ = V(x_next) as evaluated (it may be anything, NaN included, where done is set: it is
// not selected), v_cur = V(the observation the step started from), carry = A[k + 1] (not selected behind an end).
GYMRS_HD void advantage_step(float gamma, float gl, float reward, bool done, bool ended, float v_succ, float v_cur, float carry, float& adv,
                             float& ret)
{
    const float v_next = done ? 0.0f : v_succ;
    const float delta = fmaf_(gamma, v_next, reward) - v_cur;
    const float c = ended ? 0.0f : carry;
    adv = fmaf_(gl, c, delta);
    ret = adv + v_cur;
}

} // namespace gymrs
