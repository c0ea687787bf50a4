// gymrs_policy.h -- evaluation of a small policy (affine, or one hidden ReLU layer) on the observation tile of a work-item:
// shared by policy_actions_kernel, the closed-loop rollout kernels (rollout_policy_body, gymrs_rollout_impl.h) and the episodic
// evaluation kernel (gymrs_evaluate_impl.h).  gfx950 device code, and the host's choice of the env type of a policy launch.
//
// The arithmetic is fixed to the bit (include/gymrs_amd.h, "closed-loop rollouts"): every multiply-add is ONE fused
// v_fma_f32 in the order written there, the ReLU is a compare-select (NaN and -0 give +0), the action is the first maximum
// (a NaN never wins).  Nothing here may be contracted or reordered; the library is built with -ffp-contract=off.
//
// Where the weights come from is decided per wave, wave-uniformly (UNI):
//   * every lane of the wave uses the same policy: the weights are wave-uniform operands, fetched through the scalar path
//     (loads from the constant address space at a wave-uniform address) straight into SGPRs, a few rows of the hidden layer at
//     a time: up to 450 floats do not live in registers across a step.
//   * lanes of one wave use different policies (e.g. lanes_per_policy = 1): every lane gathers its own weights through the
//     vector memory path from the table, which a population of small policies keeps in the L2.
// Both give the same bits: the same operations on the same values.
// Three action sources for rollout_block use it: PolicyActions (the argmax), ExploringActions (epsilon-greedy) and SamplingActions
// (softmax sampling, gymrs_sample.h).
#pragma once
#include "gymrs_sample.h"
#include "gymrs_tile.h"

namespace gymrs {

// Which policy the VEC lanes of a work-item use: lane (g0 + k) of the batch uses policy ((g0 + k) / lanes_per_policy) %
// n_policies.  Two 64-bit divisions per work-item and launch, the other lanes follow by counting.  `uniform` (wave-uniform):
// the 64 * VEC lanes of this wavefront all use pol[0].  Must be called with every work-item of the wave active.
template <int VEC>
__device__ __forceinline__ void policy_select(const PolicyArgs& p, uint64_t g0, uint32_t (&pol)[VEC], bool& uniform)
{
    const uint64_t q0 = g0 / p.lanes_per_policy;
    uint64_t r = g0 - q0 * p.lanes_per_policy;
    uint32_t m = (uint32_t)(q0 % p.n_policies);
    // the wave's first lane is lane 0 of its first work-item: how many lanes its block of lanes_per_policy still has
    const uint32_t r_lo = __builtin_amdgcn_readfirstlane((uint32_t)r), r_hi = __builtin_amdgcn_readfirstlane((uint32_t)(r >> 32));
    const uint64_t r_first = ((uint64_t)r_hi << 32) | r_lo;
    uniform = p.n_policies == 1 || p.lanes_per_policy - r_first >= (uint64_t)(64 * VEC);
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
        pol[k] = m;
        if (++r == p.lanes_per_policy) {
            r = 0;
            if (++m == p.n_policies) m = 0;
        }
    }
}

// The weights as a work-item reads them.  UNI: one wave-uniform base in the constant address space (scalar loads);
// else one policy index per lane (vector loads from the table).
template <int VEC, bool UNI>
struct PolicyWeights;
template <int VEC>
struct PolicyWeights<VEC, true> {
    typedef const __attribute__((address_space(4))) float* Ptr;
    Ptr w;
    __device__ __forceinline__ PolicyWeights(const PolicyArgs& p, const uint32_t (&pol)[VEC])
    {
        const uint64_t addr = reinterpret_cast<uint64_t>(p.weights) + (uint64_t)__builtin_amdgcn_readfirstlane(pol[0]) * p.stride * sizeof(float);
        w = reinterpret_cast<Ptr>(addr);
    }
    __device__ __forceinline__ float operator()(int, uint32_t i) const { return w[i]; }
};
template <int VEC>
struct PolicyWeights<VEC, false> {
    const float* __restrict__ base;
    uint32_t stride;
    uint32_t pol[VEC];
    __device__ __forceinline__ PolicyWeights(const PolicyArgs& p, const uint32_t (&pol_)[VEC]) : base(p.weights), stride(p.stride)
    {
#pragma unroll
        for (int k = 0; k < VEC; ++k) pol[k] = pol_[k];
    }
    __device__ __forceinline__ float operator()(int k, uint32_t i) const { return base[(uint64_t)pol[k] * stride + i]; }
};

// The logits y[a][k] of the VEC lanes of a work-item from their observations x[j].v[k] (D rows in gymrs_obs_ptrs order).  The
// hidden layer is consumed unit by unit: A accumulators and one temporary per lane, whatever H is; its loop stays rolled (four
// units per trip), so H = 64 costs no more code than H = 4.
// policy_eval below keeps its own copy of this arithmetic: routed through policy_logits, 240 of the 480 existing closed-loop and
// evaluation kernels came out with different machine code (profiles/policy_sample.md), and those kernels keep their code.
template <class Env, int VEC, bool UNI>
__device__ __forceinline__ void policy_logits(const PolicyWeights<VEC, UNI>& W, uint32_t H, const Vec<float, VEC> (&x)[Env::kState],
                                              float (&y)[Env::kActions][VEC])
{
    constexpr int D = Env::kState, A = (int)Env::kActions;
    static_assert(A >= 2 && sizeof(typename Env::Action) == 1, "policies are for the Discrete envs");
    if (H == 0) { // affine: W[A][D], b[A]
#pragma unroll
        for (int a = 0; a < A; ++a) {
#pragma unroll
            for (int k = 0; k < VEC; ++k) y[a][k] = W(k, A * D + a);
#pragma unroll
            for (int j = 0; j < D; ++j) {
#pragma unroll
                for (int k = 0; k < VEC; ++k) y[a][k] = __builtin_fmaf(W(k, a * D + j), x[j].v[k], y[a][k]);
            }
        }
    } else { // W1[H][D], b1[H], W2[A][H], b2[A]
        const uint32_t o_b1 = H * D, o_w2 = o_b1 + H, o_b2 = o_w2 + A * H;
#pragma unroll
        for (int a = 0; a < A; ++a) {
#pragma unroll
            for (int k = 0; k < VEC; ++k) y[a][k] = W(k, o_b2 + a);
        }
        constexpr int kUnits = UNI ? 4 : 1; // gathered: one unit's 1 + D + A vector loads per lane in flight, not four units' weights
#pragma unroll kUnits
        for (uint32_t h = 0; h < H; ++h) {
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                float z = W(k, o_b1 + h);
#pragma unroll
                for (int j = 0; j < D; ++j) z = __builtin_fmaf(W(k, h * D + j), x[j].v[k], z);
                const float r = (z > 0.0f) ? z : 0.0f;
#pragma unroll
                for (int a = 0; a < A; ++a) y[a][k] = __builtin_fmaf(W(k, o_w2 + a * H + h), r, y[a][k]);
            }
        }
    }
}

// The actions of the VEC lanes of a work-item from their observations x[j].v[k] (D rows in gymrs_obs_ptrs order).  The hidden
// layer is consumed unit by unit: A accumulators and one temporary per lane, whatever H is; its loop stays rolled (four
// units per trip), so H = 64 costs no more code than H = 4.
template <class Env, int VEC, bool UNI>
__device__ __forceinline__ void policy_eval(const PolicyWeights<VEC, UNI>& W, uint32_t H, const Vec<float, VEC> (&x)[Env::kState],
                                            Vec<uint8_t, VEC>& act)
{
    constexpr int D = Env::kState, A = (int)Env::kActions;
    static_assert(A >= 2 && sizeof(typename Env::Action) == 1, "policies are for the Discrete envs");
    float y[A][VEC];
    if (H == 0) { // affine: W[A][D], b[A]
#pragma unroll
        for (int a = 0; a < A; ++a) {
#pragma unroll
            for (int k = 0; k < VEC; ++k) y[a][k] = W(k, A * D + a);
#pragma unroll
            for (int j = 0; j < D; ++j) {
#pragma unroll
                for (int k = 0; k < VEC; ++k) y[a][k] = __builtin_fmaf(W(k, a * D + j), x[j].v[k], y[a][k]);
            }
        }
    } else { // W1[H][D], b1[H], W2[A][H], b2[A]
        const uint32_t o_b1 = H * D, o_w2 = o_b1 + H, o_b2 = o_w2 + A * H;
#pragma unroll
        for (int a = 0; a < A; ++a) {
#pragma unroll
            for (int k = 0; k < VEC; ++k) y[a][k] = W(k, o_b2 + a);
        }
        constexpr int kUnits = UNI ? 4 : 1; // gathered: one unit's 1 + D + A vector loads per lane in flight, not four units' weights
#pragma unroll kUnits
        for (uint32_t h = 0; h < H; ++h) {
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                float z = W(k, o_b1 + h);
#pragma unroll
                for (int j = 0; j < D; ++j) z = __builtin_fmaf(W(k, h * D + j), x[j].v[k], z);
                const float r = (z > 0.0f) ? z : 0.0f;
#pragma unroll
                for (int a = 0; a < A; ++a) y[a][k] = __builtin_fmaf(W(k, o_w2 + a * H + h), r, y[a][k]);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
        uint8_t best = 0;
        float yb = y[0][k];
#pragma unroll
        for (int a = 1; a < A; ++a) {
            if (y[a][k] > yb) {
                yb = y[a][k];
                best = (uint8_t)a;
            }
        }
        act.v[k] = best;
    }
}

// The action source of rollout_block (gymrs_rollout_impl.h) that closes the loop: d.act from d.st.
template <class Env, int VEC, bool UNI>
struct PolicyActions {
    static constexpr bool kPolicy = true, kExplore = false;
    PolicyWeights<VEC, UNI> w;
    uint32_t hidden;
    __device__ __forceinline__ PolicyActions(const PolicyArgs& p, const uint32_t (&pol)[VEC]) : w(p, pol), hidden(p.hidden) {}
    __device__ __forceinline__ void fill(const Vec<float, VEC> (&st)[Env::kState], Vec<uint8_t, VEC>& act) const
    {
        policy_eval<Env, VEC, UNI>(w, hidden, st, act);
    }
};

// Epsilon-greedy (include/gymrs_amd.h, "exploration"): the lanes of a work-item whose draw of this step says so take the random
// action in place of act.v[k].  gid = the global id of the work-item's first lane, tick = the engine tick the step starts from.
// aligned (wave-uniform: the shard offset is a multiple of 4): four lanes share one Philox block, else every lane evaluates the
// block its word lies in (same values, slower).  A = the env's number of actions.
template <int VEC, uint32_t A>
__device__ __forceinline__ void explore_mix(const ExploreArgs& x, uint64_t gid, uint64_t tick, bool aligned, Vec<uint8_t, VEC>& act)
{
    if (aligned) {
#pragma unroll
        for (int b = 0; b < VEC / 4; ++b) {
            const u32x4 blk = explore_block(x.seed, gid + 4 * b, tick);
#pragma unroll
            for (int i = 0; i < 4; ++i)
                act.v[4 * b + i] = explore_decides(blk.v[i], x.threshold) ? explore_random(blk.v[i], A) : act.v[4 * b + i];
        }
    } else {
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            const uint32_t w = explore_word(x.seed, gid + i, tick);
            act.v[i] = explore_decides(w, x.threshold) ? explore_random(w, A) : act.v[i];
        }
    }
}

// The exploring action source of rollout_block: the policy's argmax, then the select above.  Both ends of the threshold are
// wave-uniform shortcuts that give the bits of the definition: at 0 no draw is below it (no Philox block is evaluated: the greedy
// launch at the greedy launch's cost), at 65536 every draw is (the policy is not evaluated: its action would be replaced).
template <class Env, int VEC, bool UNI>
struct ExploringActions {
    static constexpr bool kPolicy = true, kExplore = true;
    PolicyWeights<VEC, UNI> w;
    uint32_t hidden;
    ExploreArgs x;
    __device__ __forceinline__ ExploringActions(const PolicyArgs& p, const uint32_t (&pol)[VEC], const ExploreArgs& x_) : w(p, pol), hidden(p.hidden), x(x_) {}
    __device__ __forceinline__ void fill(const Vec<float, VEC> (&st)[Env::kState], Vec<uint8_t, VEC>& act, uint64_t gid, uint64_t tick,
                                         bool aligned) const
    {
        if (x.threshold < kExploreOne) {
            policy_eval<Env, VEC, UNI>(w, hidden, st, act);
        } else {
#pragma unroll
            for (int k = 0; k < VEC; ++k) act.v[k] = 0;
        }
        if (x.threshold != 0) explore_mix<VEC, (uint32_t)Env::kActions>(x, gid, tick, aligned, act);
    }
};

// Softmax sampling (include/gymrs_amd.h, "sampling"): every lane of a work-item takes the action its draw of this step selects
// under the weights of its logits (gymrs_sample.h: the text gymrs_sample_draw compiles).  gid, tick and aligned as in explore_mix:
// with an aligned offset four lanes share one Philox block of stream 3.  prob (may be NULL) gets prob[action] of every lane.
template <class Env, int VEC>
__device__ __forceinline__ void sample_pick(const SampleArgs& x, const float (&y)[Env::kActions][VEC], uint64_t gid, uint64_t tick, bool aligned,
                                            Vec<uint8_t, VEC>& act, Vec<float, VEC>* prob = nullptr)
{
    constexpr uint32_t A = (uint32_t)Env::kActions;
    uint32_t word[VEC];
    if (aligned) {
#pragma unroll
        for (int b = 0; b < VEC / 4; ++b) {
            const u32x4 blk = sample_block(x.seed, gid + 4 * b, tick);
#pragma unroll
            for (int i = 0; i < 4; ++i) word[4 * b + i] = blk.v[i];
        }
    } else {
#pragma unroll
        for (int i = 0; i < VEC; ++i) word[i] = sample_word(x.seed, gid + i, tick);
    }
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
        float yl[A], w[A];
#pragma unroll
        for (uint32_t a = 0; a < A; ++a) yl[a] = y[a][k];
        const uint32_t greedy = sample_greedy(yl, A);
        sample_weights(yl, A, greedy, x.scale, w);
        const float total = sample_total(w, A);
        const uint32_t action = sample_select(w, A, total, word[k], greedy);
        act.v[k] = (uint8_t)action;
        if (prob) prob->v[k] = sample_prob(w, total, greedy, action);
    }
}

// The sampling action source of rollout_block: the policy's logits, then the pick above.  Told which step this is like
// ExploringActions (kExplore: the same fill).
template <class Env, int VEC, bool UNI>
struct SamplingActions {
    static constexpr bool kPolicy = true, kExplore = true;
    PolicyWeights<VEC, UNI> w;
    uint32_t hidden;
    SampleArgs x;
    __device__ __forceinline__ SamplingActions(const PolicyArgs& p, const uint32_t (&pol)[VEC], const SampleArgs& x_) : w(p, pol), hidden(p.hidden), x(x_) {}
    __device__ __forceinline__ void fill(const Vec<float, VEC> (&st)[Env::kState], Vec<uint8_t, VEC>& act, uint64_t gid, uint64_t tick,
                                         bool aligned, Vec<float, VEC>* prob = nullptr) const
    {
        float y[Env::kActions][VEC];
        policy_logits<Env, VEC, UNI>(w, hidden, st, y);
        sample_pick<Env, VEC>(x, y, gid, tick, aligned, act, prob);
    }
};

// Host side: the envs that take a policy (the Discrete ones), by kind.  fn(EnvTag<Env>); any other kind is refused.
template <class Env>
struct EnvTag {
    using type = Env;
};
template <class Fn>
hipError_t dispatch_policy_env(gymrs_env_kind kind, Fn&& fn)
{
    switch (kind) {
    case GYMRS_CARTPOLE: return fn(EnvTag<CartPoleT>{});
    case GYMRS_MOUNTAIN_CAR: return fn(EnvTag<MountainCarT>{});
    default: return hipErrorInvalidValue;
    }
}

} // namespace gymrs
