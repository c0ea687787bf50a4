// gymrs_rollout_sample_impl.h -- the closed-loop fused kernels of gymrs_rollout_explore_impl.h and the transitions kernel of
// gymrs_rollout_transitions_impl.h once more with the softmax sampling action source (SamplingActions, gymrs_policy.h):
// gymrs_rollout_closed_loop and gymrs_rollout_transitions with GYMRS_CLOSED_LOOP_SAMPLE.  gfx950.  Kernels of their own: the greedy
// and exploring families keep their names, their code and their register budgets; the body is the text they share
// (GYMRS_CLOSED_LOOP_ENTRY, #undef'd at the end of this header: the last one that expands it).  Included by gymrs_sample.hip and
// gymrs_sample_fitness.hip (the uniform envs) and by gymrs_table_sample_<env>.hip (TableT: per-lane parameter tables).
#pragma once
#include "gymrs_rollout_transitions_impl.h"

namespace gymrs {

// Waves per SIMD the register allocator aims for (FIT: the fitness kernel), as ExploreWaves: the sampling kernels hold the A logits
// and A weights of a lane and, for the length of the pick, a Philox block per four lanes.  The uniform envs keep the greedy kernels'
// 16 / VEC (they spill there already); a TableT family gets the highest budget at which none of its ten flag sets spills a vector
// register to scratch: ExploreWaves' but for MountainCar's recording kernel (REC), whose A | S | T | F set spills 4 registers (20 B) at
// 3 waves.  profiles/policy_sample.md lists the registers and scratch of every family at these budgets.
template <class Env, int VEC, bool FIT, bool REC = false>
struct SampleWaves {
    static constexpr int value = ExploreWaves<Env, VEC, FIT>::value;
};
template <>
struct SampleWaves<TableT<MountainCarT>, 4, false, true> {
    static constexpr int value = 2;
};
// ... and for the transitions kernel, as TransitionWaves.
template <class Env>
struct SampleTransitionWaves {
    static constexpr int value = TransitionWaves<Env>::value;
};

// rollout_explore_kernel with the sampling source.
template <class Env, int VEC, uint32_t FLAGS, bool REC>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(SampleWaves<Env, VEC, false, REC>::value, SampleWaves<Env, VEC, false, REC>::value))) void rollout_sample_kernel(
    const StepArgs a, const RolloutArgs r, const typename Env::Consts c, const PolicyArgs p, const SampleArgs x)
{
    GYMRS_CLOSED_LOOP_ENTRY(SamplingActions, (p, pol, x), REC, /* no hook */, (a, r, c, lds, src))
}
template <class Env, int VEC, uint32_t FLAGS, bool REC>
static hipError_t closed_loop_kernel(Family<ClosedLoopFamily::sample>, const ClosedLoopLaunch& l)
{
    return closed_loop_submit<Env, VEC>(rollout_sample_kernel<Env, VEC, FLAGS, REC>, l, l.sample);
}

// rollout_explore_fitness_kernel with the sampling source.
template <class Env, int VEC, uint32_t FLAGS>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(SampleWaves<Env, VEC, true>::value, SampleWaves<Env, VEC, true>::value))) void rollout_sample_fitness_kernel(
    const StepArgs a, const RolloutArgs r, const typename Env::Consts c, const PolicyArgs p, const SampleArgs x, gymrs_policy_fitness* const fitness)
{
    GYMRS_CLOSED_LOOP_ENTRY(SamplingActions, (p, pol, x), false, GYMRS_FITNESS_HOOK, (a, r, c, lds, src, &fit))
}
template <class Env, int VEC, uint32_t FLAGS, bool REC>
static hipError_t closed_loop_kernel(Family<ClosedLoopFamily::sample_fitness>, const ClosedLoopLaunch& l)
{
    return closed_loop_submit<Env, VEC>(rollout_sample_fitness_kernel<Env, VEC, FLAGS>, l, l.sample, l.fitness);
}

// rollout_transitions_kernel with the sampling source.
template <class Env, uint32_t FLAGS>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(SampleTransitionWaves<Env>::value, SampleTransitionWaves<Env>::value))) void rollout_sample_transitions_kernel(
    const StepArgs a, const RolloutArgs r, const typename Env::Consts c, const PolicyArgs p, const SampleArgs x, const TransitionArgs t)
{
    constexpr int VEC = 4; // the record's rule
    static_assert((FLAGS & GYMRS_AUTO_RESET) != 0, "without auto-reset nothing is re-armed: the record's obs rows are the final observations");
    FinalObsRows<Env, VEC> sink(t, r);
    GYMRS_CLOSED_LOOP_ENTRY(SamplingActions, (p, pol, x), true, /* no hook */, (a, r, c, lds, src, static_cast<NoFitness*>(nullptr), &sink))
}
template <class Env, int VEC, uint32_t FLAGS, bool REC>
static hipError_t closed_loop_kernel(Family<ClosedLoopFamily::sample_transitions>, const ClosedLoopLaunch& l)
{
    static_assert(VEC == 4 && REC, "the record's rule");
    return closed_loop_submit<Env, VEC>(rollout_sample_transitions_kernel<Env, FLAGS>, l, l.sample, *l.transitions);
}

#undef GYMRS_CLOSED_LOOP_ENTRY // the last header that expands them
#undef GYMRS_FITNESS_HOOK

} // namespace gymrs
