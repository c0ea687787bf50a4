// gymrs_rollout_sample_impl.h -- the closed-loop fused kernels of gymrs_rollout_explore_impl.h and the transitions kernel of
// gymrs_rollout_transitions_impl.h once more with the softmax sampling action source (SamplingActions, gymrs_policy.h):
// gymrs_rollout_closed_loop and gymrs_rollout_transitions with GYMRS_CLOSED_LOOP_SAMPLE.  gfx950.  Kernels of their own: the greedy
// and exploring families keep their names, their code and their register budgets.  Included by gymrs_sample.hip and
// gymrs_sample_fitness.hip (the uniform envs) and by gymrs_table_sample_<env>.hip (TableT: per-lane parameter tables).
#pragma once
#include "gymrs_rollout_transitions_impl.h"

namespace gymrs {

// Waves per SIMD the register allocator aims for (FIT: the fitness kernel), as ExploreWaves: the sampling copies hold the A logits
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
    constexpr int LPB = kBlock * VEC;
    __shared__ ResetLds<Env, VEC, kBlock> lds;
    const uint64_t base = (uint64_t)blockIdx.x * LPB + (uint64_t)threadIdx.x * VEC;
    uint32_t pol[VEC];
    bool uniform;
    policy_select<VEC>(p, a.gid0 + base, pol, uniform);
    const bool full = (uint64_t)blockIdx.x * LPB + (uint64_t)((threadIdx.x >> 6) + 1) * (64 * VEC) <= a.n; // wave-uniform, see step_kernel
    if (uniform) {
        const SamplingActions<Env, VEC, true> src(p, pol, x);
        if (full)
            rollout_block<Env, VEC, FLAGS, true, REC>(a, r, c, lds, src);
        else
            rollout_block<Env, VEC, FLAGS, false, REC>(a, r, c, lds, src);
    } else {
        const SamplingActions<Env, VEC, false> src(p, pol, x);
        if (full)
            rollout_block<Env, VEC, FLAGS, true, REC>(a, r, c, lds, src);
        else
            rollout_block<Env, VEC, FLAGS, false, REC>(a, r, c, lds, src);
    }
}

// rollout_explore_fitness_kernel with the sampling source: the counters follow the action taken.
template <class Env, int VEC, uint32_t FLAGS>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(SampleWaves<Env, VEC, true>::value, SampleWaves<Env, VEC, true>::value))) void rollout_sample_fitness_kernel(
    const StepArgs a, const RolloutArgs r, const typename Env::Consts c, const PolicyArgs p, const SampleArgs x, gymrs_policy_fitness* const fitness)
{
    constexpr int LPB = kBlock * VEC;
    constexpr bool TLIM = (FLAGS & GYMRS_TIME_LIMIT) != 0;
    __shared__ ResetLds<Env, VEC, kBlock> lds;
    const uint64_t base = (uint64_t)blockIdx.x * LPB + (uint64_t)threadIdx.x * VEC;
    uint32_t pol[VEC];
    bool uniform;
    policy_select<VEC>(p, a.gid0 + base, pol, uniform);
    const bool full = (uint64_t)blockIdx.x * LPB + (uint64_t)((threadIdx.x >> 6) + 1) * (64 * VEC) <= a.n; // wave-uniform, see step_kernel
    if (uniform) {
        const SamplingActions<Env, VEC, true> src(p, pol, x);
        PolicyFitness<VEC, TLIM, true> fit(fitness, pol);
        if (full)
            rollout_block<Env, VEC, FLAGS, true, false>(a, r, c, lds, src, &fit);
        else
            rollout_block<Env, VEC, FLAGS, false, false>(a, r, c, lds, src, &fit);
    } else {
        const SamplingActions<Env, VEC, false> src(p, pol, x);
        PolicyFitness<VEC, TLIM, false> fit(fitness, pol);
        if (full)
            rollout_block<Env, VEC, FLAGS, true, false>(a, r, c, lds, src, &fit);
        else
            rollout_block<Env, VEC, FLAGS, false, false>(a, r, c, lds, src, &fit);
    }
}

// rollout_transitions_kernel with the sampling source.
template <class Env, uint32_t FLAGS>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(SampleTransitionWaves<Env>::value, SampleTransitionWaves<Env>::value))) void rollout_sample_transitions_kernel(
    const StepArgs a, const RolloutArgs r, const typename Env::Consts c, const PolicyArgs p, const SampleArgs x, const TransitionArgs t)
{
    constexpr int VEC = 4; // the record's rule
    static_assert((FLAGS & GYMRS_AUTO_RESET) != 0, "without auto-reset nothing is re-armed: the record's obs rows are the final observations");
    constexpr int LPB = kBlock * VEC;
    __shared__ ResetLds<Env, VEC, kBlock> lds;
    const uint64_t base = (uint64_t)blockIdx.x * LPB + (uint64_t)threadIdx.x * VEC;
    uint32_t pol[VEC];
    bool uniform;
    policy_select<VEC>(p, a.gid0 + base, pol, uniform);
    const bool full = (uint64_t)blockIdx.x * LPB + (uint64_t)((threadIdx.x >> 6) + 1) * (64 * VEC) <= a.n; // wave-uniform, see step_kernel
    FinalObsRows<Env, VEC> sink(t, r);
    if (uniform) {
        const SamplingActions<Env, VEC, true> src(p, pol, x);
        if (full)
            rollout_block<Env, VEC, FLAGS, true, true>(a, r, c, lds, src, static_cast<NoFitness*>(nullptr), &sink);
        else
            rollout_block<Env, VEC, FLAGS, false, true>(a, r, c, lds, src, static_cast<NoFitness*>(nullptr), &sink);
    } else {
        const SamplingActions<Env, VEC, false> src(p, pol, x);
        if (full)
            rollout_block<Env, VEC, FLAGS, true, true>(a, r, c, lds, src, static_cast<NoFitness*>(nullptr), &sink);
        else
            rollout_block<Env, VEC, FLAGS, false, true>(a, r, c, lds, src, static_cast<NoFitness*>(nullptr), &sink);
    }
}

// The launches: lanes per work-item x flag set (gymrs_launch.h) x recording, for one env type.
template <class Env>
static hipError_t rollout_sample_vec(int vec, uint32_t flags, const StepArgs& a, const RolloutArgs& r, const void* consts, const PolicyArgs& p,
                                     const SampleArgs& x, hipStream_t stream)
{
    return dispatch_table(vec, flags, hipErrorInvalidValue, [&](auto lanes, auto flag_set) {
        constexpr int VEC = decltype(lanes)::value;
        return dispatch_recording<VEC>(r.rec_obs != nullptr, hipErrorInvalidValue, [&](auto rec) {
            launch_begin();
            hipLaunchKernelGGL((rollout_sample_kernel<Env, VEC, decltype(flag_set)::value, decltype(rec)::value>), dim3(step_grid(a.n, VEC)),
                               dim3(kBlock), 0, stream, a, r, *static_cast<const typename Env::Consts*>(consts), p, x);
            return hipGetLastError();
        });
    });
}

template <class Env>
static hipError_t rollout_sample_fitness_vec(int vec, uint32_t flags, const StepArgs& a, const RolloutArgs& r, const void* consts,
                                             const PolicyArgs& p, const SampleArgs& x, gymrs_policy_fitness* fitness, hipStream_t stream)
{
    return dispatch_table(vec, flags, hipErrorInvalidValue, [&](auto lanes, auto flag_set) {
        constexpr int VEC = decltype(lanes)::value;
        launch_begin();
        hipLaunchKernelGGL((rollout_sample_fitness_kernel<Env, VEC, decltype(flag_set)::value>), dim3(step_grid(a.n, VEC)), dim3(kBlock), 0, stream,
                           a, r, *static_cast<const typename Env::Consts*>(consts), p, x, fitness);
        return hipGetLastError();
    });
}

// The eight flag sets with GYMRS_AUTO_RESET, 4 lanes per work-item.
template <class Env>
static hipError_t rollout_sample_transitions_env(uint32_t flags, const StepArgs& a, const RolloutArgs& r, const void* consts, const PolicyArgs& p,
                                                 const SampleArgs& x, const TransitionArgs& t, hipStream_t stream)
{
    return dispatch_auto_reset_flag_set(flags, hipErrorInvalidValue, [&](auto flag_set) {
        launch_begin();
        hipLaunchKernelGGL((rollout_sample_transitions_kernel<Env, decltype(flag_set)::value>), dim3(step_grid(a.n, 4)), dim3(kBlock), 0, stream, a,
                           r, *static_cast<const typename Env::Consts*>(consts), p, x, t);
        return hipGetLastError();
    });
}

// The plain / recording family and the transitions family of one env type behind one entry (t != NULL: transitions).
template <class Env>
static hipError_t rollout_sample_env(int vec, uint32_t flags, const StepArgs& a, const RolloutArgs& r, const void* consts, const PolicyArgs& p,
                                     const SampleArgs& x, const TransitionArgs* t, hipStream_t stream)
{
    if (t) return rollout_sample_transitions_env<Env>(flags, a, r, consts, p, x, *t, stream);
    return rollout_sample_vec<Env>(vec, flags, a, r, consts, p, x, stream);
}

} // namespace gymrs
