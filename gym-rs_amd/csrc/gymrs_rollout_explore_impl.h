// gymrs_rollout_explore_impl.h -- the closed-loop fused kernels of gymrs_rollout_policy_impl.h once more with the epsilon-greedy
// action source (ExploringActions, gymrs_policy.h): gymrs_rollout_closed_loop with GYMRS_CLOSED_LOOP_EXPLORE.  gfx950.  Kernels of
// their own and not a template parameter of the greedy ones: those keep their names, their code and their register budgets.
// Included by gymrs_explore.hip (the uniform envs) and by gymrs_table_explore_<env>.hip (TableT: per-lane parameter tables).
#pragma once
#include "gymrs_rollout_policy_impl.h"

namespace gymrs {

// Waves per SIMD the register allocator aims for (FIT: the fitness kernel), as PolicyWaves: the exploring copies hold the seed and
// threshold and, for the length of the mix, a Philox block per four lanes on top of what the greedy kernels hold.  The uniform
// envs keep the greedy kernels' 16 / VEC and, like them, spill in the heavier flag sets (up to 204 B of scratch at 4 lanes per
// work-item, 288 B at 8, both CartPole's fitness kernel; the greedy kernels: 164 B and 220 B).  A TableT family gets the highest
// budget at which none of its ten flag sets spills a vector register to scratch: PolicyWaves' but for MountainCar's plain kernel
// at 8 lanes per work-item (at 2 waves all ten spill, up to 116 B) and its fitness kernel at 4 (at 3 waves the A | S | T | F set
// spills 20 B).  profiles/policy_explore.md lists the registers and scratch of every family at these budgets.
template <class Env, int VEC, bool FIT>
struct ExploreWaves {
    static constexpr int value = PolicyWaves<Env, VEC, FIT>::value;
};
template <int VEC, bool FIT>
struct ExploreWaves<TableT<MountainCarT>, VEC, FIT> {
    static constexpr int value = VEC == 4 ? (FIT ? 2 : 3) : 1;
};

// rollout_policy_kernel with the exploring source.
template <class Env, int VEC, uint32_t FLAGS, bool REC>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(ExploreWaves<Env, VEC, false>::value, ExploreWaves<Env, VEC, false>::value))) void rollout_explore_kernel(
    const StepArgs a, const RolloutArgs r, const typename Env::Consts c, const PolicyArgs p, const ExploreArgs x)
{
    constexpr int LPB = kBlock * VEC;
    __shared__ ResetLds<Env, VEC, kBlock> lds;
    const uint64_t base = (uint64_t)blockIdx.x * LPB + (uint64_t)threadIdx.x * VEC;
    uint32_t pol[VEC];
    bool uniform;
    policy_select<VEC>(p, a.gid0 + base, pol, uniform);
    const bool full = (uint64_t)blockIdx.x * LPB + (uint64_t)((threadIdx.x >> 6) + 1) * (64 * VEC) <= a.n; // wave-uniform, see step_kernel
    if (uniform) {
        const ExploringActions<Env, VEC, true> src(p, pol, x);
        if (full)
            rollout_block<Env, VEC, FLAGS, true, REC>(a, r, c, lds, src);
        else
            rollout_block<Env, VEC, FLAGS, false, REC>(a, r, c, lds, src);
    } else {
        const ExploringActions<Env, VEC, false> src(p, pol, x);
        if (full)
            rollout_block<Env, VEC, FLAGS, true, REC>(a, r, c, lds, src);
        else
            rollout_block<Env, VEC, FLAGS, false, REC>(a, r, c, lds, src);
    }
}

// rollout_policy_fitness_kernel with the exploring source: the counters follow the action taken.
template <class Env, int VEC, uint32_t FLAGS>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(ExploreWaves<Env, VEC, true>::value, ExploreWaves<Env, VEC, true>::value))) void rollout_explore_fitness_kernel(
    const StepArgs a, const RolloutArgs r, const typename Env::Consts c, const PolicyArgs p, const ExploreArgs x, gymrs_policy_fitness* const fitness)
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
        const ExploringActions<Env, VEC, true> src(p, pol, x);
        PolicyFitness<VEC, TLIM, true> fit(fitness, pol);
        if (full)
            rollout_block<Env, VEC, FLAGS, true, false>(a, r, c, lds, src, &fit);
        else
            rollout_block<Env, VEC, FLAGS, false, false>(a, r, c, lds, src, &fit);
    } else {
        const ExploringActions<Env, VEC, false> src(p, pol, x);
        PolicyFitness<VEC, TLIM, false> fit(fitness, pol);
        if (full)
            rollout_block<Env, VEC, FLAGS, true, false>(a, r, c, lds, src, &fit);
        else
            rollout_block<Env, VEC, FLAGS, false, false>(a, r, c, lds, src, &fit);
    }
}

// The launches: lanes per work-item x flag set (gymrs_launch.h) x recording, for one env type.
template <class Env>
static hipError_t rollout_explore_vec(int vec, uint32_t flags, const StepArgs& a, const RolloutArgs& r, const void* consts, const PolicyArgs& p,
                                      const ExploreArgs& x, hipStream_t stream)
{
    return dispatch_table(vec, flags, hipErrorInvalidValue, [&](auto lanes, auto flag_set) {
        constexpr int VEC = decltype(lanes)::value;
        return dispatch_recording<VEC>(r.rec_obs != nullptr, hipErrorInvalidValue, [&](auto rec) {
            launch_begin();
            hipLaunchKernelGGL((rollout_explore_kernel<Env, VEC, decltype(flag_set)::value, decltype(rec)::value>), dim3(step_grid(a.n, VEC)),
                               dim3(kBlock), 0, stream, a, r, *static_cast<const typename Env::Consts*>(consts), p, x);
            return hipGetLastError();
        });
    });
}

template <class Env>
static hipError_t rollout_explore_fitness_vec(int vec, uint32_t flags, const StepArgs& a, const RolloutArgs& r, const void* consts,
                                              const PolicyArgs& p, const ExploreArgs& x, gymrs_policy_fitness* fitness, hipStream_t stream)
{
    return dispatch_table(vec, flags, hipErrorInvalidValue, [&](auto lanes, auto flag_set) {
        constexpr int VEC = decltype(lanes)::value;
        launch_begin();
        hipLaunchKernelGGL((rollout_explore_fitness_kernel<Env, VEC, decltype(flag_set)::value>), dim3(step_grid(a.n, VEC)), dim3(kBlock), 0, stream,
                           a, r, *static_cast<const typename Env::Consts*>(consts), p, x, fitness);
        return hipGetLastError();
    });
}

// Both families of one env type behind one entry (fitness != NULL: the fitness kernel; it has no recording variant).
template <class Env>
static hipError_t rollout_explore_env(int vec, uint32_t flags, const StepArgs& a, const RolloutArgs& r, const void* consts, const PolicyArgs& p,
                                      const ExploreArgs& x, gymrs_policy_fitness* fitness, hipStream_t stream)
{
    if (fitness) return rollout_explore_fitness_vec<Env>(vec, flags, a, r, consts, p, x, fitness, stream);
    return rollout_explore_vec<Env>(vec, flags, a, r, consts, p, x, stream);
}

} // namespace gymrs
