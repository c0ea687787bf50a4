// gymrs_rollout_explore_impl.h -- the closed-loop fused kernels of gymrs_rollout_policy_impl.h once more with the epsilon-greedy
// action source (ExploringActions, gymrs_policy.h): gymrs_rollout_closed_loop with GYMRS_CLOSED_LOOP_EXPLORE.  gfx950.  Kernels of
// their own and not a template parameter of the greedy ones: those keep their names, their code and their register budgets.  The
// body is the greedy kernels' text (GYMRS_CLOSED_LOOP_ENTRY): what is this header's own is the budgets and the declarations.
// Included by gymrs_explore.hip (the uniform envs) and by gymrs_table_explore_<env>.hip (TableT: per-lane parameter tables).
#pragma once
#include "gymrs_rollout_policy_impl.h"

namespace gymrs {

// Waves per SIMD the register allocator aims for (FIT: the fitness kernel), as PolicyWaves: the exploring kernels hold the seed and
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
    GYMRS_CLOSED_LOOP_ENTRY(ExploringActions, (p, pol, x), REC, /* no hook */, (a, r, c, lds, src))
}
template <class Env, int VEC, uint32_t FLAGS, bool REC>
static hipError_t closed_loop_kernel(Family<ClosedLoopFamily::explore>, const ClosedLoopLaunch& l)
{
    return closed_loop_submit<Env, VEC>(rollout_explore_kernel<Env, VEC, FLAGS, REC>, l, l.explore);
}

// rollout_policy_fitness_kernel with the exploring source.
template <class Env, int VEC, uint32_t FLAGS>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(ExploreWaves<Env, VEC, true>::value, ExploreWaves<Env, VEC, true>::value))) void rollout_explore_fitness_kernel(
    const StepArgs a, const RolloutArgs r, const typename Env::Consts c, const PolicyArgs p, const ExploreArgs x, gymrs_policy_fitness* const fitness)
{
    GYMRS_CLOSED_LOOP_ENTRY(ExploringActions, (p, pol, x), false, GYMRS_FITNESS_HOOK, (a, r, c, lds, src, &fit))
}
template <class Env, int VEC, uint32_t FLAGS, bool REC>
static hipError_t closed_loop_kernel(Family<ClosedLoopFamily::explore_fitness>, const ClosedLoopLaunch& l)
{
    return closed_loop_submit<Env, VEC>(rollout_explore_fitness_kernel<Env, VEC, FLAGS>, l, l.explore, l.fitness);
}

} // namespace gymrs
