// gymrs_table_policy_cartpole.hip -- the closed-loop fused kernels (gymrs_rollout_policy_impl.h) of CartPole with per-lane
// parameter tables (TableT, gymrs_tile.h): gymrs_rollout_closed_loop with GYMRS_CLOSED_LOOP_LANE_PARAMS.  Every flag set and
// lanes-per-work-item of the uniform tables, with and without the fitness hook, recording at 4; in a translation unit of its
// own so that the build compiles it in parallel with the others.
#include "gymrs_rollout_policy_impl.h"

namespace gymrs {

hipError_t launch_rollout_policy_table_cartpole(int vec, uint32_t flags, const StepArgs& a, const RolloutArgs& r, const void* consts,
                                                    const PolicyArgs& p, hipStream_t stream)
{
    return rollout_policy_vec<TableT<CartPoleT>>(vec, flags, a, r, consts, p, stream);
}

hipError_t launch_rollout_policy_fitness_table_cartpole(int vec, uint32_t flags, const StepArgs& a, const RolloutArgs& r, const void* consts,
                                                            const PolicyArgs& p, gymrs_policy_fitness* fitness, hipStream_t stream)
{
    return rollout_policy_fitness_vec<TableT<CartPoleT>>(vec, flags, a, r, consts, p, fitness, stream);
}

} // namespace gymrs
