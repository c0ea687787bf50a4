// gymrs_table_explore_mountain_car.hip -- the exploring closed-loop kernels (gymrs_rollout_explore_impl.h) of MountainCar with per-lane
// parameter tables (TableT, gymrs_tile.h): gymrs_rollout_closed_loop with GYMRS_CLOSED_LOOP_EXPLORE | GYMRS_CLOSED_LOOP_LANE_PARAMS.
// Every flag set and lanes-per-work-item of the uniform tables, with and without the fitness hook, recording at 4; in a
// translation unit of its own so that the build compiles it in parallel with the others.
#include "gymrs_rollout_explore_impl.h"

namespace gymrs {

hipError_t launch_rollout_explore_table_mountain_car(int vec, uint32_t flags, const StepArgs& a, const RolloutArgs& r, const void* consts,
                                           const PolicyArgs& p, const ExploreArgs& x, gymrs_policy_fitness* fitness, hipStream_t stream)
{
    return rollout_explore_env<TableT<MountainCarT>>(vec, flags, a, r, consts, p, x, fitness, stream);
}

} // namespace gymrs
