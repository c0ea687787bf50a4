// gymrs_table_policy_mountain_car.hip -- the closed-loop fused kernels (gymrs_rollout_policy_impl.h) of MountainCar with per-lane
// parameter tables (TableT, gymrs_tile.h): gymrs_rollout_closed_loop with GYMRS_CLOSED_LOOP_LANE_PARAMS.  Every flag set and
// lanes-per-work-item of the uniform tables, with and without the fitness hook, recording at 4; in a translation unit of its
// own so that the build compiles it in parallel with the others.
#include "gymrs_rollout_policy_impl.h"

namespace gymrs {

hipError_t closed_loop_table_policy_mountain_car(const ClosedLoopLaunch& l)
{
    return closed_loop_unit<TableT<MountainCarT>, ClosedLoopFamily::policy, ClosedLoopFamily::policy_fitness>(l);
}

} // namespace gymrs
