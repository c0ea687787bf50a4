// gymrs_explore_fitness.hip -- the launch of rollout_explore_fitness_kernel (gymrs_rollout_explore_impl.h) for the uniform envs:
// gymrs_rollout_closed_loop with GYMRS_CLOSED_LOOP_EXPLORE | GYMRS_CLOSED_LOOP_FITNESS.  In a translation unit of its own so that
// the build compiles it in parallel with gymrs_explore.hip.
#include "gymrs_rollout_explore_impl.h"

namespace gymrs {

hipError_t closed_loop_explore_fitness_cartpole(const ClosedLoopLaunch& l) { return closed_loop_unit<CartPoleT, ClosedLoopFamily::explore_fitness>(l); }
hipError_t closed_loop_explore_fitness_mountain_car(const ClosedLoopLaunch& l) { return closed_loop_unit<MountainCarT, ClosedLoopFamily::explore_fitness>(l); }

} // namespace gymrs
