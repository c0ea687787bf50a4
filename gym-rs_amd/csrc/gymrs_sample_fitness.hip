// gymrs_sample_fitness.hip -- the launch of rollout_sample_fitness_kernel (gymrs_rollout_sample_impl.h) for the uniform envs:
// gymrs_rollout_closed_loop with GYMRS_CLOSED_LOOP_SAMPLE | GYMRS_CLOSED_LOOP_FITNESS.  In a translation unit of its own so that
// the build compiles it in parallel with gymrs_sample.hip.
#include "gymrs_rollout_sample_impl.h"

namespace gymrs {

hipError_t closed_loop_sample_fitness_cartpole(const ClosedLoopLaunch& l) { return closed_loop_unit<CartPoleT, ClosedLoopFamily::sample_fitness>(l); }
hipError_t closed_loop_sample_fitness_mountain_car(const ClosedLoopLaunch& l) { return closed_loop_unit<MountainCarT, ClosedLoopFamily::sample_fitness>(l); }

} // namespace gymrs
