// gymrs_rollout_fitness.hip -- gymrs_rollout_policy_fitness: the launch of rollout_policy_fitness_kernel
// (gymrs_rollout_policy_impl.h) for the uniform envs; the parameter-table instantiations live in gymrs_table_policy_<env>.hip.
#include "gymrs_rollout_policy_impl.h"

namespace gymrs {

hipError_t closed_loop_rollout_fitness_cartpole(const ClosedLoopLaunch& l) { return closed_loop_unit<CartPoleT, ClosedLoopFamily::policy_fitness>(l); }
hipError_t closed_loop_rollout_fitness_mountain_car(const ClosedLoopLaunch& l) { return closed_loop_unit<MountainCarT, ClosedLoopFamily::policy_fitness>(l); }

} // namespace gymrs
