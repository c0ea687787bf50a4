// gymrs_transitions.hip -- gymrs_rollout_transitions (include/gymrs_amd.h, "transitions"): the launches of
// rollout_transitions_kernel (gymrs_rollout_transitions_impl.h) for CartPole and MountainCar with uniform constants.  The parameter-table instantiations (kFlagTable) live in gymrs_table_transitions_<env>.hip.
#include "gymrs_rollout_transitions_impl.h"

namespace gymrs {

hipError_t closed_loop_transitions_cartpole(const ClosedLoopLaunch& l) { return closed_loop_unit<CartPoleT, ClosedLoopFamily::transitions>(l); }
hipError_t closed_loop_transitions_mountain_car(const ClosedLoopLaunch& l) { return closed_loop_unit<MountainCarT, ClosedLoopFamily::transitions>(l); }

} // namespace gymrs
