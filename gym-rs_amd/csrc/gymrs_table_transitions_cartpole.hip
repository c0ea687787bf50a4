// gymrs_table_transitions_cartpole.hip -- the transition kernels (gymrs_rollout_transitions_impl.h) of CartPole with per-lane
// parameter tables (TableT, gymrs_tile.h): gymrs_rollout_transitions with GYMRS_CLOSED_LOOP_LANE_PARAMS.  The eight flag sets with
// auto-reset at 4 lanes per work-item; in a translation unit of its own so that the build compiles it in parallel with the others.
#include "gymrs_rollout_transitions_impl.h"

namespace gymrs {

hipError_t closed_loop_table_transitions_cartpole(const ClosedLoopLaunch& l) { return closed_loop_unit<TableT<CartPoleT>, ClosedLoopFamily::transitions>(l); }

} // namespace gymrs
