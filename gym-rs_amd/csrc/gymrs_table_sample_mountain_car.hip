// gymrs_table_sample_mountain_car.hip -- the sampling closed-loop and transitions kernels (gymrs_rollout_sample_impl.h) of MountainCar with
// per-lane parameter tables (TableT, gymrs_tile.h): GYMRS_CLOSED_LOOP_SAMPLE | GYMRS_CLOSED_LOOP_LANE_PARAMS.  Every flag set and
// lanes-per-work-item of the uniform tables, with and without the fitness hook, recording and transitions at 4; in a translation
// unit of its own so that the build compiles it in parallel with the others.
#include "gymrs_rollout_sample_impl.h"

namespace gymrs {

hipError_t closed_loop_table_sample_mountain_car(const ClosedLoopLaunch& l)
{
    return closed_loop_unit<TableT<MountainCarT>, ClosedLoopFamily::sample, ClosedLoopFamily::sample_fitness, ClosedLoopFamily::sample_transitions>(l);
}

} // namespace gymrs
