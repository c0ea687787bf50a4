// gymrs_table_sample_cartpole.hip -- the sampling closed-loop and transitions kernels (gymrs_rollout_sample_impl.h) of CartPole with
// per-lane parameter tables (TableT, gymrs_tile.h): GYMRS_CLOSED_LOOP_SAMPLE | GYMRS_CLOSED_LOOP_LANE_PARAMS.  Every flag set and
// lanes-per-work-item of the uniform tables, with and without the fitness hook, recording and transitions at 4; in a translation
// unit of its own so that the build compiles it in parallel with the others.
#include "gymrs_rollout_sample_impl.h"

namespace gymrs {

hipError_t launch_rollout_sample_table_cartpole(int vec, uint32_t flags, const StepArgs& a, const RolloutArgs& r, const void* consts,
                                          const PolicyArgs& p, const SampleArgs& x, gymrs_policy_fitness* fitness, const TransitionArgs* t,
                                          hipStream_t stream)
{
    if (fitness) return rollout_sample_fitness_vec<TableT<CartPoleT>>(vec, flags, a, r, consts, p, x, fitness, stream);
    return rollout_sample_env<TableT<CartPoleT>>(vec, flags, a, r, consts, p, x, t, stream);
}

} // namespace gymrs
