// gymrs_sample_fitness.hip -- the launch of rollout_sample_fitness_kernel (gymrs_rollout_sample_impl.h) for the uniform envs:
// gymrs_rollout_closed_loop with GYMRS_CLOSED_LOOP_SAMPLE | GYMRS_CLOSED_LOOP_FITNESS.  In a translation unit of its own so that
// the build compiles it in parallel with gymrs_sample.hip.
#include "gymrs_rollout_sample_impl.h"

namespace gymrs {

hipError_t launch_rollout_sample_fitness(gymrs_env_kind kind, int vec, uint32_t flags, const StepArgs& a, const RolloutArgs& r, const void* consts,
                                         const PolicyArgs& p, const SampleArgs& x, gymrs_policy_fitness* fitness, hipStream_t stream)
{
    return dispatch_policy_env(kind, [&](auto env) {
        return rollout_sample_fitness_vec<typename decltype(env)::type>(vec, flags, a, r, consts, p, x, fitness, stream);
    });
}

} // namespace gymrs
