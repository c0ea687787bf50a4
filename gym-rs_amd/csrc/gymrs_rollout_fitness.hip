// gymrs_rollout_fitness.hip -- gymrs_rollout_policy_fitness: the launch of rollout_policy_fitness_kernel
// (gymrs_rollout_policy_impl.h) for the uniform envs; the parameter-table instantiations live in gymrs_table_policy_<env>.hip.
#include "gymrs_rollout_policy_impl.h"

namespace gymrs {

hipError_t launch_rollout_policy_fitness_table_cartpole(int vec, uint32_t flags, const StepArgs& a, const RolloutArgs& r, const void* consts,
                                                        const PolicyArgs& p, gymrs_policy_fitness* fitness, hipStream_t stream);
hipError_t launch_rollout_policy_fitness_table_mountain_car(int vec, uint32_t flags, const StepArgs& a, const RolloutArgs& r, const void* consts,
                                                            const PolicyArgs& p, gymrs_policy_fitness* fitness, hipStream_t stream);

hipError_t launch_rollout_policy_fitness(gymrs_env_kind kind, int vec, uint32_t flags, const StepArgs& a, const RolloutArgs& r, const void* consts,
                                         const PolicyArgs& p, gymrs_policy_fitness* fitness, hipStream_t stream)
{
    if (a.n == 0 || r.n_steps == 0) return hipSuccess;
    if (r.rec_obs || !fitness || r.n_steps > kMaxFitnessSteps) return hipErrorInvalidValue;
    if (flags & kFlagTable) {
        switch (kind) {
        case GYMRS_CARTPOLE: return launch_rollout_policy_fitness_table_cartpole(vec, flags, a, r, consts, p, fitness, stream);
        case GYMRS_MOUNTAIN_CAR: return launch_rollout_policy_fitness_table_mountain_car(vec, flags, a, r, consts, p, fitness, stream);
        default: return hipErrorInvalidValue;
        }
    }
    return dispatch_policy_env(kind, [&](auto env) {
        return rollout_policy_fitness_vec<typename decltype(env)::type>(vec, flags, a, r, consts, p, fitness, stream);
    });
}

} // namespace gymrs
