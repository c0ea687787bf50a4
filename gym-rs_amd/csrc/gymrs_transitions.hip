// gymrs_transitions.hip -- gymrs_rollout_transitions (include/gymrs_amd.h, "transitions"): the launches of
// rollout_transitions_kernel (gymrs_rollout_transitions_impl.h) for CartPole and MountainCar with uniform constants, and the one
// entry the engine calls.  The parameter-table instantiations (kFlagTable) live in gymrs_table_transitions_<env>.hip.
#include "gymrs_rollout_transitions_impl.h"

namespace gymrs {

hipError_t launch_rollout_transitions_table_cartpole(uint32_t flags, const StepArgs& a, const RolloutArgs& r, const void* consts, const PolicyArgs& p,
                                                     const ExploreArgs& x, const TransitionArgs& t, hipStream_t stream);
hipError_t launch_rollout_transitions_table_mountain_car(uint32_t flags, const StepArgs& a, const RolloutArgs& r, const void* consts,
                                                         const PolicyArgs& p, const ExploreArgs& x, const TransitionArgs& t, hipStream_t stream);

hipError_t launch_rollout_transitions(gymrs_env_kind kind, uint32_t flags, const StepArgs& a, const RolloutArgs& r, const void* consts,
                                      const PolicyArgs& p, const ExploreArgs& x, const TransitionArgs& t, hipStream_t stream)
{
    if (a.n == 0 || r.n_steps == 0) return hipSuccess;
    // every store is addressed inside a row of rec_stride lanes: the caller's checks (check_trajectory) are what makes that safe
    if (!r.rec_obs || !t.final_obs || r.rec_stride < a.n) return hipErrorInvalidValue;
    if (flags & kFlagTable) {
        switch (kind) {
        case GYMRS_CARTPOLE: return launch_rollout_transitions_table_cartpole(flags, a, r, consts, p, x, t, stream);
        case GYMRS_MOUNTAIN_CAR: return launch_rollout_transitions_table_mountain_car(flags, a, r, consts, p, x, t, stream);
        default: return hipErrorInvalidValue;
        }
    }
    return dispatch_policy_env(kind, [&](auto env) { return rollout_transitions_env<typename decltype(env)::type>(flags, a, r, consts, p, x, t, stream); });
}

} // namespace gymrs
