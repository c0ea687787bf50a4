// gymrs_advantages.hip -- gymrs_advantages (include/gymrs_amd.h, "advantages"): the launches of advantages_kernel
// (gymrs_advantages_impl.h) for CartPole and MountainCar, critic on and off, and the one entry the engine calls.
#include "gymrs_advantages_impl.h"

namespace gymrs {

hipError_t launch_advantages(gymrs_env_kind kind, const AdvantageArgs& a, const PolicyArgs* critic, hipStream_t stream)
{
    if (a.n == 0 || a.n_steps == 0) return hipSuccess;
    // every access is addressed inside a row of `stride` lanes: the caller's checks (gymrs_advantages) are what makes that safe
    if (!a.reward || !a.done || !a.advantages || a.stride < a.n || a.stride % 16 != 0) return hipErrorInvalidValue;
    if (critic && (!critic->weights || !a.obs || !a.start_obs || critic->n_policies == 0 || critic->lanes_per_policy == 0)) return hipErrorInvalidValue;
    return dispatch_policy_env(kind, [&](auto env) { return advantages_env<typename decltype(env)::type>(a, critic, stream); });
}

} // namespace gymrs
