// gymrs_vtrace.hip -- gymrs_vtrace (include/gymrs_amd.h, "V-trace"): the launches of vtrace_kernel (gymrs_vtrace_impl.h) for CartPole
// and MountainCar, and the one entry the engine calls.
#include "gymrs_vtrace_impl.h"

namespace gymrs {

hipError_t launch_vtrace(gymrs_env_kind kind, const VtraceArgs& a, const PolicyArgs& policy, const PolicyArgs& critic, hipStream_t stream)
{
    if (a.n == 0 || a.n_steps == 0) return hipSuccess;
    // every access is addressed inside a row of `stride` lanes: the caller's checks (gymrs_vtrace) are what makes that safe
    if (!a.obs || !a.actions || !a.reward || !a.done || !a.start_obs || !a.old_prob || !a.vs || !a.pg || a.stride < a.n || a.stride % 16 != 0)
        return hipErrorInvalidValue;
    if (!policy.weights || !critic.weights || policy.n_policies == 0 || policy.lanes_per_policy == 0 || critic.n_policies == 0 || critic.lanes_per_policy == 0)
        return hipErrorInvalidValue;
    return dispatch_policy_env(kind, [&](auto env) { return vtrace_env<typename decltype(env)::type>(a, policy, critic, stream); });
}

} // namespace gymrs
