// gymrs_value.hip -- gymrs_value_gradient (include/gymrs_amd.h, "value loss"): the launches of value_kernel (gymrs_value_impl.h)
// for CartPole and MountainCar, in a translation unit of their own, and the one entry the engine calls.
#include "gymrs_value_impl.h"

namespace gymrs {

hipError_t launch_value_gradient(gymrs_env_kind kind, const ValueArgs& a, const PolicyArgs& p, hipStream_t stream)
{
    if (a.n == 0 || a.n_steps == 0) return hipSuccess;
    // every access is addressed inside a row of `stride` lanes, a table of n_policies * stride words and n_policies pairs of sums
    // and counters: the caller's checks (gymrs_value_gradient) are what makes that safe
    if (!a.obs || !a.start_obs || !a.returns || !a.grad || !a.excluded || a.stride < a.n || a.stride % 16 != 0) return hipErrorInvalidValue;
    if (a.v_row && (a.v_row == a.returns || a.v_row == a.old_values)) return hipErrorInvalidValue;
    if (!p.weights || p.n_policies == 0 || p.lanes_per_policy == 0 || p.hidden > kMaxPolicyHidden) return hipErrorInvalidValue;
    if (p.stride != critic_floats(kind, p.hidden)) return hipErrorInvalidValue;
    if (p.hidden != 0 && !a.v_row) return hipErrorInvalidValue; // the chunks read V from it
    return dispatch_policy_env(kind, [&](auto env) {
        using Env = typename decltype(env)::type;
        return value_env<Env>(a, p, stream);
    });
}

} // namespace gymrs
