// gymrs_gradient.hip -- gymrs_policy_gradient (include/gymrs_amd.h, "gradients"): the launches of gradient_kernel
// (gymrs_gradient_impl.h) for CartPole and MountainCar, policy and critic head, and the one entry the engine calls.
#include "gymrs_gradient_impl.h"

namespace gymrs {

hipError_t launch_policy_gradient(gymrs_env_kind kind, bool critic, const GradientArgs& a, const PolicyArgs& p, hipStream_t stream)
{
    if (a.n == 0 || a.n_steps == 0) return hipSuccess;
    // every access is addressed inside a row of `stride` lanes and a table of n_policies * stride words: the caller's checks
    // (gymrs_policy_gradient) are what makes that safe
    if (!a.obs || !a.start_obs || !a.coef || !a.grad || !a.excluded || a.stride < a.n || a.stride % 16 != 0) return hipErrorInvalidValue;
    if (!critic && !a.actions) return hipErrorInvalidValue;
    if (critic && a.prob) return hipErrorInvalidValue;
    if (!p.weights || p.n_policies == 0 || p.lanes_per_policy == 0 || p.hidden > kMaxPolicyHidden) return hipErrorInvalidValue;
    if (p.stride != (critic ? critic_floats(kind, p.hidden) : policy_floats(kind, p.hidden))) return hipErrorInvalidValue;
    return dispatch_policy_env(kind, [&](auto env) {
        using Env = typename decltype(env)::type;
        return critic ? gradient_env<Env, true>(a, p, stream) : gradient_env<Env, false>(a, p, stream);
    });
}

} // namespace gymrs
