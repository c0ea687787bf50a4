// gymrs_gradient_ppo.hip -- gymrs_ppo_gradient (include/gymrs_amd.h, "clipped surrogate"): the launches of gradient_ppo_kernel
// (gymrs_gradient_impl.h, the policy head with PPO = true) for CartPole and MountainCar, in a translation unit of their own so that
// they compile next to gymrs_gradient.hip, and the one entry the engine calls.
#include "gymrs_gradient_impl.h"

namespace gymrs {

hipError_t launch_ppo_gradient(gymrs_env_kind kind, const PpoArgs& a, const PolicyArgs& p, hipStream_t stream)
{
    const GradientArgs& g = a.g;
    if (g.n == 0 || g.n_steps == 0) return hipSuccess;
    // every access is addressed inside a row of `stride` lanes, a table of n_policies * stride words and n_policies pairs of
    // counters: the caller's checks (gymrs_ppo_gradient) are what makes that safe
    if (!g.obs || !g.start_obs || !g.actions || !g.coef || !a.old_prob || !g.grad || !g.excluded || g.stride < g.n || g.stride % 16 != 0)
        return hipErrorInvalidValue;
    if (g.prob == a.old_prob) return hipErrorInvalidValue;
    if (!p.weights || p.n_policies == 0 || p.lanes_per_policy == 0 || p.hidden > kMaxPolicyHidden) return hipErrorInvalidValue;
    if (p.stride != policy_floats(kind, p.hidden)) return hipErrorInvalidValue;
    return dispatch_policy_env(kind, [&](auto env) {
        using Env = typename decltype(env)::type;
        return gradient_ppo_env<Env>(a, p, stream);
    });
}

} // namespace gymrs
