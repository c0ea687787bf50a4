// gymrs_entropy.hip -- gymrs_entropy_gradient (include/gymrs_amd.h, "Entropy"): the launches of entropy_kernel (gymrs_entropy_impl.h) for
// CartPole and MountainCar, with and without the KL estimate, in a translation unit of their own so that they compile next to
// gymrs_gradient.hip and gymrs_gradient_ppo.hip, and the one entry the engine calls.
#include "gymrs_entropy_impl.h"

namespace gymrs {

hipError_t launch_entropy_gradient(gymrs_env_kind kind, const EntropyArgs& a, const PolicyArgs& p, hipStream_t stream)
{
    if (a.n == 0 || a.n_steps == 0) return hipSuccess;
    // every access is addressed inside a row of `stride` lanes, a table of n_policies * stride words and n_policies pairs of sums
    // and counters: the caller's checks (gymrs_entropy_gradient) are what makes that safe
    if (!a.obs || !a.start_obs || !a.grad || !a.excluded || !a.sums || a.stride < a.n || a.stride % 16 != 0) return hipErrorInvalidValue;
    if (a.old_prob && !a.actions) return hipErrorInvalidValue;
    if (!p.weights || p.n_policies == 0 || p.lanes_per_policy == 0 || p.hidden > kMaxPolicyHidden) return hipErrorInvalidValue;
    if (p.stride != policy_floats(kind, p.hidden)) return hipErrorInvalidValue;
    return dispatch_policy_env(kind, [&](auto env) {
        using Env = typename decltype(env)::type;
        return a.old_prob ? entropy_env<Env, true>(a, p, stream) : entropy_env<Env, false>(a, p, stream);
    });
}

} // namespace gymrs
