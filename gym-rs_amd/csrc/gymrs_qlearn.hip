// gymrs_qlearn.hip -- gymrs_q_gradient (include/gymrs_amd.h, "Q-learning"): the launches of q_td_kernel and q_gradient_kernel
// (gymrs_qlearn_impl.h) for CartPole and MountainCar, and the one entry the engine calls.
#include "gymrs_qlearn_impl.h"

namespace gymrs {

hipError_t launch_q_gradient(gymrs_env_kind kind, const QArgs& a, const PolicyArgs& p, const PolicyArgs& pt, hipStream_t stream)
{
    if (a.n == 0 || a.n_steps == 0) return hipSuccess;
    // every access is addressed inside a row of `stride` lanes, a table of n_policies * stride words and n_policies counters (pairs
    // of counters): the caller's checks (gymrs_q_gradient) are what makes that safe
    if (!a.obs || !a.actions || !a.reward || !a.done || !a.final_obs || !a.start_obs || !a.td || !a.grad || !a.excluded || a.stride < a.n ||
        a.stride % 16 != 0)
        return hipErrorInvalidValue;
    if (a.flags & ~GYMRS_Q_DOUBLE) return hipErrorInvalidValue;
    if (!p.weights || !pt.weights || p.n_policies == 0 || p.lanes_per_policy == 0 || p.hidden > kMaxPolicyHidden) return hipErrorInvalidValue;
    if (p.stride != policy_floats(kind, p.hidden)) return hipErrorInvalidValue;
    if (pt.n_policies != p.n_policies || pt.lanes_per_policy != p.lanes_per_policy || pt.hidden != p.hidden || pt.stride != p.stride)
        return hipErrorInvalidValue;
    return dispatch_policy_env(kind, [&](auto env) {
        using Env = typename decltype(env)::type;
        return q_gradient_env<Env>(a, p, pt, stream);
    });
}

} // namespace gymrs
