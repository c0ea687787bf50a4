// gymrs_evaluate.hip -- gymrs_evaluate_policy: the evaluation kernels of the uniform envs (gymrs_evaluate_impl.h), the identity
// launch of the records and the dispatch of a launch (a parameter table: gymrs_table_<env>.hip).
#include "gymrs_evaluate_impl.h"

namespace gymrs {

__global__ __launch_bounds__(kBlock) void policy_eval_identity_kernel(gymrs_policy_eval* table, uint32_t n_policies)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i < n_policies) table[i] = gymrs_policy_eval{0, 0, 0, 0, 0, 0, INT64_MAX, INT64_MIN};
}

hipError_t launch_policy_eval_identity(gymrs_policy_eval* table, uint32_t n_policies, hipStream_t stream)
{
    if (!table || n_policies == 0) return hipErrorInvalidValue;
    launch_begin();
    hipLaunchKernelGGL(policy_eval_identity_kernel, dim3((n_policies + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, table, n_policies);
    return hipGetLastError();
}

// the evaluation kernels of an engine with a parameter table live in the translation unit of the env's other table kernels
hipError_t launch_evaluate_table_cartpole(const EvalArgs& a, const TableConsts& c, const PolicyArgs& p, hipStream_t stream);
hipError_t launch_evaluate_table_mountain_car(const EvalArgs& a, const TableConsts& c, const PolicyArgs& p, hipStream_t stream);

hipError_t launch_evaluate_policy(gymrs_env_kind kind, uint32_t flags, const EvalArgs& a, const void* consts, const PolicyArgs& p, hipStream_t stream)
{
    if (a.n == 0) return hipSuccess;
    if (!a.table || !p.weights || p.n_policies == 0 || p.lanes_per_policy == 0 || a.episodes == 0 || a.max_steps == 0 ||
        (uint64_t)a.episodes * a.max_steps > kMaxEvalSteps)
        return hipErrorInvalidValue;
    launch_begin();
    if (flags & kFlagTable) { // (consts is a TableConsts)
        const TableConsts& tc = *static_cast<const TableConsts*>(consts);
        if (!tc.rows || !tc.index || tc.k == 0 || tc.k > kMaxParamRows) return hipErrorInvalidValue;
        switch (kind) {
        case GYMRS_CARTPOLE: return launch_evaluate_table_cartpole(a, tc, p, stream);
        case GYMRS_MOUNTAIN_CAR: return launch_evaluate_table_mountain_car(a, tc, p, stream);
        default: return hipErrorInvalidValue;
        }
    }
    return dispatch_policy_env(kind, [&](auto env) {
        using Env = typename decltype(env)::type;
        hipLaunchKernelGGL((evaluate_policy_kernel<Env>), dim3(step_grid(a.n, kEvalVec)), dim3(kBlock), 0, stream, a,
                           *static_cast<const typename Env::Consts*>(consts), p);
        return hipGetLastError();
    });
}

} // namespace gymrs
