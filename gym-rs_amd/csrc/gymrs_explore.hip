// gymrs_explore.hip -- epsilon-greedy exploration (include/gymrs_amd.h, "exploration"): explore_actions_kernel (the per-step
// counterpart: gymrs_policy_actions mixed with the draw of the engine's tick) and the launches of rollout_explore_kernel
// (gymrs_rollout_explore_impl.h) for CartPole and MountainCar with uniform constants.  The fitness variant lives in
// gymrs_explore_fitness.hip, the parameter-table instantiations (kFlagTable) in gymrs_table_explore_<env>.hip.
#include "gymrs_rollout_explore_impl.h"

namespace gymrs {

// gymrs_explore_actions: policy_actions_kernel (gymrs_rollout_policy.hip) with the exploring source's fill.
template <class Env, bool UNI>
__device__ __forceinline__ void explore_actions_block(const float* const (&s)[4], uint8_t* __restrict__ actions, uint64_t n, uint64_t base,
                                                      bool full, uint64_t gid, uint64_t tick, const PolicyArgs& p, const ExploreArgs& x,
                                                      const uint32_t (&pol)[4])
{
    Vec<float, 4> obs[Env::kState];
#pragma unroll
    for (int j = 0; j < Env::kState; ++j) obs[j] = load_vec<float, 4, false>(s[j], base, n, full, 0.0f);
    const ExploringActions<Env, 4, UNI> src(p, pol, x);
    Vec<uint8_t, 4> act;
    src.fill(obs, act, gid, tick, (gid & 3u) == 0); // (base is a multiple of 4: the offset decides, wave-uniformly)
    store_vec<uint8_t, 4, false>(actions, base, n, full, act);
}

template <class Env>
__global__ __launch_bounds__(kBlock) void explore_actions_kernel(const float* s0, const float* s1, const float* s2, const float* s3,
                                                                 uint8_t* actions, uint64_t n, uint64_t n_fast, uint64_t gid0, uint64_t tick,
                                                                 const PolicyArgs p, const ExploreArgs x)
{
    const uint64_t base = (uint64_t)blockIdx.x * (kBlock * 4) + (uint64_t)threadIdx.x * 4;
    uint32_t pol[4];
    bool uniform;
    policy_select<4>(p, gid0 + base, pol, uniform);
    const float* const s[4] = {s0, s1, s2, s3};
    // wave-uniform, see step_kernel; n_fast = n, or 0 when the caller's buffer is not aligned for the vector store
    const bool full = (uint64_t)blockIdx.x * (kBlock * 4) + (uint64_t)((threadIdx.x >> 6) + 1) * (64 * 4) <= n_fast;
    if (uniform)
        explore_actions_block<Env, true>(s, actions, n, base, full, gid0 + base, tick, p, x, pol);
    else
        explore_actions_block<Env, false>(s, actions, n, base, full, gid0 + base, tick, p, x, pol);
}

hipError_t launch_explore_actions(gymrs_env_kind kind, const float* const* s, void* actions, uint64_t n, uint64_t gid0, uint64_t tick,
                                  const PolicyArgs& p, const ExploreArgs& x, hipStream_t stream)
{
    if (n == 0) return hipSuccess;
    const uint64_t n_fast = (reinterpret_cast<uintptr_t>(actions) % 4 == 0) ? n : 0;
    uint8_t* out = static_cast<uint8_t*>(actions);
    return dispatch_policy_env(kind, [&](auto env) {
        using Env = typename decltype(env)::type;
        launch_begin();
        // (the kernel takes four rows whatever the env: a 2-row observation passes its own again)
        hipLaunchKernelGGL(explore_actions_kernel<Env>, dim3(step_grid(n, 4)), dim3(kBlock), 0, stream, s[0], s[1], s[2 % Env::kState],
                           s[3 % Env::kState], out, n, n_fast, gid0, tick, p, x);
        return hipGetLastError();
    });
}

hipError_t closed_loop_explore_cartpole(const ClosedLoopLaunch& l) { return closed_loop_unit<CartPoleT, ClosedLoopFamily::explore>(l); }
hipError_t closed_loop_explore_mountain_car(const ClosedLoopLaunch& l) { return closed_loop_unit<MountainCarT, ClosedLoopFamily::explore>(l); }

} // namespace gymrs
