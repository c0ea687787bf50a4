// gymrs_sample.hip -- softmax action sampling (include/gymrs_amd.h, "sampling"): sample_actions_kernel (the per-step counterpart:
// the sampled action and its probability at the engine's tick) and the launches of rollout_sample_kernel and
// rollout_sample_transitions_kernel (gymrs_rollout_sample_impl.h) for CartPole and MountainCar with uniform constants.  The fitness
// variant lives in gymrs_sample_fitness.hip, the parameter-table instantiations (kFlagTable) in gymrs_table_sample_<env>.hip.
#include "gymrs_rollout_sample_impl.h"

namespace gymrs {

// gymrs_sample_actions: explore_actions_kernel (gymrs_explore.hip) with the sampling source's fill.
template <class Env, bool UNI, bool PROB>
__device__ __forceinline__ void sample_actions_block(const float* const (&s)[4], uint8_t* __restrict__ actions, float* __restrict__ prob, uint64_t n,
                                                     uint64_t base, bool full, uint64_t gid, uint64_t tick, const PolicyArgs& p, const SampleArgs& x,
                                                     const uint32_t (&pol)[4])
{
    Vec<float, 4> obs[Env::kState];
#pragma unroll
    for (int j = 0; j < Env::kState; ++j) obs[j] = load_vec<float, 4, false>(s[j], base, n, full, 0.0f);
    const SamplingActions<Env, 4, UNI> src(p, pol, x);
    Vec<uint8_t, 4> act;
    Vec<float, 4> pr;
    src.fill(obs, act, gid, tick, (gid & 3u) == 0, PROB ? &pr : nullptr); // (base is a multiple of 4: the offset decides, wave-uniformly)
    store_vec<uint8_t, 4, false>(actions, base, n, full, act);
    if constexpr (PROB) store_vec<float, 4, false>(prob, base, n, full, pr);
}

template <class Env, bool PROB>
__global__ __launch_bounds__(kBlock) void sample_actions_kernel(const float* s0, const float* s1, const float* s2, const float* s3, uint8_t* actions,
                                                                float* prob, uint64_t n, uint64_t n_fast, uint64_t gid0, uint64_t tick,
                                                                const PolicyArgs p, const SampleArgs x)
{
    const uint64_t base = (uint64_t)blockIdx.x * (kBlock * 4) + (uint64_t)threadIdx.x * 4;
    uint32_t pol[4];
    bool uniform;
    policy_select<4>(p, gid0 + base, pol, uniform);
    const float* const s[4] = {s0, s1, s2, s3};
    // wave-uniform, see step_kernel; n_fast = n, or 0 when a buffer of the caller is not aligned for its vector store
    const bool full = (uint64_t)blockIdx.x * (kBlock * 4) + (uint64_t)((threadIdx.x >> 6) + 1) * (64 * 4) <= n_fast;
    if (uniform)
        sample_actions_block<Env, true, PROB>(s, actions, prob, n, base, full, gid0 + base, tick, p, x, pol);
    else
        sample_actions_block<Env, false, PROB>(s, actions, prob, n, base, full, gid0 + base, tick, p, x, pol);
}

hipError_t launch_sample_actions(gymrs_env_kind kind, const float* const* s, void* actions, float* prob, uint64_t n, uint64_t gid0, uint64_t tick,
                                 const PolicyArgs& p, const SampleArgs& x, hipStream_t stream)
{
    if (n == 0) return hipSuccess;
    const uint64_t n_fast = (reinterpret_cast<uintptr_t>(actions) % 4 == 0 && reinterpret_cast<uintptr_t>(prob) % 16 == 0) ? n : 0;
    uint8_t* out = static_cast<uint8_t*>(actions);
    return dispatch_policy_env(kind, [&](auto env) {
        using Env = typename decltype(env)::type;
        launch_begin();
        // (the kernel takes four rows whatever the env: a 2-row observation passes its own again)
        if (prob)
            hipLaunchKernelGGL((sample_actions_kernel<Env, true>), dim3(step_grid(n, 4)), dim3(kBlock), 0, stream, s[0], s[1], s[2 % Env::kState],
                               s[3 % Env::kState], out, prob, n, n_fast, gid0, tick, p, x);
        else
            hipLaunchKernelGGL((sample_actions_kernel<Env, false>), dim3(step_grid(n, 4)), dim3(kBlock), 0, stream, s[0], s[1], s[2 % Env::kState],
                               s[3 % Env::kState], out, prob, n, n_fast, gid0, tick, p, x);
        return hipGetLastError();
    });
}

hipError_t closed_loop_sample_cartpole(const ClosedLoopLaunch& l)
{
    return closed_loop_unit<CartPoleT, ClosedLoopFamily::sample, ClosedLoopFamily::sample_transitions>(l);
}
hipError_t closed_loop_sample_mountain_car(const ClosedLoopLaunch& l)
{
    return closed_loop_unit<MountainCarT, ClosedLoopFamily::sample, ClosedLoopFamily::sample_transitions>(l);
}

} // namespace gymrs
