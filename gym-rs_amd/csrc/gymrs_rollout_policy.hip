// gymrs_rollout_policy.hip -- the closed-loop kernels (gymrs_policy.h) and their launches: policy_actions_kernel (the per-step
// counterpart: observations -> actions) and rollout_policy_kernel (gymrs_rollout_policy_impl.h), the fused multi-step kernel with
// the policy as its action source, for CartPole and MountainCar (the Discrete envs) with uniform constants.  The parameter-table
// instantiations (kFlagTable) live in one translation unit per env type, gymrs_table_policy_<env>.hip.  Also launch_closed_loop: the
// one entry the engine calls for every closed-loop rollout, whichever translation unit holds its kernel.
#include "gymrs_rollout_policy_impl.h"

namespace gymrs {

// gymrs_policy_actions: one launch, 4 lanes per work-item: loads the observation tile, evaluates, one 4-byte store of actions.
template <class Env, bool UNI>
__device__ __forceinline__ void policy_actions_block(const float* const (&s)[4], uint8_t* __restrict__ actions, uint64_t n, uint64_t base,
                                                     bool full, const PolicyArgs& p, const uint32_t (&pol)[4])
{
    Vec<float, 4> x[Env::kState];
#pragma unroll
    for (int j = 0; j < Env::kState; ++j) x[j] = load_vec<float, 4, false>(s[j], base, n, full, 0.0f);
    const PolicyWeights<4, UNI> w(p, pol);
    Vec<uint8_t, 4> act;
    policy_eval<Env, 4, UNI>(w, p.hidden, x, act);
    store_vec<uint8_t, 4, false>(actions, base, n, full, act);
}

template <class Env>
__global__ __launch_bounds__(kBlock) void policy_actions_kernel(const float* s0, const float* s1, const float* s2, const float* s3,
                                                                uint8_t* actions, uint64_t n, uint64_t n_fast, uint64_t gid0, const PolicyArgs p)
{
    const uint64_t base = (uint64_t)blockIdx.x * (kBlock * 4) + (uint64_t)threadIdx.x * 4;
    uint32_t pol[4];
    bool uniform;
    policy_select<4>(p, gid0 + base, pol, uniform);
    const float* const s[4] = {s0, s1, s2, s3};
    // wave-uniform, see step_kernel; n_fast = n, or 0 when the caller's buffer is not aligned for the vector store
    const bool full = (uint64_t)blockIdx.x * (kBlock * 4) + (uint64_t)((threadIdx.x >> 6) + 1) * (64 * 4) <= n_fast;
    if (uniform)
        policy_actions_block<Env, true>(s, actions, n, base, full, p, pol);
    else
        policy_actions_block<Env, false>(s, actions, n, base, full, p, pol);
}

hipError_t launch_policy_actions(gymrs_env_kind kind, const float* const* s, void* actions, uint64_t n, uint64_t gid0, const PolicyArgs& p,
                                 hipStream_t stream)
{
    if (n == 0) return hipSuccess;
    const uint64_t n_fast = (reinterpret_cast<uintptr_t>(actions) % 4 == 0) ? n : 0;
    uint8_t* out = static_cast<uint8_t*>(actions);
    return dispatch_policy_env(kind, [&](auto env) {
        using Env = typename decltype(env)::type;
        launch_begin();
        // (the kernel takes four rows whatever the env: a 2-row observation passes its own again)
        hipLaunchKernelGGL(policy_actions_kernel<Env>, dim3(step_grid(n, 4)), dim3(kBlock), 0, stream, s[0], s[1], s[2 % Env::kState],
                           s[3 % Env::kState], out, n, n_fast, gid0, p);
        return hipGetLastError();
    });
}

// ---- launch_closed_loop: the one way from a closed-loop request to its kernel.  The kernels are spread over translation units so
// that the build compiles them in parallel; every unit exports closed_loop_unit (gymrs_rollout_policy_impl.h) once per env type
// under the name of its file.
using ClosedLoopUnit = hipError_t(const ClosedLoopLaunch&);
ClosedLoopUnit closed_loop_rollout_policy_cartpole, closed_loop_rollout_policy_mountain_car, closed_loop_rollout_fitness_cartpole,
    closed_loop_rollout_fitness_mountain_car, closed_loop_explore_cartpole, closed_loop_explore_mountain_car, closed_loop_explore_fitness_cartpole,
    closed_loop_explore_fitness_mountain_car, closed_loop_sample_cartpole, closed_loop_sample_mountain_car, closed_loop_sample_fitness_cartpole,
    closed_loop_sample_fitness_mountain_car, closed_loop_transitions_cartpole, closed_loop_transitions_mountain_car,
    closed_loop_table_policy_cartpole, closed_loop_table_policy_mountain_car, closed_loop_table_explore_cartpole,
    closed_loop_table_explore_mountain_car, closed_loop_table_sample_cartpole, closed_loop_table_sample_mountain_car,
    closed_loop_table_transitions_cartpole, closed_loop_table_transitions_mountain_car;

hipError_t closed_loop_rollout_policy_cartpole(const ClosedLoopLaunch& l) { return closed_loop_unit<CartPoleT, ClosedLoopFamily::policy>(l); }
hipError_t closed_loop_rollout_policy_mountain_car(const ClosedLoopLaunch& l) { return closed_loop_unit<MountainCarT, ClosedLoopFamily::policy>(l); }

// The unit that holds a family: [family][kFlagTable set][CartPole, MountainCar].  A table unit holds a source's plain and fitness
// families (and the sampling one its transitions family) where the uniform envs have a unit each.
static ClosedLoopUnit* const kClosedLoopUnits[kClosedLoopFamilies][2][2] = {
    /* policy             */ {{closed_loop_rollout_policy_cartpole, closed_loop_rollout_policy_mountain_car},
                              {closed_loop_table_policy_cartpole, closed_loop_table_policy_mountain_car}},
    /* policy_fitness     */ {{closed_loop_rollout_fitness_cartpole, closed_loop_rollout_fitness_mountain_car},
                              {closed_loop_table_policy_cartpole, closed_loop_table_policy_mountain_car}},
    /* explore            */ {{closed_loop_explore_cartpole, closed_loop_explore_mountain_car},
                              {closed_loop_table_explore_cartpole, closed_loop_table_explore_mountain_car}},
    /* explore_fitness    */ {{closed_loop_explore_fitness_cartpole, closed_loop_explore_fitness_mountain_car},
                              {closed_loop_table_explore_cartpole, closed_loop_table_explore_mountain_car}},
    /* sample             */ {{closed_loop_sample_cartpole, closed_loop_sample_mountain_car},
                              {closed_loop_table_sample_cartpole, closed_loop_table_sample_mountain_car}},
    /* sample_fitness     */ {{closed_loop_sample_fitness_cartpole, closed_loop_sample_fitness_mountain_car},
                              {closed_loop_table_sample_cartpole, closed_loop_table_sample_mountain_car}},
    /* transitions        */ {{closed_loop_transitions_cartpole, closed_loop_transitions_mountain_car},
                              {closed_loop_table_transitions_cartpole, closed_loop_table_transitions_mountain_car}},
    /* sample_transitions */ {{closed_loop_sample_cartpole, closed_loop_sample_mountain_car},
                              {closed_loop_table_sample_cartpole, closed_loop_table_sample_mountain_car}},
};

hipError_t launch_closed_loop(gymrs_env_kind kind, const ClosedLoopLaunch& l)
{
    if (l.a.n == 0 || l.r.n_steps == 0) return hipSuccess;
    if (kind != GYMRS_CARTPOLE && kind != GYMRS_MOUNTAIN_CAR) return hipErrorInvalidValue;
    if (l.fitness && l.r.n_steps > kMaxFitnessSteps) return hipErrorInvalidValue;
    // transitions: every store is addressed inside a row of rec_stride lanes (the caller's check_trajectory is what makes that safe)
    if (l.transitions && (!l.transitions->final_obs || l.r.rec_stride < l.a.n)) return hipErrorInvalidValue;
    const int table = (l.flags & kFlagTable) ? 1 : 0, env = kind == GYMRS_CARTPOLE ? 0 : 1;
    ClosedLoopUnit* const unit = dispatch_closed_loop(l.source, l.fitness != nullptr, l.r.rec_obs != nullptr, l.transitions != nullptr, l.vec, l.flags,
                                                      static_cast<ClosedLoopUnit*>(nullptr),
                                                      [&](auto family, auto, auto, auto) { return kClosedLoopUnits[(int)decltype(family)::value][table][env]; });
    return unit ? unit(l) : hipErrorInvalidValue;
}

} // namespace gymrs
