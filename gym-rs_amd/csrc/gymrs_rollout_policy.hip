// gymrs_rollout_policy.hip -- the closed-loop kernels (gymrs_policy.h): policy_actions_kernel (the per-step counterpart:
// observations -> actions) and rollout_policy_kernel, the fused multi-step kernel of gymrs_rollout_impl.h with the policy as
// its action source.  CartPole and MountainCar (the Discrete envs), uniform constants only (no parameter table).
#include "gymrs_policy.h"
#include "gymrs_rollout_impl.h"

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
    store_vec<uint8_t, 4, 0>(actions, base, n, full, act);
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
    launch_begin();
    const uint64_t n_fast = (reinterpret_cast<uintptr_t>(actions) % 4 == 0) ? n : 0;
    uint8_t* out = static_cast<uint8_t*>(actions);
    switch (kind) {
    case GYMRS_CARTPOLE:
        hipLaunchKernelGGL(policy_actions_kernel<CartPoleT>, dim3(step_grid(n, 4)), dim3(kBlock), 0, stream, s[0], s[1], s[2], s[3], out, n, n_fast,
                           gid0, p);
        break;
    case GYMRS_MOUNTAIN_CAR:
        hipLaunchKernelGGL(policy_actions_kernel<MountainCarT>, dim3(step_grid(n, 4)), dim3(kBlock), 0, stream, s[0], s[1], s[0], s[1], out, n,
                           n_fast, gid0, p);
        break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// gymrs_rollout_policy / _record: rollout_block with the policy as its action source.  FULL / ragged and uniform / gathered
// weights are both chosen per wave, wave-uniformly.  The register budget is rollout_kernel's (16 / VEC waves per SIMD).
template <class Env, int VEC, uint32_t FLAGS, bool REC>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(16 / VEC, 16 / VEC))) void rollout_policy_kernel(
    const StepArgs a, const RolloutArgs r, const typename Env::Consts c, const PolicyArgs p)
{
    constexpr int LPB = kBlock * VEC;
    __shared__ ResetLds<Env, VEC, kBlock> lds;
    const uint64_t base = (uint64_t)blockIdx.x * LPB + (uint64_t)threadIdx.x * VEC;
    uint32_t pol[VEC];
    bool uniform;
    policy_select<VEC>(p, a.gid0 + base, pol, uniform);
    const bool full = (uint64_t)blockIdx.x * LPB + (uint64_t)((threadIdx.x >> 6) + 1) * (64 * VEC) <= a.n; // wave-uniform, see step_kernel
    if (uniform) {
        const PolicyActions<Env, VEC, true> src(p, pol);
        if (full)
            rollout_block<Env, VEC, FLAGS, true, REC>(a, r, c, lds, src);
        else
            rollout_block<Env, VEC, FLAGS, false, REC>(a, r, c, lds, src);
    } else {
        const PolicyActions<Env, VEC, false> src(p, pol);
        if (full)
            rollout_block<Env, VEC, FLAGS, true, REC>(a, r, c, lds, src);
        else
            rollout_block<Env, VEC, FLAGS, false, REC>(a, r, c, lds, src);
    }
}

template <class Env, int VEC, uint32_t FLAGS>
static hipError_t rollout_policy_one(const StepArgs& a, const RolloutArgs& r, const void* consts, const PolicyArgs& p, hipStream_t stream)
{
    launch_begin();
    if constexpr (VEC == 4) { // the recording variant exists at 4 lanes per work-item only
        if (r.rec_obs) {
            hipLaunchKernelGGL((rollout_policy_kernel<Env, VEC, FLAGS, true>), dim3(step_grid(a.n, VEC)), dim3(kBlock), 0, stream, a, r,
                               *static_cast<const typename Env::Consts*>(consts), p);
            return hipGetLastError();
        }
    }
    if (r.rec_obs) return hipErrorInvalidValue;
    hipLaunchKernelGGL((rollout_policy_kernel<Env, VEC, FLAGS, false>), dim3(step_grid(a.n, VEC)), dim3(kBlock), 0, stream, a, r,
                       *static_cast<const typename Env::Consts*>(consts), p);
    return hipGetLastError();
}

template <class Env, int VEC>
static hipError_t rollout_policy_flags(uint32_t flags, const StepArgs& a, const RolloutArgs& r, const void* consts, const PolicyArgs& p,
                                       hipStream_t stream)
{
    constexpr uint32_t A = GYMRS_AUTO_RESET, S = GYMRS_TRACK_STATS, T = GYMRS_TIME_LIMIT, F = GYMRS_FINAL_OBS;
    if (!(flags & A)) flags &= ~(S | F);
    switch (flags & (A | S | T | F)) {
    case 0: return rollout_policy_one<Env, VEC, 0>(a, r, consts, p, stream);
    case A: return rollout_policy_one<Env, VEC, A>(a, r, consts, p, stream);
    case A | S: return rollout_policy_one<Env, VEC, A | S>(a, r, consts, p, stream);
    case T: return rollout_policy_one<Env, VEC, T>(a, r, consts, p, stream);
    case A | T: return rollout_policy_one<Env, VEC, A | T>(a, r, consts, p, stream);
    case A | S | T: return rollout_policy_one<Env, VEC, A | S | T>(a, r, consts, p, stream);
    case A | F: return rollout_policy_one<Env, VEC, A | F>(a, r, consts, p, stream);
    case A | S | F: return rollout_policy_one<Env, VEC, A | S | F>(a, r, consts, p, stream);
    case A | T | F: return rollout_policy_one<Env, VEC, A | T | F>(a, r, consts, p, stream);
    case A | S | T | F: return rollout_policy_one<Env, VEC, A | S | T | F>(a, r, consts, p, stream);
    default: return hipErrorInvalidValue;
    }
}

template <class Env>
static hipError_t rollout_policy_vec(int vec, uint32_t flags, const StepArgs& a, const RolloutArgs& r, const void* consts, const PolicyArgs& p,
                                     hipStream_t stream)
{
    switch (vec) {
    case 4: return rollout_policy_flags<Env, 4>(flags, a, r, consts, p, stream);
    case 8: return rollout_policy_flags<Env, 8>(flags, a, r, consts, p, stream);
    default: return hipErrorInvalidValue;
    }
}

hipError_t launch_rollout_policy(gymrs_env_kind kind, int vec, uint32_t flags, const StepArgs& a, const RolloutArgs& r, const void* consts,
                                 const PolicyArgs& p, hipStream_t stream)
{
    if (a.n == 0 || r.n_steps == 0) return hipSuccess;
    if (flags & kFlagTable) return hipErrorInvalidValue; // no policy x table kernels (the engine refuses first)
    switch (kind) {
    case GYMRS_CARTPOLE: return rollout_policy_vec<CartPoleT>(vec, flags, a, r, consts, p, stream);
    case GYMRS_MOUNTAIN_CAR: return rollout_policy_vec<MountainCarT>(vec, flags, a, r, consts, p, stream);
    default: return hipErrorInvalidValue;
    }
}

} // namespace gymrs
