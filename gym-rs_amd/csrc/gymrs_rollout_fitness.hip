// gymrs_rollout_fitness.hip -- gymrs_rollout_policy_fitness: rollout_policy_kernel (gymrs_rollout_policy.hip) that also counts,
// per policy, what every step of the launch paid and ended (include/gymrs_amd.h, "per-policy fitness").  The counters live in
// registers for the K steps of a launch (no memory traffic per step) and reach the table fitness[n_policies] once per launch
// through 64-bit INTEGER atomics: the sums are exact, whatever the order of the adds and however a batch is cut into engines.
#include "gymrs_policy.h"
#include "gymrs_rollout_impl.h"

namespace gymrs {

// One record's worth of accumulators.  32 bits each: a launch adds at most n_steps to a lane's counter and VEC * n_steps to a
// work-item's, and the host refuses n_steps > kMaxFitnessSteps (2^24; VEC <= 8).  Without GYMRS_TIME_LIMIT (TLIM) no step is
// truncated: `truncated` stays 0 and `episodes` is `done`, so two registers do (the gathered path holds a set per LANE).
template <bool TLIM>
struct FitnessAcc {
    int32_t reward = 0;
    uint32_t done = 0, trunc = 0, ended = 0;
    __device__ __forceinline__ void add(float rw, uint8_t dn, uint8_t tr)
    {
        reward += (int32_t)rw; // 0, 1 or -1: the conversion is exact
        done += dn;
        if constexpr (TLIM) {
            trunc += tr;
            ended += (dn | tr) != 0 ? 1u : 0u;
        }
    }
    __device__ __forceinline__ void add(const FitnessAcc& o)
    {
        reward += o.reward;
        done += o.done;
        if constexpr (TLIM) {
            trunc += o.trunc;
            ended += o.ended;
        }
    }
    __device__ __forceinline__ uint32_t episodes() const { return TLIM ? ended : done; }
};

__device__ __forceinline__ void fitness_commit(gymrs_policy_fitness* rec, long long reward, unsigned long long episodes, unsigned long long done,
                                               unsigned long long trunc)
{
    unsigned long long* w = reinterpret_cast<unsigned long long*>(rec); // {reward_sum (two's complement), episodes, done, truncated}
    atomic_add_nonzero(w + 0, (unsigned long long)reward);
    atomic_add_nonzero(w + 1, episodes);
    atomic_add_nonzero(w + 2, done);
    atomic_add_nonzero(w + 3, trunc);
}

// The Fit hook of rollout_block.  UNI (the wave's lanes all use one policy): one accumulator set per work-item, an integer wave
// reduction and one lane's atomics at the end.  Otherwise a work-item's lanes can belong to different policies: one set per lane;
// at the end consecutive lanes of one policy are merged inside the work-item and every run is added on its own.
template <int VEC, bool TLIM, bool UNI>
struct PolicyFitness;
template <int VEC, bool TLIM>
struct PolicyFitness<VEC, TLIM, true> {
    static constexpr bool kOn = true;
    gymrs_policy_fitness* rec;
    FitnessAcc<TLIM> acc;
    __device__ __forceinline__ PolicyFitness(gymrs_policy_fitness* table, const uint32_t (&pol)[VEC])
        : rec(table + __builtin_amdgcn_readfirstlane(pol[0]))
    {
    }
    template <bool FULL>
    __device__ __forceinline__ void step(const StepOut<VEC>& out, uint64_t base, uint64_t n)
    {
#pragma unroll
        for (int k = 0; k < VEC; ++k)
            if (FULL || base + k < n) acc.add(out.reward.v[k], out.done.v[k], out.trunc.v[k]);
    }
    __device__ __forceinline__ void flush()
    {
        const long long reward = wave_sum_i64(acc.reward);
        const long long done = wave_sum_i64((int32_t)acc.done), trunc = TLIM ? wave_sum_i64((int32_t)acc.trunc) : 0,
                        episodes = TLIM ? wave_sum_i64((int32_t)acc.ended) : done;
        if ((threadIdx.x & 63u) == 0)
            fitness_commit(rec, reward, (unsigned long long)episodes, (unsigned long long)done, (unsigned long long)trunc);
    }
};
template <int VEC, bool TLIM>
struct PolicyFitness<VEC, TLIM, false> {
    static constexpr bool kOn = true;
    gymrs_policy_fitness* table;
    uint32_t pol[VEC];
    FitnessAcc<TLIM> acc[VEC];
    __device__ __forceinline__ PolicyFitness(gymrs_policy_fitness* table_, const uint32_t (&pol_)[VEC]) : table(table_)
    {
#pragma unroll
        for (int k = 0; k < VEC; ++k) pol[k] = pol_[k];
    }
    template <bool FULL>
    __device__ __forceinline__ void step(const StepOut<VEC>& out, uint64_t base, uint64_t n)
    {
#pragma unroll
        for (int k = 0; k < VEC; ++k)
            if (FULL || base + k < n) acc[k].add(out.reward.v[k], out.done.v[k], out.trunc.v[k]);
    }
    __device__ __forceinline__ void flush()
    {
        FitnessAcc<TLIM> run;
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            run.add(acc[k]);
            if (k + 1 == VEC || pol[k + 1] != pol[k]) { // a lane at or beyond n counted nothing: it adds nothing
                fitness_commit(table + pol[k], (long long)run.reward, run.episodes(), run.done, run.trunc);
                run = FitnessAcc<TLIM>();
            }
        }
    }
};

// rollout_policy_kernel's body (gymrs_rollout_policy.hip, where a note says why the two are not one function) with the hook
// above.  No recording variant.
template <class Env, int VEC, uint32_t FLAGS>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(16 / VEC, 16 / VEC))) void rollout_policy_fitness_kernel(
    const StepArgs a, const RolloutArgs r, const typename Env::Consts c, const PolicyArgs p, gymrs_policy_fitness* const fitness)
{
    constexpr int LPB = kBlock * VEC;
    constexpr bool TLIM = (FLAGS & GYMRS_TIME_LIMIT) != 0;
    __shared__ ResetLds<Env, VEC, kBlock> lds;
    const uint64_t base = (uint64_t)blockIdx.x * LPB + (uint64_t)threadIdx.x * VEC;
    uint32_t pol[VEC];
    bool uniform;
    policy_select<VEC>(p, a.gid0 + base, pol, uniform);
    const bool full = (uint64_t)blockIdx.x * LPB + (uint64_t)((threadIdx.x >> 6) + 1) * (64 * VEC) <= a.n; // wave-uniform, see step_kernel
    if (uniform) {
        const PolicyActions<Env, VEC, true> src(p, pol);
        PolicyFitness<VEC, TLIM, true> fit(fitness, pol);
        if (full)
            rollout_block<Env, VEC, FLAGS, true, false>(a, r, c, lds, src, &fit);
        else
            rollout_block<Env, VEC, FLAGS, false, false>(a, r, c, lds, src, &fit);
    } else {
        const PolicyActions<Env, VEC, false> src(p, pol);
        PolicyFitness<VEC, TLIM, false> fit(fitness, pol);
        if (full)
            rollout_block<Env, VEC, FLAGS, true, false>(a, r, c, lds, src, &fit);
        else
            rollout_block<Env, VEC, FLAGS, false, false>(a, r, c, lds, src, &fit);
    }
}

hipError_t launch_rollout_policy_fitness(gymrs_env_kind kind, int vec, uint32_t flags, const StepArgs& a, const RolloutArgs& r, const void* consts,
                                         const PolicyArgs& p, gymrs_policy_fitness* fitness, hipStream_t stream)
{
    if (a.n == 0 || r.n_steps == 0) return hipSuccess;
    if ((flags & kFlagTable) || r.rec_obs || !fitness || r.n_steps > kMaxFitnessSteps) return hipErrorInvalidValue;
    return dispatch_policy_env(kind, [&](auto env) {
        using Env = typename decltype(env)::type;
        return dispatch_table(vec, flags, hipErrorInvalidValue, [&](auto lanes, auto flag_set) {
            constexpr int VEC = decltype(lanes)::value;
            launch_begin();
            hipLaunchKernelGGL((rollout_policy_fitness_kernel<Env, VEC, decltype(flag_set)::value>), dim3(step_grid(a.n, VEC)), dim3(kBlock), 0, stream,
                               a, r, *static_cast<const typename Env::Consts*>(consts), p, fitness);
            return hipGetLastError();
        });
    });
}

} // namespace gymrs
