// gymrs_rollout_policy_impl.h -- the closed-loop fused kernels, gfx950: rollout_policy_kernel (rollout_block of
// gymrs_rollout_impl.h with the policy of gymrs_policy.h as its action source), rollout_policy_fitness_kernel (the same with the
// per-policy counters of include/gymrs_amd.h, "per-policy fitness"), the one entry text of all eight closed-loop kernels
// (GYMRS_CLOSED_LOOP_ENTRY) and the one launch of a translation unit (closed_loop_unit).  Included by gymrs_rollout_policy.hip and
// gymrs_rollout_fitness.hip (the uniform envs) and by gymrs_table_policy_<env>.hip (TableT: per-lane parameter tables,
// gymrs_rollout_closed_loop).
#pragma once
#include "gymrs_policy.h"
#include "gymrs_rollout_impl.h"

namespace gymrs {

// Waves per SIMD the register allocator aims for (FIT: the fitness kernel).  The uniform envs: rollout_kernel's 16 / VEC.  A TableT
// env holds per-lane rows and indices (gymrs_rollout_impl.h) on top of the policy's accumulators and the fitness counters: per
// family, the highest budget at which none of its ten flag sets spills a vector register to scratch, read from the code-object
// metadata (profiles/policy_rollout_table.md lists every budget tried and what it spilled).
template <class Env, int VEC, bool FIT>
struct PolicyWaves {
    static constexpr int value = 16 / VEC;
};
template <int VEC, bool FIT>
struct PolicyWaves<TableT<CartPoleT>, VEC, FIT> {
    static constexpr int value = 8 / VEC; // 2 / 1: at 3 waves (VEC = 4) up to 116 B of scratch, at 16 / VEC up to 460 B
};
template <int VEC, bool FIT>
struct PolicyWaves<TableT<MountainCarT>, VEC, FIT> {
    static constexpr int value = VEC == 4 ? 3 : (FIT ? 1 : 2); // one step above: up to 164 B (VEC = 4), 140 B (VEC = 8 with counters)
};

// The body of every closed-loop kernel (the eight rollout_*_kernel of this header and of gymrs_rollout_explore_impl.h,
// gymrs_rollout_transitions_impl.h and gymrs_rollout_sample_impl.h; the last one #undef's it): rollout_block under an action source
// built from the policy set.  FULL / ragged and uniform / gathered weights are both chosen per wave, wave-uniformly.
//
// A macro and not a function, because the kernels must keep their machine code.  Tried on gymrs_table_explore_mountain_car.hip (50
// kernels), disassembly compared line by line with the separate bodies': as a __device__ __forceinline__ function template taking
// the kernel arguments by const&, 7.3e5 differing lines (other SGPR allocation from the first kernel on, other code length: the
// kernel-argument pointer loads of the state rows leave the two weight branches for the kernel's entry, and every instantiation
// comes out with other register spills); taking them by value, 8.0e5; as text expanded inside each __global__ function, none.
//
// Expects in scope: the kernel parameters a (StepArgs), r (RolloutArgs), c (Env::Consts), p (PolicyArgs) and whatever SOURCE_ARGS,
// HOOK and BLOCK_ARGS name; Env, VEC and FLAGS (template parameters or constants of the kernel).
// Declares: LPB, lds, base, pol, uniform, full; then per weight branch UNI, `src` -- a SOURCE<Env, VEC, UNI> built from SOURCE_ARGS
// (parenthesised) -- and what HOOK says (GYMRS_FITNESS_HOOK, below: a Fit hook `fit` that depends on UNI; or nothing), and calls
// rollout_block<Env, VEC, FLAGS, FULL, REC> with BLOCK_ARGS (parenthesised).  A Sink (the transitions kernels') does not depend on
// the branch: the kernel declares it before the expansion.
#define GYMRS_CLOSED_LOOP_ENTRY(SOURCE, SOURCE_ARGS, REC, HOOK, BLOCK_ARGS)                                                                        \
    constexpr int LPB = kBlock * VEC;                                                                                                               \
    __shared__ ResetLds<Env, VEC, kBlock> lds;                                                                                                      \
    const uint64_t base = (uint64_t)blockIdx.x * LPB + (uint64_t)threadIdx.x * VEC;                                                                 \
    uint32_t pol[VEC];                                                                                                                              \
    bool uniform;                                                                                                                                   \
    policy_select<VEC>(p, a.gid0 + base, pol, uniform);                                                                                             \
    const bool full = (uint64_t)blockIdx.x * LPB + (uint64_t)((threadIdx.x >> 6) + 1) * (64 * VEC) <= a.n; /* wave-uniform, see step_kernel */     \
    if (uniform) {                                                                                                                                  \
        constexpr bool UNI = true;                                                                                                                  \
        const SOURCE<Env, VEC, UNI> src SOURCE_ARGS;                                                                                                \
        HOOK                                                                                                                                        \
        if (full)                                                                                                                                   \
            rollout_block<Env, VEC, FLAGS, true, REC> BLOCK_ARGS;                                                                                   \
        else                                                                                                                                        \
            rollout_block<Env, VEC, FLAGS, false, REC> BLOCK_ARGS;                                                                                  \
    } else {                                                                                                                                        \
        constexpr bool UNI = false;                                                                                                                 \
        const SOURCE<Env, VEC, UNI> src SOURCE_ARGS;                                                                                                \
        HOOK                                                                                                                                        \
        if (full)                                                                                                                                   \
            rollout_block<Env, VEC, FLAGS, true, REC> BLOCK_ARGS;                                                                                   \
        else                                                                                                                                        \
            rollout_block<Env, VEC, FLAGS, false, REC> BLOCK_ARGS;                                                                                  \
    }

// gymrs_rollout_policy / _record: the policy's greedy action.  The register budget: PolicyWaves above.
template <class Env, int VEC, uint32_t FLAGS, bool REC>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(PolicyWaves<Env, VEC, false>::value, PolicyWaves<Env, VEC, false>::value))) void rollout_policy_kernel(
    const StepArgs a, const RolloutArgs r, const typename Env::Consts c, const PolicyArgs p)
{
    GYMRS_CLOSED_LOOP_ENTRY(PolicyActions, (p, pol), REC, /* no hook */, (a, r, c, lds, src))
}

// ---- per-policy fitness: the counters live in registers for the K steps of a launch (no memory traffic per step) and reach the
// table fitness[n_policies] once per launch through 64-bit INTEGER atomics: the sums are exact, whatever the order of the adds.

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

// The same with the hook above: the counters follow the action taken.  No recording variant.
#define GYMRS_FITNESS_HOOK PolicyFitness<VEC, (FLAGS & GYMRS_TIME_LIMIT) != 0, UNI> fit(fitness, pol);
template <class Env, int VEC, uint32_t FLAGS>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(PolicyWaves<Env, VEC, true>::value, PolicyWaves<Env, VEC, true>::value))) void rollout_policy_fitness_kernel(
    const StepArgs a, const RolloutArgs r, const typename Env::Consts c, const PolicyArgs p, gymrs_policy_fitness* const fitness)
{
    GYMRS_CLOSED_LOOP_ENTRY(PolicyActions, (p, pol), false, GYMRS_FITNESS_HOOK, (a, r, c, lds, src, &fit))
}

// ---- the launches (host side).  One closed-loop launch of kernel `kernel` (any of the eight: they share their first four
// parameters; `extra`: the rest) at VEC lanes per work-item.
template <class Env, int VEC, class Kernel, class... Extra>
static hipError_t closed_loop_submit(Kernel kernel, const ClosedLoopLaunch& l, const Extra&... extra)
{
    launch_begin();
    hipLaunchKernelGGL(kernel, dim3(step_grid(l.a.n, VEC)), dim3(kBlock), 0, l.stream, l.a, l.r, *static_cast<const typename Env::Consts*>(l.consts),
                       l.p, extra...);
    return hipGetLastError();
}

// The kernel of a family tag (gymrs_launch.h) and its launch: one overload per family, next to its kernel.
template <class Env, int VEC, uint32_t FLAGS, bool REC>
static hipError_t closed_loop_kernel(Family<ClosedLoopFamily::policy>, const ClosedLoopLaunch& l)
{
    return closed_loop_submit<Env, VEC>(rollout_policy_kernel<Env, VEC, FLAGS, REC>, l);
}
template <class Env, int VEC, uint32_t FLAGS, bool REC>
static hipError_t closed_loop_kernel(Family<ClosedLoopFamily::policy_fitness>, const ClosedLoopLaunch& l)
{
    return closed_loop_submit<Env, VEC>(rollout_policy_fitness_kernel<Env, VEC, FLAGS>, l, l.fitness);
}

// What a translation unit exports, once per env type it is built for (the one signature launch_closed_loop's table holds,
// gymrs_rollout_policy.hip): the launch of `l` in the instantiation dispatch_closed_loop (gymrs_launch.h) picks for it.  BUILT: the
// families this unit instantiates; a request for another one is the table's mistake and launches nothing.
template <class Env, ClosedLoopFamily... BUILT>
static hipError_t closed_loop_unit(const ClosedLoopLaunch& l)
{
    return dispatch_closed_loop(l.source, l.fitness != nullptr, l.r.rec_obs != nullptr, l.transitions != nullptr, l.vec, l.flags, hipErrorInvalidValue,
                                [&](auto family, auto lanes, auto flag_set, auto rec) {
                                    if constexpr (((decltype(family)::value == BUILT) || ...))
                                        return closed_loop_kernel<Env, decltype(lanes)::value, decltype(flag_set)::value, decltype(rec)::value>(family, l);
                                    else
                                        return hipErrorInvalidValue;
                                });
}

} // namespace gymrs
