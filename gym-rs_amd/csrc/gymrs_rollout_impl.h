// gymrs_rollout_impl.h -- the fused multi-step kernel, gfx950: rollout_block (also the body of the closed-loop kernels of
// gymrs_rollout_policy_impl.h) and the random-policy rollout_kernel with its launch: included by
// gymrs_rollout.hip (the uniform envs) and by gymrs_table_<env>.hip (TableT, per-lane parameter tables).
#pragma once
#include "gymrs_launch.h"
#include "gymrs_tile.h"

namespace gymrs {

// ---------------------------------------------------------------------------------------------
// Fused multi-step kernel: the caller loop of examples/cartpole.rs:15-30 -- draw a random
// action, step, reset on done, accumulate the return -- for every lane, n_steps iterations in ONE launch.
// State stays in registers between steps: HBM is touched once per launch, so this path is VALU-bound
// (physics + one Philox block per lane per 4 steps for the actions + the compacted reset pass), not
// HBM-bound.  Bit-identical to n_steps calls of gymrs_fill_actions + gymrs_step: it calls the same
// advance_tile, step after step, and leaves the arrays as the last of those steps would.
// REC (gymrs_rollout_record): additionally every step's observation, action, reward and flags are written to
// trajectory buffers -- what a random-policy data collection loop keeps.  Then HBM sees 22 B per CartPole
// lane-step (no state re-read, no launch per step) instead of 38 B + a launch + an action-generation kernel.
// Src = where a step's actions come from: RandomActions (the Philox draws of gymrs_fill_actions, below), or a source with
// kPolicy that computes d.act from d.st (PolicyActions, gymrs_policy.h: gymrs_rollout_policy).  A source with kExplore
// (ExploringActions, same header) is also told which step this is -- the work-item's first global id, the engine tick the step
// starts from and whether four of its lanes share a Philox block: the epsilon-greedy draw is keyed by them.
struct RandomActions {
    static constexpr bool kPolicy = false, kExplore = false;
};
// Fit = what is folded out of every step's reward / done / truncated while they are still in registers: nothing (NoFitness: every
// line that names it compiles away), or the per-policy counters of gymrs_rollout_policy_fitness (gymrs_rollout_policy_impl.h).
struct NoFitness {
    static constexpr bool kOn = false;
};
// Sink = where the pre-reset observation of the lanes a step re-arms goes, step by step (advance_tile): nowhere (NoFinalSink), or the
// rows of gymrs_rollout_transitions (FinalObsRows, gymrs_rollout_transitions_impl.h), which also takes the observations the launch
// starts from.
template <class Env, int VEC, uint32_t FLAGS, bool FULL, bool REC, class Src = RandomActions, class Fit = NoFitness, class Sink = NoFinalSink>
__device__ __forceinline__ void rollout_block(StepArgs a, const RolloutArgs& r, const typename Env::Consts& c,
                                              ResetLds<Env, VEC, kBlock>& lds, const Src& src = Src(), Fit* fit = nullptr, Sink* sink = nullptr)
{
    constexpr int kVec = VEC;
    using R = TileRegs<Env, VEC, FLAGS>;
    using Action = typename Env::Action;
    const uint64_t base = (uint64_t)blockIdx.x * (kBlock * kVec) + (uint64_t)threadIdx.x * kVec;
    R d;
    load_tile<Env, VEC, FLAGS, FULL, true>(a, base, d);
    load_param_index<Env, VEC, FLAGS, FULL>(a, c, base, d); // (TableT: the index stays in registers for the whole rollout)
    if constexpr (Sink::kOn) sink->template start<FULL>(d.st, base, a.n);
    unsigned long long resets = 0;
    double ret = 0.0, open = 0.0;
    const size_t wave_slot = (size_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    unsigned long long* bs = a.block_stats + wave_slot * 2;
    if (R::STATS) {
        resets = bs[0];
        if (!Env::kConstReward) {
            ret = reinterpret_cast<const double*>(bs)[1];
            open = a.wave_open[wave_slot];
        }
    }
    StepOut<VEC> out;
    constexpr bool kDiscrete = sizeof(Action) == 1;
    constexpr int kBlocks = kVec / 4;     // a work-item's lanes are kVec consecutive global ids: kVec/4 aligned groups
    u32x4 blk[kBlocks];                    // of four lanes that share one action block (gymrs_philox.h) ...
    const uint64_t gid = a.gid0 + base;
    const bool aligned = (a.gid0 & 3u) == 0; // ... when the shard starts on a multiple of 4 (wave-uniform)
    const uint64_t tick0 = a.tick;
    uint64_t ustart = r.uniform_start;
    for (uint32_t k = 0; k < r.n_steps; ++k) {
        const uint64_t t = r.action_t0 + k;
        const uint64_t slot = kDiscrete ? (t >> 1) : t; // Discrete: a block serves two steps (16-bit halves)
        if constexpr (Src::kExplore) {
            src.fill(d.st, d.act, gid, tick0 + k, aligned);
        } else if constexpr (Src::kPolicy) {
            src.fill(d.st, d.act);
        } else if (aligned) {
            if (!kDiscrete || k == 0 || (t & 1u) == 0) {
#pragma unroll
                for (int b = 0; b < kBlocks; ++b) blk[b] = action_block(r.action_seed, gid + 4 * b, slot);
            }
#pragma unroll
            for (int i = 0; i < kVec; ++i) {
                const uint32_t w = blk[i / 4].v[i % 4];
                if constexpr (kDiscrete)
                    d.act.v[i] = discrete_from_word(w, t, r.n_actions);
                else
                    d.act.v[i] = uniform_between(w, -r.max_torque, r.max_torque);
            }
        } else { // shard offset not a multiple of 4: every lane evaluates its own block (same values, slower)
#pragma unroll
            for (int i = 0; i < kVec; ++i) {
                const uint32_t w = action_word(r.action_seed, gid + i, slot);
                if constexpr (kDiscrete)
                    d.act.v[i] = discrete_from_word(w, t, r.n_actions);
                else
                    d.act.v[i] = uniform_between(w, -r.max_torque, r.max_torque);
            }
        }
        a.tick = tick0 + k;
        if (Env::kNeverTerminates && R::TLIM) { // the uniform episode clock of gymrs_engine.hip step_args()
            a.truncate_all = (a.tick + 1 - ustart >= c.max_steps) ? 1u : 0u;
            if (a.truncate_all && R::AUTO) ustart = a.tick + 1;
        }
        if constexpr (Sink::kOn) {
            sink->step(k);
            advance_tile<Env, VEC, FLAGS, FULL, true, kBlock, Sink>(a, c, base, d, lds, resets, ret, open, out, sink);
        } else
            advance_tile<Env, VEC, FLAGS, FULL, true, kBlock>(a, c, base, d, lds, resets, ret, open, out);
        if constexpr (Fit::kOn) fit->template step<FULL>(out, base, a.n);
        if constexpr (REC) {
            const uint64_t row = (uint64_t)k * r.rec_stride;
            constexpr int kObs = Env::kHasObsExtra ? 3 : Env::kState;
            float* obs = r.rec_obs + row * kObs;
            if constexpr (Env::kHasObsExtra) { // Pendulum: (cos, sin, theta_dot) as store_tile writes them
                Vec<float, kVec> oc, os;
#pragma unroll
                for (int i = 0; i < kVec; ++i) sincosf_(d.st[0].v[i], &os.v[i], &oc.v[i]);
                store_vec<float, kVec, true>(obs, base, a.n, FULL, oc);
                store_vec<float, kVec, true>(obs + r.rec_stride, base, a.n, FULL, os);
                store_vec<float, kVec, true>(obs + 2 * r.rec_stride, base, a.n, FULL, d.st[1]);
            } else {
#pragma unroll
                for (int j = 0; j < Env::kState; ++j) store_vec<float, kVec, true>(obs + j * r.rec_stride, base, a.n, FULL, d.st[j]);
            }
            store_vec<Action, kVec, true>(static_cast<Action*>(r.rec_action) + row, base, a.n, FULL, d.act);
            store_vec<float, kVec, true>(r.rec_reward + row, base, a.n, FULL, out.reward);
            store_vec<uint8_t, kVec, true>(r.rec_done + row, base, a.n, FULL, out.done);
            if (R::TLIM && r.rec_trunc) store_vec<uint8_t, kVec, true>(r.rec_trunc + row, base, a.n, FULL, out.trunc);
        }
    }
    store_tile<Env, VEC, FLAGS, FULL, true>(a, base, d, out);
    if constexpr (Fit::kOn) fit->flush();
    if (R::STATS && (threadIdx.x & 63u) == 0) {
        bs[0] = resets;
        if (!Env::kConstReward) {
            reinterpret_cast<double*>(bs)[1] = ret;
            a.wave_open[wave_slot] = open;
        }
    }
}

// Waves per SIMD the register allocator aims for: 16 / VEC.  A TableT rollout (per-lane rows and indices on top of a state that
// already fills the 128 registers of 4 waves at VEC = 4) gets half that: at 16 / VEC it spilled up to 84 registers per work-item.
template <class Env, int VEC, uint32_t FLAGS, bool REC>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu((Env::kTable ? 8 : 16) / VEC, (Env::kTable ? 8 : 16) / VEC))) void rollout_kernel(
    const StepArgs a, const RolloutArgs r, const typename Env::Consts c)
{
    constexpr int LPB = kBlock * VEC;
    __shared__ ResetLds<Env, VEC, kBlock> lds;
    if ((uint64_t)blockIdx.x * LPB + (uint64_t)((threadIdx.x >> 6) + 1) * (64 * VEC) <= a.n) // wave-uniform, see step_kernel
        rollout_block<Env, VEC, FLAGS, true, REC>(a, r, c, lds);
    else
        rollout_block<Env, VEC, FLAGS, false, REC>(a, r, c, lds);
}

// The launch: lanes per work-item x flag set (gymrs_launch.h) x recording.
template <class Env>
static hipError_t rollout_vec(int vec, uint32_t flags, const StepArgs& a, const RolloutArgs& r, const void* consts, hipStream_t stream)
{
    return dispatch_table(vec, flags, hipErrorInvalidValue, [&](auto lanes, auto flag_set) {
        constexpr int VEC = decltype(lanes)::value;
        return dispatch_recording<VEC>(r.rec_obs != nullptr, hipErrorInvalidValue, [&](auto rec) {
            launch_begin();
            hipLaunchKernelGGL((rollout_kernel<Env, VEC, decltype(flag_set)::value, decltype(rec)::value>), dim3(step_grid(a.n, VEC)), dim3(kBlock), 0,
                               stream, a, r, *static_cast<const typename Env::Consts*>(consts));
            return hipGetLastError();
        });
    });
}

} // namespace gymrs
