// gymrs_rollout_transitions_impl.h -- the recording closed-loop kernel once more with a final-observation sink: the kernels of
// gymrs_rollout_transitions (include/gymrs_amd.h, "transitions").  gfx950.  rollout_block with REC set writes the five record rows
// as gymrs_rollout_closed_loop does; the sink adds, per step, the pre-re-arm observation of every lane that step re-armed, and
// once per launch the observations the launch starts from.  Kernels of their own: the existing families keep their names, their
// code and their register budgets.  Included by gymrs_transitions.hip (the uniform envs) and by gymrs_table_transitions_<env>.hip
// (TableT: per-lane parameter tables).
#pragma once
#include "gymrs_rollout_explore_impl.h"

namespace gymrs {

// The Sink of rollout_block / advance_tile.
//   * start: one dense vector store per component, right behind the tile's loads (the state is the observation).
//   * store: called by advance_tile where store_final_obs is, in a wave that re-arms at least one lane, with the state after the
//     physics and before the re-arm: one scattered dword per component and finished lane into the step's row, as store_final_obs
//     does for CartPole / MountainCar.  A lane that is not re-armed (beyond n, not stepped, still running) writes nothing.
template <class Env, int VEC>
struct FinalObsRows {
    static constexpr bool kOn = true;
    static_assert(!Env::kHasObsExtra, "the observation is the state: CartPole and MountainCar");
    float* const final_obs;
    float* const start_obs;
    const uint64_t stride;
    float* row; // final_obs of the step being played
    __device__ __forceinline__ FinalObsRows(const TransitionArgs& t, const RolloutArgs& r)
        : final_obs(t.final_obs), start_obs(t.start_obs), stride(r.rec_stride), row(t.final_obs)
    {
    }
    template <bool FULL>
    __device__ __forceinline__ void start(const Vec<float, VEC> (&st)[Env::kState], uint64_t base, uint64_t n) const
    {
        if (start_obs) { // wave-uniform
#pragma unroll
            for (int j = 0; j < Env::kState; ++j) store_vec<float, VEC, true>(start_obs + j * stride, base, n, FULL, st[j]);
        }
    }
    __device__ __forceinline__ void step(uint32_t k) { row = final_obs + (uint64_t)k * Env::kState * stride; }
    __device__ __forceinline__ void store(uint64_t base, const float (&ls)[Env::kState][VEC], const bool (&need_reset)[VEC]) const
    {
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            if (need_reset[k]) {
#pragma unroll
                for (int j = 0; j < Env::kState; ++j) row[(uint64_t)j * stride + base + k] = ls[j][k];
            }
        }
    }
};

// Waves per SIMD the register allocator aims for, as PolicyWaves / ExploreWaves: per family the highest budget at which none of
// its eight flag sets spills a vector register to scratch (profiles/transitions.md lists the budgets tried and what they spilled).
// At 3 waves per SIMD rollout_transitions_kernel<CartPoleT> and <TableT<MountainCarT>> spill 4 VGPRs (20 B of scratch) in the
// A | S | T | F flag set and nowhere else; <MountainCarT> spills nowhere at 3; <TableT<CartPoleT>> starts from PolicyWaves' 2.
template <class Env>
struct TransitionWaves {
    static constexpr int value = 2;
};
template <>
struct TransitionWaves<MountainCarT> {
    static constexpr int value = 3;
};

// rollout_explore_kernel<.., REC = true> with the sink.  One action source serves greedy and exploring launches: a greedy launch
// passes threshold 0, where ExploringActions is defined to give the greedy bits without evaluating a Philox block (gymrs_policy.h).
template <class Env, uint32_t FLAGS>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(TransitionWaves<Env>::value, TransitionWaves<Env>::value))) void rollout_transitions_kernel(
    const StepArgs a, const RolloutArgs r, const typename Env::Consts c, const PolicyArgs p, const ExploreArgs x, const TransitionArgs t)
{
    constexpr int VEC = 4; // the record's rule
    static_assert((FLAGS & GYMRS_AUTO_RESET) != 0, "without auto-reset nothing is re-armed: the record's obs rows are the final observations");
    FinalObsRows<Env, VEC> sink(t, r);
    GYMRS_CLOSED_LOOP_ENTRY(ExploringActions, (p, pol, x), true, /* no hook */, (a, r, c, lds, src, static_cast<NoFitness*>(nullptr), &sink))
}
template <class Env, int VEC, uint32_t FLAGS, bool REC>
static hipError_t closed_loop_kernel(Family<ClosedLoopFamily::transitions>, const ClosedLoopLaunch& l)
{
    static_assert(VEC == 4 && REC, "the record's rule");
    return closed_loop_submit<Env, VEC>(rollout_transitions_kernel<Env, FLAGS>, l, l.source == ClosedLoopSource::exploring ? l.explore : ExploreArgs{},
                                        *l.transitions);
}

} // namespace gymrs
