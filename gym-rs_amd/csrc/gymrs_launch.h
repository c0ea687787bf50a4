// gymrs_launch.h -- THE launch table of the kernel library: which (lanes per work-item, flag set) pairs a kernel family is
// built for, and how a launch's run-time values reach the instantiation built for them.  Every family with a table goes
// through here: the per-step kernels (gymrs_step_impl.h), the random-policy rollout (gymrs_rollout_impl.h) and the eight
// closed-loop rollout families (gymrs_rollout_policy_impl.h and the headers on top of it), whose routing decision -- which family
// a request reaches, and which requests reach none -- is dispatch_closed_loop at the end of this file.  The internal launch flags
// and the size of the reset-log ring live here too: the kernels and the engine's HIP-free step plan (gymrs_step_plan.h) both need
// them.
//
// Plain host C++17, no HIP: a function here turns a run-time value into a compile-time constant (a std::integral_constant
// handed to a generic callable, whose body names the kernel template) or refuses it with the caller's `invalid` result.
// tests/test_launch_table.py compiles this header alone and walks it.
#pragma once
#include <cstdint>
#include <type_traits>

#include "gymrs_amd.h"

namespace gymrs {

constexpr uint32_t kFlagNonTemporal = 0x100u; // internal launch flag (not an engine flag): non-temporal loads/stores
// Hints per class of access, for the launches of a chain (gymrs_aql.h): only the stores nobody reads again (reward, done,
// truncated, Pendulum's cos / sin), and additionally the state LOADS (the state stores stay plain: the next launch reads them
// out of the L2).  Measured per size in profiles/r03_chain_hints.log; the engine picks (hint_bits, gymrs_step_plan.h).
constexpr uint32_t kFlagNtOut = 0x200u;
constexpr uint32_t kFlagNtStateLoads = 0x400u;
constexpr uint32_t kFlagHintMask = kFlagNonTemporal | kFlagNtOut | kFlagNtStateLoads;
// Internal launch flag (not an engine flag, not a hint): the engine holds a parameter table (gymrs_set_param_table), so the
// launch goes to the table instantiations (TableT, gymrs_table_<env>.hip) with a TableConsts instead of the env's Consts.
constexpr uint32_t kFlagTable = 0x800u;
// Rows of the reset log.  Measured at 2^20 CartPole lanes (128 KiB per row, no folding): a ring of <= 8 rows stays where a
// write is cheap (6.10 us per launch; 8 steps x 40 MB is about what passes through the 256 MB Infinity Cache before a line
// is evicted), 16 rows 6.22, >= 32 rows 6.40 (touching the next row one step ahead with a scalar load made it worse:
// 7.1); the scattered ep_start stores it replaces: 6.65.  Must be a power of two; the folding launch is written for 8.
constexpr uint32_t kResetLogRows = 8;

template <uint32_t V>
using FlagSet = std::integral_constant<uint32_t, V>;
template <int V>
using Lanes = std::integral_constant<int, V>;

// Developer builds (tools/devbuild.py, -DGYMRS_DEV_MINIMAL): a table dispatched with MINIMAL = kDevMinimal shrinks to the
// headline flag sets at 4 lanes per work-item -- seconds instead of minutes.  The per-step table does; the others stay whole.
#ifdef GYMRS_DEV_MINIMAL
constexpr bool kDevMinimal = true;
#else
constexpr bool kDevMinimal = false;
#endif

namespace detail {
template <bool BUILT, class C, class R, class Fn>
R reach(R invalid, Fn& fn)
{
    if constexpr (BUILT)
        return fn(C{});
    else
        return invalid;
}
} // namespace detail

// The ten flag sets.  Statistics and final observations need auto-reset: without it both bits are dropped.
template <bool MINIMAL = false, class R, class Fn>
R dispatch_flag_set(uint32_t flags, R invalid, Fn&& fn)
{
    constexpr uint32_t A = GYMRS_AUTO_RESET, S = GYMRS_TRACK_STATS, T = GYMRS_TIME_LIMIT, F = GYMRS_FINAL_OBS;
    constexpr bool ALL = !MINIMAL;
    if (!(flags & A)) flags &= ~(S | F);
    switch (flags & (A | S | T | F)) {
    case 0: return detail::reach<ALL, FlagSet<0>>(invalid, fn);
    case A: return detail::reach<ALL, FlagSet<A>>(invalid, fn);
    case A | S: return detail::reach<true, FlagSet<A | S>>(invalid, fn);
    case T: return detail::reach<ALL, FlagSet<T>>(invalid, fn);
    case A | T: return detail::reach<ALL, FlagSet<A | T>>(invalid, fn);
    case A | S | T: return detail::reach<true, FlagSet<A | S | T>>(invalid, fn);
    case A | F: return detail::reach<ALL, FlagSet<A | F>>(invalid, fn);
    case A | S | F: return detail::reach<ALL, FlagSet<A | S | F>>(invalid, fn);
    case A | T | F: return detail::reach<ALL, FlagSet<A | T | F>>(invalid, fn);
    case A | S | T | F: return detail::reach<ALL, FlagSet<A | S | T | F>>(invalid, fn);
    default: return invalid;
    }
}

// The eight of them with auto-reset, for a family that is only built where lanes are re-armed (gymrs_rollout_transitions_impl.h).
template <class R, class Fn>
R dispatch_auto_reset_flag_set(uint32_t flags, R invalid, Fn&& fn)
{
    constexpr uint32_t A = GYMRS_AUTO_RESET, S = GYMRS_TRACK_STATS, T = GYMRS_TIME_LIMIT, F = GYMRS_FINAL_OBS;
    switch (flags & (A | S | T | F)) {
    case A: return fn(FlagSet<A>{});
    case A | S: return fn(FlagSet<A | S>{});
    case A | T: return fn(FlagSet<A | T>{});
    case A | S | T: return fn(FlagSet<A | S | T>{});
    case A | F: return fn(FlagSet<A | F>{});
    case A | S | F: return fn(FlagSet<A | S | F>{});
    case A | T | F: return fn(FlagSet<A | T | F>{});
    case A | S | T | F: return fn(FlagSet<A | S | T | F>{});
    default: return invalid;
    }
}

// Lanes per work-item: 4 or 8.
template <bool MINIMAL = false, class R, class Fn>
R dispatch_lanes(int vec, R invalid, Fn&& fn)
{
    switch (vec) {
    case 4: return detail::reach<true, Lanes<4>>(invalid, fn);
    case 8: return detail::reach<!MINIMAL, Lanes<8>>(invalid, fn);
    default: return invalid;
    }
}

// Both: fn(Lanes<VEC>, FlagSet<FLAGS>).
template <bool MINIMAL = false, class R, class Fn>
R dispatch_table(int vec, uint32_t flags, R invalid, Fn&& fn)
{
    return dispatch_lanes<MINIMAL>(vec, invalid, [&](auto lanes) {
        return dispatch_flag_set<MINIMAL>(flags, invalid, [&](auto flag_set) { return fn(lanes, flag_set); });
    });
}

// A rollout that records its trajectory (RolloutArgs::rec_obs): the recording variant of a rollout kernel exists at 4 lanes per
// work-item only.  fn(std::bool_constant<REC>).
template <int VEC, class R, class Fn>
R dispatch_recording(bool record, R invalid, Fn&& fn)
{
    if (record) return detail::reach<VEC == 4, std::true_type>(invalid, fn);
    return detail::reach<true, std::false_type>(invalid, fn);
}

// ---- the closed-loop fused rollouts: eight kernel families (gymrs_rollout_policy_impl.h and the three headers on top of it), one
// routing decision.  Where a request's actions come from ...
enum class ClosedLoopSource {
    policy,    // the greedy action of the engine's policy set
    exploring, // its epsilon-greedy action (ExploreArgs)
    sampling,  // an action drawn from the softmax of its logits (SampleArgs)
};
// ... and the kernel it reaches: rollout_<name>_kernel.
enum class ClosedLoopFamily {
    policy,
    policy_fitness,
    explore,
    explore_fitness,
    sample,
    sample_fitness,
    transitions,
    sample_transitions,
};
constexpr int kClosedLoopFamilies = 8;
template <ClosedLoopFamily V>
using Family = std::integral_constant<ClosedLoopFamily, V>;

namespace detail {
// fn(Family<..>): GREEDY, EXPLORING or SAMPLING by the source.
template <ClosedLoopFamily GREEDY, ClosedLoopFamily EXPLORING, ClosedLoopFamily SAMPLING, class R, class Fn>
R dispatch_source(ClosedLoopSource source, R invalid, Fn&& fn)
{
    switch (source) {
    case ClosedLoopSource::policy: return fn(Family<GREEDY>{});
    case ClosedLoopSource::exploring: return fn(Family<EXPLORING>{});
    case ClosedLoopSource::sampling: return fn(Family<SAMPLING>{});
    default: return invalid;
    }
}
} // namespace detail

// fn(Family<FAMILY>, Lanes<VEC>, FlagSet<FLAGS>, std::bool_constant<REC>) for a closed-loop request, or `invalid`:
//   * the fitness counters go with neither a record nor transitions (no such kernel is built);
//   * transitions need a record and auto-reset (without it nothing is re-armed); they run at 4 lanes per work-item whatever `vec`
//     says, in the eight flag sets with auto-reset.  Greedy and exploring requests share the transitions family (a greedy launch
//     plays threshold 0), sampling has its own;
//   * fitness: the source's fitness family, the ten flag sets at 4 or 8 lanes, REC = false;
//   * otherwise the source's plain family, the ten flag sets at 4 or 8 lanes; a record at 4 lanes only.
template <class R, class Fn>
R dispatch_closed_loop(ClosedLoopSource source, bool fitness, bool record, bool transitions, int vec, uint32_t flags, R invalid, Fn&& fn)
{
    using F = ClosedLoopFamily;
    if (fitness && (record || transitions)) return invalid;
    if (transitions) {
        if (!record || !(flags & GYMRS_AUTO_RESET)) return invalid;
        return dispatch_auto_reset_flag_set(flags, invalid, [&](auto flag_set) {
            return detail::dispatch_source<F::transitions, F::transitions, F::sample_transitions>(
                source, invalid, [&](auto family) { return fn(family, Lanes<4>{}, flag_set, std::true_type{}); });
        });
    }
    return dispatch_table(vec, flags, invalid, [&](auto lanes, auto flag_set) {
        if (fitness)
            return detail::dispatch_source<F::policy_fitness, F::explore_fitness, F::sample_fitness>(
                source, invalid, [&](auto family) { return fn(family, lanes, flag_set, std::false_type{}); });
        return dispatch_recording<decltype(lanes)::value>(record, invalid, [&](auto rec) {
            return detail::dispatch_source<F::policy, F::explore, F::sample>(source, invalid,
                                                                             [&](auto family) { return fn(family, lanes, flag_set, rec); });
        });
    });
}

} // namespace gymrs
