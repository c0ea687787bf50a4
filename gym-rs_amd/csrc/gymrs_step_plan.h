// gymrs_step_plan.h -- the decisions of the host-side stepping path that need no device: which memory hints a launch gets, what
// the reset-log ring does before and after it, how many steps one captured graph holds, and Pendulum's uniform episode clock.
// The engine (gymrs_engine.hip) asks here and does the HIP side itself.
//
// Plain host C++17, no HIP, like gymrs_launch.h (the only header it includes): tests/test_step_plan.py compiles this header
// alone and walks it.
#pragma once
#include "gymrs_launch.h"

namespace gymrs {

// ---- memory hints ------------------------------------------------------------------------------------------------------------
// What one step moves per lane: 8 bytes per state component (read + written), 10 of reward, flags and ep_start, Pendulum's cos / sin.
inline uint64_t bytes_per_step(gymrs_env_kind kind, int state_dim, uint64_t n)
{
    return n * ((uint64_t)state_dim * 8 + 10 + (kind == GYMRS_PENDULUM ? 8 : 0));
}

// Non-temporal accesses pay off (profiles/r02_size_sweep.log, r04_hints_by_size.log) while one step's arrays are small next to
// the 256 MB Infinity Cache (CartPole 2^20 lanes: 6.6 vs 7.0 us: the next reader of every array is the next kernel), and again
// once one step's traffic is far beyond it (2^25 lanes: 231 vs 242 us: nothing survives until the next step anyway).  In
// between only the stores nobody reads again -- reward, done, truncated, Pendulum's cos / sin -- are streamed and leave the
// cache to the state, which the next step reads (CartPole 2^21 lanes 13.3 -> 12.1 us, 2^24 112.2 -> 96.0 against hinting all).
constexpr uint64_t kHintAllUpToBytes = 48ull << 20;
constexpr uint64_t kHintAllFromBytes = 1024ull << 20;

// The hint bits of one per-step launch.  nt_mode (gymrs_set_tuning): 1 always non-temporal, 2 never, 3 outputs only, else by size.
// chain = a launch of a chain (gymrs_aql.h; profiles/r03_chain_hints.log): it lives off the lines the previous launch left in
// the L2s, so while the arrays are small the state STORES are not streamed; the outputs are (CartPole 2^20 lanes 5.44 -> 5.02 us)
// and the state LOADS too (4.91; at 2^21 that costs 1.3 us).  (Streaming the ACTION loads alone costs a full microsecond.)
inline uint32_t hint_bits(int nt_mode, uint64_t per_step, bool chain)
{
    switch (nt_mode) {
    case 1: return kFlagNonTemporal;
    case 2: return 0u;
    case 3: return kFlagNtOut;
    default: break;
    }
    if (per_step >= kHintAllFromBytes) return kFlagNonTemporal;
    if (per_step > kHintAllUpToBytes) return kFlagNtOut;
    return chain ? (kFlagNtOut | kFlagNtStateLoads) : kFlagNonTemporal;
}

// ---- the reset-log ring ------------------------------------------------------------------------------------------------------
// Invariant: the rows of the steps first_tick .. first_tick + pending - 1 (pending < kResetLogRows) may hold bits; every other
// row of the ring is zero.  vec = lanes per work-item of the launches that wrote the pending rows: rows are laid out per
// wavefront of ONE launch shape.
struct ResetLogRing {
    uint32_t pending;
    uint64_t first_tick;
    int vec;
};

struct ResetLogStep {
    bool fold_first;    // the pending rows are folded by the stand-alone kernel before this launch
    uint32_t fold_step; // StepArgs::fold_step: this launch is the folding variant (the ring would be full after it; it folds
                        // the whole ring inside the kernel, its own masks included)
    ResetLogRing after; // the ring once the launch is submitted
};

// About to launch ONE per-step kernel of `vec` lanes per work-item at `tick`.  logged = the launch keeps its episode
// bookkeeping in the ring; one that does not reads ep_start itself, so nothing may be pending.
inline ResetLogStep reset_log_step(ResetLogRing ring, bool logged, uint64_t tick, int vec)
{
    ResetLogStep s{false, 0u, ring};
    if (ring.pending != 0 && (!logged || ring.vec != vec)) {
        s.fold_first = true;
        s.after.pending = 0;
    }
    if (!logged) return s;
    if (s.after.pending == 0) {
        s.after.first_tick = tick;
        s.after.vec = vec;
    }
    if (s.after.pending == kResetLogRows - 1) {
        s.fold_step = 1;
        s.after.pending = 0;
    } else {
        s.after.pending += 1;
    }
    return s;
}

// ---- captured graphs -----------------------------------------------------------------------------------------------------------
// Steps one captured graph holds: a whole number of passes over the ring of n_buffers action buffers, at least 32 steps, and
// (reset-logged launches) a whole number of ring periods, so that a replay both starts and ends on an empty ring.
inline uint32_t graph_steps(uint32_t n_buffers, bool logged)
{
    uint32_t passes = (32 + n_buffers - 1) / n_buffers;
    if (logged) {
        uint32_t g = n_buffers, r = kResetLogRows; // gcd
        while (r) {
            const uint32_t tmp = g % r;
            g = r;
            r = tmp;
        }
        const uint32_t unit = kResetLogRows / g;
        passes = (passes + unit - 1) / unit * unit;
    }
    return n_buffers * passes;
}

// ---- Pendulum's uniform episode clock ----------------------------------------------------------------------------------------
// Pendulum never terminates, so under GYMRS_TIME_LIMIT every lane's episode started at the same tick, uniform_start, and the
// host knows which step truncates them all (StepArgs::truncate_all).
// Does the step launched at `tick` take every lane to the limit?
inline bool uniform_clock_hits(uint64_t tick, uint64_t uniform_start, uint32_t max_steps) { return tick + 1 - uniform_start >= max_steps; }
// uniform_start after that step: under auto-reset a step that hit re-armed every lane, and they all start at the next tick.
inline uint64_t uniform_clock_after(uint64_t tick, uint64_t uniform_start, bool hit, bool auto_reset)
{
    return hit && auto_reset ? tick + 1 : uniform_start;
}

} // namespace gymrs
