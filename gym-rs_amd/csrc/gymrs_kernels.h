// gymrs_kernels.h — launch interface between the engine (gymrs_engine.hip, gymrs_engine_io.hip, gymrs_engine_learn.hip) and the gfx950 kernels.  Plain
// structs passed by value as kernel arguments (uniform -> SGPRs).  The kernel files:
//   gymrs_step_<env>.hip     the per-step kernel table of one env type (gymrs_step_impl.h), one translation unit each
//   gymrs_table_<env>.hip    the per-step, rollout and evaluation kernels of one env type with a parameter table (TableT)
//   gymrs_step_aql.hip       the per-step kernels once more, as the code object of the engine's own AQL dispatcher
//   gymrs_rollout.hip        the fused random-policy rollout (gymrs_rollout_impl.h)
//   gymrs_rollout_policy.hip the closed-loop kernels: policy actions, the fused rollout under a policy (gymrs_policy.h); launch_closed_loop
//   gymrs_rollout_fitness.hip  that rollout with per-policy fitness counters
//   gymrs_explore.hip        the closed-loop kernels once more with the epsilon-greedy action source (gymrs_rollout_explore_impl.h)
//   gymrs_sample.hip         the closed-loop and transitions kernels with the softmax sampling source (gymrs_rollout_sample_impl.h)
//   gymrs_transitions.hip    the recording closed-loop kernel with per-step final observations (gymrs_rollout_transitions_impl.h)
//   gymrs_evaluate.hip       episodic policy evaluation (gymrs_evaluate.h, gymrs_evaluate_impl.h)
//   gymrs_aux.hip            everything off the per-step path: reset, action fill, statistics, folds
// gymrs_launch.h holds the one launch table (flag sets x lanes per work-item) the step and rollout families dispatch through, and
// the internal launch flags; gymrs_step_plan.h the host-side decisions around a step launch that need no device (the engine's
// alone: no kernel file includes it); gymrs_tile.h the device code the kernels share.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "gymrs_launch.h"
#include "gymrs_physics.h"

namespace gymrs {

constexpr int kBlock = 256; // work-items per workgroup of the small kernels (reset, fill, statistics) and of the rollout kernel

// ---- per-lane physics parameters (gymrs_set_param_table) -------------------------------------------------------------------
// One row of a parameter table on the device: the f32 constants make_consts derives from one gymrs_<kind>_params, without the
// fields every row shares (CartPole's integrator, max_steps).  CartPole: the 8 floats of CartPoleConsts in order; MountainCar:
// the 7 floats of MountainCarConsts, padded.  32 bytes: two dwordx4 loads per lane.
struct alignas(16) ParamRow {
    float v[8];
};
constexpr uint32_t kMaxParamRows = 65536; // the lane index is a uint16_t
static_assert(offsetof(CartPoleConsts, integrator) == 8 * sizeof(float) && offsetof(MountainCarConsts, max_steps) == 7 * sizeof(float),
              "a ParamRow holds the leading floats of the env's Consts");
__host__ __device__ inline ParamRow param_row(const CartPoleConsts& c)
{
    return ParamRow{{c.gravity, c.tau, c.force_over_tm, c.pml_over_tm, c.len_43, c.len_mp_over_tm, c.theta_thr, c.x_thr}};
}
__host__ __device__ inline ParamRow param_row(const MountainCarConsts& c)
{
    return ParamRow{{c.min_position, c.max_position, c.max_speed, c.goal_position, c.goal_velocity, c.force, c.gravity, 0.0f}};
}
// the inverse, with the engine-wide fields added back
__host__ __device__ inline void consts_of_row(const ParamRow& r, int32_t integrator, uint32_t max_steps, CartPoleConsts& c)
{
    c.gravity = r.v[0];
    c.tau = r.v[1];
    c.force_over_tm = r.v[2];
    c.pml_over_tm = r.v[3];
    c.len_43 = r.v[4];
    c.len_mp_over_tm = r.v[5];
    c.theta_thr = r.v[6];
    c.x_thr = r.v[7];
    c.integrator = integrator;
    c.max_steps = max_steps;
}
__host__ __device__ inline void consts_of_row(const ParamRow& r, int32_t, uint32_t max_steps, MountainCarConsts& c)
{
    c.min_position = r.v[0];
    c.max_position = r.v[1];
    c.max_speed = r.v[2];
    c.goal_position = r.v[3];
    c.goal_velocity = r.v[4];
    c.force = r.v[5];
    c.gravity = r.v[6];
    c.max_steps = max_steps;
}
// The by-value constants of a table launch (the kernel's `Consts` parameter; StepArgs keeps its layout): lane i steps with
// rows[index[i]] when index[i] < k; a lane whose index is >= k is not stepped and is reported like an invalid action.
struct TableConsts {
    const ParamRow* rows;   // [k] device rows
    const uint16_t* index;  // [n] device: the row of every lane
    uint32_t k;             // rows in the table, 1 .. kMaxParamRows
    int32_t integrator;     // CartPole: shared by every row (TableT::variant hoists it out of the lane code)
    uint32_t max_steps;     // shared by every row (the time limit)
    uint32_t pad_;
};

// Everything one step() launch needs.  Device pointers are SoA arrays of n lanes.
struct StepArgs {
    float* s[4];       // state: CartPole x,x_dot,theta,theta_dot | MountainCar position,velocity | Pendulum theta,theta_dot
    float* obs_cos;    // Pendulum only
    float* obs_sin;    // Pendulum only
    const void* action; // u8 (CartPole, MountainCar) or f32 (Pendulum)
    float* reward;
    uint8_t* done;
    uint8_t* truncated; // written only with GYMRS_TIME_LIMIT
    // CartPole without auto-reset: steps_beyond_terminated.is_some().  The same slot carries, for the GYMRS_FINAL_OBS
    // instantiations (auto-reset on, so `beyond` is never read there), the base of the final-observation arrays: obs_dim rows
    // of final_obs_stride(n) lanes (TileRegs::FINAL, advance_tile).  A union and not a new member: every launch's kernel
    // arguments keep their layout (KernArgView::fetch and the AQL dispatcher address them by offset).
    union {
        uint8_t* beyond;
        float* final_obs;
    };
    uint32_t* ep_start; // tick at which the lane's current episode started (low 32 bits)
    uint32_t* wave_clean; // [n_waves] constant-reward envs under auto-reset that elide the reward store: != 0 = the wave's part of `reward` holds the constant
    double* wave_open;  // [n_waves] Pendulum with GYMRS_TRACK_STATS: per-wavefront sum of the rewards of the open episodes
    unsigned long long* block_stats; // [n_waves][2] per-wavefront slots: finished episodes, sum of returns (f64 bits; Pendulum only)
    // Reset log (constant-reward envs with GYMRS_TRACK_STATS and without GYMRS_TIME_LIMIT): instead of one scattered 4-byte
    // ep_start store per re-armed lane and a read-modify-write of the wavefront's episode counter on every step, a
    // wavefront that re-armed lanes stores its VEC done-masks (one bit per lane) into row (tick % kResetLogRows) of a small
    // ring, and every kResetLogRows-th launch (fold_step) each wavefront folds its own column of the ring into ep_start and
    // its episode counter.  See step_block (gymrs_step_impl.h) and launch_fold_reset_log.
    unsigned long long* reset_log; // [kResetLogRows][reset_log_row_words]; word (wave * VEC + k), bit = work-item of the wave
    uint32_t reset_log_row_words;
    uint32_t fold_step;            // this launch folds the ring (wave-uniform branch in step_block)
    uint32_t elide_reward;         // constant-reward envs whose kernel does not elide the reward store unconditionally (CartPole): != 0 = this engine elides it (step_block)
    uint32_t div_in_range;         // CartPole's per-step kernel: != 0 = the host has bounded the division's `den` inside [0.25, 2) (div_in_range_ok, gymrs_physics.h), the
                                   // fast path may divide scale-free (CartPoleT::advance_fast_tile).  It fills what was a 4-byte hole: no other member moves.
    uint32_t* err;      // [0] number of invalid actions seen, [1] lowest offending lane (0xffffffff = none)
    uint32_t* err_seen; // mapped host words: [0] a wave that saw an invalid action sets it to 1: gymrs_sync looks there first and
                        // fetches err[] only then (no device-to-host copy per synchronisation); [1] a wave of a CHAIN launch that found
                        // itself on another XCD than the dispatcher's self-check saw for its workgroup index stores that index + 1
    uint64_t n;         // lanes in this engine
    uint64_t n_fast;    // n, or 0 when the action buffer is not aligned for the vector load (step_kernel)
    uint64_t gid0;      // global id of lane 0
    uint64_t seed;
    uint64_t tick;      // engine tick of this launch; when tick_base != NULL it is an OFFSET added to *tick_base
    const unsigned long long* tick_base; // device-resident tick for captured HIP graphs (NULL in eager launches)
    SampleBox box;      // reset sampling box, prepared on the host (gymrs_philox.h)
    uint32_t truncate_all; // envs that never terminate (Pendulum): this step hits the time limit for every lane
    uint32_t skip_trunc_store; // same envs: the `truncated` array already holds this step's (uniform) value
    unsigned long long* trace; // developer instrumentation (GYMRS_TRACE_TIMES builds), else NULL
    // Launches of a chain (gymrs_aql.h) carry no release fence between them, which is only right while tile i is stepped on the SAME
    // XCD (= the same L2) in every launch of the chain.  Where a queue's workgroups start is NOT a constant of the queue (round 4: it
    // differs between queues and changes while a queue sits idle), so the premise is checked per chain: the FIRST step launch after
    // aql_begin (xcc_check == 2) has its workgroups 0 .. 7 store {chain number, XCC id} into xcc_table (entry k at word k * kXccTableStride:
    // one cache line each; a plain store, which stays in that XCD's L2), every later launch of the chain (xcc_check == 1) compares the
    // XCC it runs on (HW_REG_XCC_ID) and the chain number with entry (blockIdx.x & 7) and reports a mismatch through err_seen[1]: a
    // workgroup on the wrong XCD does not see the entry at all (it reads an older chain's).  Between two chains everything is written back and
    // re-acquired, so a deal that changed THERE is harmless.  HIP launches (a release fence each) pass xcc_check == 0.
    uint32_t* xcc_table; // [8 * kXccTableStride] device words
    uint32_t xcc_check;
    uint32_t xcc_seq;    // the chain's number (24 bits)
    uint32_t trace_wpb; // wavefronts per workgroup of this launch (the stamps' index; blockDim would be a hidden kernel argument, which
                        // the engine's own dispatcher does not supply)
};

static_assert(offsetof(StepArgs, final_obs) == offsetof(StepArgs, beyond) && sizeof(float*) == sizeof(uint8_t*) && sizeof(StepArgs) == 296,
              "GYMRS_FINAL_OBS shares the slot of `beyond`: the layout of StepArgs must not move");
static_assert(offsetof(StepArgs, elide_reward) == 136 && offsetof(StepArgs, div_in_range) == 140 && offsetof(StepArgs, err) == 144,
              "div_in_range sits in the padding behind elide_reward: KernArgView::fetch and the AQL dispatcher address StepArgs by offset");
// Lanes between two rows of the final-observation arrays: n rounded up to 16, so that every row starts aligned for a vector store.
__host__ __device__ inline uint64_t final_obs_stride(uint64_t n) { return (n + 15) & ~15ull; }

// The kernel-argument segment of step_kernel as the host sees it (the engine's own AQL dispatcher, gymrs_aql.h, fills it by
// hand; HIP launches marshal the same thing themselves): the parameters in order, naturally aligned.
template <class Consts>
struct StepKernArgs {
    float* s0;
    float* s1;
    float* s2;
    float* s3;
    const void* action;
    uint64_t n_fast;
    StepArgs rest;
    Consts c;
};
// KernArgView::fetch reads `rest` and `c` of a table launch at these offsets (nothing else would notice a change)
static_assert(offsetof(StepKernArgs<TableConsts>, rest) == 6 * 8 && alignof(TableConsts) <= 8 && sizeof(StepArgs) % alignof(TableConsts) == 0 &&
                  offsetof(StepKernArgs<TableConsts>, c) == 6 * 8 + sizeof(StepArgs),
              "the kernel-argument layout of the table launches");

// The fused multi-step kernel (gymrs_rollout): n_steps consecutive steps of every lane in ONE launch, with
// the random-policy actions of gymrs_fill_actions(action_seed, action_t0 + k) generated in registers.
struct RolloutArgs {
    uint64_t action_seed, action_t0;
    uint64_t uniform_start; // Pendulum time limit: the tick at which every lane's current episode started
    uint32_t n_steps;
    uint32_t n_actions;     // Discrete(n) envs
    float max_torque;       // Pendulum
    // gymrs_rollout_record: every step's outputs go to trajectory buffers, row k = step k (NULL = not recorded)
    float* rec_obs;         // [n_steps][obs_dim][rec_stride]
    void* rec_action;       // [n_steps][rec_stride] u8 (f32 for Pendulum)
    float* rec_reward;      // [n_steps][rec_stride]
    uint8_t* rec_done;      // [n_steps][rec_stride]
    uint8_t* rec_trunc;     // [n_steps][rec_stride], written with GYMRS_TIME_LIMIT only; may be NULL
    uint64_t rec_stride;    // lanes per row: >= n, a multiple of 16
};

struct ResetArgs {
    float* s[4];
    float* obs_cos;
    float* obs_sin;
    float* reward;
    uint8_t* done;
    uint8_t* truncated;
    uint8_t* beyond;
    uint32_t* ep_start;
    uint64_t n, gid0, seed, tick;
    SampleBox box;
    // gymrs_reset_pcg64 (gymrs_pcg64.h): lane i draws its state from Pcg64::seed_from_u64(pcg_seeds ? pcg_seeds[i] :
    // seed + gid0 + i) over [pcg_low, pcg_low + pcg_scale) instead of from the Philox reset stream
    int pcg64;
    const uint64_t* pcg_seeds;
    double pcg_low[4], pcg_scale[4];
};

// Work-items per workgroup of a per-step launch: CartPole uses 512 once the launch still puts two such workgroups on every
// CU (measured 2 % faster there; small batches want many small workgroups), everything else kBlock.  launch_one
// (gymrs_step_impl.h) and the engine's AQL dispatcher both go by this.
// ... and only while the launch is at most two generations of waves: from 2^22 lanes on a CU refills better in units of 4 waves (round 4,
// profiles/r04_wave_variants.log: 2^22 lanes 25.7 -> 24.8 us, 2^23 48.7 -> 47.4; 2^21 12.0 vs 12.2 the other way).
constexpr int kCartPoleThreads = 512;
constexpr uint64_t kBigGroupsFrom = 512, kBigGroupsBelow = 2048; // (where the window ends: profiles/r05_cartpole_2p21.log)
inline bool step_uses_big_groups(uint64_t n, int threads, int vec)
{
    return n >= (uint64_t)threads * vec * kBigGroupsFrom && n < (uint64_t)threads * vec * kBigGroupsBelow;
}
inline int step_threads_of(gymrs_env_kind kind, uint64_t n, int vec)
{
    return (kind == GYMRS_CARTPOLE && step_uses_big_groups(n, kCartPoleThreads, vec)) ? kCartPoleThreads : kBlock;
}

constexpr uint32_t kXccTableStride = 32; // words between two entries of StepArgs::xcc_table: one 128-byte line per entry

// Number of workgroups of `threads` work-items for n lanes at `vec` lanes per work-item (4 or 8).
inline uint32_t step_grid(uint64_t n, int vec, int threads = kBlock)
{
    const uint64_t per_block = (uint64_t)threads * vec;
    return (uint32_t)((n + per_block - 1) / per_block);
}

hipError_t launch_step(gymrs_env_kind kind, int vec, uint32_t flags, const StepArgs& a, const void* consts,
                       hipStream_t stream);
hipError_t launch_rollout(gymrs_env_kind kind, int vec, uint32_t flags, const StepArgs& a, const RolloutArgs& r,
                          const void* consts, hipStream_t stream);
hipError_t launch_reset(gymrs_env_kind kind, const ResetArgs& a, hipStream_t stream);
// Fold the `pending` (< kResetLogRows) not yet folded rows of the reset log (the steps first_tick .. first_tick + pending - 1,
// lanes-per-work-item `vec`) into ep_start (start tick of every lane's open episode) and the per-wavefront episode
// counters, and zero them again: on demand, off the hot path (the step kernel folds a full ring itself).
hipError_t launch_fold_reset_log(unsigned long long* log, uint32_t row_words, uint64_t first_tick, uint32_t pending, int vec,
                                 uint32_t* ep_start, uint64_t n, unsigned long long* block_stats, hipStream_t stream);
// wave_open[0] += sum of the others, others = 0 (before a launch whose lanes-per-wave differs from the last one's)
hipError_t launch_fold_open(double* wave_open, uint32_t n_slots, hipStream_t stream);
hipError_t launch_tick_advance(unsigned long long* tick_dev, unsigned long long by, hipStream_t stream);
hipError_t launch_fill_actions(gymrs_env_kind kind, void* actions, uint64_t n, uint64_t gid0, uint64_t seed, uint64_t t,
                               float max_torque, hipStream_t stream);
// A kernel launch (hipLaunchKernelGGL) reports its failure only through the calling thread's last-error word -- and since ROCm 7 that word keeps the last
// ERROR any earlier runtime call of the thread returned until somebody reads it (a successful call no longer overwrites it): a probe of this library
// that was allowed to fail, or an error the APPLICATION has not looked at.  Round 6's GPU suite met exactly that (an "invalid device ordinal" of a refused
// sharder creation surfaced three test files later as a failed reset).  Every launch site therefore reads the word once BEFORE it launches: what it
// returns afterwards is its own launch's.
inline void launch_begin() { (void)hipGetLastError(); }
constexpr int kStatsPartials = 256; // workgroups of the statistics read-out (= work-items of its finalize step)
struct StatsArgs {
    const uint32_t* ep_start;
    uint64_t n;
    uint64_t epoch;    // the tick reset() wrote into ep_start (all 64 bits of it: ep_start keeps the low 32)
    uint64_t tick;     // the engine tick now: no episode started after it, and an open one is younger than 2^32 steps
    const unsigned long long* block_stats;
    uint32_t n_blocks;
    unsigned long long* partials; // [kStatsPartials][3] scratch: one {sum of open ages, E, R} triple per workgroup of the read-out
    unsigned long long* base; // [kStatsBaseWords] {L, E, R (f64 bits)} at the last stats_clear: the BASELINE a read-out subtracts (see launch_stats)
    // the reset log's rows that are not folded yet: the read-out looks THROUGH them (read-only) instead of folding them first
    const unsigned long long* log;
    uint32_t log_row_words, log_pending;
    uint64_t log_first_tick;
    int log_vec;
    int track;                // GYMRS_TRACK_STATS set
    int reward_sign;          // +1 CartPole, -1 MountainCar (return = +-length), 0 Pendulum (summed)
    double n_steps;
    double* out4;             // {sum_return, sum_length, n_episodes, n_steps}
    double* host_out4;        // the same four into device-visible host memory (or NULL): a read-out without the copy engine
};
// mode 0 read, 1 clear (base = the totals now), 2 after reset (base = 0).
// The read-out WRITES NOTHING a step kernel reads (round 6; VERDICT r5 "next" #1c): gymrs_stats_clear used to zero the per-wavefront counters with a
// memset on the stream and to fold the reset log with an atomic-add kernel -- stream-side writes into memory the next launches (of the stream or of a chain on
// the engine's own queue) read-modify-write, the one place where round 5's stale episode counter could come from.  Now the counters only ever grow, written by
// the one wavefront that owns each slot; a clear remembers the totals and a read subtracts them (u64: exact; Pendulum's f64 return sum: to an ulp of the
// total), and rows of the reset log that are still pending are counted where they lie.
constexpr int kStatsBaseWords = 4;
hipError_t launch_stats(const StatsArgs& a, int mode, hipStream_t stream);
// The age of the oldest open episode, max over lanes of (uint32_t)(tick_ref - ep_start[lane]), from which the host derives
// the tick before which no lane's episode started (GYMRS_TIME_LIMIT elision, gymrs_engine.hip).  partials = kStatsPartials
// device words of scratch; the result goes to host_out2 (device-visible host memory): [0] = the age, then [1] = seq.
hipError_t launch_max_age(const uint32_t* ep_start, uint64_t n, uint32_t tick_ref, uint32_t* partials, uint32_t* host_out2, uint32_t seq,
                          hipStream_t stream);

// ---- closed-loop rollouts (gymrs_set_policy) --------------------------------------------------------------------------------
// A policy set on the device: n_policies policies of `stride` floats back to back (the layout of include/gymrs_amd.h); lane i
// of the batch (GLOBAL id) uses policy (i / lanes_per_policy) % n_policies.  Passed by value next to the other kernel arguments
// of the policy kernels (gymrs_rollout_policy.hip); the launch arguments of every other kernel keep their layout.
struct PolicyArgs {
    const float* weights;
    uint64_t lanes_per_policy; // >= 1
    uint32_t n_policies;       // >= 1
    uint32_t hidden;           // H: 0 = affine, else the width of the one hidden ReLU layer (<= kMaxPolicyHidden)
    uint32_t stride;           // S = policy_floats(kind, hidden)
    uint32_t pad_;
};
constexpr uint32_t kMaxPolicyHidden = 64;
// The exploration settings of an engine (gymrs_set_exploration) as the exploring kernels get them by value, after PolicyArgs
// (gymrs_explore.hip): the draw is keyed (seed, global id, engine tick) on stream 2 of gymrs_philox.h.
struct ExploreArgs {
    uint64_t seed;
    uint32_t threshold; // 0 .. 65536: a step explores when the low half of its word is below it
    uint32_t pad_;
};
// The sampling settings of an engine (gymrs_set_sampling) as the sampling kernels get them by value, in ExploreArgs' place
// (gymrs_sample.hip): the draw is keyed (seed, global id, engine tick) on stream 3 of gymrs_philox.h.
struct SampleArgs {
    uint64_t seed;
    float scale; // log2(e) / temperature: finite, >= 0
    uint32_t pad_;
};
// S: floats of one policy; 0 for an env kind that takes none (Pendulum: a Box action)
inline uint64_t policy_floats(gymrs_env_kind kind, uint32_t hidden)
{
    const uint64_t d = kind == GYMRS_CARTPOLE ? 4 : 2, a = kind == GYMRS_CARTPOLE ? 2 : 3;
    if (kind != GYMRS_CARTPOLE && kind != GYMRS_MOUNTAIN_CAR) return 0;
    return hidden == 0 ? a * (d + 1) : (uint64_t)hidden * (d + 1) + a * ((uint64_t)hidden + 1);
}
// actions[i] = policy(observation of lane i) for the n lanes whose observation rows are s[0 .. obs_dim)
hipError_t launch_policy_actions(gymrs_env_kind kind, const float* const* s, void* actions, uint64_t n, uint64_t gid0, const PolicyArgs& p,
                                 hipStream_t stream);
// ---- epsilon-greedy exploration (gymrs_set_exploration; gymrs_explore.hip) ----------------------------------------------------
// launch_policy_actions mixed with the exploration draw of engine tick `tick`
hipError_t launch_explore_actions(gymrs_env_kind kind, const float* const* s, void* actions, uint64_t n, uint64_t gid0, uint64_t tick,
                                  const PolicyArgs& p, const ExploreArgs& x, hipStream_t stream);
// ---- softmax sampling (gymrs_set_sampling; gymrs_sample.hip) -------------------------------------------------------------------
// launch_policy_actions with the sampled action of engine tick `tick`; prob (may be NULL) gets the probability of every lane's action
hipError_t launch_sample_actions(gymrs_env_kind kind, const float* const* s, void* actions, float* prob, uint64_t n, uint64_t gid0, uint64_t tick,
                                 const PolicyArgs& p, const SampleArgs& x, hipStream_t stream);
// ---- the closed-loop fused rollouts (gymrs_rollout_closed_loop, gymrs_rollout_transitions and the calls from before them) -----
// The two buffers of a gymrs_transitions_desc as the transitions kernels get them by value, after the source's arguments.  Rows are
// RolloutArgs::rec_stride lanes apart, like the record's.
struct TransitionArgs {
    float* final_obs; // [n_steps][obs_dim][rec_stride]: written where a step re-armed a lane, nowhere else
    float* start_obs; // [obs_dim][rec_stride] or NULL
};
constexpr uint32_t kMaxFitnessSteps = GYMRS_POLICY_FITNESS_MAX_STEPS;
// One closed-loop launch: launch_rollout with the policy set as the action source (r.action_seed / action_t0 / n_actions are not
// read).  Which of the eight kernel families it reaches, and which combinations reach none, is dispatch_closed_loop's decision
// (gymrs_launch.h) over source, fitness != NULL, r.rec_obs != NULL, transitions != NULL, vec and flags.
struct ClosedLoopLaunch {
    int vec;        // lanes per work-item: 4 or 8, 4 with a record
    uint32_t flags; // the engine's flags, with kFlagTable: `consts` is a TableConsts and the TableT instantiations play
    StepArgs a;
    RolloutArgs r;
    const void* consts;
    PolicyArgs p;
    ClosedLoopSource source;
    ExploreArgs explore; // read when source is exploring (the transitions kernel of a greedy launch gets threshold 0: the greedy bits)
    SampleArgs sample;   // read when source is sampling
    // != NULL: the kernel also adds every step's reward / done / truncated of every lane to the record of the lane's policy in
    // fitness[n_policies]: integer atomics, once per wave and launch.  The in-register accumulators are 32 bits wide:
    // r.n_steps <= kMaxFitnessSteps.
    gymrs_policy_fitness* fitness;
    const TransitionArgs* transitions; // != NULL: a record that also keeps final and start observations; engines with GYMRS_AUTO_RESET only
    hipStream_t stream;
};
// hipErrorInvalidValue for what dispatch_closed_loop refuses, for n_steps > kMaxFitnessSteps with fitness, and for transitions
// without final_obs or with rec_stride < n (every store is addressed inside a row of rec_stride lanes: the caller's
// check_trajectory is what makes that safe).  No lanes or no steps: nothing is launched.
hipError_t launch_closed_loop(gymrs_env_kind kind, const ClosedLoopLaunch& l);
// ---- advantages (gymrs_advantages; gymrs_advantages.hip) -----------------------------------------------------------------------
// S: floats of one critic (the policy layout with one action); 0 for an env kind that takes none
inline uint64_t critic_floats(gymrs_env_kind kind, uint32_t hidden)
{
    const uint64_t d = kind == GYMRS_CARTPOLE ? 4 : 2;
    if (kind != GYMRS_CARTPOLE && kind != GYMRS_MOUNTAIN_CAR) return 0;
    return hidden == 0 ? d + 1 : (uint64_t)hidden * (d + 2) + 1;
}
// A gymrs_advantages_desc as the kernel gets it by value, before the critic set (a PolicyArgs whose stride is critic_floats).
// Rows are `stride` lanes apart (>= n, a multiple of 16), every buffer 16-byte aligned.
struct AdvantageArgs {
    const float* obs;         // [n_steps][obs_dim][stride]; read with a critic only
    const float* reward;      // [n_steps][stride]
    const uint8_t* done;      // [n_steps][stride]
    const uint8_t* truncated; // [n_steps][stride] or NULL
    const float* final_obs;   // [n_steps][obs_dim][stride] or NULL; read on truncated-only steps with a critic
    const float* start_obs;   // [obs_dim][stride]; read with a critic only
    float* advantages;        // [n_steps][stride]
    float* returns;           // [n_steps][stride] or NULL
    float* values;            // [n_steps][stride] or NULL
    uint64_t stride, n, gid0;
    uint32_t n_steps;
    float gamma, gl; // gl = gamma * lambda, one multiply on the host
    uint32_t pad_;
};
// critic == NULL: V = +0.0f everywhere (no observation is read)
hipError_t launch_advantages(gymrs_env_kind kind, const AdvantageArgs& a, const PolicyArgs* critic, hipStream_t stream);
// ---- gradients (gymrs_policy_gradient; gymrs_gradient.hip) ---------------------------------------------------------------------
// A gymrs_gradient_desc as the kernel gets it by value, before the set (the policy's PolicyArgs, or the critic's).  Rows are
// `stride` lanes apart (>= n, a multiple of 16) and 16-byte aligned; grad and excluded are 8-byte aligned and ADDED to.
struct GradientArgs {
    const float* obs;             // [n_steps][obs_dim][stride]; rows 0 .. n_steps - 2 are read
    const uint8_t* actions;       // [n_steps][stride]; policy head only
    const float* start_obs;       // [obs_dim][stride]
    const float* coef;            // [n_steps][stride]
    float* prob;                  // [n_steps][stride] or NULL; policy head only
    unsigned long long* grad;     // [n_sets][S], S = the set's PolicyArgs::stride
    unsigned long long* excluded; // [n_sets]
    uint64_t stride, n, gid0;
    uint32_t n_steps;
    float scale; // policy head only
};
// critic: p is the critic set (one output, `actions`, `prob` and `scale` unused), else the policy set
hipError_t launch_policy_gradient(gymrs_env_kind kind, bool critic, const GradientArgs& a, const PolicyArgs& p, hipStream_t stream);
// ---- clipped surrogate (gymrs_ppo_gradient; gymrs_gradient_ppo.hip) ------------------------------------------------------------
// A gymrs_ppo_desc as the kernel gets it: the policy head's GradientArgs with the advantages row in the `coef` slot, and what the
// coefficient is computed from.  counts is 8-byte aligned and ADDED to; old_prob is a row like coef.
struct PpoArgs {
    GradientArgs g;
    const float* old_prob;      // [n_steps][stride]
    unsigned long long* counts; // [n_sets][2] or NULL
    float clip_low, clip_high;
};
hipError_t launch_ppo_gradient(gymrs_env_kind kind, const PpoArgs& a, const PolicyArgs& p, hipStream_t stream);
} // namespace gymrs
