// gymrs_engine.hip — host side of the C ABI (include/gymrs_amd.h): owns the SoA device buffers,
// the HIP stream and the engine tick; every entry point cites the reference interface it
// replaces in the header.  No CPU fallback exists: without a HIP device every call fails loudly.
// A per-step launch has ONE submission sequence, whoever submits it: prepare_step (flags, hints, StepArgs, the reset-log ring)
// and record_step (what the engine remembers once it is submitted); the decisions in it that need no device are
// gymrs_step_plan.h's.  The fused rollouts take a RolloutRequest that their entry points validate and fill.
#include "gymrs_engine_priv.h"

// ---------------------------------------------------------------------------------------------
static thread_local std::string g_last_error;

gymrs_status fail(gymrs_status st, const std::string& msg)
{
    g_last_error = msg;
    return st;
}


// The engine that launched the last per-step kernel on each device.  An engine that takes over from ANOTHER one finds its
// arrays pushed out of the Infinity Cache, and launches with the non-temporal hint bring them back only slowly (6.9 instead
// of 6.45 us per 2^20-lane CartPole step for ~4000 steps, profiles/r02_mall_residency.log): its first launch after the
// take-over uses plain, allocating accesses once.  (Periodically doing so for one engine costs more than it brings.)
constexpr int kMaxDevices = 64;
static std::atomic<const gymrs_engine*> g_last_stepper[kMaxDevices];
// Consecutive per-step launches of g_last_stepper: the plain "install" launch is only worth it when the other engine ran long
// enough to have pushed this one's arrays out of the cache.  Engines stepped alternately (train + eval, several shards
// per GPU) keep their hints (they used to lose the non-temporal hint on EVERY launch).
static std::atomic<uint32_t> g_stepper_run[kMaxDevices];
constexpr uint32_t kTakeOverAfter = 64;

static size_t action_size(gymrs_env_kind kind) { return kind == GYMRS_PENDULUM ? sizeof(float) : sizeof(uint8_t); }

constexpr uint64_t kHostPoolMaxLanes = 64;

static uint64_t os_entropy()
{
    // seeding.rs:22 `thread_rng().gen()`: a fresh seed from the OS
    std::random_device rd;
    return ((uint64_t)rd() << 32) ^ (uint64_t)rd();
}

// The flags of a per-step launch before the take-over and the time-limit elision have had their say (hint_bits, gymrs_step_plan.h).
static uint32_t launch_flags_of(const gymrs_engine* e)
{
    return e->flags | hint_bits(e->nt_mode, bytes_per_step(e->kind, e->state_dim, e->n), /*chain=*/false) | table_bit(e);
}

// Pendulum under GYMRS_TIME_LIMIT: every lane's episode clock is the host's (gymrs_step_plan.h)
static bool has_uniform_clock(const gymrs_engine* e) { return e->kind == GYMRS_PENDULUM && (e->flags & GYMRS_TIME_LIMIT); }

static StepArgs step_args(const gymrs_engine* e, const void* actions)
{
    StepArgs a;
    std::memset(&a, 0, sizeof(a));
    for (int j = 0; j < 4; ++j) a.s[j] = e->s[j];
    a.obs_cos = e->obs_cos;
    a.obs_sin = e->obs_sin;
    a.action = actions;
    a.reward = e->reward;
    a.done = e->done;
    a.truncated = e->truncated;
    a.beyond = e->beyond;
    a.ep_start = e->ep_start;
    if (e->final_obs) a.final_obs = e->final_obs; // (GYMRS_FINAL_OBS needs auto-reset: no launch of such an engine reads `beyond`)
    a.wave_open = e->wave_open;
    a.wave_clean = e->wave_clean;
    a.block_stats = e->block_stats;
    a.reset_log = e->reset_log;
    a.reset_log_row_words = e->log_row_words;
    a.fold_step = 0;
    a.elide_reward = e->elide_reward ? 1u : 0u;
    a.div_in_range = (e->kind == GYMRS_CARTPOLE && div_in_range_ok(e->consts.cp)) ? 1u : 0u; // (a table launch never reads it: TableT divides with `/`)
    a.err = e->err;
    a.err_seen = e->err_seen_dev;
    a.n = e->n;
    // the vector load of a work-item's actions needs vec * sizeof(action) alignment; any other address is read lane by
    // lane (n_fast = 0 sends every wavefront through the guarded code)
    a.n_fast = (reinterpret_cast<uintptr_t>(actions) % ((size_t)e->vec * action_size(e->kind)) == 0) ? e->n : 0;
    a.gid0 = e->gid0;
    a.seed = e->seed;
    a.tick = e->tick;
    a.box = make_sample_box(e->lo, e->hi, e->state_dim);
    a.truncate_all = (has_uniform_clock(e) && uniform_clock_hits(e->tick, e->uniform_start, e->max_steps)) ? 1u : 0u;
    a.skip_trunc_store = (e->kind == GYMRS_PENDULUM && e->trunc_held == (int)a.truncate_all) ? 1u : 0u;
    a.trace = e->trace;
    a.trace_wpb = (uint32_t)step_threads_of(e->kind, e->n, e->vec) / 64u;
    return a;
}

StatsArgs stats_args(const gymrs_engine* e)
{
    StatsArgs a;
    a.ep_start = e->ep_start;
    a.n = e->n;
    a.epoch = e->epoch;
    a.tick = e->tick;
    a.block_stats = e->block_stats;
    a.n_blocks = e->n_stat_blocks;
    a.partials = e->stats_acc;
    a.base = e->stats_base;
    a.log = e->reset_log;
    a.log_row_words = e->log_row_words;
    a.log_pending = e->reset_log ? e->log_pending : 0u;
    a.log_first_tick = e->log_first_tick;
    a.log_vec = e->log_vec;
    a.track = (e->flags & GYMRS_TRACK_STATS) != 0;
    a.reward_sign = e->kind == GYMRS_CARTPOLE ? 1 : (e->kind == GYMRS_MOUNTAIN_CAR ? -1 : 0);
    a.n_steps = e->n_steps_total;
    a.out4 = e->stats_dev;
    a.host_out4 = e->stats_host_dev;
    return a;
}

// A chain of per-step launches (gymrs_aql.h) runs on the engine's own queue; until it is closed the engine's HIP stream is not
// held back, and what the chain wrote may still sit dirty in the L2s.  Whatever the host side of a step has to put on the
// stream in mid-call -- the stand-alone fold of the reset log, a refresh of the time-limit bound, the memset of `truncated` --
// therefore first closes the open chain (release + hand-over); step_many_aql opens the next one behind it.
static gymrs_status stream_op_barrier(gymrs_engine* e)
{
    if (!e->chain_open) return GYMRS_OK;
    e->chain_open = false;
    std::string err;
    if (!aql_end(e->aql, e->stream, &err)) return fail(GYMRS_EHIP, "AQL dispatcher: " + err);
    e->aql_chains += 1;
    return GYMRS_OK;
}

// ---- reset log bookkeeping (host side; the ring's invariant and its step: gymrs_step_plan.h) -----------------------------------
// Fold the pending rows now, with the stand-alone kernel: before anything reads ep_start or the episode counters
// (statistics, snapshot, clone, the rollout kernel) and when the launch shape changes.
gymrs_status fold_reset_log(gymrs_engine* e)
{
    if (!e->reset_log || e->log_pending == 0) return GYMRS_OK;
    if (gymrs_status st = stream_op_barrier(e)) return st;
    HIP_TRY(launch_fold_reset_log(e->reset_log, e->log_row_words, e->log_first_tick, e->log_pending, e->log_vec, e->ep_start, e->n,
                                  e->block_stats, e->stream));
    e->log_pending = 0;
    return GYMRS_OK;
}

// Does a launch with these flags keep its episode bookkeeping in the reset log?  (= TileRegs<CartPoleT, ..>::LOGGED)
static bool launch_is_logged(const gymrs_engine* e, uint32_t flags)
{
    return e->reset_log && (flags & GYMRS_TRACK_STATS) && (flags & GYMRS_AUTO_RESET) && !(flags & GYMRS_TIME_LIMIT);
}

// About to launch ONE per-step kernel at the engine's current tick: the HIP side of reset_log_step.  *fold = StepArgs::fold_step.
static gymrs_status log_before_step(gymrs_engine* e, uint32_t flags, uint32_t* fold)
{
    *fold = 0;
    if (!e->reset_log) return GYMRS_OK;
    const ResetLogStep s = reset_log_step({e->log_pending, e->log_first_tick, e->log_vec}, launch_is_logged(e, flags), e->tick, e->vec);
    if (s.fold_first)
        if (gymrs_status st = fold_reset_log(e)) return st;
    e->log_pending = s.after.pending;
    e->log_first_tick = s.after.first_tick;
    e->log_vec = s.after.vec;
    *fold = s.fold_step;
    return GYMRS_OK;
}

// ---- GYMRS_TIME_LIMIT elision (host side) -----------------------------------------------------------------------------
static uint32_t limit_of(const gymrs_engine* e) { return e->consts.cp.max_steps; } // elidable engines are CartPole

// What is known about every lane's episode clock after something rewrote ep_start wholesale (reset: all start at
// `bound`; snapshot load: nothing, bound = 0 makes the next launches keep the limit until a refresh has come back).
void limit_restart(gymrs_engine* e, uint64_t bound, bool trunc_zero)
{
    e->start_bound = bound;
    e->trunc_zero = trunc_zero;
    e->age_pending = false; // a refresh still in flight measured another episode clock: its result is never adopted
    e->age_gave_up = false;
    e->age_near_done = false;
    e->last_elided = false;
    e->age_next_refresh = 0;
    e->age_backoff = 8;
}

// Wait -- for a BOUNDED time -- until the refresh in flight has published its result (mapped host memory; the device writes
// the age, then the sequence number).  A caller that waits for every step finds it there; one that queues launches far
// ahead of the GPU waits here until the GPU has caught up with the refresh, which caps its lead.  *arrived = false when the
// answer is not there after kAgeWaitNs: the caller then launches the kernel WITH the limit, which is always correct
// (a caller-provided stream may be blocked on work this very thread has not submitted yet -- an event it
// records later, a capture -- and an unbounded spin would never end).
constexpr uint64_t kAgeWaitNs = 2'000'000;        // a caller-provided stream (it may be blocked on work nobody has submitted yet): ~300 headline launches
constexpr uint64_t kAgeWaitOwnNs = 200'000'000;   // the engine's own stream always drains: long enough for a whole chain segment (the host runs
                                                  // thousands of launches ahead of the device inside a chain), short enough to notice a dead device
static gymrs_status wait_for_age(gymrs_engine* e, bool* arrived)
{
    const auto t0 = std::chrono::steady_clock::now();
    *arrived = true;
    for (uint64_t spins = 0; e->age_host[1] != e->age_seq; ++spins) {
        if ((spins & 0xfffu) == 0xfffu) { // every few microseconds: is the stream still alive, is there time left?
            const hipError_t q = hipStreamQuery(e->stream);
            if (q != hipSuccess && q != hipErrorNotReady) return fail(GYMRS_EHIP, std::string("time-limit refresh: ") + hipGetErrorString(q));
            if (q == hipSuccess && e->age_host[1] != e->age_seq)
                return fail(GYMRS_EHIP, "time-limit refresh: the stream is idle but the result never arrived");
            if ((uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count() >
                (e->own_stream ? kAgeWaitOwnNs : kAgeWaitNs)) {
                *arrived = false;
                return GYMRS_OK;
            }
        }
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    return GYMRS_OK;
}

// Is the engine's stream under a capture this library did not start?  Only a caller-provided stream can be.  1 = yes, 0 = no,
// -1 = the query itself failed: each caller then keeps to its safe side (the elision stays on, chains stay off).
static int stream_capturing(const gymrs_engine* e)
{
    if (e->own_stream) return 0;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(e->stream, &cs) != hipSuccess) return -1;
    return cs != hipStreamCaptureStatusNone ? 1 : 0;
}

// The elision is off when GYMRS_NO_LIMIT_ELISION=1 is in the environment (every launch checks the limit, as in round 1), and
// for launches into a stream that is being captured (what is baked into a graph cannot follow start_bound).
static bool elision_disabled(const gymrs_engine* e)
{
    static const bool off = [] {
        const char* v = std::getenv("GYMRS_NO_LIMIT_ELISION");
        return v && v[0] == '1';
    }();
    return off || stream_capturing(e) == 1;
}

// About to submit a per-step launch: note who steps on the device.  Returns `flags`, without the hint bits when this launch is
// the plain "install" launch after a take-over (see g_last_stepper).
static uint32_t take_over_device(gymrs_engine* e, uint32_t flags)
{
    if (e->device < 0 || e->device >= kMaxDevices) return flags;
    const gymrs_engine* prev = g_last_stepper[e->device].exchange(e, std::memory_order_relaxed);
    if (prev == e) {
        g_stepper_run[e->device].fetch_add(1, std::memory_order_relaxed);
        return flags;
    }
    const uint32_t run = g_stepper_run[e->device].exchange(1, std::memory_order_relaxed);
    // taking over the device from an engine that ran for a while (or first launch): install the lines
    if ((prev == nullptr || run >= kTakeOverAfter) && e->nt_mode == 0) flags &= ~kFlagHintMask;
    return flags;
}

// The time limit of ONE per-step launch at the engine's current tick: *io = the launch's flags, on return without
// GYMRS_TIME_LIMIT where no lane can reach the limit.  A step takes a lane to the limit iff
// tick + 1 - ep_start >= max_steps (advance_tile); with ep_start >= start_bound for every lane, none can while
// tick + 1 - start_bound < max_steps.  start_bound comes from max_age_kernel, launched
//   * once per approach, `margin` launches before the bound would expire -- under a policy whose episodes end long before
//     the limit (random CartPole: the oldest of 2^20 open episodes is a few hundred steps old) the result moves the bound on
//     and the limit is never checked;
//   * while the limit IS reachable: right after the first launch that checked it (if that launch truncated the few old
//     episodes there were, the refresh behind it says so and the launches go on without the limit), then at a doubling
//     distance up to 256 launches (a policy that keeps lanes alive up to the limit pays one 4 MB reduction and one
//     drained queue per 256 steps).
static gymrs_status elide_time_limit(gymrs_engine* e, uint32_t* io)
{
    if (!e->limit_elidable) return GYMRS_OK;
    if (elision_disabled(e)) {
        e->trunc_zero = false;
        e->last_elided = false;
        return GYMRS_OK;
    }
    const uint64_t limit = limit_of(e);
    const uint64_t margin = limit / 4 < 16 ? limit / 4 : 16;
    auto adopt = [e]() {
        e->age_pending = false;
        e->age_gave_up = false;
        const uint64_t bound = e->age_ref_tick - (uint64_t)e->age_host[0];
        if (bound > e->start_bound) e->start_bound = bound;
    };
    if (e->age_pending && e->age_host[1] == e->age_seq) { // one load from host memory per launch, no runtime call
        std::atomic_thread_fence(std::memory_order_acquire);
        adopt();
    }
    if (e->age_pending && !e->age_gave_up && e->tick + 1 - e->start_bound >= limit) { // the answer decides THIS launch
        if (gymrs_status st = stream_op_barrier(e)) return st; // (the refresh sits on the stream BEHIND the open chain's hand-over)
        const auto t0 = std::chrono::steady_clock::now();
        bool arrived = false;
        if (gymrs_status st = wait_for_age(e, &arrived)) return st;
        e->age_waits += 1;
        e->age_wait_ns += (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
        if (arrived) adopt();
        else e->age_gave_up = true; // the bound stays stale, `reachable` below is true and this launch checks the limit itself
    }
    const uint64_t oldest = e->tick + 1 - e->start_bound; // no episode is older than this after the step
    const bool reachable = oldest >= limit, near = oldest + margin >= limit;
    if (!near) e->age_near_done = false;
    bool refresh = false;
    if (!e->age_pending) {
        if (reachable) {
            if (e->last_elided) { // first launch that has to check the limit: look again BEHIND it
                e->age_next_refresh = e->tick + 1;
                e->age_backoff = 8;
            } else if (e->tick >= e->age_next_refresh) {
                refresh = true;
                e->age_next_refresh = e->tick + e->age_backoff;
                e->age_backoff = e->age_backoff < 256 ? e->age_backoff * 2 : 256;
            }
        } else if (near && !e->age_near_done) {
            refresh = true;
            e->age_near_done = true;
        }
    }
    if (refresh) {
        if (gymrs_status st = stream_op_barrier(e)) return st;
        e->age_seq += 1;
        HIP_TRY(launch_max_age(e->ep_start, e->n, (uint32_t)e->tick, e->age_dev, e->age_host_dev, e->age_seq, e->stream));
        e->age_pending = true;
        e->age_ref_tick = e->tick;
        e->age_refreshes += 1;
    }
    if (!reachable) {
        *io &= ~(uint32_t)GYMRS_TIME_LIMIT;
        if (!e->trunc_zero) { // the last launch with the limit may have left ones behind
            if (gymrs_status st = stream_op_barrier(e)) return st;
            HIP_TRY(hipMemsetAsync(e->truncated, 0, (size_t)e->n, e->stream));
            e->trunc_zero = true;
        }
        e->limit_elided_launches += 1;
    } else {
        e->trunc_zero = false;
    }
    e->last_elided = !reachable;
    return GYMRS_OK;
}

template <class T>
static gymrs_status dev_alloc(T** p, size_t count)
{
    void* q = nullptr;
    hipError_t err = hipMalloc(&q, (count ? count : 1) * sizeof(T));
    if (err != hipSuccess) return fail(err == hipErrorOutOfMemory ? GYMRS_ENOMEM : GYMRS_EHIP, std::string("hipMalloc: ") + hipGetErrorString(err));
    *p = static_cast<T*>(q);
    return GYMRS_OK;
}

// A zeroed block of mapped, coherent host memory and the device's address of it.  On failure nothing is left allocated.
template <class H, class D>
static hipError_t mapped_host_block(size_t bytes, H** host, D** dev)
{
    void *h = nullptr, *d = nullptr;
    hipError_t err = hipHostMalloc(&h, bytes, hipHostMallocMapped | hipHostMallocCoherent);
    if (err == hipSuccess) err = hipHostGetDevicePointer(&d, h, 0);
    if (err != hipSuccess) {
        if (h) (void)hipHostFree(h);
        return err;
    }
    std::memset(h, 0, bytes);
    *host = static_cast<H*>(h);
    *dev = static_cast<D*>(d);
    return hipSuccess;
}

// ---------------------------------------------------------------------------------------------
extern "C" {

const char* gymrs_last_error(void) { return g_last_error.c_str(); }
int gymrs_abi_version(void) { return GYMRS_ABI_VERSION; }

int gymrs_discrete_contains(uint64_t n, uint64_t value) { return value < n; } // discrete.rs:14-19

gymrs_status gymrs_default_params(gymrs_env_kind kind, void* params)
{
    if (!params) return fail(GYMRS_EINVAL, "gymrs_default_params: params is NULL");
    switch (kind) {
    case GYMRS_CARTPOLE: {
        auto* p = static_cast<gymrs_cartpole_params*>(params);
        p->gravity = 9.8;
        p->masscart = 1.0;
        p->masspole = 0.1;
        p->length = 0.5;
        p->force_mag = 10.0;
        p->tau = 0.02;
        p->theta_threshold_radians = 12. * 2. * 3.14159265358979323846 / 360.;
        p->x_threshold = 2.4;
        p->kinematics_integrator = 0;
        p->max_episode_steps = 500;
        return GYMRS_OK;
    }
    case GYMRS_MOUNTAIN_CAR: {
        auto* p = static_cast<gymrs_mountain_car_params*>(params);
        p->min_position = -1.2;
        p->max_position = 0.6;
        p->max_speed = 0.07;
        p->goal_position = 0.5;
        p->goal_velocity = 0.;
        p->force = 0.001;
        p->gravity = 0.0025;
        p->max_episode_steps = 200;
        p->_pad = 0;
        return GYMRS_OK;
    }
    case GYMRS_PENDULUM: {
        auto* p = static_cast<gymrs_pendulum_params*>(params);
        p->max_speed = 8.;
        p->max_torque = 2.;
        p->dt = 0.05;
        p->g = 10.;
        p->m = 1.;
        p->l = 1.;
        p->max_episode_steps = 200;
        p->_pad = 0;
        return GYMRS_OK;
    }
    }
    return fail(GYMRS_EINVAL, "gymrs_default_params: unknown env kind");
}

gymrs_status gymrs_action_space(gymrs_env_kind kind, uint32_t* n, double* box_low, double* box_high)
{
    if (!n) return fail(GYMRS_EINVAL, "gymrs_action_space: n is NULL");
    switch (kind) {
    case GYMRS_CARTPOLE: *n = 2; break;     // cartpole.rs:114
    case GYMRS_MOUNTAIN_CAR: *n = 3; break; // mountain_car.rs:362
    case GYMRS_PENDULUM:
        *n = 0;
        if (box_low) *box_low = -2.0;
        if (box_high) *box_high = 2.0;
        break;
    default: return fail(GYMRS_EINVAL, "gymrs_action_space: unknown env kind");
    }
    return GYMRS_OK;
}

gymrs_status gymrs_observation_space(gymrs_env_kind kind, const void* params, double* low, double* high, int* dim)
{
    if (!low || !high || !dim) return fail(GYMRS_EINVAL, "gymrs_observation_space: NULL output");
    const double inf = std::numeric_limits<double>::infinity();
    switch (kind) {
    case GYMRS_CARTPOLE: {
        gymrs_cartpole_params d;
        gymrs_default_params(kind, &d);
        const auto* p = params ? static_cast<const gymrs_cartpole_params*>(params) : &d;
        // cartpole.rs:105-113: high = (2*x_thr, inf, 2*theta_thr, inf), low = -high
        high[0] = p->x_threshold * 2.;
        high[1] = inf;
        high[2] = p->theta_threshold_radians * 2.;
        high[3] = inf;
        for (int j = 0; j < 4; ++j) low[j] = -high[j];
        *dim = 4;
        return GYMRS_OK;
    }
    case GYMRS_MOUNTAIN_CAR: {
        gymrs_mountain_car_params d;
        gymrs_default_params(kind, &d);
        const auto* p = params ? static_cast<const gymrs_mountain_car_params*>(params) : &d;
        // mountain_car.rs:353-354
        low[0] = p->min_position;
        low[1] = -p->max_speed;
        high[0] = p->max_position;
        high[1] = p->max_speed;
        *dim = 2;
        return GYMRS_OK;
    }
    case GYMRS_PENDULUM: {
        gymrs_pendulum_params d;
        gymrs_default_params(kind, &d);
        const auto* p = params ? static_cast<const gymrs_pendulum_params*>(params) : &d;
        low[0] = -1.;
        low[1] = -1.;
        low[2] = -p->max_speed;
        high[0] = 1.;
        high[1] = 1.;
        high[2] = p->max_speed;
        *dim = 3;
        return GYMRS_OK;
    }
    }
    return fail(GYMRS_EINVAL, "gymrs_observation_space: unknown env kind");
}

// How gymrs_step_many submits its launches (GYMRS_AQL, looked up per call).  DEFAULT (unset, "0"): HIP launches on the engine's stream -- the submission
// that has never produced a wrong result, and the only one the headline is measured on.  "1" OPTS IN to chains: the engine's own HSA queue, agent-scope
// acquire on every launch, one release at the end (gymrs_aql.h) -- 25 % faster per launch at 2^20 CartPole lanes, reported separately.  "2": the engine's queue
// with HIP's OWN packet header (acquire + RELEASE on every launch) and the memory hints HIP launches use: the per-step-visible shape without the HIP
// runtime's 2.5-4 us of host time per launch.
// Why opt-in (round 6; VERDICT r5 "next" #1d): round 5 ended with an unexplained wrong episode counter in a run that used chains (3 occurrences in ~450 runs
// of 8 processes sharing a GPU).  Round 6 could not reproduce it -- 0 wrong counts in > 10^6 chain hand-overs under tools/handover_amp.py, 0 in 2176 cold
// process starts under tools/coldstart_amp.py -- and therefore cannot name its cause; an unexplained fast path is not a default.  An engine created without the
// opt-in sets up no HSA queue, runs no self-check and no hand-over calibration: first contact with a device is one HSA-free code path.
static int aql_mode_by_env()
{
    const char* v = std::getenv("GYMRS_AQL");
    return (v && v[0] == '1') ? 1 : ((v && v[0] == '2') ? 2 : 0);
}
static bool aql_enabled_by_env() { return aql_mode_by_env() != 0; }

// ---------------------------------------------------------------------------------------------
gymrs_status gymrs_engine_destroy(gymrs_engine* e)
{
    if (!e) return GYMRS_OK;
    (void)hipSetDevice(e->device);
    const bool idle = !e->stream || hipStreamSynchronize(e->stream) == hipSuccess;
    comm_destroy(e);
    // parked for the next engine of the device only when the stream really is idle (every chain ended with a wait on it) and no chain is open
    aql_destroy(e->aql, /*discard=*/!idle || e->chain_open || (e->err_seen && e->err_seen[1] != 0));
    if (e->device >= 0 && e->device < kMaxDevices) { // a later engine at the same address must not pass for this one
        const gymrs_engine* self = e;
        g_last_stepper[e->device].compare_exchange_strong(self, nullptr, std::memory_order_relaxed);
    }
    if (e->pool_host)
        (void)hipHostFree(e->pool_host);
    else
        (void)hipFree(e->pool); // all per-lane arrays
    (void)hipFree(e->block_stats);
    (void)hipFree(e->reset_log);
    (void)hipFree(e->age_dev);
    if (e->age_host) (void)hipHostFree(const_cast<uint32_t*>(e->age_host));
    (void)hipFree(e->wave_open);
    (void)hipFree(e->wave_clean);
    (void)hipFree(e->err);
    (void)hipFree(e->table_dev);
    (void)hipFree(e->param_index);
    (void)hipFree(e->policy.dev);
    (void)hipFree(e->critic.dev);
    (void)hipFree(e->fitness_dev);
    (void)hipFree(e->eval_dev);
    if (e->err_seen) (void)hipHostFree(const_cast<uint32_t*>(e->err_seen));
    if (e->graph_exec) (void)hipGraphExecDestroy(e->graph_exec);
    (void)hipFree(e->tick_dev);
    (void)hipFree(e->stats_dev);
    if (e->stats_host) (void)hipHostFree(const_cast<double*>(e->stats_host));
    (void)hipFree(e->stats_acc);
    (void)hipFree(e->stats_base);
    if (e->staging_host)
        (void)hipHostFree(e->staging_host);
    else
        (void)hipFree(e->action_staging);
    if (e->own_stream && e->stream) (void)hipStreamDestroy(e->stream);
    delete e;
    return GYMRS_OK;
}

gymrs_status gymrs_engine_create(gymrs_env_kind kind, uint64_t n_envs, uint64_t global_env_offset, int device,
                                 const void* params, uint32_t flags, gymrs_engine** out)
{
    if (!out) return fail(GYMRS_EINVAL, "gymrs_engine_create: out is NULL");
    *out = nullptr;
    if (kind != GYMRS_CARTPOLE && kind != GYMRS_MOUNTAIN_CAR && kind != GYMRS_PENDULUM)
        return fail(GYMRS_EINVAL, "gymrs_engine_create: unknown env kind");
    if (gymrs_status st = check_params(kind, params, "gymrs_engine_create")) return st;
    if (n_envs == 0) return fail(GYMRS_EINVAL, "gymrs_engine_create: n_envs must be > 0");
    if (n_envs > (1ull << 32)) return fail(GYMRS_EINVAL, "gymrs_engine_create: n_envs must be <= 2^32 per engine");
    if (flags & ~(uint32_t)(GYMRS_AUTO_RESET | GYMRS_TRACK_STATS | GYMRS_TIME_LIMIT | GYMRS_FINAL_OBS))
        return fail(GYMRS_EINVAL, "gymrs_engine_create: unknown flag bits");
    if ((flags & GYMRS_TRACK_STATS) && !(flags & GYMRS_AUTO_RESET))
        return fail(GYMRS_EINVAL, "gymrs_engine_create: GYMRS_TRACK_STATS needs GYMRS_AUTO_RESET");
    if ((flags & GYMRS_FINAL_OBS) && !(flags & GYMRS_AUTO_RESET))
        return fail(GYMRS_EINVAL, "gymrs_engine_create: GYMRS_FINAL_OBS needs GYMRS_AUTO_RESET");
    int n_dev = 0;
    hipError_t derr = hipGetDeviceCount(&n_dev);
    if (derr != hipSuccess || n_dev <= 0)
        return fail(GYMRS_EHIP, std::string("gymrs_engine_create: no HIP device available (") +
                                    (derr != hipSuccess ? hipGetErrorString(derr) : "device count 0") +
                                    "); this library has no CPU fallback");
    if (device < 0 || device >= n_dev) return fail(GYMRS_EINVAL, "gymrs_engine_create: device index out of range");
    HIP_TRY(hipSetDevice(device));

    gymrs_engine* e = new (std::nothrow) gymrs_engine();
    if (!e) return fail(GYMRS_ENOMEM, "gymrs_engine_create: host allocation failed");
    e->kind = kind;
    e->n = n_envs;
    e->gid0 = global_env_offset;
    e->device = device;
    e->flags = flags;
    switch (kind) {
    case GYMRS_CARTPOLE: {
        gymrs_cartpole_params d;
        gymrs_default_params(kind, &d);
        e->params.cp = params ? *static_cast<const gymrs_cartpole_params*>(params) : d;
        e->consts.cp = make_consts(e->params.cp);
        e->state_dim = 4;
        e->obs_dim = 4;
        for (int j = 0; j < 4; ++j) { // cartpole.rs:353-361
            e->dflt_lo[j] = -0.05f;
            e->dflt_hi[j] = 0.05f;
        }
        break;
    }
    case GYMRS_MOUNTAIN_CAR: {
        gymrs_mountain_car_params d;
        gymrs_default_params(kind, &d);
        e->params.mc = params ? *static_cast<const gymrs_mountain_car_params*>(params) : d;
        e->consts.mc = make_consts(e->params.mc);
        e->state_dim = 2;
        e->obs_dim = 2;
        e->dflt_lo[0] = -0.6f; // mountain_car.rs:176-187
        e->dflt_hi[0] = -0.4f;
        break;
    }
    case GYMRS_PENDULUM: {
        gymrs_pendulum_params d;
        gymrs_default_params(kind, &d);
        e->params.pd = params ? *static_cast<const gymrs_pendulum_params*>(params) : d;
        const auto& p = e->params.pd;
        e->consts.pd = make_consts(p);
        e->max_steps = e->consts.pd.max_steps;
        e->max_torque = (float)p.max_torque;
        e->state_dim = 2;
        e->obs_dim = 3;
        e->dflt_lo[0] = -kPiF;
        e->dflt_hi[0] = kPiF;
        e->dflt_lo[1] = -1.0f;
        e->dflt_hi[1] = 1.0f;
        break;
    }
    }
    std::memcpy(e->lo, e->dflt_lo, sizeof(e->lo));
    std::memcpy(e->hi, e->dflt_hi, sizeof(e->hi));

    gymrs_status st = GYMRS_OK;
    auto chk = [&](gymrs_status s_) {
        if (st == GYMRS_OK) st = s_;
    };
    // Arrays are padded to a multiple of 16 lanes so the last vector access of the engine's own
    // arrays stays inside the allocation; the caller's action buffer is never read past n.
    const size_t npad = (size_t)((n_envs + 15) & ~15ull);
    // All per-lane arrays live in ONE allocation, each array start skewed by a different odd multiple of
    // `skew` bytes.  With separate power-of-two sized allocations (2^20 lanes = exactly 4 MiB per f32 array)
    // lane i of every array maps to the same memory channel / cache set and a wave's 5 loads and 6 stores
    // pile onto it (measured: 7.7 us per launch at 2^20 lanes against 7.1 us per 2^20 at 1.5 * 2^20).
    {
        constexpr size_t skew = 4352; // 4 KiB + 256 B (other skews: profiles/r04_array_skew.log)
        size_t off = 0;
        int index = 0;
        auto place = [&](size_t bytes) {
            const size_t at = off + (size_t)index * skew;
            ++index;
            off = (at + bytes + 255) & ~(size_t)255;
            return at;
        };
        size_t at_s[4] = {0, 0, 0, 0}, at_cos = 0, at_sin = 0;
        for (int j = 0; j < e->state_dim; ++j) at_s[j] = place(npad * 4);
        const bool pend = kind == GYMRS_PENDULUM;
        if (pend) {
            at_cos = place(npad * 4);
            at_sin = place(npad * 4);
        }
        const size_t at_reward = place(npad * 4), at_done = place(npad), at_trunc = place(npad), at_beyond = place(npad),
                     at_start = place(npad * 4);
        // GYMRS_FINAL_OBS: placed last, so that every other array lies where it lies without the flag
        const size_t at_final = (flags & GYMRS_FINAL_OBS) ? place((size_t)final_obs_stride(n_envs) * 4 * e->obs_dim) : 0;
        void* pool = nullptr;
        hipError_t perr;
        if (n_envs <= kHostPoolMaxLanes)
            perr = mapped_host_block(off + 256, &e->pool_host, &pool);
        else
            perr = hipMalloc(&pool, off + 256);
        if (perr != hipSuccess) {
            delete e;
            return fail(perr == hipErrorOutOfMemory ? GYMRS_ENOMEM : GYMRS_EHIP, std::string("hipMalloc: ") + hipGetErrorString(perr));
        }
        e->pool = pool;
        e->pool_bytes = off + 256;
        char* b = static_cast<char*>(pool);
        for (int j = 0; j < e->state_dim; ++j) e->s[j] = reinterpret_cast<float*>(b + at_s[j]);
        if (pend) {
            e->obs_cos = reinterpret_cast<float*>(b + at_cos);
            e->obs_sin = reinterpret_cast<float*>(b + at_sin);
        }
        e->reward = reinterpret_cast<float*>(b + at_reward);
        e->done = reinterpret_cast<uint8_t*>(b + at_done);
        e->truncated = reinterpret_cast<uint8_t*>(b + at_trunc);
        e->beyond = reinterpret_cast<uint8_t*>(b + at_beyond);
        e->ep_start = reinterpret_cast<uint32_t*>(b + at_start);
        if (flags & GYMRS_FINAL_OBS) e->final_obs = reinterpret_cast<float*>(b + at_final);
    }
    // one statistics slot per wavefront: most waves at 4 lanes per work-item (256 lanes per wave), rounded up to whole
    // workgroups of up to 16 waves
    e->n_stat_blocks = (uint32_t)((((n_envs + 255) / 256) + 15) / 16 * 16);
    chk(dev_alloc(&e->block_stats, (size_t)e->n_stat_blocks * 2));
    // with all three flags a launch drops the time limit whenever no lane can reach it (elide_time_limit)
    constexpr uint32_t kAllThree = GYMRS_AUTO_RESET | GYMRS_TRACK_STATS | GYMRS_TIME_LIMIT;
    // CartPole only: there the launch without the limit is the reset-logged kernel (6.5 vs 6.7-6.9 us at 2^20 lanes).  For
    // MountainCar it would only spare the dense ep_start read, and under a random policy every lane is truncated in the
    // same step every 200 steps: the two refreshes and two exact launches per cycle cost what the 198 others gain.
    e->limit_elidable = kind == GYMRS_CARTPOLE && (flags & kAllThree) == kAllThree;
    // CartPole under auto-reset pays 1.0 on every step (cartpole.rs:455-459), like MountainCar its -1.0: from kElideRewardFromBytes per step on the
    // kernel stops rewriting a wave's part of `reward` while it holds the constant (StepArgs::elide_reward; 8-13 % of the step at 2^22 .. 2^25 lanes,
    // profiles/r04_cartpole_reward_elision.log).  Below that the store stays: it is a wash there, and BASELINE's 2^20-lane configuration moves every
    // byte it is credited with.  (GYMRS_DEV_ELIDE_REWARD=0|1: developer knob, forces it off / on at any size -- the tests' way to reach both paths.)
    {
        constexpr uint64_t kElideRewardFromBytes = 128ull << 20;
        bool on = kind == GYMRS_CARTPOLE && (flags & GYMRS_AUTO_RESET) && bytes_per_step(kind, e->state_dim, n_envs) >= kElideRewardFromBytes;
        if (const char* v = std::getenv("GYMRS_DEV_ELIDE_REWARD"))
            if (kind == GYMRS_CARTPOLE && (flags & GYMRS_AUTO_RESET) && (v[0] == '0' || v[0] == '1')) on = v[0] == '1';
        e->elide_reward = on;
    }
    if ((flags & GYMRS_TRACK_STATS) && (flags & GYMRS_AUTO_RESET) && kind == GYMRS_CARTPOLE &&
        (!(flags & GYMRS_TIME_LIMIT) || e->limit_elidable)) { // launches that are TileRegs<CartPoleT, ..>::LOGGED will happen
        // reset log: kResetLogRows rows of one bit per lane (2^20 lanes: 128 KiB per row)
        e->log_row_words = e->n_stat_blocks * 4;
        chk(dev_alloc(&e->reset_log, (size_t)kResetLogRows * e->log_row_words));
    }
    if (e->limit_elidable) {
        chk(dev_alloc(&e->age_dev, (size_t)kStatsPartials)); // scratch of the refresh: one maximum per workgroup
        if (st == GYMRS_OK && mapped_host_block(2 * sizeof(uint32_t), &e->age_host, &e->age_host_dev) != hipSuccess)
            st = fail(GYMRS_EHIP, "hipHostMalloc (age words)");
    }
    chk(dev_alloc(&e->wave_open, (size_t)e->n_stat_blocks));
    chk(dev_alloc(&e->wave_clean, (size_t)e->n_stat_blocks));
    chk(dev_alloc(&e->err, 2));
    // [0] invalid action seen, [1] a chain launch on the wrong XCD
    if (st == GYMRS_OK && mapped_host_block(2 * sizeof(uint32_t), &e->err_seen, &e->err_seen_dev) != hipSuccess)
        st = fail(GYMRS_EHIP, "hipHostMalloc (error flags)");
    chk(dev_alloc(&e->stats_dev, 4));
    if (st == GYMRS_OK && mapped_host_block(4 * sizeof(double), &e->stats_host, &e->stats_host_dev) != hipSuccess)
        st = fail(GYMRS_EHIP, "hipHostMalloc (statistics read-out)");
    chk(dev_alloc(&e->stats_acc, (size_t)kStatsPartials * 3));
    chk(dev_alloc(&e->stats_base, (size_t)kStatsBaseWords));
    chk(dev_alloc(&e->tick_dev, 1));
    if (st != GYMRS_OK) {
        std::string msg = g_last_error;
        gymrs_engine_destroy(e);
        return fail(st, msg);
    }
    hipError_t serr = hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking);
    if (serr != hipSuccess) {
        gymrs_engine_destroy(e);
        return fail(GYMRS_EHIP, std::string("hipStreamCreate: ") + hipGetErrorString(serr));
    }
    e->own_stream = true;
    static const uint32_t err_init[2] = {0u, 0xffffffffu};
    hipError_t merr = hipMemcpyAsync(e->err, err_init, sizeof(err_init), hipMemcpyHostToDevice, e->stream);
    if (merr == hipSuccess && e->reset_log) merr = hipMemsetAsync(e->reset_log, 0, (size_t)kResetLogRows * e->log_row_words * 8, e->stream);
    if (merr == hipSuccess) merr = hipMemsetAsync(e->truncated, 0, npad, e->stream);
    if (merr == hipSuccess) merr = hipMemsetAsync(e->stats_dev, 0, 4 * sizeof(double), e->stream);
    if (merr != hipSuccess) {
        gymrs_engine_destroy(e);
        return fail(GYMRS_EHIP, std::string("engine init: ") + hipGetErrorString(merr));
    }
    // ::new samples an initial state from an OS seed (cartpole.rs:92,120; mountain_car.rs:342,358)
    st = gymrs_reset(e, 0, 0, nullptr, nullptr);
    if (st == GYMRS_OK) st = gymrs_sync(e);
    if (st != GYMRS_OK) {
        std::string msg = g_last_error;
        gymrs_engine_destroy(e);
        return fail(st, msg);
    }
    // The engine's own AQL dispatcher (chains of gymrs_step_many launches, gymrs_aql.h) is set up HERE, next to the other allocations,
    // and the hand-over is timed on the engine's own, idle stream -- not inside the first gymrs_step_many, which is documented as
    // asynchronous (queue creation, the device's self-check, hipMalloc and ~3 ms of probe chains used to happen there, on
    // whatever stream the caller had set).  Without the path (GYMRS_AQL=0, a failed self-check, too many queues) the engine steps
    // through HIP launches and says why in gymrs_env_json.
    if (aql_enabled_by_env() && !e->pool_host) {
        e->aql_tried = true;
        e->aql = aql_create(e->device, &e->aql_why);
        if (e->aql)
            if (const char* how = aql_calibrate(e->aql, e->stream, true)) e->aql_handover = how;
    }
    *out = e;
    return GYMRS_OK;
}

gymrs_status gymrs_set_stream(gymrs_engine* e, void* hip_stream)
{
    if (!e) return fail(GYMRS_EINVAL, "gymrs_set_stream: engine is NULL");
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (e->own_stream) HIP_TRY(hipStreamDestroy(e->stream));
    e->stream = static_cast<hipStream_t>(hip_stream);
    e->own_stream = false;
    if (e->graph_exec) { // the cached graph was captured on the old stream's arguments only, but keep it simple
        (void)hipGraphExecDestroy(e->graph_exec);
        e->graph_exec = nullptr;
    }
    return GYMRS_OK;
}

gymrs_status gymrs_get_stream(gymrs_engine* e, void** hip_stream)
{
    if (!e || !hip_stream) return fail(GYMRS_EINVAL, "gymrs_get_stream: NULL argument");
    *hip_stream = e->stream;
    return GYMRS_OK;
}

gymrs_status gymrs_set_tuning(gymrs_engine* e, int lanes_per_thread, int memory_hint)
{
    if (!e) return fail(GYMRS_EINVAL, "gymrs_set_tuning: engine is NULL");
    if (lanes_per_thread != 4 && lanes_per_thread != 8)
        return fail(GYMRS_EINVAL, "gymrs_set_tuning: lanes_per_thread must be 4 or 8");
    if (memory_hint < 0 || memory_hint > 3) return fail(GYMRS_EINVAL, "gymrs_set_tuning: memory_hint must be 0, 1, 2 or 3");
    e->vec = lanes_per_thread;
    e->nt_mode = memory_hint;
    return GYMRS_OK;
}

// ---------------------------------------------------------------------------------------------
// The default sampling box of `sample_between` in f64 (cartpole.rs:353-360: +-0.05 in every component;
// mountain_car.rs:175-186: position in [-0.6, -0.4)).
static double default_reset_low_f64(gymrs_env_kind kind, int) { return kind == GYMRS_CARTPOLE ? -0.05 : -0.6; }
static double default_reset_high_f64(gymrs_env_kind kind, int) { return kind == GYMRS_CARTPOLE ? 0.05 : -0.4; }

// What both reset entry points share once the seed and the sampling box are known: `pcg` = NULL draws from the Philox
// reset stream, otherwise from one reference-style PCG64 per lane (gymrs_pcg64.h).
struct PcgReset {
    const uint64_t* seeds_dev;
    double low[4], scale[4];
};

static gymrs_status reset_lanes(gymrs_engine* e, uint64_t seed, const float* lo, const float* hi, const PcgReset* pcg)
{
    std::memcpy(e->lo, lo, sizeof(e->lo));
    std::memcpy(e->hi, hi, sizeof(e->hi));
    if (gymrs_status st = fold_reset_log(e)) return st; // leaves the ring all zero; reset_kernel rewrites ep_start below
    // seeding.rs:21-26: the generator is re-created on every reset
    e->seed = seed;
    e->tick = 0;
    if (e->graph_exec) { // the reset box and the seed are baked into a captured graph
        (void)hipGraphExecDestroy(e->graph_exec);
        e->graph_exec = nullptr;
    }

    ResetArgs a;
    std::memset(&a, 0, sizeof(a));
    for (int j = 0; j < 4; ++j) a.s[j] = e->s[j];
    a.obs_cos = e->obs_cos;
    a.obs_sin = e->obs_sin;
    a.reward = e->reward;
    a.done = e->done;
    a.truncated = e->truncated;
    a.beyond = e->beyond;
    a.ep_start = e->ep_start;
    a.n = e->n;
    a.gid0 = e->gid0;
    a.seed = e->seed;
    a.tick = e->tick;
    a.box = make_sample_box(lo, hi, e->state_dim);
    if (pcg) {
        a.pcg64 = 1;
        a.pcg_seeds = pcg->seeds_dev;
        std::memcpy(a.pcg_low, pcg->low, sizeof(a.pcg_low));
        std::memcpy(a.pcg_scale, pcg->scale, sizeof(a.pcg_scale));
    }
    HIP_TRY(launch_reset(e->kind, a, e->stream));
    if (e->final_obs) HIP_TRY(hipMemsetAsync(e->final_obs, 0, (size_t)final_obs_stride(e->n) * 4 * e->obs_dim, e->stream)); // no episode has ended yet
    e->tick += 1;
    e->uniform_start = e->tick;
    e->epoch = e->tick; // what reset_kernel wrote into ep_start
    limit_restart(e, e->tick, true); // every episode starts now; reset_kernel cleared `truncated`
    // a reset discards the open episodes and starts the statistics afresh
    HIP_TRY(hipMemsetAsync(e->block_stats, 0, (size_t)e->n_stat_blocks * 2 * sizeof(unsigned long long), e->stream));
    HIP_TRY(hipMemsetAsync(e->wave_open, 0, (size_t)e->n_stat_blocks * sizeof(double), e->stream));
    e->open_vec = 0;
    e->trunc_held = 0; // reset_kernel cleared the flags
    HIP_TRY(hipMemsetAsync(e->wave_clean, 0, (size_t)e->n_stat_blocks * sizeof(uint32_t), e->stream)); // and the rewards
    e->clean_shape = 0;
    HIP_TRY(launch_stats(stats_args(e), 2, e->stream));
    e->n_steps_total = 0;
    return GYMRS_OK;
}

gymrs_status gymrs_reset(gymrs_engine* e, int has_seed, uint64_t seed, const float* bounds, uint64_t* seed_used)
{
    if (!e) return fail(GYMRS_EINVAL, "gymrs_reset: engine is NULL");
    HIP_TRY(hipSetDevice(e->device));
    float lo[4], hi[4];
    std::memcpy(lo, e->dflt_lo, sizeof(lo));
    std::memcpy(hi, e->dflt_hi, sizeof(hi));
    if (bounds) {
        // `options: Option<BoxR<Observation>>` (core.rs:49): state_dim lows then state_dim highs.
        const int d = e->state_dim;
        const int sampled = (e->kind == GYMRS_MOUNTAIN_CAR) ? 1 : d; // velocity is not sampled (mountain_car.rs:165)
        for (int j = 0; j < sampled; ++j) {
            lo[j] = bounds[j];
            hi[j] = bounds[d + j];
            // rand's Uniform::new panics unless low < high and both are finite, and on a range that overflows [RECALLED]; a width
            // whose 2^-24 share is not a normal float would draw one value for every lane (sample_range_ok)
            if (!sample_range_ok(lo[j], hi[j]))
                return fail(GYMRS_EINVAL, "gymrs_reset: bounds need finite low < high, a finite f32 width high - low, and a width of at least 2^-102");
        }
    }
    const uint64_t s = has_seed ? seed : os_entropy();
    if (seed_used) *seed_used = s;
    return reset_lanes(e, s, lo, hi, nullptr);
}

// rand 0.8 `UniformFloat::<f64>::new(low, high)` [RECALLED, SURVEY App. B.2]: scale = high - low, then one ulp less for
// as long as the largest draw (1 - 2^-52) * scale + low would reach `high`.
static bool uniform_f64_scale(double low, double high, double* scale_out)
{
    if (!(low < high) || !std::isfinite(low) || !std::isfinite(high)) return false;
    double scale = high - low;
    if (!std::isfinite(scale)) return false; // "Uniform::new: range overflow"
    const double max_rand = 1.0 - 0x1p-52;
    // The loop takes ~ulp(high) / (2 ulp(scale)) rounds, so a box that is very narrow for where it lies (say
    // [1e5, 1e5 + 1e-10)) keeps the reference busy for 1e15 iterations; such boxes are refused after 2^22 rounds.
    for (long rounds = 0;; ++rounds) {
        volatile double product = scale * max_rand; // rounded on its own, as in the reference (no fma)
        if (!(product + low >= high)) break;
        if (rounds == (1L << 22)) return false;
        uint64_t bits;
        std::memcpy(&bits, &scale, sizeof(bits));
        bits -= 1;
        std::memcpy(&scale, &bits, sizeof(bits));
    }
    *scale_out = scale;
    return true;
}

gymrs_status gymrs_reset_pcg64(gymrs_engine* e, int has_seed, uint64_t seed, const uint64_t* seeds_dev,
                               const double* bounds, uint64_t* seed_used)
{
    if (!e) return fail(GYMRS_EINVAL, "gymrs_reset_pcg64: engine is NULL");
    if (e->kind == GYMRS_PENDULUM)
        return fail(GYMRS_EINVAL, "gymrs_reset_pcg64: the reference has no Pendulum, so there is no PCG64 reset stream to reproduce");
    HIP_TRY(hipSetDevice(e->device));
    const int d = e->state_dim;
    const int sampled = (e->kind == GYMRS_MOUNTAIN_CAR) ? 1 : d;
    PcgReset pcg;
    std::memset(&pcg, 0, sizeof(pcg));
    pcg.seeds_dev = seeds_dev;
    float lo[4], hi[4]; // the box the Philox re-arms of GYMRS_AUTO_RESET keep using
    std::memcpy(lo, e->dflt_lo, sizeof(lo));
    std::memcpy(hi, e->dflt_hi, sizeof(hi));
    for (int j = 0; j < sampled; ++j) {
        // the f64 defaults of cartpole.rs:353-360 / mountain_car.rs:175-186, not their f32 roundings
        double low = bounds ? bounds[j] : default_reset_low_f64(e->kind, j);
        double high = bounds ? bounds[d + j] : default_reset_high_f64(e->kind, j);
        if (!uniform_f64_scale(low, high, &pcg.scale[j]))
            return fail(GYMRS_EINVAL, "gymrs_reset_pcg64: bounds need finite low < high, a finite high - low, and a width of at least ~1e-6 of |high|");
        pcg.low[j] = low;
        if (bounds) {
            lo[j] = (float)low;
            hi[j] = (float)high;
            if (!(lo[j] < hi[j])) return fail(GYMRS_EINVAL, "gymrs_reset_pcg64: bounds collapse in f32");
            if (!sample_range_ok(lo[j], hi[j])) // gymrs_reset's rule, for the box the re-arms draw from
                return fail(GYMRS_EINVAL, "gymrs_reset_pcg64: the f32 box of the re-arms needs finite low < high, a finite f32 width high - low, and a width of at least 2^-102");
        }
    }
    const uint64_t s = has_seed ? seed : os_entropy();
    if (seed_used) *seed_used = s;
    return reset_lanes(e, s, lo, hi, &pcg);
}

// Pendulum's open-episode reward sums live in per-wavefront slots whose lane coverage depends on the lanes per
// work-item of the launch: when that changes, gather them into slot 0 (every launch shape has a wave 0) so that
// no slot the new shape never visits keeps a stranded partial sum.
// The same for the reward-elision flags (step_block): they describe a wave's lanes, so a launch of another shape
// starts from "rewrite everything".
static gymrs_status prepare_wave_flags(gymrs_engine* e, int vec)
{
    if (e->clean_shape != vec) {
        if (e->clean_shape != 0) HIP_TRY(hipMemsetAsync(e->wave_clean, 0, (size_t)e->n_stat_blocks * sizeof(uint32_t), e->stream));
        e->clean_shape = vec;
    }
    return GYMRS_OK;
}

static gymrs_status prepare_open_sums(gymrs_engine* e, int vec)
{
    if (gymrs_status st = prepare_wave_flags(e, vec)) return st;
    if (e->kind != GYMRS_PENDULUM || (e->flags & (GYMRS_TRACK_STATS | GYMRS_AUTO_RESET)) != (GYMRS_TRACK_STATS | GYMRS_AUTO_RESET)) return GYMRS_OK;
    if (e->open_vec != 0 && e->open_vec != vec) HIP_TRY(launch_fold_open(e->wave_open, e->n_stat_blocks, e->stream));
    e->open_vec = vec;
    return GYMRS_OK;
}

// ---- the submission sequence of ONE per-step launch: prepare_step, submit (HIP launch or chain packet), record_step -----------
struct StepLaunch {
    uint32_t flags; // engine flags | hint bits | table bit
    StepArgs args;
};

// The launch at the engine's current tick.  May put work on the stream first, in this order: the barrier that closes an open
// chain, a refresh of the time-limit bound, the memset of `truncated`, the stand-alone fold.  chain = it gets a chain's hints.
static gymrs_status prepare_step(gymrs_engine* e, const void* actions, bool chain, StepLaunch* l)
{
    l->flags = take_over_device(e, launch_flags_of(e));
    if (gymrs_status st = elide_time_limit(e, &l->flags)) return st;
    if (chain) l->flags = (l->flags & ~kFlagHintMask) | hint_bits(e->nt_mode, bytes_per_step(e->kind, e->state_dim, e->n), /*chain=*/true);
    l->args = step_args(e, actions);
    return log_before_step(e, l->flags, &l->args.fold_step);
}

// The launch has been submitted.  path: 1 a HIP launch, 2 a launch of a chain (gymrs_engine::last_path).
static void record_step(gymrs_engine* e, const StepLaunch& l, int path)
{
    e->last_flags = l.flags;
    e->last_path = path;
    if (has_uniform_clock(e)) {
        e->trunc_held = (int)l.args.truncate_all;
        e->uniform_start = uniform_clock_after(e->tick, e->uniform_start, l.args.truncate_all != 0, (e->flags & GYMRS_AUTO_RESET) != 0);
    }
    e->tick += 1;
    if (path == 2) e->aql_launches += 1;
    e->n_steps_total += (double)e->n;
}

// prepare, submit as a HIP launch on the engine's stream, record
static gymrs_status step_through_hip(gymrs_engine* e, const void* actions)
{
    StepLaunch l;
    if (gymrs_status st = prepare_step(e, actions, /*chain=*/false, &l)) return st;
    HIP_TRY(launch_step(e->kind, e->vec, l.flags, l.args, launch_consts(e), e->stream));
    record_step(e, l, 1);
    return GYMRS_OK;
}

gymrs_status gymrs_step(gymrs_engine* e, const void* actions_dev)
{
    if (!e || !actions_dev) return fail(GYMRS_EINVAL, "gymrs_step: NULL argument");
    HIP_TRY(hipSetDevice(e->device));
    if (gymrs_status st = prepare_open_sums(e, e->vec)) return st;
    return step_through_hip(e, actions_dev);
}

// the buffer checks of the recording rollouts (gymrs_trajectory)
static gymrs_status check_trajectory(const gymrs_engine* e, const gymrs_trajectory* rec, const char* who)
{
    if (!rec->obs || !rec->actions || !rec->reward || !rec->done)
        return fail(GYMRS_EINVAL, std::string(who) + ": obs, actions, reward and done buffers are required");
    if (rec->lane_stride < e->n || rec->lane_stride % 16 != 0)
        return fail(GYMRS_EINVAL, std::string(who) + ": lane_stride must be >= n_envs and a multiple of 16");
    const uintptr_t bits = reinterpret_cast<uintptr_t>(rec->obs) | reinterpret_cast<uintptr_t>(rec->actions) |
                           reinterpret_cast<uintptr_t>(rec->reward) | reinterpret_cast<uintptr_t>(rec->done) |
                           reinterpret_cast<uintptr_t>(rec->truncated);
    if (bits % 16 != 0) return fail(GYMRS_EINVAL, std::string(who) + ": trajectory buffers must be 16-byte aligned");
    return GYMRS_OK;
}

static gymrs_status check_fitness_steps(bool fitness, uint32_t n_steps, const char* who)
{
    if (!fitness || n_steps <= kMaxFitnessSteps) return GYMRS_OK;
    return fail(GYMRS_EINVAL, std::string(who) + ": n_steps is above GYMRS_POLICY_FITNESS_MAX_STEPS (the in-register counters are 32 bits wide)");
}

// What one fused rollout launches.  The C entry points validate and fill it; rollout_impl validates nothing.
enum class ActionSource {
    Random,    // the Philox action stream (action_seed, action_t0): gymrs_rollout, gymrs_rollout_record
    Policy,    // the engine's policy set (gymrs_set_policy): the closed-loop calls
    Exploring, // the policy set's epsilon-greedy action under the engine's exploration settings (gymrs_explore.hip)
    Sampling,  // an action drawn from the softmax of the policy's logits under the engine's sampling settings (gymrs_sample.hip)
};
struct RolloutRequest {
    ActionSource actions;
    uint64_t action_seed = 0, action_t0 = 0;     // Random only
    bool fitness = false;                        // the kernel adds to the per-policy counters (not with Random)
    const gymrs_trajectory* record = nullptr;    // checked by check_trajectory
    const TransitionArgs* transitions = nullptr; // with a record and a policy: the kernel also writes these two buffers (gymrs_transitions.hip)
};
// (Lane parameters are not part of it: a launch under an active table always plays them; check_table_opt_in guards the calls.)

// The caller loop of the reference's examples (examples/cartpole.rs:15-30: random action, step, reset on
// done, accumulate the return) fused into one launch; see rollout_kernel.
static gymrs_status rollout_impl(gymrs_engine* e, uint32_t n_steps, const RolloutRequest& q)
{
    if (n_steps == 0) return GYMRS_OK;
    HIP_TRY(hipSetDevice(e->device));
    StepArgs a = step_args(e, nullptr);
    a.skip_trunc_store = 0; // the kernel stores the LAST step's flags, whatever the array holds now
    RolloutArgs r;
    std::memset(&r, 0, sizeof(r));
    r.action_seed = q.action_seed;
    r.action_t0 = q.action_t0;
    r.uniform_start = e->uniform_start;
    r.n_steps = n_steps;
    r.n_actions = e->kind == GYMRS_CARTPOLE ? 2u : 3u;
    r.max_torque = e->max_torque;
    int vec = e->vec == 8 ? 8 : 4;
    if (const gymrs_trajectory* rec = q.record) {
        r.rec_obs = rec->obs;
        r.rec_action = rec->actions;
        r.rec_reward = rec->reward;
        r.rec_done = rec->done;
        r.rec_trunc = rec->truncated;
        r.rec_stride = rec->lane_stride;
        vec = 4;
    }
    if (gymrs_status st = prepare_open_sums(e, vec)) return st;
    if (gymrs_status st = fold_reset_log(e)) return st; // the rollout kernel carries ep_start and the counters itself
    if (q.fitness)
        if (gymrs_status st = policy_fitness_table(e)) return st;
    if (q.actions == ActionSource::Random)
        HIP_TRY(launch_rollout(e->kind, vec, e->flags | table_bit(e), a, r, launch_consts(e), e->stream));
    else {
        const ClosedLoopSource source = q.actions == ActionSource::Sampling    ? ClosedLoopSource::sampling
                                        : q.actions == ActionSource::Exploring ? ClosedLoopSource::exploring
                                                                               : ClosedLoopSource::policy;
        HIP_TRY(launch_closed_loop(e->kind, {vec, e->flags | table_bit(e), a, r, launch_consts(e), e->policy.args, source, e->explore, e->sample,
                                             q.fitness ? e->fitness_dev : nullptr, q.transitions, e->stream}));
    }
    if (e->flags & GYMRS_TIME_LIMIT) e->trunc_zero = false; // the kernel stored the last step's flags
    // ... and every lane's reward, without looking at the reward-elision words (step_block) or updating them.  Without a table every lane
    // of a fused launch is stepped and earns the constant, so words that say "clean" stay true.  Under a table a lane whose index is out of
    // it is not stepped and is paid 0.0: what the words say is no longer known, and the next per-step launch starts from "rewrite everything".
    if (e->table_k) {
        HIP_TRY(hipMemsetAsync(e->wave_clean, 0, (size_t)e->n_stat_blocks * sizeof(uint32_t), e->stream));
        e->clean_shape = 0;
    }
    for (uint32_t k = 0; k < n_steps; ++k) { // the host copy of the uniform episode clock (Pendulum time limit)
        if (has_uniform_clock(e)) {
            const bool hit = uniform_clock_hits(e->tick, e->uniform_start, e->max_steps);
            e->trunc_held = hit ? 1 : 0; // the rollout kernel stores the last step's flags
            e->uniform_start = uniform_clock_after(e->tick, e->uniform_start, hit, (e->flags & GYMRS_AUTO_RESET) != 0);
        }
        e->tick += 1;
    }
    e->n_steps_total += (double)e->n * (double)n_steps;
    return GYMRS_OK;
}

// The rollout calls from before the descriptors.  They have no way to opt in to a parameter table, and a call of 0 steps returns
// before its buffers are looked at.
static gymrs_status plain_rollout(gymrs_engine* e, uint32_t n_steps, const RolloutRequest& q, const char* who)
{
    if (!e) return fail(GYMRS_EINVAL, std::string(who) + ": NULL engine");
    if (q.actions == ActionSource::Policy) {
        if (q.fitness)
            if (gymrs_status st = check_discrete_env(e->kind, who)) return st;
        if (gymrs_status st = check_policy_set(e, who)) return st;
        if (gymrs_status st = check_table_opt_in(e, false, who, "; policy x table is not built yet: use gymrs_policy_actions + gymrs_step")) return st;
        if (gymrs_status st = check_fitness_steps(q.fitness, n_steps, who)) return st;
    }
    if (q.record && n_steps != 0)
        if (gymrs_status st = check_trajectory(e, q.record, who)) return st;
    return rollout_impl(e, n_steps, q);
}

gymrs_status gymrs_rollout(gymrs_engine* e, uint32_t n_steps, uint64_t action_seed, uint64_t action_t0)
{
    return plain_rollout(e, n_steps, {ActionSource::Random, action_seed, action_t0}, "gymrs_rollout");
}

gymrs_status gymrs_rollout_record(gymrs_engine* e, uint32_t n_steps, uint64_t action_seed, uint64_t action_t0,
                                  const gymrs_trajectory* out)
{
    if (!out) return fail(GYMRS_EINVAL, "gymrs_rollout_record: trajectory is NULL");
    return plain_rollout(e, n_steps, {ActionSource::Random, action_seed, action_t0, false, out}, "gymrs_rollout_record");
}

gymrs_status gymrs_rollout_policy(gymrs_engine* e, uint32_t n_steps) { return plain_rollout(e, n_steps, {ActionSource::Policy}, "gymrs_rollout_policy"); }

gymrs_status gymrs_rollout_policy_fitness(gymrs_engine* e, uint32_t n_steps)
{
    return plain_rollout(e, n_steps, {ActionSource::Policy, 0, 0, true}, "gymrs_rollout_policy_fitness");
}

gymrs_status gymrs_rollout_policy_record(gymrs_engine* e, uint32_t n_steps, const gymrs_trajectory* out)
{
    if (!e) return fail(GYMRS_EINVAL, "gymrs_rollout_policy_record: NULL engine");
    if (!out) return fail(GYMRS_EINVAL, "gymrs_rollout_policy_record: trajectory is NULL");
    return plain_rollout(e, n_steps, {ActionSource::Policy, 0, 0, false, out}, "gymrs_rollout_policy_record");
}

// What the two descriptor calls check alike, in this order, between their NULL checks and their own fields.
static gymrs_status check_closed_loop_call(const gymrs_engine* e, const char* who)
{
    if (gymrs_status st = check_discrete_env(e->kind, who)) return st;
    return check_policy_set(e, who);
}
static ActionSource closed_loop_actions(uint32_t flags)
{
    if (flags & GYMRS_CLOSED_LOOP_SAMPLE) return ActionSource::Sampling;
    return (flags & GYMRS_CLOSED_LOOP_EXPLORE) ? ActionSource::Exploring : ActionSource::Policy;
}
// ... and once their flags word is known to hold known bits only
static gymrs_status check_explore_flag(const gymrs_engine* e, uint32_t flags, const char* who)
{
    if ((flags & GYMRS_CLOSED_LOOP_SAMPLE) && (flags & GYMRS_CLOSED_LOOP_EXPLORE))
        return fail(GYMRS_EINVAL, std::string(who) + ": GYMRS_CLOSED_LOOP_SAMPLE together with GYMRS_CLOSED_LOOP_EXPLORE: a launch has one action source");
    if ((flags & GYMRS_CLOSED_LOOP_SAMPLE) && !e->sample_set)
        return fail(GYMRS_EINVAL, std::string(who) + ": GYMRS_CLOSED_LOOP_SAMPLE without sampling settings on the engine (gymrs_set_sampling)");
    if (!(flags & GYMRS_CLOSED_LOOP_EXPLORE) || e->explore_set) return GYMRS_OK;
    return fail(GYMRS_EINVAL, std::string(who) + ": GYMRS_CLOSED_LOOP_EXPLORE without exploration settings on the engine (gymrs_set_exploration)");
}

// The closed-loop calls behind one descriptor with a flags word (include/gymrs_amd.h): what gymrs_rollout_policy, _record and
// _fitness do, and -- with GYMRS_CLOSED_LOOP_LANE_PARAMS -- the same under an active parameter table.
gymrs_status gymrs_rollout_closed_loop(gymrs_engine* e, const gymrs_closed_loop_desc* d)
{
    const char* who = "gymrs_rollout_closed_loop";
    if (!e) return fail(GYMRS_EINVAL, std::string(who) + ": NULL engine");
    if (!d) return fail(GYMRS_EINVAL, std::string(who) + ": NULL desc");
    if (gymrs_status st = check_closed_loop_call(e, who)) return st;
    if (d->reserved != 0) return fail(GYMRS_EINVAL, std::string(who) + ": reserved must be 0");
    if (d->flags & ~(GYMRS_CLOSED_LOOP_FITNESS | GYMRS_CLOSED_LOOP_LANE_PARAMS | GYMRS_CLOSED_LOOP_EXPLORE | GYMRS_CLOSED_LOOP_SAMPLE))
        return fail(GYMRS_EINVAL, std::string(who) + ": unknown flag bits (GYMRS_CLOSED_LOOP_FITNESS, GYMRS_CLOSED_LOOP_LANE_PARAMS, "
                                                     "GYMRS_CLOSED_LOOP_EXPLORE and GYMRS_CLOSED_LOOP_SAMPLE are the only ones)");
    const bool fitness = (d->flags & GYMRS_CLOSED_LOOP_FITNESS) != 0;
    if (gymrs_status st = check_explore_flag(e, d->flags, who)) return st;
    if (fitness && d->record) return fail(GYMRS_EINVAL, std::string(who) + ": GYMRS_CLOSED_LOOP_FITNESS with a record: there is no recording fitness kernel");
    if (gymrs_status st = check_table_opt_in(e, (d->flags & GYMRS_CLOSED_LOOP_LANE_PARAMS) != 0, who, kAdviceLaneParamsFlag)) return st;
    if (d->record)
        if (gymrs_status st = check_trajectory(e, d->record, who)) return st;
    if (gymrs_status st = check_fitness_steps(fitness, d->n_steps, who)) return st;
    return rollout_impl(e, d->n_steps, {closed_loop_actions(d->flags), 0, 0, fitness, d->record});
}

// gymrs_rollout_closed_loop with a record that also keeps every step's final observations (include/gymrs_amd.h, "transitions").
gymrs_status gymrs_rollout_transitions(gymrs_engine* e, const gymrs_transitions_desc* d)
{
    const char* who = "gymrs_rollout_transitions";
    if (!e) return fail(GYMRS_EINVAL, std::string(who) + ": NULL engine");
    if (!d) return fail(GYMRS_EINVAL, std::string(who) + ": NULL desc");
    if (gymrs_status st = check_closed_loop_call(e, who)) return st;
    if (!(e->flags & GYMRS_AUTO_RESET))
        return fail(GYMRS_EINVAL, std::string(who) + ": the engine has no GYMRS_AUTO_RESET: nothing is re-armed, the record's obs rows already hold "
                                                     "the final observations (gymrs_rollout_closed_loop)");
    if (d->reserved != 0) return fail(GYMRS_EINVAL, std::string(who) + ": reserved must be 0");
    if (d->flags & ~(GYMRS_CLOSED_LOOP_LANE_PARAMS | GYMRS_CLOSED_LOOP_EXPLORE | GYMRS_CLOSED_LOOP_SAMPLE))
        return fail(GYMRS_EINVAL, std::string(who) + ": unknown flag bits (GYMRS_CLOSED_LOOP_LANE_PARAMS, GYMRS_CLOSED_LOOP_EXPLORE and "
                                                     "GYMRS_CLOSED_LOOP_SAMPLE are the only ones; GYMRS_CLOSED_LOOP_FITNESS: there is no recording "
                                                     "fitness kernel)");
    if (gymrs_status st = check_explore_flag(e, d->flags, who)) return st;
    if (gymrs_status st = check_table_opt_in(e, (d->flags & GYMRS_CLOSED_LOOP_LANE_PARAMS) != 0, who, kAdviceLaneParamsFlag)) return st;
    if (gymrs_status st = check_trajectory(e, &d->record, who)) return st;
    if (!d->final_obs) return fail(GYMRS_EINVAL, std::string(who) + ": final_obs is required");
    if ((reinterpret_cast<uintptr_t>(d->final_obs) | reinterpret_cast<uintptr_t>(d->start_obs)) % 16 != 0)
        return fail(GYMRS_EINVAL, std::string(who) + ": final_obs and start_obs must be 16-byte aligned");
    const TransitionArgs t{d->final_obs, d->start_obs};
    return rollout_impl(e, d->n_steps, {closed_loop_actions(d->flags), 0, 0, false, &d->record, &t});
}

gymrs_status gymrs_step_host(gymrs_engine* e, const void* actions_host)
{
    if (!e || !actions_host) return fail(GYMRS_EINVAL, "gymrs_step_host: NULL argument");
    HIP_TRY(hipSetDevice(e->device));
    const size_t bytes = (size_t)e->n * action_size(e->kind);
    if (e->pool_host) { // small engine: the staging buffer is mapped host memory, the "copy" a memcpy
        if (!e->action_staging)
            if (hipError_t err = mapped_host_block((bytes + 63) & ~(size_t)63, &e->staging_host, &e->action_staging))
                return fail(GYMRS_EHIP, std::string("hipHostMalloc(&host, ((bytes + 63) & ~(size_t)63), hipHostMallocMapped | hipHostMallocCoherent): ") +
                                            hipGetErrorString(err));
        HIP_TRY(hipStreamSynchronize(e->stream)); // a step still in flight may be reading the buffer
        std::memcpy(e->staging_host, actions_host, bytes);
        return gymrs_step(e, e->action_staging);
    }
    if (!e->action_staging) HIP_TRY(hipMalloc(&e->action_staging, ((bytes + 63) & ~(size_t)63)));
    HIP_TRY(hipMemcpyAsync(e->action_staging, actions_host, bytes, hipMemcpyHostToDevice, e->stream));
    return gymrs_step(e, e->action_staging);
}

// Capture `steps` consecutive step launches into a HIP graph.  What changes from one replay to the next is
// only the tick, so it is read from device memory (tick_dev) and bumped by a one-thread kernel at the end of
// the graph; everything else (pointers, flags, reset box, seed) is baked in and part of the cache key.
static gymrs_status build_graph(gymrs_engine* e, const char* base, uint64_t stride_bytes, uint32_t n_buffers, uint32_t steps)
{
    if (e->graph_exec) {
        (void)hipGraphExecDestroy(e->graph_exec);
        e->graph_exec = nullptr;
    }
    hipGraph_t graph = nullptr;
    HIP_TRY(hipStreamBeginCapture(e->stream, hipStreamCaptureModeThreadLocal));
    hipError_t err = hipSuccess;
    // (a captured launch keeps the engine's own flags, time limit included: what is baked in cannot follow start_bound)
    const uint32_t flags = launch_flags_of(e);
    ResetLogRing ring{0, 0, e->vec}; // a replay starts on an empty ring
    for (uint32_t t = 0; t < steps && err == hipSuccess; ++t) {
        StepArgs a = step_args(e, base + (size_t)(t % n_buffers) * stride_bytes);
        a.tick = t;
        a.tick_base = e->tick_dev;
        const ResetLogStep s = reset_log_step(ring, launch_is_logged(e, flags), t, e->vec);
        a.fold_step = s.fold_step;
        ring = s.after;
        err = launch_step(e->kind, e->vec, flags, a, launch_consts(e), e->stream);
    }
    if (err == hipSuccess) err = launch_tick_advance(e->tick_dev, steps, e->stream);
    hipError_t end = hipStreamEndCapture(e->stream, &graph);
    if (err != hipSuccess || end != hipSuccess) {
        if (graph) (void)hipGraphDestroy(graph);
        return fail(GYMRS_EHIP, std::string("HIP graph capture: ") + hipGetErrorString(err != hipSuccess ? err : end));
    }
    err = hipGraphInstantiate(&e->graph_exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (err != hipSuccess) return fail(GYMRS_EHIP, std::string("hipGraphInstantiate: ") + hipGetErrorString(err));
    e->graph_actions = base;
    e->graph_stride = stride_bytes;
    e->graph_nbuf = n_buffers;
    e->graph_steps = steps;
    e->graph_flags = flags;
    e->graph_vec = e->vec;
    e->graph_seed = e->seed;
    return GYMRS_OK;
}

// ---- chains of per-step launches through the engine's own AQL dispatcher (gymrs_aql.h) ---------------------------------
// Which launches it takes: every flag set at 4 lanes per work-item (what the stand-alone code object holds, gymrs_step_aql.hip), on
// engines whose arrays live in device memory and that were created without GYMRS_FINAL_OBS (no chain kernel has that bit); chains of at least kAqlMinChain steps (a chain costs three small packets and two
// stream operations of its own).  Everything else -- and every device on which the dispatcher's self-check fails -- goes
// through HIP launches.
constexpr uint32_t kAqlMinChain = 8;

extern "C++" std::string aql_kernel_name(const gymrs_engine* e, uint32_t flags, int threads) // (declared in gymrs_engine_priv.h)
{
    constexpr uint32_t A = GYMRS_AUTO_RESET, S = GYMRS_TRACK_STATS, T = GYMRS_TIME_LIMIT;
    uint32_t f = flags & (A | S | T);
    if (!(f & A)) f &= ~S; // statistics need auto-reset (as in the launch table, gymrs_step_impl.h)
    const char* env = e->kind == GYMRS_CARTPOLE ? "cartpole" : (e->kind == GYMRS_MOUNTAIN_CAR ? "mountain_car" : "pendulum");
    const uint32_t h = flags & kFlagHintMask;
    const char* hint = (h & kFlagNonTemporal) ? "_nt" : (h == (kFlagNtOut | kFlagNtStateLoads) ? "_so" : (h == kFlagNtOut ? "_o" : (h == 0 ? "_pl" : nullptr)));
    if (!hint) return std::string();
    char name[96];
    std::snprintf(name, sizeof(name), "gymrs_aql_%s_f%u_t%d%s", env, f, threads, hint); // (the names of gymrs_step_aql.hip)
    return name;
}

static bool aql_usable(gymrs_engine* e, uint32_t n_steps)
{
    if (n_steps < kAqlMinChain || e->vec != 4 || e->pool_host) return false;
    if (e->flags & GYMRS_FINAL_OBS) return false; // the chain's code object holds no final-observation kernels: HIP launches
    if (e->table_k) return false;                 // nor any parameter-table kernels
    if (!aql_enabled_by_env()) return false;
    if (stream_capturing(e) != 0) return false; // a caller-provided stream may be under a capture: a chain cannot be captured
    if (!e->aql_tried) { // (an engine created under GYMRS_AQL=0 and stepped without it: set up on first use)
        e->aql_tried = true;
        e->aql = aql_create(e->device, &e->aql_why);
    }
    if (!e->aql) return false;
    // which hand-over: decided at creation for the engine's own stream; again when another chain object has appeared on the device
    // since, or the stream has changed (a caller-provided stream is never timed or waited for: asynchronous hand-over)
    if (const char* how = aql_calibrate(e->aql, e->stream, e->own_stream)) e->aql_handover = how;
    // the synchronous hand-over makes the HOST wait for the stream: never on a stream the engine does not own (it may be blocked on
    // work its owner has not submitted yet) -- such an engine keeps to HIP launches where the asynchronous form is not available
    if (!e->own_stream && aql_is_synchronous(e->aql)) return false;
    return true;
}

extern "C++" {
// The kernel-argument block of a launch of the chain's code object, filled by hand: it must be exactly what the code object's
// metadata says the kernel reads (no hidden arguments, no drifted layout).
template <class Consts>
static void fill_kern_args(StepKernArgs<Consts>* ka, const StepArgs& a, const Consts& c)
{
    std::memset(ka, 0, sizeof(*ka));
    ka->s0 = a.s[0];
    ka->s1 = a.s[1];
    ka->s2 = a.s[2];
    ka->s3 = a.s[3];
    ka->action = a.action;
    ka->n_fast = a.n_fast;
    ka->rest = a;
    ka->c = c;
}

template <class Consts>
static bool aql_step(gymrs_engine* e, const AqlKernel& k, int threads, const StepArgs& a, const Consts& c, std::string* err, bool release, bool first)
{
    StepKernArgs<Consts> ka;
    fill_kern_args(&ka, a, c);
    static_assert(sizeof(ka) <= kAqlKernargSlot, "kernel arguments larger than a ring slot");
    // (a kernel that read beyond sizeof(ka) would find whatever the ring slot held a lap ago)
    if (k.kernarg_bytes != sizeof(ka)) {
        *err = "kernel-argument segment of the chain kernel is " + std::to_string(k.kernarg_bytes) + " bytes, the dispatcher fills " + std::to_string(sizeof(ka));
        return false;
    }
    return aql_dispatch(e->aql, k, step_grid(a.n, 4, threads) * (uint32_t)threads, (uint32_t)threads, &ka, sizeof(ka), err, release, first);
}
} // extern "C++"

// steps [first, n_steps) of a gymrs_step_many call as ONE chain.  *taken = false: nothing was dispatched, use HIP launches.
static gymrs_status step_many_aql(gymrs_engine* e, const char* base, uint64_t stride_bytes, uint32_t n_buffers, uint32_t first, uint32_t n_steps,
                                  bool* taken)
{
    *taken = false;
    std::string err;
    // reset-log rows laid out for another launch shape are folded by a HIP kernel: BEFORE the chain, on the stream it waits for
    if (e->reset_log && e->log_pending != 0 && e->log_vec != e->vec) {
        if (gymrs_status st = fold_reset_log(e)) return st;
    }
    // (test hook, tests/test_gpu_aql_chain.py: a table nobody's XCC matches -- and no recording launch -- stands in for a deal that changed
    // in mid-chain; the memset sits on the stream ahead of the hand-over into the chain; set through gymrs_dev_set_hooks -- not in the header, not
    // read from the environment on the stepping path)
    const bool poisoned = (e->dev_hooks & 1u) != 0;
    if (poisoned) HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(aql_xcc_table(e->aql)), 0x11, 8 * kXccTableStride, e->stream));
    if (!aql_begin(e->aql, e->stream, &err)) { // nothing dispatched, no host state touched: this engine goes back to HIP launches for good
        e->aql_why = "aql_begin: " + err;
        aql_destroy(e->aql, /*discard=*/true); // (an object whose hand-over failed is not parked for the next engine)
        e->aql = nullptr;
        return GYMRS_OK;
    }
    e->chain_open = e->chain_first = true;
    *taken = true;
    // GYMRS_AQL=2: every launch RELEASES (HIP's header) and uses HIP launches' hints: nothing rests on lines staying in an XCD's L2, so no XCD check either
    const bool visible = aql_mode_by_env() == 2;
    const int threads = step_threads_of(e->kind, e->n, e->vec);
    uint32_t last_key = ~0u;
    AqlKernel k;
    auto bail = [e](gymrs_status st) { // close the chain (what was dispatched still runs and hands the stream back), keep the error
        const std::string msg = g_last_error;
        (void)stream_op_barrier(e);
        g_last_error = msg;
        return st;
    };
    for (uint32_t t = first; t < n_steps; ++t) {
        // The host side of the step first: on an engine that elides its time limit it may have to put something on the stream (a
        // refresh of the bound, a memset, the stand-alone fold) or wait for the device -- each of which closes the open chain
        // (stream_op_barrier).  The step itself then goes into the open chain, or into a new one behind whatever that was.
        StepLaunch l;
        if (gymrs_status st = prepare_step(e, base + (size_t)(t % n_buffers) * stride_bytes, /*chain=*/!visible, &l)) return bail(st);
        if (!e->chain_open) { // (the host side of this step closed the chain: the step opens the next one)
            if (!aql_begin(e->aql, e->stream, &err)) return fail(GYMRS_EHIP, "AQL dispatcher: " + err);
            e->chain_open = e->chain_first = true;
        }
        const uint32_t key = (l.flags & kFlagHintMask) | (l.flags & (GYMRS_AUTO_RESET | GYMRS_TRACK_STATS | GYMRS_TIME_LIMIT));
        if (key != last_key) {
            const std::string name = aql_kernel_name(e, l.flags, threads);
            if (name.empty() || !aql_kernel(e->aql, name.c_str(), &k)) return bail(fail(GYMRS_EHIP, "AQL dispatcher: no kernel for this launch"));
            last_key = key;
        }
        // every wavefront of a chain launch checks where it runs; the chain's first launch records the table (StepArgs::xcc_table)
        StepArgs& a = l.args;
        a.xcc_table = aql_xcc_table(e->aql);
        a.xcc_check = (e->chain_first && !poisoned) ? 2u : 1u;
        a.xcc_seq = aql_chain_number(e->aql);
        const bool first_of_chain = e->chain_first; // its packet carries the acquire that follows the hand-over (aql_dispatch)
        e->chain_first = false;
        if (visible) a.xcc_check = 0u;
        if (!visit_consts(e, [&](const auto& c) { return aql_step(e, k, threads, a, c, &err, visible, first_of_chain); }))
            return bail(fail(GYMRS_EHIP, "AQL dispatcher: " + err));
        record_step(e, l, 2);
    }
    return stream_op_barrier(e);
}

gymrs_status gymrs_step_many(gymrs_engine* e, const void* actions_dev, uint64_t stride_bytes, uint32_t n_buffers,
                             uint32_t n_steps, int use_graph)
{
    if (!e || !actions_dev) return fail(GYMRS_EINVAL, "gymrs_step_many: NULL argument");
    if (n_buffers == 0) return fail(GYMRS_EINVAL, "gymrs_step_many: n_buffers must be > 0");
    HIP_TRY(hipSetDevice(e->device));
    if (gymrs_status st = prepare_open_sums(e, e->vec)) return st;
    const char* base = static_cast<const char*>(actions_dev);
    uint32_t done = 0;
    // Graph replay pays when the step kernel is shorter than a host launch (~3 us: small batches).  The
    // Pendulum time limit is a host-computed kernel argument, so that combination stays eager.
    const bool graph_ok = use_graph && !(e->kind == GYMRS_PENDULUM && (e->flags & GYMRS_TIME_LIMIT));
    if (use_graph && !graph_ok) return fail(GYMRS_EINVAL, "gymrs_step_many: use_graph is not available for Pendulum with GYMRS_TIME_LIMIT");
    if (graph_ok) {
        const uint32_t per_graph = graph_steps(n_buffers, launch_is_logged(e, launch_flags_of(e)));
        if (n_steps >= per_graph) {
            const bool hit = e->graph_exec && e->graph_actions == base && e->graph_stride == stride_bytes &&
                             e->graph_nbuf == n_buffers && e->graph_steps == per_graph && e->graph_flags == launch_flags_of(e) &&
                             e->graph_vec == e->vec && e->graph_seed == e->seed;
            if (!hit) {
                if (gymrs_status st = build_graph(e, base, stride_bytes, n_buffers, per_graph)) return st;
            }
            const unsigned long long tick_now = e->tick;
            HIP_TRY(hipMemcpyAsync(e->tick_dev, &tick_now, sizeof(tick_now), hipMemcpyHostToDevice, e->stream));
            HIP_TRY(hipStreamSynchronize(e->stream)); // tick_now is a stack variable; the copy must finish before return
            if (gymrs_status st = fold_reset_log(e)) return st; // the captured fold steps assume an empty ring at the start
            if (e->device >= 0 && e->device < kMaxDevices) {
                g_last_stepper[e->device].store(e, std::memory_order_relaxed);
                g_stepper_run[e->device].store(kTakeOverAfter, std::memory_order_relaxed); // a replay is many launches
            }
            while (n_steps - done >= per_graph) {
                HIP_TRY(hipGraphLaunch(e->graph_exec, e->stream));
                done += per_graph;
                e->tick += per_graph;
                e->n_steps_total += (double)e->n * (double)per_graph;
            }
            if (e->flags & GYMRS_TIME_LIMIT) e->trunc_zero = false; // the replayed launches wrote the flags themselves
        }
    }
    if (!use_graph && aql_usable(e, n_steps - done)) { // a chain through the engine's own AQL dispatcher
        bool taken = false;
        if (gymrs_status st = step_many_aql(e, base, stride_bytes, n_buffers, done, n_steps, &taken)) return st;
        if (taken) done = n_steps;
    }
    for (uint32_t t = done; t < n_steps; ++t) // eager launches (and the remainder after graph replays)
        if (gymrs_status st = step_through_hip(e, base + (size_t)(t % n_buffers) * stride_bytes)) return st;
    return GYMRS_OK;
}

} // extern "C"

// Wait for the engine's stream, then look at what a chain may have reported meanwhile: EVERY read-out that synchronises goes through here (gymrs_sync,
// the host copies, statistics, snapshot, clone, the serde view), so that arrays a tripped chain may have left stale are never handed out with GYMRS_OK
// (only gymrs_sync used to look).
gymrs_status stream_sync_checked(gymrs_engine* e)
{
    HIP_TRY(hipStreamSynchronize(e->stream));
    std::atomic_thread_fence(std::memory_order_acquire);
    if (e->aql) {
        if (const uint32_t bad = aql_take_error(e->aql)) {
            if (bad & 2u) return fail(GYMRS_EHIP, "the AQL queue reported an error");
            if (bad & 4u) return fail(GYMRS_EHIP, "the engine's stream gave up waiting for a gymrs_step_many chain (120 s)");
            return fail(GYMRS_EHIP, "a gymrs_step_many chain ran without waiting for the engine's stream: the stream did not reach the "
                                    "hand-over point within ~10 s (is it blocked on work that was never submitted?)");
        }
    }
    if (const uint32_t where = e->err_seen[1]) { // a wavefront of a chain launch found itself on another XCD than the chain's first launch recorded
        e->err_seen[1] = 0;
        aql_destroy(e->aql, /*discard=*/true); // (the stream is idle: every chain ended with a wait on it; a queue that tripped the check is not handed on)
        e->aql = nullptr;
        char buf[400];
        std::snprintf(buf, sizeof(buf), "a gymrs_step_many chain ran workgroup %u on another XCD than the chain's first launch recorded for its index: the launches of a "
                                        "chain carry no release fence, so the arrays may hold stale values since the last gymrs_sync; this engine now steps through HIP launches",
                      where - 1u);
        e->aql_why = "a chain launch ran on an unexpected XCD; HIP launches from then on";
        return fail(GYMRS_EHIP, buf);
    }
    return GYMRS_OK;
}

extern "C" {

gymrs_status gymrs_sync(gymrs_engine* e)
{
    if (!e) return fail(GYMRS_EINVAL, "gymrs_sync: engine is NULL");
    HIP_TRY(hipSetDevice(e->device));
    if (gymrs_status st = stream_sync_checked(e)) return st;
    if (*e->err_seen == 0) return GYMRS_OK; // no kernel saw an invalid action: nothing to fetch
    uint32_t err[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(err, e->err, sizeof(err), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    *e->err_seen = 0;
    if (err[0] != 0) {
        static const uint32_t err_init[2] = {0u, 0xffffffffu};
        HIP_TRY(hipMemcpyAsync(e->err, err_init, sizeof(err_init), hipMemcpyHostToDevice, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
        char buf[200];
        if (e->table_k) // (a lane whose parameter index is >= K is rejected like an invalid action)
            std::snprintf(buf, sizeof(buf), "%u invalid action or parameter index(es); first offending lane %u (usize invalid)", err[0], err[1]);
        else
            std::snprintf(buf, sizeof(buf), "%u invalid action(s); first offending lane %u (usize invalid)", err[0], err[1]);
        return fail(GYMRS_EACTION, buf);
    }
    return GYMRS_OK;
}

} // extern "C"
