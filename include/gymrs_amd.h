/*
 * gymrs_amd.h — C ABI of the MI355X-native batched classic-control stepper.
 *
 * This is the drop-in boundary for the ONE hot path of MathisWellmann/gym-rs:
 * Env::step() (+ the reset() that re-arms a finished lane) of CartPole / MountainCar
 * (/ a spec-derived Pendulum).  The reference has no FFI; its boundary is the trait pair in
 * src/core.rs.  Each entry point below cites the reference interface it replaces, with
 * paths relative to /root/reference.  The binding a gym-rs maintainer would add (a Rust
 * `extern "C"` block + `impl Env`) is shown in INTEGRATION.md.
 *
 * Conventions
 *   - Plain pointers and sizes only.  Device pointers are HIP device addresses.
 *   - Every function returns a gymrs_status instead of panicking (the reference asserts:
 *     cartpole.rs:402-406); gymrs_last_error() gives the message for the calling thread.
 *   - The engine owns its device buffers.  The caller owns every host buffer it passes.
 *   - gymrs_step* are asynchronous on the engine's HIP stream; gymrs_sync() waits.
 *   - One engine is driven by one host thread at a time (the reference's methods take
 *     `&mut self`, core.rs:42-50).  Engines on different GPUs may be driven concurrently.
 *   - N independent envs ("lanes") live as SoA f32 arrays in HBM; lane i of an engine has the
 *     global id global_env_offset + i, which (with the seed and the engine tick) fully
 *     determines its reset draws, so results do not depend on how lanes are sharded over GPUs.
 */
#ifndef GYMRS_AMD_H
#define GYMRS_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 3 (round 5): + gymrs_sharded_*, gymrs_allreduce_stats_multi; - gymrs_copy_probe (a measurement tool now: tools/copy_probe)
 *   additive since, without a version bump (detect by symbol): GYMRS_FINAL_OBS, gymrs_final_obs_ptrs, gymrs_get_final_obs;
 *   the parameter tables gymrs_set_param_table .. gymrs_get_lane_params */
#define GYMRS_ABI_VERSION 3

typedef struct gymrs_engine gymrs_engine; /* opaque; owns device buffers + stream */

typedef enum {
    GYMRS_OK = 0,
    GYMRS_EINVAL = 1,  /* bad argument */
    GYMRS_EHIP = 2,    /* HIP runtime error */
    GYMRS_ENCCL = 3,   /* RCCL error */
    GYMRS_ENOMEM = 4,  /* allocation failed */
    GYMRS_EACTION = 5, /* an action outside the action space was seen (reference: assert! panic,
                          cartpole.rs:402-406, mountain_car.rs:402-406).  The offending lanes' STATE is
                          left untouched (the reference panics before touching the env); their reward /
                          done / truncated entries of that step read 0.  The engine tick still advances
                          for every lane, so with GYMRS_TIME_LIMIT / GYMRS_TRACK_STATS the episode clock
                          and the statistics of a lane whose action was rejected count the rejected
                          step: treat statistics as undefined once GYMRS_EACTION has been reported
                          (the reference would have aborted the process). */
} gymrs_status;

/* classical_control/mod.rs:1-4 exports cartpole and mountain_car.  Pendulum is NOT in the
 * reference (spec-derived from Gym's Pendulum-v1). */
typedef enum { GYMRS_CARTPOLE = 0, GYMRS_MOUNTAIN_CAR = 1, GYMRS_PENDULUM = 2 } gymrs_env_kind;

/* Engine flags.  The reference has none of these behaviours: with flags = 0 a
 * lane behaves exactly like one reference env (no auto-reset, no truncation). */
enum {
    GYMRS_AUTO_RESET = 1u,  /* a lane whose step returned done (or truncated) is re-armed inside
                               the same kernel: the caller loop of examples/cartpole.rs:23-28 */
    GYMRS_TRACK_STATS = 2u, /* accumulate {sum_return, sum_length, n_episodes} of finished episodes
                               (needs GYMRS_AUTO_RESET) */
    GYMRS_TIME_LIMIT = 4u,  /* truncated = (steps in episode >= max_episode_steps); the cap the
                               reference leaves to its callers (examples/cartpole.rs:18) */
    GYMRS_FINAL_OBS = 8u,   /* keep the observation an episode ended in (needs GYMRS_AUTO_RESET):
                               see gymrs_final_obs_ptrs */
};

/* Physics constants: the `pub` fields of the reference env structs, in f64 like the reference
 * (O64).  They are converted to f32 once at engine creation.  Pass NULL for the defaults. */
typedef struct {
    double gravity;                 /* 9.8    cartpole.rs:94  */
    double masscart;                /* 1.0    cartpole.rs:95  */
    double masspole;                /* 0.1    cartpole.rs:96  */
    double length;                  /* 0.5    cartpole.rs:97  */
    double force_mag;               /* 10.0   cartpole.rs:98  */
    double tau;                     /* 0.02   cartpole.rs:99  */
    double theta_threshold_radians; /* 12*2*pi/360  cartpole.rs:102 */
    double x_threshold;             /* 2.4    cartpole.rs:103 */
    int32_t kinematics_integrator;  /* 0 Euler (cartpole.rs:100), 1 Other (cartpole.rs:436-441) */
    uint32_t max_episode_steps;     /* used with GYMRS_TIME_LIMIT; 0 -> 500 (doc cartpole.rs:50) */
} gymrs_cartpole_params;

typedef struct {
    double min_position;  /* -1.2   mountain_car.rs:344 */
    double max_position;  /* 0.6    mountain_car.rs:345 */
    double max_speed;     /* 0.07   mountain_car.rs:346 */
    double goal_position; /* 0.5    mountain_car.rs:347 */
    double goal_velocity; /* 0.0    mountain_car.rs:348 */
    double force;         /* 0.001  mountain_car.rs:350 */
    double gravity;       /* 0.0025 mountain_car.rs:351 */
    uint32_t max_episode_steps; /* 0 -> 200 (doc mountain_car.rs:45) */
    uint32_t _pad;
} gymrs_mountain_car_params;

typedef struct { /* spec-derived (Gym Pendulum-v1), not in the reference */
    double max_speed;  /* 8    */
    double max_torque; /* 2    */
    double dt;         /* 0.05 */
    double g;          /* 10   */
    double m;          /* 1    */
    double l;          /* 1    */
    uint32_t max_episode_steps; /* 0 -> 200 */
    uint32_t _pad;
} gymrs_pendulum_params;

/* Fill *params (a gymrs_*_params of the right kind) with the defaults of CartPoleEnv::new /
 * MountainCarEnv::new (cartpole.rs:91-144, mountain_car.rs:341-390). */
gymrs_status gymrs_default_params(gymrs_env_kind kind, void* params);

/* ---- spaces: EnvProperties::action_space / observation_space (core.rs:86-89) -------------- */
/* Discrete(n) for CartPole (2, cartpole.rs:114) and MountainCar (3, mountain_car.rs:362);
 * *n = 0 for Pendulum, whose action space is the box [-max_torque, max_torque]. */
gymrs_status gymrs_action_space(gymrs_env_kind kind, uint32_t* n, double* box_low, double* box_high);
/* BoxR{low, high}: cartpole.rs:105-115, mountain_car.rs:353-364.  low/high hold *dim doubles
 * (capacity >= 4). */
gymrs_status gymrs_observation_space(gymrs_env_kind kind, const void* params, double* low, double* high,
                                     int* dim);
/* Discrete::contains (spaces/discrete.rs:14-19): value < n. */
int gymrs_discrete_contains(uint64_t n, uint64_t value);

/* ---- lifetime: CartPoleEnv::new / MountainCarEnv::new -------------------------------------- */
/* Like ::new (cartpole.rs:92,120), creation seeds from OS entropy and samples an initial state,
 * so the engine is steppable before the first gymrs_reset(). */
gymrs_status gymrs_engine_create(gymrs_env_kind kind, uint64_t n_envs, uint64_t global_env_offset, int device,
                                 const void* params /* NULL = defaults */, uint32_t flags, gymrs_engine** out);
/* Env::close (core.rs:56) + drop. */
gymrs_status gymrs_engine_destroy(gymrs_engine* e);

/* Use an externally created hipStream_t (e.g. the host framework's) instead of the engine's own. */
gymrs_status gymrs_set_stream(gymrs_engine* e, void* hip_stream);
gymrs_status gymrs_get_stream(gymrs_engine* e, void** hip_stream);

/* ---- Env::reset(seed, return_info, options) (core.rs:45-50) -------------------------------- */
/* has_seed = 0 re-seeds from OS entropy (seeding.rs:22); the same seed always gives the same
 * states.  bounds_low_high = obs_dim lows then obs_dim highs replacing the default
 * sampling box (`options`, cartpole.rs:352-364, mountain_car.rs:175-190), or NULL.  The box stays in force for
 * every GYMRS_AUTO_RESET re-arm until the next reset (NULL returns to the default box); clones and snapshots carry it.
 * Every sampled component (MountainCar: the position only) needs finite low < high, a finite f32 width high - low
 * ([-1.5e38, 1.5e38) is accepted, [-2e38, 2e38) is not) and a width of at least 2^-102, so that the step of a draw,
 * width * 2^-24, is a normal float: GYMRS_EINVAL otherwise, and the engine keeps the box it had.  The same rule holds
 * for the f32 box gymrs_reset_pcg64 keeps for the re-arms.
 * *seed_used (may be NULL) receives the seed number, like rand_random's second return value
 * (seeding.rs:21-26). */
gymrs_status gymrs_reset(gymrs_engine* e, int has_seed, uint64_t seed, const float* bounds_low_high,
                         uint64_t* seed_used);
/* Optional: the same reset, but every lane draws its state from the REFERENCE's own generator chain instead of the
 * Philox reset stream: `Pcg64::seed_from_u64(s)` (seeding.rs:21-26) and `Uniform::new(low, high).sample(rng)` over
 * f64 (cartpole.rs:293-297,317-324,352-364; mountain_car.rs:145,162-167,175-190), so that lane i holds, rounded once
 * to f32, the state the reference's `reset(Some(s), _, options)` returns for
 *     s = seeds_dev[i]                       (n_envs seed numbers on the device), or, with seeds_dev = NULL,
 *     s = seed + global_env_offset + i       (wrapping; a one-lane engine at offset 0 is the reference env itself).
 * bounds_low_high = obs_dim lows then obs_dim highs in f64 (the reference's BoxR is f64), or NULL for the defaults.
 * CartPole and MountainCar only (the reference has no Pendulum): GYMRS_EINVAL otherwise.  Everything else -- cleared
 * flags, statistics, the seed echo, the Philox key of later GYMRS_AUTO_RESET re-arms -- is as for gymrs_reset.
 * The third-party algorithms (rand 0.8, rand_pcg 0.3, rand_core 0.6) are restated from their publications and pinned
 * by rand_pcg's own known answers (tests/golden/pcg64.json); SURVEY App. B.2.
 * Rounding: the reference's f64 draw lies in [low, high); this call stores its NEAREST f32, so that a caller comparing start
 * states with gym-rs sees every component within half an f32 ulp of the reference's.  The stored value therefore lies in the
 * CLOSED f32 box [fl32(low), fl32(high)]: a draw within half an ulp of `high` rounds onto fl32(high) (probability ~2^-25 per
 * draw), which may exceed `high` itself (fl32(0.05) > 0.05).  gymrs_reset (Philox) keeps its samples strictly below
 * fl32(high); later GYMRS_AUTO_RESET re-arms of an engine reset through this call use that half-open f32 box. */
gymrs_status gymrs_reset_pcg64(gymrs_engine* e, int has_seed, uint64_t seed, const uint64_t* seeds_dev,
                               const double* bounds_low_high, uint64_t* seed_used);

/* ---- Env::step(action) (core.rs:42) --------------------------------------------------------- */
/* actions_dev: n_envs actions on the device: uint8_t for CartPole {0,1} / MountainCar {0,1,2},
 * float for Pendulum.  Asynchronous.  Results land in the arrays below.
 * (One exception to "asynchronous": a CartPole engine with all three flags runs the launches that cannot take any lane to
 * the time limit without the limit check, and learns the age of the oldest open episode from the device a few launches
 * before that knowledge runs out.  A caller that has queued steps far ahead of the GPU may wait in this call until the
 * GPU has reached that refresh -- at most once per approach to the limit; the queue does not run dry.)
 * Alignment: a buffer aligned to lanes_per_thread * sizeof(action) bytes (4 or 8 B for u8 actions, 16 or 32 B
 * for f32; any hipMalloc / torch allocation is) is read with one vector load per work-item.  Any other address
 * is accepted too and read lane by lane (every wavefront then takes the guarded per-lane code: correct, slower).
 * The same holds for every ring slot actions_dev + k * stride_bytes of gymrs_step_many. */
gymrs_status gymrs_step(gymrs_engine* e, const void* actions_dev);
/* Same with a host action buffer (copied first); for the single-env compatibility layer. */
gymrs_status gymrs_step_host(gymrs_engine* e, const void* actions_host);
/* n_steps consecutive step() calls; step t reads its actions at
 * actions_dev + (t % n_buffers) * stride_bytes.  use_graph != 0 replays a captured HIP graph of >= 32 steps
 * (a whole number of passes over the action ring; the remainder is launched eagerly): worth it when the step
 * kernel is shorter than a host launch (~3 us, i.e. small batches); results are identical.  Not available
 * for Pendulum with GYMRS_TIME_LIMIT (GYMRS_EINVAL).
 * Submission (round 6): HIP launches on the engine's stream -- every step's arrays are released when its launch ends, exactly what a loop of
 * gymrs_step enqueues.  GYMRS_AQL=1 in the environment OPTS IN to chains on the engine's own HSA queue (release only at the end of the call,
 * 25 % less per launch; one process per GPU: INTEGRATION.md "gymrs_step_many"); results are the same bits either way. */
gymrs_status gymrs_step_many(gymrs_engine* e, const void* actions_dev, uint64_t stride_bytes,
                             uint32_t n_buffers, uint32_t n_steps, int use_graph);
/* Fused random-policy rollout: exactly the effect of
 *     for (k = 0; k < n_steps; ++k) { gymrs_fill_actions(e, buf, action_seed, action_t0 + k); gymrs_step(e, buf); }
 * in ONE kernel launch with the state held in registers (the caller loop of examples/cartpole.rs:15-30 --
 * `rng.gen_range`, `step`, `reset` on done, `episode reward +=` -- for every lane).  Afterwards the state, the
 * reward/done/truncated arrays (those of the LAST step), the statistics and the tick are bit-identical to that
 * loop; the intermediate observations are never materialised, which is why this is a separate entry point and
 * not what bench.py's headline measures.  VALU-bound instead of HBM-bound. */
gymrs_status gymrs_rollout(gymrs_engine* e, uint32_t n_steps, uint64_t action_seed, uint64_t action_t0);
/* gymrs_rollout that also keeps the trajectory: what a random-policy data-collection loop around Env::step stores
 * (examples/cartpole.rs:15-30 with the observation, action, reward and done of every step kept).  Row k of each
 * buffer is step k; a row holds lane_stride lanes (>= n_envs, a multiple of 16); all buffers are device memory,
 * 16-byte aligned:
 *   obs      [n_steps][obs_dim][lane_stride] f32   observation AFTER the step (a re-armed lane shows its fresh state,
 *                                                  exactly what gymrs_obs_ptrs would show after that step)
 *   actions  [n_steps][lane_stride] u8 (f32 for Pendulum)   the action taken
 *   reward   [n_steps][lane_stride] f32,  done [n_steps][lane_stride] u8
 *   truncated[n_steps][lane_stride] u8    written with GYMRS_TIME_LIMIT only; may be NULL
 * Everything else is as gymrs_rollout (engine arrays, statistics and tick end up identical). */
typedef struct {
    float* obs;
    void* actions;
    float* reward;
    uint8_t* done;
    uint8_t* truncated;
    uint64_t lane_stride;
} gymrs_trajectory;
gymrs_status gymrs_rollout_record(gymrs_engine* e, uint32_t n_steps, uint64_t action_seed, uint64_t action_t0,
                                  const gymrs_trajectory* out);
/* `Env: Clone + Serialize` (core.rs:25; the serde-visible fields of cartpole.rs:51-87 / mountain_car.rs:46-80).
 * gymrs_engine_clone: a second engine (own stream, same device) with a deep copy of everything a step can observe:
 * lane state, episode bookkeeping, statistics, physics constants, reset box and the RNG position (seed, tick).
 * Like the reference's Clone (which drops the GUI handle, screen.rs:66-77) it does not copy the HIP stream binding,
 * the RCCL communicator or a captured graph.
 * gymrs_snapshot_*: the same content as an opaque host blob of gymrs_snapshot_size() bytes.  Loading requires an
 * engine created with the same kind, n_envs and flags (GYMRS_EINVAL otherwise); physics constants, reset box,
 * global_env_offset, seed and tick come from the snapshot.  A restored or cloned engine continues bit-identically
 * to the original. */
gymrs_status gymrs_engine_clone(gymrs_engine* src, gymrs_engine** out);
gymrs_status gymrs_snapshot_size(gymrs_engine* e, uint64_t* bytes);
gymrs_status gymrs_snapshot_save(gymrs_engine* e, void* host_buf, uint64_t bytes);
gymrs_status gymrs_snapshot_load(gymrs_engine* e, const void* host_buf, uint64_t bytes);
/* Wait for the stream; returns GYMRS_EACTION if any step since the last sync saw an invalid action. */
gymrs_status gymrs_sync(gymrs_engine* e);

/* ---- ActionReward{observation, reward, done, truncated} (core.rs:94-106), batched ------------ */
/* Zero-copy SoA device views, valid until destroy.  CartPole obs = (x, x_dot, theta, theta_dot)
 * (cartpole.rs:336-349), MountainCar obs = (position, velocity) (mountain_car.rs:193-197); for
 * these the observation IS the state array.  Pendulum obs = (cos, sin, theta_dot).
 * The views are for READING: a step does not rewrite an output that already holds the right value (MountainCar's -1.0,
 * CartPole's 1.0 on engines of >= 2^22 lanes, Pendulum's done / uniform truncated flag), so whoever overwrites the reward or
 * flag arrays between two steps finds them repaired only by gymrs_reset or a snapshot load. */
gymrs_status gymrs_obs_ptrs(gymrs_engine* e, float** out_ptrs /* capacity 4 */, int* obs_dim);
gymrs_status gymrs_state_ptrs(gymrs_engine* e, float** out_ptrs /* capacity 4 */, int* state_dim);
gymrs_status gymrs_reward_ptr(gymrs_engine* e, float** out);
gymrs_status gymrs_done_ptr(gymrs_engine* e, uint8_t** out);
gymrs_status gymrs_truncated_ptr(gymrs_engine* e, uint8_t** out);
/* GYMRS_FINAL_OBS: the observation each lane's most recently finished episode ended in -- what a Gymnasium vector env
 * returns as `final_obs`, and what a learner bootstraps a truncated episode from.  The engine owns obs_dim
 * SoA f32 arrays of n_envs lanes, laid out like gymrs_obs_ptrs: CartPole (x, x_dot, theta, theta_dot), MountainCar
 * (position, velocity), Pendulum (cos, sin, theta_dot).
 *   - When lane i returns done or truncated in a step (and is therefore re-armed), row i receives, bit for bit, the
 *     observation lane i would have shown after that step without GYMRS_AUTO_RESET.  Rows of lanes that did not finish
 *     in that step are not written; a lane whose action was rejected (GYMRS_EACTION) is not stepped and not written.
 *   - gymrs_engine_create, gymrs_reset and gymrs_reset_pcg64 set every row to 0.0f; gymrs_set_state leaves them alone.
 *   - Every stepping path keeps them: gymrs_step / _host / _many (eager, use_graph; with this flag gymrs_step_many always
 *     submits HIP launches, GYMRS_AQL is not consulted), gymrs_rollout / _record (the arrays end as the equivalent
 *     fill_actions + step loop leaves them; trajectories are unchanged), the blocks of a sharded engine.  Clone and
 *     snapshot carry them (the snapshot of an engine without the flag is unchanged).
 * Both calls return GYMRS_EINVAL on an engine created without the flag. */
gymrs_status gymrs_final_obs_ptrs(gymrs_engine* e, float** out_ptrs /* capacity 4 */, int* obs_dim);

/* Host copies (synchronising).  SoA: dim arrays of `count` floats, back to back.
 * get/set_state is the engine's Clone/Serialize equivalent (core.rs:25). */
gymrs_status gymrs_get_obs(gymrs_engine* e, uint64_t first, uint64_t count, float* host_out);
gymrs_status gymrs_get_final_obs(gymrs_engine* e, uint64_t first, uint64_t count, float* host_out);
gymrs_status gymrs_get_state(gymrs_engine* e, uint64_t first, uint64_t count, float* host_out);
gymrs_status gymrs_set_state(gymrs_engine* e, uint64_t first, uint64_t count, const float* host_in);
gymrs_status gymrs_get_step_result(gymrs_engine* e, uint64_t first, uint64_t count, float* reward,
                                   uint8_t* done, uint8_t* truncated /* each may be NULL */);

/* ---- episode statistics (the all-reduce payload) --------------------------------------------- */
/* out = {sum_return, sum_length, n_episodes, n_steps} for this engine's lanes since the last gymrs_stats_clear / gymrs_reset (synchronising).
 * The read-out writes nothing a step reads (round 6): gymrs_stats_clear remembers the totals as a baseline that later read-outs subtract (integers:
 * exact; Pendulum's sum_return: a difference of two f64 sums) -- asynchronous on the engine's stream, no counter is zeroed. */
gymrs_status gymrs_stats(gymrs_engine* e, double out[4]);
gymrs_status gymrs_stats_clear(gymrs_engine* e);
/* Reduce the per-workgroup partials into 4 doubles in device memory (async on the engine's stream)
 * and return that device address, e.g. to hand it to an RCCL all-reduce. */
gymrs_status gymrs_stats_device(gymrs_engine* e, double** dev_out4);

/* RCCL over xGMI: one process per GPU.  Rank 0 makes an id, the host framework distributes the
 * 128 bytes, every rank joins, then gymrs_allreduce_stats sums the 4 doubles over all ranks. */
gymrs_status gymrs_comm_unique_id(uint8_t id_out[128]);
gymrs_status gymrs_comm_init(gymrs_engine* e, int n_ranks, int rank, const uint8_t id[128]);
gymrs_status gymrs_allreduce_stats(gymrs_engine* e, double out[4]);

/* ---- one batch over several GPUs, in ONE process ------------------------------------------- */
/* The in-process form of gymrs_allreduce_stats (`gymrs_allreduce_stats(gymrs_engine** shards, int n, double out[4])`): one host
 * thread holds every shard of a batch.  Shards on n DISTINCT devices: one RCCL communicator over exactly these engines (made on the first
 * call, all ranks inside one ncclGroupStart/End -- a bare gymrs_comm_init per engine from one thread would wait for the other ranks for
 * ever), then n grouped all-reduces of 32 bytes over xGMI, each on its engine's stream.  Shards sharing a device (RCCL refuses two ranks
 * on one GPU) or n = 1: the same four doubles are summed on the host.  *used_rccl (may be NULL) says which: 1 RCCL, 0 the host-side sum, -1 the
 * host-side sum BECAUSE RCCL could not be loaded or its communicator could not be made (round 6: first contact with RCCL does not cost the caller
 * its result; gymrs_last_error() then holds RCCL's message although the status is GYMRS_OK).  Synchronising; the calling thread's current HIP device
 * is left on the last shard's. */
gymrs_status gymrs_allreduce_stats_multi(gymrs_engine** shards, int n, double out[4], int* used_rccl);

/* A batch of n_total lanes cut into n_shards contiguous blocks, one engine per block on devices[r] (NULL = devices 0 .. n_shards-1; a
 * device may appear more than once), lane i of the batch carrying the global id global_env_offset + i whatever the cut -- so every result
 * below is bit-identical to ONE engine of n_total lanes (one exception: Pendulum's sum_return is a float sum over wavefront slots, and k engines
 * add their slots in another order than one -- equal to ~1e-12 relative; every integer statistic, every state bit, every reward / flag is identical).
 * Blocks are whole 1024-lane tiles dealt evenly (the first `tiles % n_shards` blocks hold one more), the ragged tail in the last.  Each engine is driven by its own host thread, bound to its device, for its
 * whole life: the calls below hand one command to every thread and return when all have ENQUEUED (the step calls stay asynchronous on
 * each engine's stream).  One gymrs_sharded is driven by one caller thread at a time (`&mut self`, core.rs:42-50).
 * Creation seeds every block with ONE OS-entropy seed (cartpole.rs:92,120).  Error messages name the shard and its device. */
typedef struct gymrs_sharded gymrs_sharded;
gymrs_status gymrs_sharded_create(gymrs_env_kind kind, uint64_t n_total, uint64_t global_env_offset, int n_shards,
                                  const int* devices, const void* params, uint32_t flags, gymrs_sharded** out);
gymrs_status gymrs_sharded_destroy(gymrs_sharded* h);
gymrs_status gymrs_sharded_count(gymrs_sharded* h, int* n_shards);
/* Block r: its engine (for the zero-copy views gymrs_obs_ptrs / gymrs_reward_ptr / ... and the stream; do not step it directly while
 * the sharder is in use), its first lane within the batch, its lane count and its device.  Any out pointer may be NULL. */
gymrs_status gymrs_sharded_shard(gymrs_sharded* h, int shard, gymrs_engine** engine, uint64_t* first_lane,
                                 uint64_t* n_lanes, int* device);
/* Env::reset for the whole batch: gymrs_reset on every block with the same seed (has_seed = 0: one fresh OS seed). */
gymrs_status gymrs_sharded_reset(gymrs_sharded* h, int has_seed, uint64_t seed, const float* bounds_low_high,
                                 uint64_t* seed_used);
/* Env::step / n_steps of them: actions_dev[r] = block r's action buffer (ring) ON ITS DEVICE, laid out as for gymrs_step / gymrs_step_many. */
gymrs_status gymrs_sharded_step(gymrs_sharded* h, const void* const* actions_dev);
gymrs_status gymrs_sharded_step_many(gymrs_sharded* h, const void* const* actions_dev, uint64_t stride_bytes,
                                     uint32_t n_buffers, uint32_t n_steps, int use_graph);
gymrs_status gymrs_sharded_fill_actions(gymrs_sharded* h, void* const* actions_dev, uint64_t seed, uint64_t t);
/* gymrs_rollout / gymrs_set_params on every block (the rollout's action stream is keyed by global lane ids: same bits as one engine). */
gymrs_status gymrs_sharded_rollout(gymrs_sharded* h, uint32_t n_steps, uint64_t action_seed, uint64_t action_t0);
gymrs_status gymrs_sharded_set_params(gymrs_sharded* h, const void* params);
/* Waits for every block's stream; GYMRS_EACTION etc. as gymrs_sync (the first failing shard is reported). */
gymrs_status gymrs_sharded_sync(gymrs_sharded* h);
/* {sum_return, sum_length, n_episodes, n_steps} of the whole batch = gymrs_allreduce_stats_multi over the blocks. */
gymrs_status gymrs_sharded_stats(gymrs_sharded* h, double out[4]);
gymrs_status gymrs_sharded_stats_clear(gymrs_sharded* h);
/* "rccl" | "host" | "host (RCCL unavailable, ...: <RCCL's message>)" | "none": how the last gymrs_sharded_stats summed. */
const char* gymrs_sharded_reduce_path(gymrs_sharded* h);
/* Host copies over lanes [first, first + count) of the BATCH, laid out exactly as gymrs_get_state / gymrs_get_step_result lay out an
 * engine's lanes (SoA: state_dim arrays of `count` floats back to back).  Synchronising. */
gymrs_status gymrs_sharded_get_state(gymrs_sharded* h, uint64_t first, uint64_t count, float* host_out);
gymrs_status gymrs_sharded_get_step_result(gymrs_sharded* h, uint64_t first, uint64_t count, float* reward,
                                           uint8_t* done, uint8_t* truncated /* each may be NULL */);

/* ---- the `pub` physics fields after construction (cartpole.rs:53-82, mountain_car.rs:49-62) --- */
/* In the reference the constants are public struct fields: `env.gravity = ...` between two step() calls touches
 * nothing else -- state, steps_beyond_terminated, the episode clock and the PRNG carry on (cartpole.rs:455-464 reads
 * the fields afresh on every step).  gymrs_set_params is that assignment for every lane of the engine: only the
 * constants change (the next launch uses them; a captured HIP graph is dropped); no device array, no tick, no
 * statistics are touched.  params = the env kind's params struct (not NULL).  gymrs_get_params reads them back
 * in f64 exactly as they were set (the f32 conversion happens per launch-constant block, not in this copy). */
gymrs_status gymrs_set_params(gymrs_engine* e, const void* params);
gymrs_status gymrs_get_params(gymrs_engine* e, void* params_out);

/* ---- per-lane physics: parameter tables (CartPole, MountainCar) ------------------------------------------------------- */
/* In the reference every env value has its own pub fields, so a Vec<CartPoleEnv> can give each env its own pole length or
 * gravity (domain randomisation).  A parameter table is that for the lanes of one engine: K rows of the kind's params struct
 * (1 <= K <= 65536) and a per-lane index, uint16_t[n_envs] in device memory; lane i steps with row index[i].  Lane i gives
 * the same bits as lane i of an engine created with params = row[index[i]] (same size, offset, flags, seed and actions):
 * state, reward, done, truncated, final observations, steps_beyond_terminated; the episode statistics are sums over lanes.
 *   - Every row passes the checks of gymrs_set_params, and all rows share max_episode_steps and (CartPole)
 *     kinematics_integrator: otherwise GYMRS_EINVAL, naming the first row that differs.  Pendulum: GYMRS_EINVAL.
 *   - The first gymrs_set_param_table switches table mode on, with every index 0.  gymrs_set_param_table(e, NULL, 0) or
 *     gymrs_set_params switch it off: every lane uses one set again (after (NULL, 0): row 0).  While a table is active,
 *     gymrs_get_params reports row 0 and gymrs_step_many submits HIP launches (GYMRS_AQL is not consulted).
 *   - A table change is a gymrs_set_params: only constants change, in stream order (steps enqueued before the call use
 *     the old rows); the caller may free `rows` when the call returns.  A captured HIP graph is dropped.
 *   - Reset draws do not depend on the physics fields: the resets and auto-reset re-arms are unchanged.  Rewriting the
 *     index of lanes that just finished gives per-episode randomisation.
 *   - A lane whose index is >= K is not stepped and reads nothing outside the table: like an invalid action, the next
 *     gymrs_sync returns GYMRS_EACTION naming the lowest such lane ("invalid action or parameter index").
 *   - gymrs_engine_clone copies table and index; a snapshot of an engine with a table is version 5 (v4 + table + index).
 * gymrs_get_param_table: *k = K (0: no table); rows_out receives the K rows in f64 exactly as set (capacity >= K; rows_out
 * NULL with capacity 0 only asks for K).  gymrs_param_index_ptr: zero-copy device view of the index, under the stream rules of
 * the other *_ptr views (a kernel on the engine's stream may rewrite it between two steps).  gymrs_set_param_index /
 * gymrs_get_param_index: host copies of lanes [first, first + count) (synchronising).  These three need a table.
 * gymrs_get_lane_params: the params lane `lane` steps with (row index[lane]; without a table, gymrs_get_params).
 * Which calls honour the table: gymrs_step / gymrs_step_many / gymrs_rollout / gymrs_rollout_record (every flag set), and
 * gymrs_evaluate_policy with GYMRS_EVAL_LANE_PARAMS ("episodic policy evaluation" below) and gymrs_rollout_closed_loop with
 * GYMRS_CLOSED_LOOP_LANE_PARAMS ("closed-loop rollouts behind one descriptor" below).  gymrs_rollout_policy, _record and
 * _fitness refuse an active table (they take no flags word through which a caller could opt in).
 * A sharded batch (gymrs_sharded_*): gymrs_sharded_set_param_table puts the SAME k rows on every block (rows = NULL, k = 0
 * switches the table off); gymrs_sharded_get_param_table reads them back from block 0.  gymrs_sharded_set_param_index /
 * gymrs_sharded_get_param_index copy lanes [first, first + count) in BATCH lane numbering, split across the blocks the way
 * gymrs_sharded_get_state splits its ranges (a range beyond the batch: GYMRS_EINVAL; they need a table).  Lane i of the batch
 * then steps, rolls out and is evaluated exactly as lane i of one engine with that table and index. */
gymrs_status gymrs_set_param_table(gymrs_engine* e, const void* rows /* k x gymrs_<kind>_params */, uint32_t k);
gymrs_status gymrs_get_param_table(gymrs_engine* e, void* rows_out, uint32_t capacity, uint32_t* k);
gymrs_status gymrs_param_index_ptr(gymrs_engine* e, uint16_t** out);
gymrs_status gymrs_set_param_index(gymrs_engine* e, uint64_t first, uint64_t count, const uint16_t* host_in);
gymrs_status gymrs_get_param_index(gymrs_engine* e, uint64_t first, uint64_t count, uint16_t* host_out);
gymrs_status gymrs_get_lane_params(gymrs_engine* e, uint64_t lane, void* params_out);
gymrs_status gymrs_sharded_set_param_table(gymrs_sharded* h, const void* rows /* k x gymrs_<kind>_params */, uint32_t k);
gymrs_status gymrs_sharded_get_param_table(gymrs_sharded* h, void* rows_out, uint32_t capacity, uint32_t* k);
gymrs_status gymrs_sharded_set_param_index(gymrs_sharded* h, uint64_t first, uint64_t count, const uint16_t* index_host);
gymrs_status gymrs_sharded_get_param_index(gymrs_sharded* h, uint64_t first, uint64_t count, uint16_t* index_out);

/* ---- closed-loop rollouts: a small policy evaluated inside the kernel (CartPole, MountainCar) ----------------------------- */
/* gymrs_rollout plays the random policy only.  With a policy set, gymrs_rollout_policy advances n_steps steps in ONE launch with
 * actions computed from each lane's own observation, step after step, state in registers: population evaluation (evolution
 * strategies, random search, PBT) and on-policy data collection with a small policy (gymrs_rollout_policy_record).
 * The policy, defined to the bit.  D = observation size (4 / 2), A = number of actions (2 / 3), H = hidden width, 0 <= H <= 64;
 * all f32; x[0..D) = the lane's observation in gymrs_obs_ptrs order; fmaf = the fused multiply-add with ONE rounding, nothing else
 * is contracted or reordered:
 *     H == 0 (affine):    y[a] = b[a];  for j = 0..D-1: y[a] = fmaf(W[a][j], x[j], y[a])            for a = 0..A-1
 *     H  > 0 (one layer): y[a] = b2[a]                                                              for a = 0..A-1
 *                         for h = 0..H-1:
 *                             z = b1[h];  for j = 0..D-1: z = fmaf(W1[h][j], x[j], z)
 *                             r = (z > 0.0f) ? z : 0.0f                 (compare-select: NaN and -0 give +0)
 *                             for a = 0..A-1: y[a] = fmaf(W2[a][h], r, y[a])
 *     action = 0;  for a = 1..A-1: if (y[a] > y[action]) action = a     (first maximum; NaN never wins)
 * One policy is S consecutive floats, row-major: H == 0: W[A][D], b[A] (S = A*(D+1): 10 / 9); H > 0: W1[H][D], b1[H], W2[A][H],
 * b2[A] (S = H*(D+1) + A*(H+1); CartPole H = 16: 114).  gymrs_policy_size returns S (host only, no GPU; GYMRS_EINVAL for
 * Pendulum and hidden > 64).
 * A policy set is n_policies >= 1 policies back to back (n_policies * S floats) and a block size lanes_per_policy >= 1: lane i
 * of the engine uses policy ((global_env_offset + i) / lanes_per_policy) % n_policies -- keyed by the global id like the reset
 * and action streams, so the result does not depend on how a batch is cut into engines.
 *   - gymrs_set_policy copies the set to an engine-owned device buffer in stream order (launches enqueued before it use the old
 *     set; the caller may free weights_host on return: the call waits for its own copy, so it synchronises the engine's
 *     stream).  d == NULL removes the policy.  GYMRS_EINVAL: Pendulum, hidden > 64,
 *     n_policies == 0, lanes_per_policy == 0, NULL weights.  Non-finite weights are legal (the definition above says what they
 *     do).  It touches no lane state, tick or statistics.  gymrs_get_policy reads the set back (weights_out NULL with capacity 0
 *     only asks for the description; synchronising).
 *   - gymrs_policy_weights_ptr: zero-copy device view of the n_policies * S floats (*n_floats, may be NULL) under the stream
 *     rules of the other *_ptr views: a learner on the engine's stream rewrites weights in place and the next launch reads
 *     them.  Valid until the next gymrs_set_policy or destroy.
 *   - gymrs_policy_actions: one launch; writes n_envs uint8_t actions computed from the current observations to actions_dev (the
 *     per-step counterpart, as gymrs_fill_actions is to gymrs_rollout).  It only reads observations, so it also works while a
 *     parameter table is active.
 *   - gymrs_rollout_policy(e, K): exactly the effect of `for k in 0..K: gymrs_policy_actions(e, buf); gymrs_step(e, buf);` in ONE
 *     launch: state, reward / done / truncated of the last step, final observations, statistics, steps_beyond_terminated, tick.
 *     Every flag set gymrs_rollout accepts, both lanes_per_thread values, any n_envs and any global_env_offset.  K == 0 is a
 *     no-op.  gymrs_rollout_policy_record is to it what gymrs_rollout_record is to gymrs_rollout (same gymrs_trajectory, same
 *     buffer checks, same rows; the `actions` rows hold the policy's actions).
 *   - Without a policy set, the three stepping calls, gymrs_get_policy and gymrs_policy_weights_ptr return GYMRS_EINVAL.  While a
 *     parameter table is active, gymrs_rollout_policy / _record return GYMRS_EINVAL and say so (the per-step loop covers it, and
 *     gymrs_rollout_closed_loop below does it in one launch).
 *   - The policy is NOT part of gymrs_engine_clone or of a snapshot (its bytes and version are unchanged): set it again on the
 *     clone or the restored engine.  The sharded layer mirrors the set / rollout / fitness calls (gymrs_sharded_set_policy ...). */
typedef struct { uint32_t hidden; uint32_t n_policies; uint64_t lanes_per_policy; } gymrs_policy_desc;
gymrs_status gymrs_policy_size(gymrs_env_kind kind, uint32_t hidden, uint64_t* n_floats);
gymrs_status gymrs_set_policy(gymrs_engine* e, const gymrs_policy_desc* d, const float* weights_host);
gymrs_status gymrs_get_policy(gymrs_engine* e, gymrs_policy_desc* d_out, float* weights_out, uint64_t capacity_floats);
gymrs_status gymrs_policy_weights_ptr(gymrs_engine* e, float** dev_out, uint64_t* n_floats);
gymrs_status gymrs_policy_actions(gymrs_engine* e, void* actions_dev);
gymrs_status gymrs_rollout_policy(gymrs_engine* e, uint32_t n_steps);
gymrs_status gymrs_rollout_policy_record(gymrs_engine* e, uint32_t n_steps, const gymrs_trajectory* out);
/* Per-policy fitness: what a population search needs back from the device, counted inside the kernel.
 * gymrs_rollout_policy_fitness(e, K) leaves the engine bit for bit as gymrs_rollout_policy(e, K) does (state, reward / done /
 * truncated of the last step, final observations, statistics, steps_beyond_terminated, tick) and additionally, for every policy p,
 * every step k of the launch and every lane i of this engine with ((global_env_offset + i) / lanes_per_policy) % n_policies == p,
 * with reward, done, truncated = the values gymrs_rollout_policy_record would have written to its rows for (k, i):
 *     fitness[p].reward_sum += (int64)reward          (CartPole pays 0 or 1, MountainCar -1: the conversion is exact)
 *     fitness[p].episodes   += (done | truncated) != 0
 *     fitness[p].done       += done
 *     fitness[p].truncated  += truncated              (0 without GYMRS_TIME_LIMIT)
 * Integer sums: exact, independent of the order of addition and of how a batch is cut into engines (add the records of the
 * engines).  done and truncated can both be set in one step, hence `episodes`.  Without auto-reset the counters still follow the
 * rows (CartPole's reward_sum is then the steps survived: the reward is 0 beyond termination).  The counters are accumulated in
 * 32-bit registers over the launch and added to the table with 64-bit integer atomics once per launch, so
 * n_steps <= GYMRS_POLICY_FITNESS_MAX_STEPS (GYMRS_EINVAL above it; split the launch).  Every flag set gymrs_rollout_policy
 * accepts, both lanes_per_thread values, any n_envs and any global_env_offset; K == 0 is a no-op.
 *   - The table holds n_policies records.  It comes into being, zeroed, at the first of the four calls below after a
 *     gymrs_set_policy (not in gymrs_set_policy: 2^20 one-lane policies would pay 32 MB they may never use); every
 *     gymrs_set_policy discards it (removal included): the next use sees zeros.  Where the new set has the same n_policies -- a
 *     search's next generation -- the memory is kept and zeroed in stream order; otherwise gymrs_set_policy waits for the
 *     engine's stream and frees it.  gymrs_reset, gymrs_rollout_policy, _record, gymrs_step and the statistics calls do not
 *     touch it.
 *   - gymrs_policy_fitness_clear zeroes it in stream order.  gymrs_get_policy_fitness copies records [first, first + count) to
 *     the host and synchronises.  gymrs_policy_fitness_ptr: zero-copy device view (*n_policies may be NULL) under the stream rules
 *     of the other *_ptr views, valid until the next gymrs_set_policy or destroy.
 *   - GYMRS_EINVAL: NULL arguments, no policy set, first + count > n_policies, Pendulum (it takes no policy), an active parameter
 *     table (gymrs_rollout_policy_fitness: as gymrs_rollout_policy), n_steps above the bound.
 *   - Not part of gymrs_engine_clone or of a snapshot (like the policy; snapshot bytes and version are unchanged). */
#define GYMRS_POLICY_FITNESS_MAX_STEPS (1u << 24)
typedef struct { int64_t reward_sum; uint64_t episodes; uint64_t done; uint64_t truncated; } gymrs_policy_fitness; /* 32 B */
gymrs_status gymrs_rollout_policy_fitness(gymrs_engine* e, uint32_t n_steps);
gymrs_status gymrs_policy_fitness_ptr(gymrs_engine* e, gymrs_policy_fitness** dev_out, uint32_t* n_policies);
gymrs_status gymrs_get_policy_fitness(gymrs_engine* e, uint32_t first, uint32_t count, gymrs_policy_fitness* host_out);
gymrs_status gymrs_policy_fitness_clear(gymrs_engine* e);
/* The same on a sharded batch (gymrs_sharded_*): every block gets the same policy set -- the global-id key makes the batch do
 * what one engine would -- and the calls run on every block through its worker.  gymrs_sharded_get_policy_fitness sums the
 * blocks' records on the host (integers: exact) and synchronises; every block keeps a table of its own, so a population of
 * n_policies costs n_shards * n_policies * 32 B of device memory once fitness is used. */
gymrs_status gymrs_sharded_set_policy(gymrs_sharded* h, const gymrs_policy_desc* d, const float* weights_host);
gymrs_status gymrs_sharded_rollout_policy(gymrs_sharded* h, uint32_t n_steps);
gymrs_status gymrs_sharded_rollout_policy_fitness(gymrs_sharded* h, uint32_t n_steps);
gymrs_status gymrs_sharded_get_policy_fitness(gymrs_sharded* h, uint32_t first, uint32_t count, gymrs_policy_fitness* host_out);
gymrs_status gymrs_sharded_policy_fitness_clear(gymrs_sharded* h);
/* Closed-loop rollouts behind one descriptor, and under per-lane physics (policy x table).
 * gymrs_rollout_closed_loop(e, d) is the three fused closed-loop calls above behind a descriptor with a flags word: d->n_steps = K,
 * d->record (may be NULL) = the trajectory of gymrs_rollout_policy_record, GYMRS_CLOSED_LOOP_FITNESS in d->flags = the counters of
 * gymrs_rollout_policy_fitness.
 *   - No parameter table active: bit-identical to the call the descriptor stands for -- gymrs_rollout_policy(e, K); with record
 *     != NULL gymrs_rollout_policy_record(e, K, record); with GYMRS_CLOSED_LOOP_FITNESS gymrs_rollout_policy_fitness(e, K) -- with or
 *     without GYMRS_CLOSED_LOOP_LANE_PARAMS (the same kernels are launched), so a training loop may set that flag unconditionally,
 *     as with GYMRS_EVAL_LANE_PARAMS.
 *   - A table active, GYMRS_CLOSED_LOOP_LANE_PARAMS not set: GYMRS_EINVAL naming the flag (a plain descriptor is never played
 *     with a table behind the caller's back).
 *   - A table active and the flag set: exactly the effect of `for k in 0..K: gymrs_policy_actions(e, buf); gymrs_step(e, buf);` on
 *     this engine, in ONE launch: state, reward / done / truncated of the last step, final observations, statistics,
 *     steps_beyond_terminated, tick.  Lane i steps with rows[index[i]] ("per-lane physics"); rows and index are read in stream
 *     order (an index rewritten through gymrs_param_index_ptr on the engine's stream is seen by the next launch).  Every flag
 *     set gymrs_rollout accepts, both lanes_per_thread values (recording runs at 4, like every recording kernel), any n_envs and
 *     any global_env_offset; the policy of a lane is chosen by its global id as above.  The rows of `record` and the fitness
 *     counters are defined as above ("the values gymrs_rollout_policy_record would have written").
 *   - A lane whose index is >= K (possible through the zero-copy view only) is treated as gymrs_rollout treats it: it is not
 *     stepped, pays 0 and sets no flag in every step of the launch (its record rows say so), adds nothing to any fitness
 *     record, and the next gymrs_sync returns GYMRS_EACTION naming the lowest such lane.
 *   - GYMRS_EINVAL: NULL engine or desc, no policy set, Pendulum, reserved != 0, unknown flag bits (bits 1 and 3 are not assigned;
 *     bit 4 is GYMRS_CLOSED_LOOP_EXPLORE, "exploration" below; bit 5 is GYMRS_CLOSED_LOOP_SAMPLE, "sampling" below),
 *     GYMRS_CLOSED_LOOP_FITNESS together with a record (there is no recording fitness kernel), a record that fails the buffer
 *     checks of gymrs_rollout_policy_record, n_steps > GYMRS_POLICY_FITNESS_MAX_STEPS with GYMRS_CLOSED_LOOP_FITNESS.  n_steps == 0
 *     is a no-op after these checks.
 * gymrs_sharded_rollout_closed_loop runs it on every block through its worker; record must be NULL there (the blocks live on
 * several devices, as with lengths_dev); the fitness records are read with gymrs_sharded_get_policy_fitness.  k blocks on one
 * GPU give bit for bit what one engine gives. */
#define GYMRS_CLOSED_LOOP_FITNESS 1u
#define GYMRS_CLOSED_LOOP_LANE_PARAMS 4u /* bit 2, the bit of GYMRS_EVAL_LANE_PARAMS */
typedef struct { uint32_t n_steps; uint32_t flags; const gymrs_trajectory* record; uint64_t reserved; } gymrs_closed_loop_desc; /* 24 B */
gymrs_status gymrs_rollout_closed_loop(gymrs_engine* e, const gymrs_closed_loop_desc* d);
gymrs_status gymrs_sharded_rollout_closed_loop(gymrs_sharded* h, const gymrs_closed_loop_desc* d);
/* Exploration: epsilon-greedy inside the closed-loop fused rollout, defined to the bit.
 * The closed-loop calls above play the deterministic argmax, which is what evaluation wants; a learner that collects its batch
 * with gymrs_rollout_closed_loop and a record must also take the action it does not already prefer.  The exploration settings live
 * on the engine like the policy set: seed, and threshold in [0, 65536] with epsilon = threshold / 65536 exactly; reserved must be
 * 0.  The step that takes the lane with GLOBAL id g (global_env_offset + i) from engine tick t to t + 1 -- n_actions = 2 / 3:
 *     b        = the Philox4x32-10 block with key (seed lo, seed hi) and counter (g >> 2 lo, g >> 2 hi, t lo,
 *                (t hi & 0xffff) | 2 << 16): the counter layout of the reset (stream 0) and action (stream 1) streams, stream 2
 *     w        = word (g & 3) of b
 *     explored = (w & 0xffff) < threshold
 *     random   = ((w >> 16) * n_actions) >> 16
 *     action   = explored ? random : the policy's action (the argmax under "closed-loop rollouts", unchanged)
 * Four neighbouring lanes share one block per step (a work-item that owns four aligned lanes evaluates one); a
 * global_env_offset that is not a multiple of 4 gives the same values.  The key is the engine's own tick, so K steps in one launch
 * equal K single steps however they are split into launches, the result does not depend on how a batch is cut into engines, and
 * a CPU can recompute every draw.  Threshold 0 is greedy: bit-identical to the call without exploration.  Threshold 65536 explores
 * on every step (the policy's weights, non-finite ones included, then change nothing).
 *   - gymrs_set_exploration stores the settings (x == NULL removes them); gymrs_get_exploration reads them back.  GYMRS_EINVAL:
 *     Pendulum, threshold > 65536, reserved != 0, (get) no settings.  It needs no policy to be set, touches no lane state, tick,
 *     statistics or fitness table, survives gymrs_set_policy and takes effect in stream order: launches enqueued before it play
 *     the old settings.  NOT part of gymrs_engine_clone or of a snapshot (its bytes and version are unchanged).
 *   - GYMRS_CLOSED_LOOP_EXPLORE in gymrs_closed_loop_desc.flags: gymrs_rollout_closed_loop plays the epsilon-greedy action in every
 *     combination it has: plain, with a record (the `actions` rows hold the action TAKEN), with GYMRS_CLOSED_LOOP_FITNESS (the
 *     counters follow the action taken), with or without GYMRS_CLOSED_LOOP_LANE_PARAMS under a table.  The flag without settings
 *     on the engine: GYMRS_EINVAL naming gymrs_set_exploration.  Settings without the flag: the greedy launch, bit for bit --
 *     exploration is opt-in per launch, so a learner alternates collection and greedy validation launches.  gymrs_rollout_policy,
 *     _record and _fitness stay greedy.
 *   - gymrs_explore_actions(e, actions_dev): the per-step counterpart, gymrs_policy_actions mixed with the draw at the engine's
 *     current tick:  gymrs_rollout_closed_loop(K, EXPLORE)  ==  K x (gymrs_explore_actions(e, buf); gymrs_step(e, buf)).  It needs
 *     a policy and settings (GYMRS_EINVAL otherwise) and, like gymrs_policy_actions, works while a parameter table is active.
 *   - gymrs_explore_draw: host only, no GPU (like gymrs_policy_size): explored (0 / 1) and the random action of (global id, tick)
 *     under the settings; either output may be NULL.  A learner that needs to know which recorded actions were exploratory
 *     recomputes them; no trajectory row is spent on it.  GYMRS_EINVAL: NULL settings, settings gymrs_set_exploration would refuse,
 *     n_actions outside 1 .. 256.
 *   - gymrs_sharded_set_exploration applies the same settings to every block; gymrs_sharded_rollout_closed_loop passes the flag
 *     through.  With the global-id key, k blocks equal one engine.
 * Evaluation (gymrs_evaluate_policy) stays greedy. */
#define GYMRS_CLOSED_LOOP_EXPLORE 16u /* bit 4 */
typedef struct { uint64_t seed; uint32_t threshold; uint32_t reserved; } gymrs_exploration; /* 16 B */
gymrs_status gymrs_set_exploration(gymrs_engine* e, const gymrs_exploration* x);
gymrs_status gymrs_get_exploration(gymrs_engine* e, gymrs_exploration* x_out);
gymrs_status gymrs_explore_actions(gymrs_engine* e, void* actions_dev);
gymrs_status gymrs_explore_draw(const gymrs_exploration* x, uint32_t n_actions, uint64_t global_id, uint64_t tick, uint8_t* explored,
                                uint8_t* random_action);
gymrs_status gymrs_sharded_set_exploration(gymrs_sharded* h, const gymrs_exploration* x);
/* Sampling: a ~ softmax(logits / temperature) inside the closed-loop fused rollouts, defined to the bit.
 * A policy-gradient learner needs the action drawn from the policy's own distribution, needs to know that distribution, and needs
 * the draw to be reproducible.  The sampling settings live on the engine like the exploration settings: seed, and scale = log2(e) /
 * temperature (the rule works in base 2), finite and >= 0; 0 gives the uniform policy; reserved must be 0.  For the step that takes
 * the lane with GLOBAL id g from engine tick t to t + 1, let y[0 .. A) be the logits of "closed-loop rollouts" (unchanged) and
 * greedy its argmax (unchanged: the first maximum, a NaN at a >= 1 never wins).  All arithmetic is f32, every operation below is a
 * single IEEE operation, nothing is contracted or reordered:
 *     m     = y[greedy]
 *     d[a]  = (y[a] - m) * scale                          (one subtract, one multiply)
 *     w[a]  = !(d[a] >= -126.0f) ? 0.0f                   (NaN, -inf and the far tail weigh nothing)
 *           : ldexpf(P(d[a] - floorf(d[a])), (int)floorf(d[a]))
 *     P(f)  = Horner with fmaf from c6 down to c0:  acc = c6; acc = fmaf(acc, f, c5); ... ; acc = fmaf(acc, f, c0)
 *             c0 .. c6 = 1.0, 0x1.62e430p-1, 0x1.ebfc40p-3, 0x1.c69f6ap-5, 0x1.3c4a8ap-7, 0x1.4ca4ccp-10, 0x1.b4d1e4p-13
 *     total = ((w[0] + w[1]) + w[2])                      (index order; A = 2: w[0] + w[1])
 *     word  = word (g & 3) of the Philox4x32-10 block of stream 3: key (seed lo, seed hi), counter (g >> 2 lo, g >> 2 hi, t lo,
 *             (t hi & 0xffff) | 3 << 16) -- the counter layout of streams 0 .. 2
 *     thr   = ((float)(word >> 8) * 0x1p-24f) * total     (the first product is exact)
 *     action  = the first a with thr < w[0] + ... + w[a]  (running f32 sum in index order); if there is none, greedy
 *     prob[a] = w[a] / total  (one IEEE divide); if total is not > 0: prob[greedy] = 1, the others 0
 * P(f) approximates 2^f on [0, 1): its maximum relative error against f64 exp2 over all 2^23 values f = i / 2^23, evaluated with
 * true fmaf, is 6.7e-8 (measured: 6.704e-8, below 6.71e-8; tests/test_sample_ref.py repeats the measurement).  What follows from the rule:
 *   - c0 == 1 makes w[greedy] == 1 exactly whenever m is finite; exact ties are equally likely; an action of weight zero is never
 *     taken; a NaN or infinite m (all weights 0) plays the greedy action.
 *   - f can round up to 1.0 for a denormal d; the formula still holds there.  Every w is 0 or a normal number.
 *   - The key is the engine's own tick and the GLOBAL lane id: K steps in one launch equal K single steps however they are split
 *     into launches, k blocks equal one engine, and a CPU can recompute every draw.
 *   - gymrs_set_sampling stores the settings (x == NULL removes them); gymrs_get_sampling reads them back.  GYMRS_EINVAL: Pendulum,
 *     scale NaN, infinite or negative, reserved != 0, (get) no settings.  As with gymrs_set_exploration: no policy is needed; the
 *     settings touch no lane state, tick, statistics or fitness table, survive gymrs_set_policy, take effect in stream order and are
 *     NOT part of gymrs_engine_clone or of a snapshot.
 *   - GYMRS_CLOSED_LOOP_SAMPLE in the flags of gymrs_closed_loop_desc and gymrs_transitions_desc: the launch plays the sampled
 *     action in every combination it has: plain, with a record (the `actions` rows hold the action TAKEN), with
 *     GYMRS_CLOSED_LOOP_FITNESS (the counters follow the action taken), with or without GYMRS_CLOSED_LOOP_LANE_PARAMS under a
 *     table, and in gymrs_rollout_transitions.  Together with GYMRS_CLOSED_LOOP_EXPLORE: GYMRS_EINVAL naming both flags.  The flag
 *     without settings: GYMRS_EINVAL naming gymrs_set_sampling.  Settings without the flag: the greedy launch, bit for bit.
 *     gymrs_rollout_policy, _record, _fitness and gymrs_evaluate_policy stay greedy.
 *   - gymrs_sample_actions(e, actions_dev, prob_dev): the per-step counterpart at the engine's current tick; prob_dev (may be NULL,
 *     else n_envs floats) gets prob[action] of every lane.  gymrs_rollout_closed_loop(K, SAMPLE)  ==  K x (gymrs_sample_actions(e,
 *     buf, NULL); gymrs_step(e, buf)).  It needs a policy and settings (GYMRS_EINVAL otherwise) and works while a parameter table
 *     is active.
 *   - gymrs_sample_draw: host only, no GPU (like gymrs_explore_draw): the definition as code.  From n_actions logits it gives the
 *     action of (global id, tick) under the settings and prob[0 .. n_actions); either output may be NULL.  GYMRS_EINVAL: NULL
 *     settings or logits, settings gymrs_set_sampling would refuse, n_actions outside 2 .. 8.
 *   - The fused launches write no probability row (the record layouts are pinned): a learner recomputes pi(a|s) from the `obs` rows
 *     with the weights it already holds.
 *   - gymrs_sharded_set_sampling applies the same settings to every block; gymrs_sharded_rollout_closed_loop passes the flag through. */
#define GYMRS_CLOSED_LOOP_SAMPLE 32u /* bit 5 */
typedef struct { uint64_t seed; float scale; uint32_t reserved; } gymrs_sampling; /* 16 B */
gymrs_status gymrs_set_sampling(gymrs_engine* e, const gymrs_sampling* x);
gymrs_status gymrs_get_sampling(gymrs_engine* e, gymrs_sampling* x_out);
gymrs_status gymrs_sample_actions(gymrs_engine* e, void* actions_dev, float* prob_dev);
gymrs_status gymrs_sample_draw(const gymrs_sampling* x, uint32_t n_actions, const float* logits, uint64_t global_id, uint64_t tick, uint8_t* action,
                               float* probs);
gymrs_status gymrs_sharded_set_sampling(gymrs_sharded* h, const gymrs_sampling* x);
/* Transitions: a recorded closed-loop rollout that keeps what every ended episode ended in.
 * With GYMRS_AUTO_RESET the `obs` row of a step that ends an episode holds the re-armed state; the observation the episode ended in,
 * which a truncated step must bootstrap from, is only in the engine's GYMRS_FINAL_OBS arrays, one ending per lane.
 * gymrs_rollout_transitions(e, d) is gymrs_rollout_closed_loop with d->n_steps = K, d->flags and &d->record that also writes that
 * observation per step, and optionally the observations the launch starts from.  D = obs_dim (4 / 2), i = the lane.
 *   - Everything but the two new buffers: exactly what gymrs_rollout_closed_loop leaves with the same n_steps, flags and record,
 *     bit for bit -- the five record rows, lane state, the last step's reward / done / truncated, the engine's own
 *     final-observation arrays (engines with GYMRS_FINAL_OBS), statistics, steps_beyond_terminated and tick.
 *   - final_obs[(k * D + j) * record.lane_stride + i] is written if and only if step k of the launch re-armed lane i (done |
 *     truncated; the engine has GYMRS_AUTO_RESET).  Every other element keeps the bytes it held: lanes that went on, the padding
 *     lanes [n_envs, lane_stride), lanes whose parameter index is outside the table (they are not stepped; gymrs_sync reports
 *     them as GYMRS_EACTION as ever).  No row is cleared: `ended = done | truncated` of the record says which elements count.
 *   - The value written is component j of the observation the lane showed BEFORE the re-arm: the bits a per-step loop on an
 *     engine with GYMRS_FINAL_OBS reads from gymrs_final_obs_ptrs for that lane right after that step, and the bits the record's
 *     `obs` row would hold on an engine without auto-reset.
 *   - start_obs (may be NULL): start_obs[j * record.lane_stride + i] = component j of lane i's observation before the first step,
 *     what gymrs_obs_ptrs showed, so that transition 0 has its s.
 *   - The transition of step k is (s, a, r, s', done) with s = obs[k - 1] (start_obs for k = 0), a = actions[k], r = reward[k] and
 *     the successor s' = ended ? final_obs[k] : obs[k].
 *   - Every flag set with GYMRS_AUTO_RESET, with or without GYMRS_FINAL_OBS on the engine; with and without a parameter table
 *     (GYMRS_CLOSED_LOOP_LANE_PARAMS, as above), with and without GYMRS_CLOSED_LOOP_EXPLORE, any n_envs and global_env_offset.
 *     Like every recording kernel it runs at 4 lanes per work-item.
 *   - GYMRS_EINVAL, naming the cause: NULL engine or desc, Pendulum, no policy set, an engine without GYMRS_AUTO_RESET (nothing is
 *     re-armed there: the `obs` rows already hold the final observations), reserved != 0, any flag bit but
 *     GYMRS_CLOSED_LOOP_LANE_PARAMS and GYMRS_CLOSED_LOOP_EXPLORE (GYMRS_CLOSED_LOOP_FITNESS: there is no recording fitness kernel),
 *     GYMRS_CLOSED_LOOP_EXPLORE without exploration settings, an active table without GYMRS_CLOSED_LOOP_LANE_PARAMS, a record that
 *     fails the buffer checks of gymrs_rollout_policy_record (truncated may be NULL), final_obs NULL or not 16-byte aligned,
 *     start_obs not 16-byte aligned.  n_steps == 0 is a no-op after these checks; start_obs is not written then either.
 * There is no sharded counterpart: a sharded batch refuses records already (its blocks live on several devices). */
typedef struct {
    uint32_t n_steps;
    uint32_t flags;            /* GYMRS_CLOSED_LOOP_LANE_PARAMS | GYMRS_CLOSED_LOOP_EXPLORE, nothing else */
    gymrs_trajectory record;   /* by value; the rules of gymrs_rollout_policy_record (truncated may be NULL) */
    float* final_obs;          /* [n_steps][D][record.lane_stride], required, 16-byte aligned */
    float* start_obs;          /* [D][record.lane_stride] or NULL, 16-byte aligned */
    uint64_t reserved;         /* 0 */
} gymrs_transitions_desc;      /* 80 bytes */
gymrs_status gymrs_rollout_transitions(gymrs_engine* e, const gymrs_transitions_desc* d);
/* Advantages: GAE(lambda) advantages, returns and values over a transitions record in ONE launch, defined to the bit.
 * A learner that collects with gymrs_rollout_transitions turns the record into learning targets with a backward scan: K dependent
 * rounds over [n_envs] slices when written with tensor operations, and a three-way case split per step (the episode went on / was
 * truncated / was done) that is easy to get wrong.  gymrs_advantages(e, d) does the scan in one pass over the record, with an optional
 * critic of the policy's shape family evaluated inside the kernel.  All arithmetic is f32, every operation below is a single IEEE
 * operation, fmaf = the fused multiply-add with ONE rounding, nothing is contracted or reordered, every `?:` is a select (never a
 * multiply by a mask).
 * The critic is the policy network of "closed-loop rollouts" with a single output.  D = observation size (4 / 2), H = hidden width,
 * 0 <= H <= 64, x[0..D) in gymrs_obs_ptrs order:
 *     H == 0 (affine):    v = b;   for j = 0..D-1: v = fmaf(W[j], x[j], v)
 *     H  > 0 (one layer): v = b2;  for h = 0..H-1:
 *                             z = b1[h];  for j = 0..D-1: z = fmaf(W1[h][j], x[j], z)
 *                             r = (z > 0.0f) ? z : 0.0f                 (compare-select: NaN and -0 give +0)
 *                             v = fmaf(W2[h], r, v)
 * One critic is S consecutive floats: H == 0: W[D], b (S = D + 1: 5 / 3); H > 0: W1[H][D], b1[H], W2[H], b2 (S = H*(D+2) + 1;
 * CartPole H = 16: 97) -- the policy layout with A = 1.  gymrs_critic_size returns S (host only, no GPU; GYMRS_EINVAL for Pendulum
 * and hidden > 64).  A critic set is n_critics critics back to back and a block size: the lane with GLOBAL id g uses critic
 * (g / lanes_per_critic) % n_critics -- the policy's key, described by the same gymrs_policy_desc (n_policies = n_critics,
 * lanes_per_policy = lanes_per_critic).  Without GYMRS_ADVANTAGES_CRITIC in the launch, V(x) = +0.0f for every x.
 * The scan.  K = d->n_steps, gl = gamma * lambda (one multiply), A[K] = +0.0f; for lane i of the engine, k = K-1 down to 0, rows and
 * columns as in gymrs_rollout_transitions (obs[k], final_obs[k] = the D components of lane i in row k):
 *     ended   = done[k] != 0 || (truncated != NULL && truncated[k] != 0)
 *     x_next  = (final_obs != NULL && ended) ? final_obs[k] : obs[k]
 *     v_next  = done[k] != 0 ? +0.0f : V(x_next)
 *     v_cur   = V(k == 0 ? start_obs : obs[k-1])
 *     delta   = fmaf(gamma, v_next, reward[k]) - v_cur
 *     carry   = ended ? +0.0f : A[k+1]
 *     A[k]    = fmaf(gl, carry, delta);   R[k] = A[k] + v_cur;   values[k] = v_cur
 * What follows from the selects: an unselected final_obs element reaches no output (that buffer is written on ended lane-steps only
 * and otherwise holds whatever bytes it held); a NaN A[k+1] behind an episode end reaches no output; a NaN V(obs[k]) on a done step
 * reaches no output.  final_obs == NULL is for records of engines without auto-reset, where the `obs` row already holds the final
 * observation.  With no critic, gamma = lambda = 1, R is the reward-to-go within the episode.
 *   - gymrs_set_critic, gymrs_get_critic and gymrs_critic_weights_ptr are gymrs_set_policy, gymrs_get_policy and
 *     gymrs_policy_weights_ptr for the critic set: the copy happens in stream order and the call waits for its own copy; d == NULL
 *     removes the critic; non-finite weights are legal; GYMRS_EINVAL: Pendulum, hidden > 64, zero counts, NULL weights, (get, ptr) no
 *     critic set.  The critic touches no lane state, tick, statistics or the fitness / evaluation tables, survives gymrs_set_policy
 *     and is NOT part of gymrs_engine_clone or of a snapshot.  Through the zero-copy view a learner on the engine's stream writes the
 *     critic in place and the next launch reads it; valid until the next gymrs_set_critic or destroy.
 *   - gymrs_critic_value: host only, no GPU (like gymrs_sample_draw): the definition as code.  *v = V(obs[0..D)) under one critic of
 *     S floats.  GYMRS_EINVAL: NULL arguments, Pendulum, hidden > 64.
 *   - gymrs_advantages runs in the engine's stream order: a gymrs_rollout_transitions enqueued just before it needs no
 *     synchronisation in between.  It uses the engine only for the stream, the kind, n_envs, global_env_offset and the critic set: it
 *     reads and writes no lane array -- state, flag arrays, final observations, statistics, tick, reset log, fitness / evaluation
 *     tables and parameter index stay bit for bit.  It writes elements [k][i] for i < n_envs only: the padding lanes [n_envs,
 *     lane_stride) keep their bytes.  A critic set without the flag plays V = 0: the critic is opt-in per launch, as exploration is.
 *     Without the flag no observation buffer is read.  n_steps == 0 is a no-op after the checks.
 *   - GYMRS_EINVAL, naming the cause: NULL engine or desc, Pendulum, reserved != 0, unknown flag bits, GYMRS_ADVANTAGES_CRITIC without a
 *     critic set (naming gymrs_set_critic), gamma or lambda NaN or outside [0, 1], NULL obs / reward / done / start_obs / advantages,
 *     any buffer not 16-byte aligned, lane_stride < n_envs or not a multiple of 16.
 * There is no sharded counterpart: a sharded batch refuses records already (its blocks live on several devices). */
#define GYMRS_ADVANTAGES_CRITIC 1u
typedef struct {
    uint32_t n_steps;           /* K */
    uint32_t flags;             /* GYMRS_ADVANTAGES_CRITIC, nothing else */
    float gamma, lambda;        /* finite, in [0, 1] */
    gymrs_trajectory record;    /* by value, as in gymrs_transitions_desc; READ: obs, reward, done, truncated (may be NULL);
                                   actions is not read and may be NULL; lane_stride >= n_envs, a multiple of 16 */
    const float* final_obs;     /* [K][D][lane_stride] or NULL, 16-byte aligned */
    const float* start_obs;     /* [D][lane_stride], required, 16-byte aligned */
    float* advantages;          /* [K][lane_stride], required */
    float* returns;             /* [K][lane_stride] or NULL */
    float* values;              /* [K][lane_stride] or NULL */
    uint64_t reserved;          /* 0 */
} gymrs_advantages_desc;        /* 112 bytes */
gymrs_status gymrs_critic_size(gymrs_env_kind kind, uint32_t hidden, uint64_t* n_floats);
gymrs_status gymrs_set_critic(gymrs_engine* e, const gymrs_policy_desc* d, const float* weights_host);
gymrs_status gymrs_get_critic(gymrs_engine* e, gymrs_policy_desc* d_out, float* weights_out, uint64_t capacity_floats);
gymrs_status gymrs_critic_weights_ptr(gymrs_engine* e, float** dev_out, uint64_t* n_floats);
gymrs_status gymrs_critic_value(gymrs_env_kind kind, uint32_t hidden, const float* weights, const float* obs, float* v);
gymrs_status gymrs_advantages(gymrs_engine* e, const gymrs_advantages_desc* d);
/* Gradients: the score-function gradient of the policy set, and the value gradient of the critic set, over a transitions record in
 * ONE launch, as exact fixed-point integers.  gymrs_policy_gradient(e, d) ADDS, for every set m (policy, or critic with
 * GYMRS_GRADIENT_CRITIC) and every parameter s of its network,
 *     grad[m][s] += sum over the lanes i of set m of q(i, s),     q = the fixed point of  sum over k of coef[k][i] * d/d theta_s log pi(a[k][i] | x[k][i])
 * (critic head: of sum over k of coef[k][i] * d/d phi_s V(x[k][i])).  coef is a row the learner fills: normalised advantages give
 * REINFORCE / A2C, V - R gives the value loss, the clipped-ratio weight gives PPO (the ratio from the `prob` row below).  All
 * arithmetic is f32, every operation below is a single IEEE operation, fmaf = the fused multiply-add with ONE rounding, nothing is
 * contracted or reordered, every `?:` is a select.
 * Inputs per lane-step.  Lane i of the engine has the global id g = global_env_offset + i and uses set (g / lanes_per_policy) %
 * n_policies (the policy's key; with the flag the critic's).  For k = 0 .. K-1 in ascending order, rows and columns as in
 * gymrs_rollout_transitions:
 *     x = (k == 0 ? start_obs : obs[k-1])       (the observation the action was drawn from; obs[K-1] is not read)
 *     a = actions[k];   c = coef[k]
 * Policy head (the default).  A = number of actions, y[0..A) = the policy's logits of x as defined in "closed-loop rollouts";
 * p[b] = the probabilities of the sampling rule ("sampling") under d->scale: greedy, w[], total, p[b] exactly as gymrs_sample_draw
 * computes them.
 *     beta = scale * 0x1.62e430p-1f                                  (1 / temperature for scale = log2(e) / temperature)
 *     cb   = c * beta
 *     g[b] = cb * ((b == a ? 1.0f : 0.0f) - p[b])                    for b = 0 .. A-1
 *     a lane-step with a >= A contributes nothing: every accumulator below keeps its value (a select)
 * Critic head (GYMRS_GRADIENT_CRITIC).  The network is the critic of "advantages": one output, A = 1, g[0] = c; actions and scale are
 * not read.
 * Backward pass.  Every parameter of every lane has its own f32 accumulator, +0.0f before k = 0, updated once per step:
 *     H == 0:  dW[b][j] = fmaf(g[b], x[j], dW[b][j]);   db[b] = db[b] + g[b]
 *     H  > 0:  db2[b] = db2[b] + g[b], and per unit h = 0 .. H-1, with z and r of unit h as in the forward definition:
 *              dW2[b][h] = fmaf(g[b], r, dW2[b][h])
 *              e  = g[0] * W2[0][h];   for b = 1 .. A-1: e = fmaf(g[b], W2[b][h], e)
 *              dz = (z > 0.0f) ? e : 0.0f
 *              db1[h] = db1[h] + dz;   dW1[h][j] = fmaf(dz, x[j], dW1[h][j])
 * The table of one set has the layout of its weights (gymrs_policy_size / gymrs_critic_size): parameter s of the table is float s.
 * Fixed point, once per (lane, parameter) after the walk, L = the lane's f32 sum:
 *     L finite and |L| < 2^30:  q = (int64) rint((double)L * 16777216.0)      (scaling and rounding to nearest even, exact in f64)
 *                               grad[set][s] += q   modulo 2^64
 *     otherwise:                nothing is added, excluded[set] += 1          (one per (lane, parameter) pair left out)
 * The gradient is grad * 2^-24.  Every lane's contribution is an integer before lanes are summed, so the table is exact: it does
 * not depend on wave or block order, on lanes per work-item or on how the kernels cut the hidden layer; it is additive over engines
 * (k blocks of a batch with their global_env_offset, adding into one table, equal one engine) and over launches: the call ADDS to
 * grad and excluded, and the caller zeroes them.
 * prob (policy head only, may be NULL): prob[k][i] = p[a], or +0.0f where a >= A, for i < n_envs: the bits gymrs_sample_draw gives
 * for those logits.  A PPO learner takes its ratio from it; no logarithm enters the rule.
 *   - gymrs_policy_gradient runs in the engine's stream order: a gymrs_advantages enqueued just before it needs no synchronisation
 *     in between.  It uses the engine only for the stream, the kind, n_envs, global_env_offset and the policy (critic) set: it reads
 *     and writes no lane array.  It reads lanes i < n_envs of every row only: the padding lanes [n_envs, lane_stride) may hold
 *     anything, NaN included, and count for nothing; of prob they keep their bytes.  reward, done and truncated of the record are
 *     not read and may be NULL.  n_steps == 0 is a no-op after the checks.
 *   - GYMRS_EINVAL, naming the cause: NULL engine or desc, Pendulum, unknown flag bits, reserved != 0, no policy set (naming
 *     gymrs_set_policy; with the flag no critic set, naming gymrs_set_critic), for the policy head scale NaN, infinite or negative,
 *     NULL obs / start_obs / coef / grad / excluded, NULL actions for the policy head, prob with the flag, a row buffer not 16-byte
 *     aligned, grad or excluded not 8-byte aligned, lane_stride < n_envs or not a multiple of 16.
 *   - gymrs_gradient_lane: host only, no GPU (like gymrs_critic_value): the definition as code.  From ONE set's weights (S floats),
 *     K = n_steps, one lane's x[K][D] (x[k] as defined above), actions[K] and coef[K] it SETS q[0..S) to the lane's contributions (0
 *     for an excluded pair), *excluded to the number of excluded pairs and, when prob != NULL, prob[0..K).  flags and scale as in the
 *     descriptor.  GYMRS_EINVAL: Pendulum, hidden > 64, unknown flag bits, NULL arguments, prob with the flag, a bad scale.
 * There is no sharded counterpart: a sharded batch refuses records already. */
#define GYMRS_GRADIENT_CRITIC 1u
typedef struct {
    uint32_t n_steps;           /* K */
    uint32_t flags;             /* GYMRS_GRADIENT_CRITIC, nothing else */
    float scale;                /* policy head: log2(e) / temperature, finite, >= 0 (gymrs_sampling::scale); critic head: not read */
    uint32_t pad_;              /* 0 */
    gymrs_trajectory record;    /* by value; READ: obs, actions (policy head); reward, done, truncated are not read and may be NULL;
                                   lane_stride >= n_envs, a multiple of 16 */
    const float* start_obs;     /* [D][lane_stride], required, 16-byte aligned */
    const float* coef;          /* [K][lane_stride], required, 16-byte aligned */
    float* prob;                /* [K][lane_stride] or NULL; NULL with GYMRS_GRADIENT_CRITIC */
    int64_t* grad;              /* device int64 [n_sets][S], 8-byte aligned, ADDED to */
    uint64_t* excluded;         /* device uint64 [n_sets], ADDED to */
    uint64_t reserved;          /* 0 */
} gymrs_gradient_desc;          /* 112 bytes */
gymrs_status gymrs_policy_gradient(gymrs_engine* e, const gymrs_gradient_desc* d);
gymrs_status gymrs_gradient_lane(gymrs_env_kind kind, uint32_t hidden, uint32_t flags, float scale, const float* weights, uint32_t n_steps,
                                 const float* x, const uint8_t* actions, const float* coef, int64_t* q, uint64_t* excluded, float* prob);
/* Clipped surrogate: PPO's gradient over a transitions record in ONE launch per epoch.  gymrs_ppo_gradient(e, d) is
 * gymrs_policy_gradient with the policy head, with one difference: the coefficient of a lane-step is not read from a row, it is
 * computed from an advantage row and an old-probability row.  Everything else is as "gradients" defines it: x, a, the logits, p[],
 * beta, the accumulators, the backward pass, the fixed point, excluded, the set key (the policy's) and additivity.
 * For lane i and step k, with pa = p[a] (the value "gradients" writes to prob; +0.0f where a >= A):
 *     adv   = advantages[k][i];   po = old_prob[k][i]
 *     ratio = pa / po                                                                  (one IEEE divide)
 *     cut   = (adv > 0.0f && ratio > clip_high) || (adv < 0.0f && ratio < clip_low)    (compares: false on NaN)
 *     c     = cut ? +0.0f : adv * ratio                                                (a select, one multiply)
 *     cb    = c * beta;   g[b] = cb * ((b == a ? 1.0f : 0.0f) - p[b])                  (unchanged from here on)
 * The table receives the gradient of  sum over k of min(ratio * adv, clip(ratio, clip_low, clip_high) * adv),  the objective to
 * ASCEND: the learner adds it.  The bounds are the caller's floats (1 - epsilon and 1 + epsilon as the caller rounds them): the
 * library does no arithmetic on an epsilon.  What follows from the rule:
 *   - a lane-step with a >= A contributes nothing (as in "gradients") and is not counted below;
 *   - a c that is not finite, or one that takes a sum past 2^30, puts that lane's pairs into excluded, as such a coef does in
 *     "gradients": a NaN po or adv gives c = NaN; po = 0 gives ratio = +inf (pa > 0), which a positive adv cuts and any other adv
 *     turns into c = -inf or NaN; po = +inf gives ratio = +0, which a negative adv cuts (clip_low > 0) and a positive one
 *     multiplies to c = +0: a finite value, nothing is excluded; a negative po is arithmetic like any other (ratio < 0);
 *   - the compares are strict: ratio == clip_high (ratio == clip_low) is not cut; adv == 0 (either sign) is never cut;
 *   - by definition the call equals gymrs_policy_gradient with coef[k][i] = c, integer for integer.
 * counts (may be NULL): device uint64 [n_sets][2], ADDED to, exact: counts[set][0] += 1 per lane-step with a < A, counts[set][1] +=
 * 1 per such lane-step with cut.  The clip fraction of a set is counts[set][1] / counts[set][0].
 * prob (may be NULL) behaves exactly as in gymrs_policy_gradient and receives the new p[a]; old_prob and prob may not alias.
 *   - Like gymrs_advantages and gymrs_policy_gradient the call runs in the engine's stream order and uses the engine only for the
 *     stream, the kind, n_envs, global_env_offset and the policy set: it reads and writes no lane array.  It reads lanes i < n_envs
 *     of every row only: the padding lanes may hold anything, NaN included, and count for nothing; of prob they keep their bytes.
 *     reward, done and truncated of the record are not read and may be NULL.  n_steps == 0 is a no-op after the checks.
 *   - GYMRS_EINVAL, naming the cause: everything gymrs_policy_gradient refuses for the policy head (NULL engine or desc, Pendulum,
 *     reserved != 0, no policy set (naming gymrs_set_policy), scale NaN, infinite or negative, NULL obs / actions / start_obs / grad
 *     / excluded, a row buffer not 16-byte aligned, grad or excluded not 8-byte aligned, lane_stride < n_envs or not a multiple of
 *     16), and: flags != 0 or pad_ != 0, NULL or misaligned advantages or old_prob, prob == old_prob, bounds that are NaN, infinite
 *     or outside 0 <= clip_low <= 1 <= clip_high, counts not 8-byte aligned.
 *   - gymrs_ppo_lane: host only, no GPU: the definition as code, as gymrs_gradient_lane is for "gradients".  From ONE policy's
 *     weights, K = n_steps, one lane's x[K][D], actions[K], advantages[K] and old_prob[K] it SETS q[0..S), *excluded, counts[0..2)
 *     (when counts != NULL) and prob[0..K) (when prob != NULL).  GYMRS_EINVAL: Pendulum, hidden > 64, NULL arguments, prob ==
 *     old_prob, a bad scale, bad bounds.
 * The ABI version stays 3: the feature is detected by the symbol.  There is no sharded counterpart. */
typedef struct {
    uint32_t n_steps;           /* K */
    uint32_t flags;             /* 0, reserved */
    float scale;                /* log2(e) / temperature, finite, >= 0, as gymrs_gradient_desc */
    float clip_low;             /* 0 <= clip_low <= 1, e.g. (float)(1 - 0.2) */
    float clip_high;            /* 1 <= clip_high, finite, e.g. (float)(1 + 0.2) */
    uint32_t pad_;              /* 0 */
    gymrs_trajectory record;    /* by value; READ: obs, actions; lane_stride >= n_envs, a multiple of 16 */
    const float* start_obs;     /* [D][lane_stride], required, 16-byte aligned */
    const float* advantages;    /* [K][lane_stride], required, 16-byte aligned */
    const float* old_prob;      /* [K][lane_stride], required, 16-byte aligned: the prob row of the policy the record was drawn from */
    float* prob;                /* [K][lane_stride] or NULL; not old_prob */
    int64_t* grad;              /* device int64 [n_sets][S], 8-byte aligned, ADDED to */
    uint64_t* excluded;         /* device uint64 [n_sets], ADDED to */
    uint64_t* counts;           /* device uint64 [n_sets][2] or NULL, 8-byte aligned, ADDED to */
    uint64_t reserved;          /* 0 */
} gymrs_ppo_desc;               /* 136 bytes */
gymrs_status gymrs_ppo_gradient(gymrs_engine* e, const gymrs_ppo_desc* d);
gymrs_status gymrs_ppo_lane(gymrs_env_kind kind, uint32_t hidden, float scale, float clip_low, float clip_high, const float* weights, uint32_t n_steps,
                            const float* x, const uint8_t* actions, const float* advantages, const float* old_prob, int64_t* q, uint64_t* excluded,
                            uint64_t counts[2], float* prob);
/* Episodic policy evaluation: E whole episodes per lane in ONE launch, with exact per-policy episodic statistics.
 * gymrs_evaluate_policy(e, d) plays, for every lane i of the engine (global id g = global_env_offset + i, policy p = (g /
 * lanes_per_policy) % n_policies) and every episode index ep in [0, E = d->episodes_per_lane), the episode (g, ep):
 *   - start: the state gymrs_reset(seed = d->seed + ep (mod 2^64), no bounds) gives the lane with global id g: the default
 *     box, the Philox block keyed (seed + ep, g, tick 0, reset stream), the env's sample.  With GYMRS_EVAL_COMMON_STARTS in
 *     d->flags the id in the key is g % lanes_per_policy (what an engine at offset 0 gives lane g % lanes_per_policy): every
 *     policy meets the same lanes_per_policy x E start states (common random numbers).
 *   - steps: the action is the policy's (the definition under "closed-loop rollouts"), the physics the env's step with the
 *     engine's current uniform parameters (the general path covers out-of-range angles and NaN states, as in gymrs_step).
 *     With GYMRS_EVAL_LANE_PARAMS in d->flags every lane plays with the parameters gymrs_step would use for it right now: row
 *     index[i] of the active parameter table ("per-lane physics"), or, without a table, the uniform parameters -- then the
 *     call is bit-identical to the call without the flag, so a search loop may set it unconditionally.  Rows and index are
 *     read in stream order (an index rewritten through gymrs_param_index_ptr on the engine's stream is seen by the next
 *     evaluation); every lane fetches its row once per launch.  A lane whose index is >= K (possible through the zero-copy
 *     view only) plays no episode, adds nothing to any record and leaves its lengths_dev entries unwritten; no error is
 *     raised.  Start states do not depend on the physics fields.
 *   - end: with M = d->max_episode_steps, or the params' max_episode_steps (default 500 / 200; the one every row of a table
 *     shares) when that is 0, the episode ends
 *     at the first step k >= 1 that reports done, or at k = M.  L = k; done = the last step's done flag; truncated = (L == M)
 *     (both may be set, as in gymrs_step); return = +L (CartPole) or -L (MountainCar): both envs pay a constant per step.
 * Every episode adds to the record of its policy: return_sum += return, return_sq_sum += return^2, episodes += 1, done += done,
 * truncated += truncated, steps += L (all modulo 2^64), return_min / return_max = the lowest / highest return.  A policy with
 * no lane in this engine keeps the identity {0, 0, 0, 0, 0, 0, INT64_MAX, INT64_MIN}.  Integers throughout: exact, independent
 * of scheduling and of how a batch is cut into engines (add the sums, take the min of the mins and the max of the maxes; with
 * a table: provided the engines hold the same rows and the matching slices of the index).
 * d->lengths_dev (may be NULL): device uint32 [E][n_envs], 4-byte aligned; entry [ep][i] = L | (done ? 0x80000000 : 0).
 *   - The call reads no lane array and writes none: state, observations, reward / done / truncated, final observations,
 *     steps_beyond_terminated, tick, statistics, the reset log, the fitness table and the parameter index stay bit for bit; the
 *     engine's flags and gymrs_set_tuning do not matter (4 lanes per work-item).
 *   - The table holds n_policies records of the LATEST call: it is set to the identity in stream order and then filled; it does
 *     not accumulate.  It follows the fitness table's lifetime: allocated (as identities) at first use after a gymrs_set_policy,
 *     discarded by every gymrs_set_policy, not part of clone or snapshot.  gymrs_get_policy_eval copies records [first, first +
 *     count) and synchronises; gymrs_policy_eval_ptr is the zero-copy view (*n_policies may be NULL), valid until the next
 *     gymrs_set_policy or destroy.
 *   - GYMRS_EINVAL: NULL engine or desc, no policy set, Pendulum, an active parameter table without GYMRS_EVAL_LANE_PARAMS (a
 *     plain descriptor is never played with one set of parameters behind the caller's back), E == 0, reserved != 0, unknown
 *     flag bits (bit 1 is not assigned), a misaligned lengths_dev, E * M > GYMRS_POLICY_EVAL_MAX_STEPS (the bound of the kernel's running time, and
 *     what keeps a lane's sum of L in 32 bits).  Non-finite weights are legal.
 *   - Not built: moving episodes between the lanes of a wave (a wave runs until its slowest lane is through), 8 lanes per
 *     work-item, and policy x table for the fused rollout calls: gymrs_rollout_policy, _record and _fitness still refuse an
 *     active parameter table, because they take no flags word through which a caller could opt in (gymrs_rollout_closed_loop,
 *     above, has one: GYMRS_CLOSED_LOOP_LANE_PARAMS).
 *   - Per-(policy, row) records need no further call: replicate every policy's weights K times (n_policies' = P * K, policy
 *     q = p * K + r carries p's weights) and set index[i] = ((global_env_offset + i) / lanes_per_policy) % K; record q is then
 *     policy p under row r, and a robust objective is the minimum over r.
 * gymrs_sharded_evaluate_policy runs it on every block (lengths_dev must be NULL there; the flags pass through, so
 * GYMRS_EVAL_LANE_PARAMS works with gymrs_sharded_set_param_table / _index); gymrs_sharded_get_policy_eval merges the blocks'
 * records on the host. */
#define GYMRS_EVAL_COMMON_STARTS 1u
#define GYMRS_EVAL_LANE_PARAMS 4u /* bit 2 */
#define GYMRS_POLICY_EVAL_MAX_STEPS 16777216u
typedef struct { uint32_t episodes_per_lane, max_episode_steps; uint64_t seed; uint32_t flags, reserved; uint32_t* lengths_dev; } gymrs_eval_desc; /* 32 B */
typedef struct { int64_t return_sum; uint64_t return_sq_sum, episodes, done, truncated, steps; int64_t return_min, return_max; } gymrs_policy_eval; /* 64 B */
gymrs_status gymrs_evaluate_policy(gymrs_engine* e, const gymrs_eval_desc* d);
gymrs_status gymrs_get_policy_eval(gymrs_engine* e, uint32_t first, uint32_t count, gymrs_policy_eval* host_out);
gymrs_status gymrs_policy_eval_ptr(gymrs_engine* e, gymrs_policy_eval** dev_out, uint32_t* n_policies);
gymrs_status gymrs_sharded_evaluate_policy(gymrs_sharded* h, const gymrs_eval_desc* d);
gymrs_status gymrs_sharded_get_policy_eval(gymrs_sharded* h, uint32_t first, uint32_t count, gymrs_policy_eval* host_out);

/* ---- `#[derive(Serialize)]` view (core.rs:25; cartpole.rs:51-87, mountain_car.rs:46-80) -------- */
/* What serde_json::to_string(&env) prints for the reference env that lane `lane` stands for: the serde-visible
 * fields in declaration order with the reference's field names -- CartPole: action_space, observation_space
 * {low, high}, render_mode, state {x, x_dot, theta, theta_dot}, metadata {render_modes, render_fps, marker},
 * gravity, masscart, masspole, length, force_mag, tau, kinematics_integrator ("Euler" | "Other"),
 * theta_threshold_radians, x_threshold, steps_beyond_terminated (null | 0; the reference counts further, the engine
 * keeps is_some()); MountainCar: min_position .. gravity, render_mode, action_space, observation_space, state
 * {position, velocity}, metadata.  Non-finite floats print as null (serde_json).  `rand_random` is
 * #[serde(skip_serializing)] in the reference and absent here; the GUI-only `renderer` / `screen` members are
 * omitted (RenderMode::None, out of scope).  Engine-side additions sit under one extra key "gymrs": {kind, n_envs,
 * global_env_id, flags, seed, tick, max_episode_steps}; with a parameter table the physics fields are the lane's own row,
 * and "gymrs" adds param_set (the lane's index) and param_table_rows (K).  Pendulum (not in the reference) prints its params, state
 * and the "gymrs" object.
 * Writes at most cap bytes incl. the terminating NUL; *needed (may be NULL) receives the size required.  Returns
 * GYMRS_EINVAL when cap is too small (nothing useful written).  Synchronising (reads the lane's state). */
gymrs_status gymrs_env_json(gymrs_engine* e, uint64_t lane, char* buf, uint64_t cap, uint64_t* needed);
/* The inverse for the physics fields: parse a JSON object as printed above (unknown keys ignored, missing keys keep
 * the value already in *params, which the caller initialises, e.g. with gymrs_default_params) into the kind's
 * params struct.  If `state` (may be NULL, capacity 4) is given and the object has a "state", its numbers are stored
 * in field order and *state_dim (may be NULL) is set (0 when absent). */
gymrs_status gymrs_params_from_json(gymrs_env_kind kind, const char* json, void* params, double* state, int* state_dim);

/* ---- utilities --------------------------------------------------------------------------------- */
/* Random-policy actions for lane block [0, n_envs) at time t, written to actions_dev: the
 * `rng.gen_range(0..=1)` of examples/cartpole.rs:19, generated on the device so no PCIe traffic
 * sits in a timed loop.  Philox stream 1, key = seed, counter = (global id, t). */
gymrs_status gymrs_fill_actions(gymrs_engine* e, void* actions_dev, uint64_t seed, uint64_t t);
/* Engine tick (number of reset()/step() calls since the last seeded reset) and current seed.
 * Tick range: the tick is a 64-bit count; gymrs_reset restarts it at 0, snapshots and clones carry it.  Every random draw of a step
 * (re-arm, exploration, sampling) is keyed by its low 48 bits, so ticks 2^48 apart repeat draws.  The statistics are exact for any
 * tick below 2^48: lengths are summed modulo 2^64 lane-steps, from the 64-bit tick and the ages of the open episodes.  The episode
 * clocks keep 32 bits per lane: one episode may last at most 2^32 - 1 steps (an engine without GYMRS_TIME_LIMIT whose lane never
 * terminates for 2^32 steps is outside that range).  tests/test_gpu_high_tick.py steps every tick-keyed path across tick 2^32. */
gymrs_status gymrs_get_tick(gymrs_engine* e, uint64_t* tick, uint64_t* seed);
/* Kernel tuning knobs for benchmarks; results never depend on them.  lanes_per_thread: 4 (default) or 8
 * lanes per work-item (16 was measured 4x slower everywhere and was removed in ABI 2).  memory_hint: 0 = automatic (every access non-temporal while one step's traffic is
 * <= 48 MiB or >= 1 GiB; in between only the stores nobody reads again -- reward, flags, Pendulum's cos / sin -- so that the Infinity
 * Cache keeps the state for the next step), 1 = every access non-temporal, 2 = none, 3 = only those stores. */
gymrs_status gymrs_set_tuning(gymrs_engine* e, int lanes_per_thread, int memory_hint);

const char* gymrs_last_error(void);
int gymrs_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* GYMRS_AMD_H */
