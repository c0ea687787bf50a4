//! Raw declarations of `include/gymrs_amd.h` (ABI version 3).  Field order and types follow the header.
#![allow(missing_docs)]
use std::os::raw::{c_char, c_int, c_void};

#[repr(C)]
pub struct GymrsEngine {
    _opaque: [u8; 0],
}

/// `gymrs_sharded`: one batch over several GPUs in one process.
#[repr(C)]
pub struct GymrsSharded {
    _opaque: [u8; 0],
}

pub const GYMRS_OK: c_int = 0;
pub const GYMRS_EACTION: c_int = 5;

pub const GYMRS_CARTPOLE: c_int = 0;
pub const GYMRS_MOUNTAIN_CAR: c_int = 1;
pub const GYMRS_PENDULUM: c_int = 2;

pub const GYMRS_AUTO_RESET: u32 = 1;
pub const GYMRS_TRACK_STATS: u32 = 2;
pub const GYMRS_TIME_LIMIT: u32 = 4;
/// keep the observation an episode ended in (needs GYMRS_AUTO_RESET): gymrs_final_obs_ptrs / gymrs_get_final_obs
pub const GYMRS_FINAL_OBS: u32 = 8;

/// `gymrs_cartpole_params`: the pub physics fields of `CartPoleEnv` (cartpole.rs:53-82), f64 like the reference.
#[repr(C)]
#[derive(Clone, Copy, Debug, PartialEq)]
pub struct CartPoleParams {
    pub gravity: f64,
    pub masscart: f64,
    pub masspole: f64,
    pub length: f64,
    pub force_mag: f64,
    pub tau: f64,
    pub theta_threshold_radians: f64,
    pub x_threshold: f64,
    /// 0 = Euler, 1 = semi-implicit (`KinematicsIntegrator`, cartpole.rs:380-387)
    pub kinematics_integrator: i32,
    pub max_episode_steps: u32,
}

/// `gymrs_mountain_car_params`: the pub physics fields of `MountainCarEnv` (mountain_car.rs:49-77).
#[repr(C)]
#[derive(Clone, Copy, Debug, PartialEq)]
pub struct MountainCarParams {
    pub min_position: f64,
    pub max_position: f64,
    pub max_speed: f64,
    pub goal_position: f64,
    pub goal_velocity: f64,
    pub force: f64,
    pub gravity: f64,
    pub max_episode_steps: u32,
    pub _pad: u32,
}

/// `gymrs_trajectory`: device buffers `[n_steps][..][lane_stride]` filled by `gymrs_rollout_record`.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct Trajectory {
    pub obs: *mut f32,
    pub actions: *mut c_void,
    pub reward: *mut f32,
    pub done: *mut u8,
    pub truncated: *mut u8,
    pub lane_stride: u64,
}

/// `gymrs_policy_desc`: the shape of a policy set (`gymrs_set_policy`, include/gymrs_amd.h "closed-loop rollouts").
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct GymrsPolicyDesc {
    pub hidden: u32,
    pub n_policies: u32,
    pub lanes_per_policy: u64,
}

/// `gymrs_policy_fitness`: one policy's counters (`gymrs_rollout_policy_fitness`, include/gymrs_amd.h "per-policy fitness"), 32 bytes.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct GymrsPolicyFitness {
    pub reward_sum: i64,
    pub episodes: u64,
    pub done: u64,
    pub truncated: u64,
}

/// `GYMRS_CLOSED_LOOP_FITNESS`: `gymrs_rollout_closed_loop` also counts per-policy fitness (`gymrs_rollout_policy_fitness`).
pub const GYMRS_CLOSED_LOOP_FITNESS: u32 = 1;
/// `GYMRS_CLOSED_LOOP_LANE_PARAMS`: every lane steps with the row of the parameter table `gymrs_step` would use for it (no table: no change).
pub const GYMRS_CLOSED_LOOP_LANE_PARAMS: u32 = 4;
/// `GYMRS_CLOSED_LOOP_EXPLORE`: every step plays the epsilon-greedy action of the engine's exploration settings (`gymrs_set_exploration`).
pub const GYMRS_CLOSED_LOOP_EXPLORE: u32 = 16;

/// `GYMRS_CLOSED_LOOP_SAMPLE`: every step plays an action drawn from the softmax of the policy's logits (`gymrs_set_sampling`).
pub const GYMRS_CLOSED_LOOP_SAMPLE: u32 = 32;

/// `gymrs_sampling`: the sampling settings of an engine (include/gymrs_amd.h "sampling"), 16 bytes.  `scale` = log2(e) / temperature,
/// finite and >= 0; the draw is keyed (seed, global lane id, engine tick) on Philox stream 3.
#[repr(C)]
#[derive(Clone, Copy, Debug, PartialEq)]
pub struct GymrsSampling {
    pub seed: u64,
    pub scale: f32,
    pub reserved: u32,
}

/// `gymrs_exploration`: the exploration settings of an engine (include/gymrs_amd.h "exploration"), 16 bytes.  A step explores when the low
/// half of its Philox word, keyed (seed, global lane id, engine tick), is below `threshold` (0..=65536: epsilon = threshold / 65536).
#[repr(C)]
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub struct GymrsExploration {
    pub seed: u64,
    pub threshold: u32,
    pub reserved: u32,
}

/// `gymrs_closed_loop_desc`: what `gymrs_rollout_closed_loop` runs (include/gymrs_amd.h "closed-loop rollouts behind one descriptor"), 24 bytes.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct GymrsClosedLoopDesc {
    pub n_steps: u32,
    pub flags: u32,
    pub record: *const Trajectory,
    pub reserved: u64,
}

/// `gymrs_transitions_desc`: what `gymrs_rollout_transitions` runs (include/gymrs_amd.h "transitions"), 80 bytes: the record by value,
/// `final_obs` `[n_steps][D][record.lane_stride]` (written where a step re-armed a lane), `start_obs` `[D][record.lane_stride]` or null.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct GymrsTransitionsDesc {
    pub n_steps: u32,
    pub flags: u32,
    pub record: Trajectory,
    pub final_obs: *mut f32,
    pub start_obs: *mut f32,
    pub reserved: u64,
}

/// `GYMRS_ADVANTAGES_CRITIC`: `gymrs_advantages` evaluates the engine's critic set (`gymrs_set_critic`) inside the kernel; without it V = 0.
pub const GYMRS_ADVANTAGES_CRITIC: u32 = 1;

/// `gymrs_advantages_desc`: what `gymrs_advantages` runs (include/gymrs_amd.h "advantages"), 112 bytes: the record by value (read: `obs`,
/// `reward`, `done`, `truncated`), `final_obs` `[n_steps][D][record.lane_stride]` or null, `start_obs` `[D][record.lane_stride]`, and
/// the outputs `advantages`, `returns` (or null), `values` (or null), each `[n_steps][record.lane_stride]`.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct GymrsAdvantagesDesc {
    pub n_steps: u32,
    pub flags: u32,
    pub gamma: f32,
    pub lambda: f32,
    pub record: Trajectory,
    pub final_obs: *const f32,
    pub start_obs: *const f32,
    pub advantages: *mut f32,
    pub returns: *mut f32,
    pub values: *mut f32,
    pub reserved: u64,
}

/// `GYMRS_GRADIENT_CRITIC`: `gymrs_policy_gradient` takes the value gradient of the critic set (`gymrs_set_critic`) instead of the
/// score-function gradient of the policy set.
pub const GYMRS_GRADIENT_CRITIC: u32 = 1;

/// `gymrs_gradient_desc`: what `gymrs_policy_gradient` runs (include/gymrs_amd.h "gradients"), 112 bytes: the record by value (read:
/// `obs`, and `actions` for the policy head), `start_obs` `[D][record.lane_stride]`, `coef` and `prob` (or null)
/// `[n_steps][record.lane_stride]`, and the tables added to: `grad` int64 `[n_sets][S]` (the gradient is `grad * 2^-24`), `excluded`
/// u64 `[n_sets]`.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct GymrsGradientDesc {
    pub n_steps: u32,
    pub flags: u32,
    pub scale: f32,
    pub pad_: u32,
    pub record: Trajectory,
    pub start_obs: *const f32,
    pub coef: *const f32,
    pub prob: *mut f32,
    pub grad: *mut i64,
    pub excluded: *mut u64,
    pub reserved: u64,
}

/// `gymrs_ppo_desc`: what `gymrs_ppo_gradient` runs (include/gymrs_amd.h "clipped surrogate"), 136 bytes: `gymrs_gradient_desc` for the
/// policy head with the clip range, the `advantages` and `old_prob` rows in place of `coef`, and `counts` u64 `[n_sets][2]` (or null):
/// the lane-steps seen and the lane-steps cut, added to.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct GymrsPpoDesc {
    pub n_steps: u32,
    pub flags: u32,
    pub scale: f32,
    pub clip_low: f32,
    pub clip_high: f32,
    pub pad_: u32,
    pub record: Trajectory,
    pub start_obs: *const f32,
    pub advantages: *const f32,
    pub old_prob: *const f32,
    pub prob: *mut f32,
    pub grad: *mut i64,
    pub excluded: *mut u64,
    pub counts: *mut u64,
    pub reserved: u64,
}

/// `GYMRS_EVAL_COMMON_STARTS`: every policy meets the same `lanes_per_policy x E` start states.
pub const GYMRS_EVAL_COMMON_STARTS: u32 = 1;
/// `GYMRS_EVAL_LANE_PARAMS`: every lane plays with the row of the parameter table `gymrs_step` would use for it (no table: no change).
pub const GYMRS_EVAL_LANE_PARAMS: u32 = 4;
/// `GYMRS_POLICY_EVAL_MAX_STEPS`: the bound of `episodes_per_lane * max_episode_steps`.
pub const GYMRS_POLICY_EVAL_MAX_STEPS: u32 = 16777216;

/// `gymrs_eval_desc`: what `gymrs_evaluate_policy` plays (include/gymrs_amd.h "episodic policy evaluation"), 32 bytes.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct GymrsEvalDesc {
    pub episodes_per_lane: u32,
    pub max_episode_steps: u32,
    pub seed: u64,
    pub flags: u32,
    pub reserved: u32,
    pub lengths_dev: *mut u32,
}

/// `gymrs_policy_eval`: one policy's episodic record, 64 bytes.
#[repr(C)]
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub struct GymrsPolicyEval {
    pub return_sum: i64,
    pub return_sq_sum: u64,
    pub episodes: u64,
    pub done: u64,
    pub truncated: u64,
    pub steps: u64,
    pub return_min: i64,
    pub return_max: i64,
}

impl Default for GymrsPolicyEval {
    /// The identity record: what a policy without an episode holds.
    fn default() -> Self {
        GymrsPolicyEval { return_sum: 0, return_sq_sum: 0, episodes: 0, done: 0, truncated: 0, steps: 0, return_min: i64::MAX, return_max: i64::MIN }
    }
}

extern "C" {
    pub fn gymrs_abi_version() -> c_int;
    pub fn gymrs_last_error() -> *const c_char;
    pub fn gymrs_default_params(kind: c_int, params: *mut c_void) -> c_int;
    pub fn gymrs_observation_space(kind: c_int, params: *const c_void, low: *mut f64, high: *mut f64, dim: *mut c_int) -> c_int;
    pub fn gymrs_engine_create(
        kind: c_int,
        n_envs: u64,
        global_env_offset: u64,
        device: c_int,
        params: *const c_void,
        flags: u32,
        out: *mut *mut GymrsEngine,
    ) -> c_int;
    pub fn gymrs_engine_destroy(e: *mut GymrsEngine) -> c_int;
    pub fn gymrs_engine_clone(src: *mut GymrsEngine, out: *mut *mut GymrsEngine) -> c_int;
    pub fn gymrs_reset(e: *mut GymrsEngine, has_seed: c_int, seed: u64, bounds_low_high: *const f32, seed_used: *mut u64) -> c_int;
    pub fn gymrs_reset_pcg64(
        e: *mut GymrsEngine,
        has_seed: c_int,
        seed: u64,
        seeds_dev: *const u64,
        bounds_low_high: *const f64,
        seed_used: *mut u64,
    ) -> c_int;
    pub fn gymrs_step(e: *mut GymrsEngine, actions_dev: *const c_void) -> c_int;
    pub fn gymrs_step_host(e: *mut GymrsEngine, actions_host: *const c_void) -> c_int;
    pub fn gymrs_step_many(
        e: *mut GymrsEngine,
        actions_dev: *const c_void,
        stride_bytes: u64,
        n_buffers: u32,
        n_steps: u32,
        use_graph: c_int,
    ) -> c_int;
    pub fn gymrs_rollout(e: *mut GymrsEngine, n_steps: u32, action_seed: u64, action_t0: u64) -> c_int;
    pub fn gymrs_rollout_record(e: *mut GymrsEngine, n_steps: u32, action_seed: u64, action_t0: u64, out: *const Trajectory) -> c_int;
    pub fn gymrs_sync(e: *mut GymrsEngine) -> c_int;
    pub fn gymrs_get_state(e: *mut GymrsEngine, first: u64, count: u64, host_out: *mut f32) -> c_int;
    pub fn gymrs_final_obs_ptrs(e: *mut GymrsEngine, out_ptrs: *mut *mut f32, obs_dim: *mut c_int) -> c_int;
    pub fn gymrs_get_final_obs(e: *mut GymrsEngine, first: u64, count: u64, host_out: *mut f32) -> c_int;
    pub fn gymrs_set_state(e: *mut GymrsEngine, first: u64, count: u64, host_in: *const f32) -> c_int;
    pub fn gymrs_get_step_result(
        e: *mut GymrsEngine,
        first: u64,
        count: u64,
        reward: *mut f32,
        done: *mut u8,
        truncated: *mut u8,
    ) -> c_int;
    pub fn gymrs_stats(e: *mut GymrsEngine, out4: *mut f64) -> c_int;
    pub fn gymrs_snapshot_size(e: *mut GymrsEngine, bytes: *mut u64) -> c_int;
    pub fn gymrs_snapshot_save(e: *mut GymrsEngine, host_buf: *mut c_void, bytes: u64) -> c_int;
    pub fn gymrs_snapshot_load(e: *mut GymrsEngine, host_buf: *const c_void, bytes: u64) -> c_int;
    // ABI 2
    pub fn gymrs_set_params(e: *mut GymrsEngine, params: *const c_void) -> c_int;
    pub fn gymrs_get_params(e: *mut GymrsEngine, params_out: *mut c_void) -> c_int;
    /// per-lane physics: K rows of the kind's params and a u16 row index per lane (include/gymrs_amd.h)
    pub fn gymrs_set_param_table(e: *mut GymrsEngine, rows: *const c_void, k: u32) -> c_int;
    pub fn gymrs_get_param_table(e: *mut GymrsEngine, rows_out: *mut c_void, capacity: u32, k: *mut u32) -> c_int;
    pub fn gymrs_param_index_ptr(e: *mut GymrsEngine, out: *mut *mut u16) -> c_int;
    pub fn gymrs_set_param_index(e: *mut GymrsEngine, first: u64, count: u64, host_in: *const u16) -> c_int;
    pub fn gymrs_get_param_index(e: *mut GymrsEngine, first: u64, count: u64, host_out: *mut u16) -> c_int;
    pub fn gymrs_get_lane_params(e: *mut GymrsEngine, lane: u64, params_out: *mut c_void) -> c_int;
    /// closed-loop rollouts: a small policy evaluated inside the kernel (detect by symbol; the ABI version stays 3)
    pub fn gymrs_policy_size(kind: c_int, hidden: u32, n_floats: *mut u64) -> c_int;
    pub fn gymrs_set_policy(e: *mut GymrsEngine, d: *const GymrsPolicyDesc, weights_host: *const f32) -> c_int;
    pub fn gymrs_get_policy(e: *mut GymrsEngine, d_out: *mut GymrsPolicyDesc, weights_out: *mut f32, capacity_floats: u64) -> c_int;
    pub fn gymrs_policy_weights_ptr(e: *mut GymrsEngine, dev_out: *mut *mut f32, n_floats: *mut u64) -> c_int;
    pub fn gymrs_policy_actions(e: *mut GymrsEngine, actions_dev: *mut c_void) -> c_int;
    pub fn gymrs_rollout_policy(e: *mut GymrsEngine, n_steps: u32) -> c_int;
    pub fn gymrs_rollout_policy_record(e: *mut GymrsEngine, n_steps: u32, out: *const Trajectory) -> c_int;
    pub fn gymrs_rollout_policy_fitness(e: *mut GymrsEngine, n_steps: u32) -> c_int;
    pub fn gymrs_policy_fitness_ptr(e: *mut GymrsEngine, dev_out: *mut *mut GymrsPolicyFitness, n_policies: *mut u32) -> c_int;
    pub fn gymrs_get_policy_fitness(e: *mut GymrsEngine, first: u32, count: u32, host_out: *mut GymrsPolicyFitness) -> c_int;
    pub fn gymrs_policy_fitness_clear(e: *mut GymrsEngine) -> c_int;
    pub fn gymrs_rollout_closed_loop(e: *mut GymrsEngine, d: *const GymrsClosedLoopDesc) -> c_int;
    pub fn gymrs_rollout_transitions(e: *mut GymrsEngine, d: *const GymrsTransitionsDesc) -> c_int;
    /// advantages over a transitions record: the critic set (described by a `GymrsPolicyDesc`) and the GAE(lambda) scan in one launch
    pub fn gymrs_critic_size(kind: c_int, hidden: u32, n_floats: *mut u64) -> c_int;
    pub fn gymrs_set_critic(e: *mut GymrsEngine, d: *const GymrsPolicyDesc, weights_host: *const f32) -> c_int;
    pub fn gymrs_get_critic(e: *mut GymrsEngine, d_out: *mut GymrsPolicyDesc, weights_out: *mut f32, capacity_floats: u64) -> c_int;
    pub fn gymrs_critic_weights_ptr(e: *mut GymrsEngine, dev_out: *mut *mut f32, n_floats: *mut u64) -> c_int;
    pub fn gymrs_critic_value(kind: c_int, hidden: u32, weights: *const f32, obs: *const f32, v: *mut f32) -> c_int;
    pub fn gymrs_advantages(e: *mut GymrsEngine, d: *const GymrsAdvantagesDesc) -> c_int;
    /// gradients over a transitions record: exact fixed-point sums per set in one launch, and one lane of them on the host
    pub fn gymrs_policy_gradient(e: *mut GymrsEngine, d: *const GymrsGradientDesc) -> c_int;
    #[allow(clippy::too_many_arguments)]
    pub fn gymrs_gradient_lane(kind: c_int, hidden: u32, flags: u32, scale: f32, weights: *const f32, n_steps: u32, x: *const f32, actions: *const u8,
                               coef: *const f32, q: *mut i64, excluded: *mut u64, prob: *mut f32) -> c_int;
    /// the clipped surrogate (PPO) over a transitions record in one launch, and one lane of it on the host
    pub fn gymrs_ppo_gradient(e: *mut GymrsEngine, d: *const GymrsPpoDesc) -> c_int;
    #[allow(clippy::too_many_arguments)]
    pub fn gymrs_ppo_lane(kind: c_int, hidden: u32, scale: f32, clip_low: f32, clip_high: f32, weights: *const f32, n_steps: u32, x: *const f32,
                          actions: *const u8, advantages: *const f32, old_prob: *const f32, q: *mut i64, excluded: *mut u64, counts: *mut u64,
                          prob: *mut f32) -> c_int;
    pub fn gymrs_set_exploration(e: *mut GymrsEngine, x: *const GymrsExploration) -> c_int;
    pub fn gymrs_get_exploration(e: *mut GymrsEngine, x_out: *mut GymrsExploration) -> c_int;
    pub fn gymrs_explore_actions(e: *mut GymrsEngine, actions_dev: *mut c_void) -> c_int;
    pub fn gymrs_explore_draw(
        x: *const GymrsExploration,
        n_actions: u32,
        global_id: u64,
        tick: u64,
        explored: *mut u8,
        random_action: *mut u8,
    ) -> c_int;
    pub fn gymrs_set_sampling(e: *mut GymrsEngine, x: *const GymrsSampling) -> c_int;
    pub fn gymrs_get_sampling(e: *mut GymrsEngine, x_out: *mut GymrsSampling) -> c_int;
    pub fn gymrs_sample_actions(e: *mut GymrsEngine, actions_dev: *mut c_void, prob_dev: *mut f32) -> c_int;
    pub fn gymrs_sample_draw(
        x: *const GymrsSampling,
        n_actions: u32,
        logits: *const f32,
        global_id: u64,
        tick: u64,
        action: *mut u8,
        probs: *mut f32,
    ) -> c_int;
    pub fn gymrs_evaluate_policy(e: *mut GymrsEngine, d: *const GymrsEvalDesc) -> c_int;
    pub fn gymrs_get_policy_eval(e: *mut GymrsEngine, first: u32, count: u32, host_out: *mut GymrsPolicyEval) -> c_int;
    pub fn gymrs_policy_eval_ptr(e: *mut GymrsEngine, dev_out: *mut *mut GymrsPolicyEval, n_policies: *mut u32) -> c_int;
    pub fn gymrs_env_json(e: *mut GymrsEngine, lane: u64, buf: *mut c_char, cap: u64, needed: *mut u64) -> c_int;
    pub fn gymrs_params_from_json(kind: c_int, json: *const c_char, params: *mut c_void, state: *mut f64, state_dim: *mut c_int) -> c_int;
    // ABI 3: one batch over several GPUs in ONE process (one engine + one native host thread per block)
    pub fn gymrs_allreduce_stats_multi(shards: *mut *mut GymrsEngine, n: c_int, out4: *mut f64, used_rccl: *mut c_int) -> c_int;
    pub fn gymrs_sharded_create(
        kind: c_int,
        n_total: u64,
        global_env_offset: u64,
        n_shards: c_int,
        devices: *const c_int,
        params: *const c_void,
        flags: u32,
        out: *mut *mut GymrsSharded,
    ) -> c_int;
    pub fn gymrs_sharded_destroy(h: *mut GymrsSharded) -> c_int;
    pub fn gymrs_sharded_count(h: *mut GymrsSharded, n_shards: *mut c_int) -> c_int;
    pub fn gymrs_sharded_shard(
        h: *mut GymrsSharded,
        shard: c_int,
        engine: *mut *mut GymrsEngine,
        first_lane: *mut u64,
        n_lanes: *mut u64,
        device: *mut c_int,
    ) -> c_int;
    pub fn gymrs_sharded_reset(h: *mut GymrsSharded, has_seed: c_int, seed: u64, bounds_low_high: *const f32, seed_used: *mut u64) -> c_int;
    pub fn gymrs_sharded_step(h: *mut GymrsSharded, actions_dev: *const *const c_void) -> c_int;
    pub fn gymrs_sharded_step_many(
        h: *mut GymrsSharded,
        actions_dev: *const *const c_void,
        stride_bytes: u64,
        n_buffers: u32,
        n_steps: u32,
        use_graph: c_int,
    ) -> c_int;
    pub fn gymrs_sharded_fill_actions(h: *mut GymrsSharded, actions_dev: *const *mut c_void, seed: u64, t: u64) -> c_int;
    pub fn gymrs_sharded_rollout(h: *mut GymrsSharded, n_steps: u32, action_seed: u64, action_t0: u64) -> c_int;
    pub fn gymrs_sharded_set_policy(h: *mut GymrsSharded, d: *const GymrsPolicyDesc, weights_host: *const f32) -> c_int;
    pub fn gymrs_sharded_rollout_policy(h: *mut GymrsSharded, n_steps: u32) -> c_int;
    pub fn gymrs_sharded_rollout_policy_fitness(h: *mut GymrsSharded, n_steps: u32) -> c_int;
    pub fn gymrs_sharded_get_policy_fitness(h: *mut GymrsSharded, first: u32, count: u32, host_out: *mut GymrsPolicyFitness) -> c_int;
    pub fn gymrs_sharded_policy_fitness_clear(h: *mut GymrsSharded) -> c_int;
    pub fn gymrs_sharded_rollout_closed_loop(h: *mut GymrsSharded, d: *const GymrsClosedLoopDesc) -> c_int;
    pub fn gymrs_sharded_set_exploration(h: *mut GymrsSharded, x: *const GymrsExploration) -> c_int;
    pub fn gymrs_sharded_set_sampling(h: *mut GymrsSharded, x: *const GymrsSampling) -> c_int;
    pub fn gymrs_sharded_evaluate_policy(h: *mut GymrsSharded, d: *const GymrsEvalDesc) -> c_int;
    pub fn gymrs_sharded_set_param_table(h: *mut GymrsSharded, rows: *const c_void, k: u32) -> c_int;
    pub fn gymrs_sharded_get_param_table(h: *mut GymrsSharded, rows_out: *mut c_void, capacity: u32, k: *mut u32) -> c_int;
    pub fn gymrs_sharded_set_param_index(h: *mut GymrsSharded, first: u64, count: u64, index_host: *const u16) -> c_int;
    pub fn gymrs_sharded_get_param_index(h: *mut GymrsSharded, first: u64, count: u64, index_out: *mut u16) -> c_int;
    pub fn gymrs_sharded_get_policy_eval(h: *mut GymrsSharded, first: u32, count: u32, host_out: *mut GymrsPolicyEval) -> c_int;
    pub fn gymrs_sharded_set_params(h: *mut GymrsSharded, params: *const c_void) -> c_int;
    pub fn gymrs_sharded_sync(h: *mut GymrsSharded) -> c_int;
    pub fn gymrs_sharded_stats(h: *mut GymrsSharded, out4: *mut f64) -> c_int;
    pub fn gymrs_sharded_stats_clear(h: *mut GymrsSharded) -> c_int;
    pub fn gymrs_sharded_reduce_path(h: *mut GymrsSharded) -> *const c_char;
    pub fn gymrs_sharded_get_state(h: *mut GymrsSharded, first: u64, count: u64, host_out: *mut f32) -> c_int;
    pub fn gymrs_sharded_get_step_result(h: *mut GymrsSharded, first: u64, count: u64, reward: *mut f32, done: *mut u8, truncated: *mut u8) -> c_int;
}
