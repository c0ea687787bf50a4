//! Safe RAII wrapper of one `gymrs_engine` (one shard of lanes on one GPU, driven by one thread: `&mut self`).
use crate::ffi;
use std::ffi::CStr;
use std::os::raw::{c_int, c_void};

/// Which env the lanes of an engine are.
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum Kind {
    /// `CartPoleEnv` (cartpole.rs)
    CartPole,
    /// `MountainCarEnv` (mountain_car.rs)
    MountainCar,
}

impl Kind {
    fn raw(self) -> c_int {
        match self {
            Kind::CartPole => ffi::GYMRS_CARTPOLE,
            Kind::MountainCar => ffi::GYMRS_MOUNTAIN_CAR,
        }
    }
    /// Number of f32 state components per lane.
    pub fn state_dim(self) -> usize {
        match self {
            Kind::CartPole => 4,
            Kind::MountainCar => 2,
        }
    }
}

mod sealed {
    pub trait Sealed {}
    impl Sealed for crate::ffi::CartPoleParams {}
    impl Sealed for crate::ffi::MountainCarParams {}
}

/// The params struct of one env kind.  Sealed: only the two `#[repr(C)]` structs of [`crate::ffi`] implement it, each tied
/// to its [`Kind`], so a safe caller cannot hand `gymrs_engine_create` a struct of the wrong layout.
pub trait Params: sealed::Sealed + Copy {
    /// The env kind these params belong to.
    const KIND: Kind;
}
impl Params for ffi::CartPoleParams {
    const KIND: Kind = Kind::CartPole;
}
impl Params for ffi::MountainCarParams {
    const KIND: Kind = Kind::MountainCar;
}

/// The reference has no `Result`s: every failure is a panic (cartpole.rs:402-406, screen.rs:184-203).
/// So is every non-zero status of the C ABI here.
fn check(status: c_int) {
    if status != ffi::GYMRS_OK {
        let msg = unsafe { CStr::from_ptr(ffi::gymrs_last_error()) }.to_string_lossy().into_owned();
        panic!("gymrs_amd: status {status}: {msg}");
    }
}

/// Result of one step of one lane, as host values.
#[derive(Clone, Copy, Debug, PartialEq)]
pub struct LaneResult {
    /// reward of the step
    pub reward: f32,
    /// the episode terminated
    pub done: bool,
    /// the episode hit the time limit (only with `GYMRS_TIME_LIMIT`)
    pub truncated: bool,
}

/// Owns the engine handle; dropping it releases the device memory (`Env::close`, core.rs:56).
#[derive(Debug)]
pub struct Engine {
    raw: *mut ffi::GymrsEngine,
    kind: Kind,
    n: u64,
    device: i32,
}

impl Engine {
    /// `gymrs_engine_create` with the kind's default constants.
    pub fn with_defaults(kind: Kind, n_envs: u64, global_env_offset: u64, device: i32, flags: u32) -> Self {
        let mut raw = std::ptr::null_mut();
        check(unsafe { ffi::gymrs_engine_create(kind.raw(), n_envs, global_env_offset, device, std::ptr::null(), flags, &mut raw) });
        Engine { raw, kind, n: n_envs, device }
    }

    /// `gymrs_engine_create`; the env kind follows from the params type.
    pub fn new<P: Params>(n_envs: u64, global_env_offset: u64, device: i32, params: &P, flags: u32) -> Self {
        let mut raw = std::ptr::null_mut();
        check(unsafe {
            ffi::gymrs_engine_create(P::KIND.raw(), n_envs, global_env_offset, device, params as *const P as *const c_void, flags, &mut raw)
        });
        Engine { raw, kind: P::KIND, n: n_envs, device }
    }

    /// Assign the pub physics fields of every lane (`gymrs_set_params`): only the constants change -- state,
    /// `steps_beyond_terminated`, the episode clock, seed and tick carry on, exactly like `env.gravity = ..` on the
    /// reference struct between two `step()` calls (cartpole.rs:455-464 reads the fields afresh on every step).
    pub fn set_params<P: Params>(&mut self, params: &P) {
        assert_eq!(P::KIND, self.kind, "params of another env kind");
        check(unsafe { ffi::gymrs_set_params(self.raw, params as *const P as *const c_void) });
    }

    /// The GPU this engine lives on.
    pub fn device(&self) -> i32 {
        self.device
    }

    /// What `serde_json::to_string(&env)` prints for the reference env that lane `lane` stands for (`gymrs_env_json`).
    pub fn env_json(&mut self, lane: u64) -> String {
        let mut need = 0u64;
        let mut buf = vec![0u8; 2048];
        let mut st = unsafe { ffi::gymrs_env_json(self.raw, lane, buf.as_mut_ptr() as *mut _, buf.len() as u64, &mut need) };
        if st != ffi::GYMRS_OK && need as usize > buf.len() {
            buf = vec![0u8; need as usize];
            st = unsafe { ffi::gymrs_env_json(self.raw, lane, buf.as_mut_ptr() as *mut _, buf.len() as u64, &mut need) };
        }
        check(st);
        let end = buf.iter().position(|b| *b == 0).unwrap_or(buf.len());
        String::from_utf8_lossy(&buf[..end]).into_owned()
    }

    /// Number of lanes.
    pub fn len(&self) -> u64 {
        self.n
    }

    /// `true` for an engine without lanes.
    pub fn is_empty(&self) -> bool {
        self.n == 0
    }

    /// `Env::reset` for every lane; returns the seed used (seeding.rs:21-26 echoes it the same way).
    pub fn reset(&mut self, seed: Option<u64>, bounds_low_high: Option<&[f32]>) -> u64 {
        if let Some(b) = bounds_low_high {
            assert_eq!(b.len(), 2 * self.kind.state_dim(), "bounds = state_dim lows then state_dim highs");
        }
        let mut used = 0u64;
        check(unsafe {
            ffi::gymrs_reset(
                self.raw,
                seed.is_some() as c_int,
                seed.unwrap_or(0),
                bounds_low_high.map_or(std::ptr::null(), |b| b.as_ptr()),
                &mut used,
            )
        });
        used
    }

    /// The same reset drawn from the reference's own generator chain (`Pcg64::seed_from_u64` + `Uniform` over f64,
    /// seeding.rs:21-26): lane i holds, rounded once to f32, what gym-rs' `reset(Some(seed + offset + i))` returns.
    /// CartPole / MountainCar only.
    pub fn reset_pcg64(&mut self, seed: Option<u64>, bounds_low_high: Option<&[f64]>) -> u64 {
        if let Some(b) = bounds_low_high {
            assert_eq!(b.len(), 2 * self.kind.state_dim(), "bounds = state_dim lows then state_dim highs");
        }
        let mut used = 0u64;
        check(unsafe {
            ffi::gymrs_reset_pcg64(
                self.raw,
                seed.is_some() as c_int,
                seed.unwrap_or(0),
                std::ptr::null(),
                bounds_low_high.map_or(std::ptr::null(), |b| b.as_ptr()),
                &mut used,
            )
        });
        used
    }

    /// One `Env::step` of every lane with host actions (one u8 per lane), then wait for it.
    pub fn step_host(&mut self, actions: &[u8]) {
        assert_eq!(actions.len() as u64, self.n);
        check(unsafe { ffi::gymrs_step_host(self.raw, actions.as_ptr() as *const c_void) });
        check(unsafe { ffi::gymrs_sync(self.raw) });
    }

    /// One asynchronous `Env::step` with a device-resident action buffer (one u8 per lane).
    ///
    /// # Safety
    /// `actions_dev` must be a device address of at least `len()` bytes that stays valid until `sync()`.
    pub unsafe fn step_device(&mut self, actions_dev: *const c_void) {
        check(ffi::gymrs_step(self.raw, actions_dev));
    }

    /// `n_steps` consecutive `Env::step`s, step `t` taking its actions from buffer `t % n_buffers` of a ring of device buffers
    /// `stride_bytes` apart: ONE call, asynchronous on the engine's stream.  HIP launches by default (since round 6); with `GYMRS_AQL=1` in the
    /// process environment calls of 8 steps and more are submitted as a chain through the engine's own HSA queue (release fence only at the
    /// end of the chain: 4.9 instead of 6.4 us per 2^20-lane CartPole step; one process per GPU -- INTEGRATION.md "gymrs_step_many").  A caller
    /// that has K action buffers ready should prefer this to K `step_device` calls either way (one FFI call, one host loop).
    ///
    /// # Safety
    /// `actions_dev` must be a device address of `n_buffers` buffers of at least `len()` bytes each, valid until `sync()`.
    pub unsafe fn step_many(&mut self, actions_dev: *const c_void, stride_bytes: u64, n_buffers: u32, n_steps: u32, use_graph: bool) {
        check(ffi::gymrs_step_many(self.raw, actions_dev, stride_bytes, n_buffers, n_steps, use_graph as c_int));
    }

    /// `n_steps` random-policy steps fused into one launch (the loop of examples/cartpole.rs:15-30 per lane).
    pub fn rollout(&mut self, n_steps: u32, action_seed: u64, action_t0: u64) {
        check(unsafe { ffi::gymrs_rollout(self.raw, n_steps, action_seed, action_t0) });
    }

    /// `rollout` that also keeps every step's observation / action / reward / done in device buffers.
    ///
    /// # Safety
    /// The pointers in `out` must be device buffers of the sizes `include/gymrs_amd.h` documents for `gymrs_trajectory`
    /// and stay valid until `sync()`.
    pub unsafe fn rollout_record(&mut self, n_steps: u32, action_seed: u64, action_t0: u64, out: &ffi::Trajectory) {
        check(ffi::gymrs_rollout_record(self.raw, n_steps, action_seed, action_t0, out));
    }

    /// Install a policy set (`gymrs_set_policy`): `weights` holds `n_policies` policies of `gymrs_policy_size(kind, hidden)` floats back to
    /// back; lane `i` uses policy `((global_env_offset + i) / lanes_per_policy) % n_policies`.
    pub fn set_policy(&mut self, weights: &[f32], hidden: u32, n_policies: u32, lanes_per_policy: u64) {
        let mut size = 0u64;
        check(unsafe { ffi::gymrs_policy_size(self.kind.raw(), hidden, &mut size) });
        assert_eq!(weights.len() as u64, size * n_policies as u64);
        let d = ffi::GymrsPolicyDesc { hidden, n_policies, lanes_per_policy };
        check(unsafe { ffi::gymrs_set_policy(self.raw, &d, weights.as_ptr()) });
    }

    /// `n_steps` closed-loop steps fused into one launch: every step's actions are the policy's, computed from each lane's observation.
    pub fn rollout_policy(&mut self, n_steps: u32) {
        check(unsafe { ffi::gymrs_rollout_policy(self.raw, n_steps) });
    }

    /// `rollout_policy` that also adds every step's reward / done / truncated to the record of the lane's policy.
    pub fn rollout_policy_fitness(&mut self, n_steps: u32) {
        check(unsafe { ffi::gymrs_rollout_policy_fitness(self.raw, n_steps) });
    }

    /// `gymrs_rollout_closed_loop` without a record: `rollout_policy` (`fitness`: `rollout_policy_fitness`) behind one descriptor.
    /// `lane_params` (`GYMRS_CLOSED_LOOP_LANE_PARAMS`) lets it run while a parameter table is active: every lane steps with the row
    /// `step` would use for it, `n_steps` steps in one launch (without a table: no change).  An engine with a table refuses the plain call.
    pub fn rollout_closed_loop(&mut self, n_steps: u32, lane_params: bool, fitness: bool) {
        let flags = if lane_params { ffi::GYMRS_CLOSED_LOOP_LANE_PARAMS } else { 0 } | if fitness { ffi::GYMRS_CLOSED_LOOP_FITNESS } else { 0 };
        let d = ffi::GymrsClosedLoopDesc { n_steps, flags, record: std::ptr::null(), reserved: 0 };
        check(unsafe { ffi::gymrs_rollout_closed_loop(self.raw, &d) });
    }

    /// `rollout_closed_loop` that also keeps the trajectory (`rollout_policy_record`'s rows; no fitness: there is no recording fitness kernel).
    ///
    /// # Safety
    /// As `rollout_record`.
    pub unsafe fn rollout_closed_loop_record(&mut self, n_steps: u32, lane_params: bool, out: &ffi::Trajectory) {
        let flags = if lane_params { ffi::GYMRS_CLOSED_LOOP_LANE_PARAMS } else { 0 };
        let d = ffi::GymrsClosedLoopDesc { n_steps, flags, record: out, reserved: 0 };
        check(ffi::gymrs_rollout_closed_loop(self.raw, &d));
    }

    /// Install the exploration settings (`gymrs_set_exploration`): a step explores with probability `threshold` / 65536 (`threshold` in
    /// 0..=65536), drawing from a Philox stream keyed (`seed`, global lane id, engine tick).  `None` removes them.  Launches play them only
    /// through `rollout_closed_loop_explore`, `rollout_closed_loop_explore_record` and `explore_actions`; every other call stays greedy.
    pub fn set_exploration(&mut self, settings: Option<(u64, u32)>) {
        match settings {
            Some((seed, threshold)) => {
                let x = ffi::GymrsExploration { seed, threshold, reserved: 0 };
                check(unsafe { ffi::gymrs_set_exploration(self.raw, &x) });
            }
            None => check(unsafe { ffi::gymrs_set_exploration(self.raw, std::ptr::null()) }),
        }
    }

    /// `(seed, threshold)` as set (`gymrs_get_exploration`); panics when the engine has no exploration settings.
    pub fn exploration(&mut self) -> (u64, u32) {
        let mut x = ffi::GymrsExploration { seed: 0, threshold: 0, reserved: 0 };
        check(unsafe { ffi::gymrs_get_exploration(self.raw, &mut x) });
        (x.seed, x.threshold)
    }

    /// `rollout_closed_loop` with `GYMRS_CLOSED_LOOP_EXPLORE`: every step plays the epsilon-greedy action of `set_exploration`.
    pub fn rollout_closed_loop_explore(&mut self, n_steps: u32, lane_params: bool, fitness: bool) {
        let flags = ffi::GYMRS_CLOSED_LOOP_EXPLORE
            | if lane_params { ffi::GYMRS_CLOSED_LOOP_LANE_PARAMS } else { 0 }
            | if fitness { ffi::GYMRS_CLOSED_LOOP_FITNESS } else { 0 };
        let d = ffi::GymrsClosedLoopDesc { n_steps, flags, record: std::ptr::null(), reserved: 0 };
        check(unsafe { ffi::gymrs_rollout_closed_loop(self.raw, &d) });
    }

    /// `rollout_closed_loop_record` with `GYMRS_CLOSED_LOOP_EXPLORE`: the `actions` rows hold the action taken; which of them were
    /// exploratory is recomputed with `explore_draw` from (global lane id, tick of the row).
    ///
    /// # Safety
    /// As `rollout_record`.
    pub unsafe fn rollout_closed_loop_explore_record(&mut self, n_steps: u32, lane_params: bool, out: &ffi::Trajectory) {
        let flags = ffi::GYMRS_CLOSED_LOOP_EXPLORE | if lane_params { ffi::GYMRS_CLOSED_LOOP_LANE_PARAMS } else { 0 };
        let d = ffi::GymrsClosedLoopDesc { n_steps, flags, record: out, reserved: 0 };
        check(ffi::gymrs_rollout_closed_loop(self.raw, &d));
    }

    /// `gymrs_rollout_transitions`: `rollout_closed_loop_record` (`explore`: `rollout_closed_loop_explore_record`) that also writes, per
    /// step, the observation every ended lane showed before its re-arm into `final_obs` (`[n_steps][D][out.lane_stride]`; only the
    /// elements of ended lane-steps are written) and, unless null, the observations the launch starts from into `start_obs`
    /// (`[D][out.lane_stride]`).  The successor of step k is `final_obs[k]` where `done[k] | truncated[k]`, else `obs[k]`.  Engines with
    /// `GYMRS_AUTO_RESET` only.
    ///
    /// # Safety
    /// As `rollout_record`; `final_obs` and `start_obs` must be 16-byte aligned device addresses of those sizes, valid until `sync()`.
    pub unsafe fn rollout_transitions(&mut self, n_steps: u32, lane_params: bool, explore: bool, out: &ffi::Trajectory, final_obs: *mut f32, start_obs: *mut f32) {
        let flags = if lane_params { ffi::GYMRS_CLOSED_LOOP_LANE_PARAMS } else { 0 } | if explore { ffi::GYMRS_CLOSED_LOOP_EXPLORE } else { 0 };
        let d = ffi::GymrsTransitionsDesc { n_steps, flags, record: *out, final_obs, start_obs, reserved: 0 };
        check(ffi::gymrs_rollout_transitions(self.raw, &d));
    }

    /// Install a critic set (`gymrs_set_critic`): `n_critics` critics of `gymrs_critic_size(kind, hidden)` floats back to back; lane i
    /// uses critic `((global_env_offset + i) / lanes_per_critic) % n_critics`.  Survives `set_policy`; not part of clone or snapshot.
    pub fn set_critic(&mut self, weights: &[f32], hidden: u32, n_critics: u32, lanes_per_critic: u64) {
        let mut size = 0u64;
        check(unsafe { ffi::gymrs_critic_size(self.kind.raw(), hidden, &mut size) });
        assert_eq!(weights.len() as u64, size * n_critics as u64);
        let d = ffi::GymrsPolicyDesc { hidden, n_policies: n_critics, lanes_per_policy: lanes_per_critic };
        check(unsafe { ffi::gymrs_set_critic(self.raw, &d, weights.as_ptr()) });
    }

    /// Remove the critic set.
    pub fn clear_critic(&mut self) {
        check(unsafe { ffi::gymrs_set_critic(self.raw, std::ptr::null(), std::ptr::null()) });
    }

    /// Zero-copy device view of the critic set and its number of floats; valid until the next `set_critic` or drop.
    pub fn critic_weights_ptr(&mut self) -> (*mut f32, u64) {
        let (mut p, mut n) = (std::ptr::null_mut(), 0u64);
        check(unsafe { ffi::gymrs_critic_weights_ptr(self.raw, &mut p, &mut n) });
        (p, n)
    }

    /// `gymrs_advantages`: GAE(lambda) advantages (and, unless null, returns and values), each `[n_steps][record.lane_stride]`, from the
    /// rows `rollout_transitions` wrote, in one launch on the engine's stream.  `critic`: evaluate the critic set inside the kernel
    /// (`GYMRS_ADVANTAGES_CRITIC`), else V = 0.  `final_obs` may be null (records of engines without auto-reset).  Reads and writes no
    /// lane array.
    ///
    /// # Safety
    /// Every pointer must be a 16-byte aligned device address of the size the header names, valid until `sync()`.
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn advantages(&mut self, n_steps: u32, critic: bool, gamma: f32, lambda: f32, record: &ffi::Trajectory, final_obs: *const f32,
                             start_obs: *const f32, advantages: *mut f32, returns: *mut f32, values: *mut f32) {
        let flags = if critic { ffi::GYMRS_ADVANTAGES_CRITIC } else { 0 };
        let d = ffi::GymrsAdvantagesDesc { n_steps, flags, gamma, lambda, record: *record, final_obs, start_obs, advantages, returns, values, reserved: 0 };
        check(ffi::gymrs_advantages(self.raw, &d));
    }

    /// `gymrs_policy_gradient`: ADDS the fixed-point score-function gradient of the policy set over a transitions record (or, with
    /// `critic`, the value gradient of the critic set: `GYMRS_GRADIENT_CRITIC`) to `grad` (int64 `[n_sets][S]`; the gradient is
    /// `grad * 2^-24`) and the (lane, parameter) pairs left out to `excluded` (u64 `[n_sets]`), in one launch on the engine's stream.
    /// `scale` = log2(e) / temperature (policy head only); `prob` may be null and must be with `critic`.  Reads and writes no lane array.
    ///
    /// # Safety
    /// Every row pointer must be a 16-byte aligned device address of the size the header names, `grad` and `excluded` 8-byte aligned,
    /// all valid until `sync()`.
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn policy_gradient(&mut self, n_steps: u32, critic: bool, scale: f32, record: &ffi::Trajectory, start_obs: *const f32, coef: *const f32,
                                  prob: *mut f32, grad: *mut i64, excluded: *mut u64) {
        let flags = if critic { ffi::GYMRS_GRADIENT_CRITIC } else { 0 };
        let d = ffi::GymrsGradientDesc { n_steps, flags, scale, pad_: 0, record: *record, start_obs, coef, prob, grad, excluded, reserved: 0 };
        check(ffi::gymrs_policy_gradient(self.raw, &d));
    }

    /// `gymrs_ppo_gradient`: `policy_gradient` for the policy head with the coefficient computed in the kernel from the `advantages`
    /// row and the `old_prob` row under the clip range `[clip_low, clip_high]`: ADDS the gradient of PPO's clipped objective (to
    /// ascend) to `grad` and `excluded` and, when `counts` (u64 `[n_sets][2]`) is not null, the lane-steps seen and cut.  `prob` may be
    /// null and may not be `old_prob`.  Reads and writes no lane array.
    ///
    /// # Safety
    /// Every row pointer must be a 16-byte aligned device address of the size the header names, `grad`, `excluded` and `counts` 8-byte
    /// aligned, all valid until `sync()`.
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn ppo_gradient(&mut self, n_steps: u32, scale: f32, clip_low: f32, clip_high: f32, record: &ffi::Trajectory, start_obs: *const f32,
                               advantages: *const f32, old_prob: *const f32, prob: *mut f32, grad: *mut i64, excluded: *mut u64, counts: *mut u64) {
        let d = ffi::GymrsPpoDesc { n_steps, flags: 0, scale, clip_low, clip_high, pad_: 0, record: *record, start_obs, advantages, old_prob, prob,
                                    grad, excluded, counts, reserved: 0 };
        check(ffi::gymrs_ppo_gradient(self.raw, &d));
    }

    /// The policy's action mixed with the exploration draw at the engine's current tick, one u8 per lane (`gymrs_explore_actions`):
    /// `explore_actions` + `step_device`, K times, is `rollout_closed_loop_explore(K, ..)`.
    ///
    /// # Safety
    /// `actions_dev` must be a device address of at least `len()` bytes that stays valid until `sync()`.
    pub unsafe fn explore_actions(&mut self, actions_dev: *mut c_void) {
        check(ffi::gymrs_explore_actions(self.raw, actions_dev));
    }

    /// Install the sampling settings (`gymrs_set_sampling`): a ~ softmax(logits / temperature) with `scale` = log2(e) / temperature
    /// (finite, >= 0; 0 is the uniform policy), drawn from a Philox stream keyed (`seed`, global lane id, engine tick).  `None`
    /// removes them.  Launches play them only through `rollout_closed_loop_sample`, `rollout_closed_loop_sample_record`,
    /// `rollout_transitions_sample` and `sample_actions`; every other call stays greedy.
    pub fn set_sampling(&mut self, settings: Option<(u64, f32)>) {
        match settings {
            Some((seed, scale)) => {
                let x = ffi::GymrsSampling { seed, scale, reserved: 0 };
                check(unsafe { ffi::gymrs_set_sampling(self.raw, &x) });
            }
            None => check(unsafe { ffi::gymrs_set_sampling(self.raw, std::ptr::null()) }),
        }
    }

    /// `(seed, scale)` as set (`gymrs_get_sampling`); panics when the engine has no sampling settings.
    pub fn sampling(&mut self) -> (u64, f32) {
        let mut x = ffi::GymrsSampling { seed: 0, scale: 0.0, reserved: 0 };
        check(unsafe { ffi::gymrs_get_sampling(self.raw, &mut x) });
        (x.seed, x.scale)
    }

    /// `rollout_closed_loop` with `GYMRS_CLOSED_LOOP_SAMPLE`: every step plays the action drawn under `set_sampling`.
    pub fn rollout_closed_loop_sample(&mut self, n_steps: u32, lane_params: bool, fitness: bool) {
        let flags = ffi::GYMRS_CLOSED_LOOP_SAMPLE
            | if lane_params { ffi::GYMRS_CLOSED_LOOP_LANE_PARAMS } else { 0 }
            | if fitness { ffi::GYMRS_CLOSED_LOOP_FITNESS } else { 0 };
        let d = ffi::GymrsClosedLoopDesc { n_steps, flags, record: std::ptr::null(), reserved: 0 };
        check(unsafe { ffi::gymrs_rollout_closed_loop(self.raw, &d) });
    }

    /// `rollout_closed_loop_record` with `GYMRS_CLOSED_LOOP_SAMPLE`: the `actions` rows hold the action taken; its probability is
    /// recomputed from the `obs` rows with the weights the learner holds (`sample_draw` is the rule as code).
    ///
    /// # Safety
    /// As `rollout_record`.
    pub unsafe fn rollout_closed_loop_sample_record(&mut self, n_steps: u32, lane_params: bool, out: &ffi::Trajectory) {
        let flags = ffi::GYMRS_CLOSED_LOOP_SAMPLE | if lane_params { ffi::GYMRS_CLOSED_LOOP_LANE_PARAMS } else { 0 };
        let d = ffi::GymrsClosedLoopDesc { n_steps, flags, record: out, reserved: 0 };
        check(ffi::gymrs_rollout_closed_loop(self.raw, &d));
    }

    /// `rollout_transitions` with `GYMRS_CLOSED_LOOP_SAMPLE`.
    ///
    /// # Safety
    /// As `rollout_transitions`.
    pub unsafe fn rollout_transitions_sample(&mut self, n_steps: u32, lane_params: bool, out: &ffi::Trajectory, final_obs: *mut f32, start_obs: *mut f32) {
        let flags = ffi::GYMRS_CLOSED_LOOP_SAMPLE | if lane_params { ffi::GYMRS_CLOSED_LOOP_LANE_PARAMS } else { 0 };
        let d = ffi::GymrsTransitionsDesc { n_steps, flags, record: *out, final_obs, start_obs, reserved: 0 };
        check(ffi::gymrs_rollout_transitions(self.raw, &d));
    }

    /// The sampled action at the engine's current tick, one u8 per lane, and (unless null) the probability of that action, one f32
    /// per lane (`gymrs_sample_actions`): `sample_actions` + `step_device`, K times, is `rollout_closed_loop_sample(K, ..)`.
    ///
    /// # Safety
    /// `actions_dev` must be a device address of at least `len()` bytes, `prob_dev` null or one of `len()` floats; both stay valid
    /// until `sync()`.
    pub unsafe fn sample_actions(&mut self, actions_dev: *mut c_void, prob_dev: *mut f32) {
        check(ffi::gymrs_sample_actions(self.raw, actions_dev, prob_dev));
    }

    /// The records of policies `first..first+count` (synchronising).
    pub fn policy_fitness(&mut self, first: u32, count: u32) -> Vec<ffi::GymrsPolicyFitness> {
        let mut out = vec![ffi::GymrsPolicyFitness::default(); count as usize];
        check(unsafe { ffi::gymrs_get_policy_fitness(self.raw, first, count, out.as_mut_ptr()) });
        out
    }

    /// Zero-copy device view of the records and their number; valid until the next `set_policy` or drop.
    pub fn policy_fitness_ptr(&mut self) -> (*mut ffi::GymrsPolicyFitness, u32) {
        let (mut p, mut n) = (std::ptr::null_mut(), 0u32);
        check(unsafe { ffi::gymrs_policy_fitness_ptr(self.raw, &mut p, &mut n) });
        (p, n)
    }

    /// Zero the records (in stream order).
    pub fn policy_fitness_clear(&mut self) {
        check(unsafe { ffi::gymrs_policy_fitness_clear(self.raw) });
    }

    /// Play `episodes_per_lane` whole episodes of every lane under its policy in one launch (`gymrs_evaluate_policy`): episode `e`
    /// starts where `reset(seed + e)` would put the lane and ends at its first done or after `max_episode_steps` steps (0 = the
    /// params' limit).  `lengths_dev`: device `u32 [episodes_per_lane][n_envs]` for length | done << 31, or null.
    pub fn evaluate_policy(&mut self, episodes_per_lane: u32, max_episode_steps: u32, seed: u64, common_starts: bool, lengths_dev: *mut u32) {
        let flags = if common_starts { ffi::GYMRS_EVAL_COMMON_STARTS } else { 0 };
        let d = ffi::GymrsEvalDesc { episodes_per_lane, max_episode_steps, seed, flags, reserved: 0, lengths_dev };
        check(unsafe { ffi::gymrs_evaluate_policy(self.raw, &d) });
    }

    /// `evaluate_policy` with `GYMRS_EVAL_LANE_PARAMS`: every lane plays with the row of the parameter table `step` would use for it
    /// (without a table: exactly `evaluate_policy`).  An engine with a table refuses the plain call.
    pub fn evaluate_policy_lane_params(&mut self, episodes_per_lane: u32, max_episode_steps: u32, seed: u64, common_starts: bool, lengths_dev: *mut u32) {
        let flags = ffi::GYMRS_EVAL_LANE_PARAMS | if common_starts { ffi::GYMRS_EVAL_COMMON_STARTS } else { 0 };
        let d = ffi::GymrsEvalDesc { episodes_per_lane, max_episode_steps, seed, flags, reserved: 0, lengths_dev };
        check(unsafe { ffi::gymrs_evaluate_policy(self.raw, &d) });
    }

    /// The episodic records of policies `first..first+count` of the latest `evaluate_policy` (synchronising).
    pub fn policy_eval(&mut self, first: u32, count: u32) -> Vec<ffi::GymrsPolicyEval> {
        let mut out = vec![ffi::GymrsPolicyEval::default(); count as usize];
        check(unsafe { ffi::gymrs_get_policy_eval(self.raw, first, count, out.as_mut_ptr()) });
        out
    }

    /// Zero-copy device view of the episodic records and their number; valid until the next `set_policy` or drop.
    pub fn policy_eval_ptr(&mut self) -> (*mut ffi::GymrsPolicyEval, u32) {
        let (mut p, mut n) = (std::ptr::null_mut(), 0u32);
        check(unsafe { ffi::gymrs_policy_eval_ptr(self.raw, &mut p, &mut n) });
        (p, n)
    }

    /// Wait for everything queued on the engine's stream.
    pub fn sync(&mut self) {
        check(unsafe { ffi::gymrs_sync(self.raw) });
    }

    /// State of lanes `first..first+count`, component-major (`[component][lane]`).
    pub fn state(&mut self, first: u64, count: u64) -> Vec<f32> {
        let mut out = vec![0f32; self.kind.state_dim() * count as usize];
        check(unsafe { ffi::gymrs_get_state(self.raw, first, count, out.as_mut_ptr()) });
        out
    }

    /// Overwrite the state of lanes `first..first+count` (like assigning the pub `state` field).
    pub fn set_state(&mut self, first: u64, count: u64, component_major: &[f32]) {
        assert_eq!(component_major.len(), self.kind.state_dim() * count as usize);
        check(unsafe { ffi::gymrs_set_state(self.raw, first, count, component_major.as_ptr()) });
    }

    /// Reward / done / truncated of the last step of one lane.
    pub fn lane_result(&mut self, lane: u64) -> LaneResult {
        let (mut reward, mut done, mut truncated) = (0f32, 0u8, 0u8);
        check(unsafe { ffi::gymrs_get_step_result(self.raw, lane, 1, &mut reward, &mut done, &mut truncated) });
        LaneResult { reward, done: done != 0, truncated: truncated != 0 }
    }

    /// `[sum_return, sum_length, n_episodes, n_steps]` since the last reset / clear.
    pub fn stats(&mut self) -> [f64; 4] {
        let mut out = [0f64; 4];
        check(unsafe { ffi::gymrs_stats(self.raw, out.as_mut_ptr()) });
        out
    }

    /// Opaque blob holding everything a step can observe (`Serialize`).
    pub fn snapshot(&mut self) -> Vec<u8> {
        let mut bytes = 0u64;
        check(unsafe { ffi::gymrs_snapshot_size(self.raw, &mut bytes) });
        let mut buf = vec![0u8; bytes as usize];
        check(unsafe { ffi::gymrs_snapshot_save(self.raw, buf.as_mut_ptr() as *mut c_void, bytes) });
        buf
    }

    /// Load a `snapshot()` of an engine with the same kind, lane count and flags.
    pub fn restore(&mut self, blob: &[u8]) {
        check(unsafe { ffi::gymrs_snapshot_load(self.raw, blob.as_ptr() as *const c_void, blob.len() as u64) });
    }
}

/// `(explored, random action)` of the epsilon-greedy draw that takes the lane with global id `global_id` from engine tick `tick` to
/// `tick + 1` under `(seed, threshold)` (`gymrs_explore_draw`; host only, no GPU).
pub fn explore_draw(seed: u64, threshold: u32, n_actions: u32, global_id: u64, tick: u64) -> (bool, u8) {
    let x = ffi::GymrsExploration { seed, threshold, reserved: 0 };
    let (mut explored, mut action) = (0u8, 0u8);
    check(unsafe { ffi::gymrs_explore_draw(&x, n_actions, global_id, tick, &mut explored, &mut action) });
    (explored != 0, action)
}

/// `(action, probabilities)` of the softmax draw that takes the lane with global id `global_id` from engine tick `tick` to
/// `tick + 1` under `(seed, scale)` from 2..=8 `logits` (`gymrs_sample_draw`; host only, no GPU).
pub fn sample_draw(seed: u64, scale: f32, logits: &[f32], global_id: u64, tick: u64) -> (u8, Vec<f32>) {
    let x = ffi::GymrsSampling { seed, scale, reserved: 0 };
    let mut action = 0u8;
    let mut probs = vec![0.0f32; logits.len()];
    check(unsafe { ffi::gymrs_sample_draw(&x, logits.len() as u32, logits.as_ptr(), global_id, tick, &mut action, probs.as_mut_ptr()) });
    (action, probs)
}

impl Clone for Engine {
    /// Deep copy on the device (`gymrs_engine_clone`): state, episode bookkeeping, RNG position.
    fn clone(&self) -> Self {
        let mut raw = std::ptr::null_mut();
        check(unsafe { ffi::gymrs_engine_clone(self.raw, &mut raw) });
        Engine { raw, kind: self.kind, n: self.n, device: self.device }
    }
}

impl Drop for Engine {
    fn drop(&mut self) {
        if !self.raw.is_null() {
            unsafe { ffi::gymrs_engine_destroy(self.raw) };
            self.raw = std::ptr::null_mut();
        }
    }
}
