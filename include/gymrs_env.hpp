// gymrs_env.hpp — header-only C++ mirror of the reference's trait surface over the C ABI (gymrs_amd.h).
//
// The reference is a Rust crate; this image has no Rust toolchain, so the host side above the C ABI is
// C++ (the reference is compiled code).  Names, argument meaning and error behaviour follow
//   trait Env / EnvProperties           /root/reference/src/core.rs:25-90
//   ActionReward, RewardRange           /root/reference/src/core.rs:94-122
//   Discrete, BoxR                      /root/reference/src/spaces/discrete.rs:12-20, box_r.rs:5-13
//   CartPoleEnv, CartPoleObservation    /root/reference/src/envs/classical_control/cartpole.rs:51-87,328-349
//   MountainCarEnv, ...Observation      /root/reference/src/envs/classical_control/mountain_car.rs:46-84,122-128
// so a test written against gym-rs reads the same here.  A single env is ONE lane of the batched GPU
// engine (plumbing configuration); `VecEnv` is the batched form the hot path is built for.
// Errors: the reference panics (assert!/unwrap); here they are C++ exceptions (gymrs::Panic).
#pragma once
#include <cmath>
#include <cstdint>
#include <limits>
#include <array>
#include <optional>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "gymrs_amd.h"

namespace gymrs {

struct Panic : std::runtime_error {
    gymrs_status status;
    Panic(gymrs_status s, const std::string& m) : std::runtime_error(m), status(s) {}
};
inline void check(gymrs_status s)
{
    if (s != GYMRS_OK) throw Panic(s, gymrs_last_error());
}

enum class RenderMode { Human, SingleRgbArray, RgbArray, Ansi, None }; // utils/renderer.rs:83-114 (only None is supported)

struct Discrete { // spaces/discrete.rs:12-20
    std::size_t n;
    bool contains(std::size_t value) const { return value < n; }
    bool operator==(const Discrete& o) const { return n == o.n; }
};
template <class T>
struct BoxR { // spaces/box_r.rs:5-13
    T low, high;
};
struct RewardRange { // core.rs:109-122, default (-inf, inf) core.rs:16-19
    double lower_bound = -std::numeric_limits<double>::infinity();
    double upper_bound = std::numeric_limits<double>::infinity();
};
template <class Obs, class Info>
struct ActionReward { // core.rs:94-106
    Obs observation;
    double reward;
    bool done;
    bool truncated;
    std::optional<Info> info;
};
struct Unit {}; // Rust's ()

// Which generator reset() draws the start state from: the build's counter-based Philox stream (default), or the
// reference's own Pcg64::seed_from_u64 + Uniform chain, so that reset(Some(s)) returns the reference's state for s.
enum class ResetRng { Philox, Pcg64 };

struct CartPoleObservation { // cartpole.rs:328-334; Into<Vec<f64>> order :336-349
    double x, x_dot, theta, theta_dot;
    std::vector<double> to_vec() const { return {x, x_dot, theta, theta_dot}; }
    CartPoleObservation operator-() const { return {-x, -x_dot, -theta, -theta_dot}; } // :367-378
};
struct MountainCarObservation { // mountain_car.rs:122-128
    double position, velocity;
    std::vector<double> to_vec() const { return {position, velocity}; }
};

// The epsilon-greedy draw of (global lane id, engine tick) under settings x (gymrs_explore_draw; host only, no GPU): {explored,
// random action}.  Which actions of a recorded batch were exploratory is recomputed with it, no trajectory row is spent on them.
inline std::pair<bool, std::uint8_t> explore_draw(const gymrs_exploration& x, std::uint32_t n_actions, std::uint64_t global_id, std::uint64_t tick)
{
    std::uint8_t explored = 0, action = 0;
    check(gymrs_explore_draw(&x, n_actions, global_id, tick, &explored, &action));
    return {explored != 0, action};
}

// The softmax draw of (global lane id, engine tick) under settings x from n_actions logits (gymrs_sample_draw; host only, no GPU):
// the action; probs (may be null) gets the n_actions probabilities.  The definition of include/gymrs_amd.h, "sampling", as code.
inline std::uint8_t sample_draw(const gymrs_sampling& x, std::uint32_t n_actions, const float* logits, std::uint64_t global_id, std::uint64_t tick,
                                float* probs = nullptr)
{
    std::uint8_t action = 0;
    check(gymrs_sample_draw(&x, n_actions, logits, global_id, tick, &action, probs));
    return action;
}

// One lane's contribution to gymrs_policy_gradient (gymrs_gradient_lane; host only, no GPU): q[0 .. S) is set, the number of
// excluded (lane, parameter) pairs returned; prob (may be null, null with GYMRS_GRADIENT_CRITIC) gets p[a] of every step.  The
// definition of include/gymrs_amd.h, "gradients", as code.
inline std::uint64_t gradient_lane(gymrs_env_kind kind, std::uint32_t hidden, std::uint32_t flags, float scale, const float* weights, std::uint32_t n_steps,
                                   const float* x, const std::uint8_t* actions, const float* coef, std::int64_t* q, float* prob = nullptr)
{
    std::uint64_t excluded = 0;
    check(gymrs_gradient_lane(kind, hidden, flags, scale, weights, n_steps, x, actions, coef, q, &excluded, prob));
    return excluded;
}

// One lane's contribution to gymrs_ppo_gradient (gymrs_ppo_lane; host only, no GPU): q[0 .. S) is set, the number of excluded
// (lane, parameter) pairs returned; counts (may be null) gets the lane-steps seen and cut, prob (may be null) p[a] of every step.
// The definition of include/gymrs_amd.h, "clipped surrogate", as code.
inline std::uint64_t ppo_lane(gymrs_env_kind kind, std::uint32_t hidden, float scale, float clip_low, float clip_high, const float* weights,
                              std::uint32_t n_steps, const float* x, const std::uint8_t* actions, const float* advantages, const float* old_prob,
                              std::int64_t* q, std::uint64_t* counts = nullptr, float* prob = nullptr)
{
    std::uint64_t excluded = 0;
    check(gymrs_ppo_lane(kind, hidden, scale, clip_low, clip_high, weights, n_steps, x, actions, advantages, old_prob, q, &excluded, counts, prob));
    return excluded;
}

// ---- batched form: the shape the hot path is built for ---------------------------------------------
class VecEnv {
public:
    VecEnv(gymrs_env_kind kind, std::uint64_t n_envs, std::uint32_t flags = 0, const void* params = nullptr,
           std::uint64_t global_env_offset = 0, int device = 0)
        : kind_(kind), n_(n_envs)
    {
        check(gymrs_engine_create(kind, n_envs, global_env_offset, device, params, flags, &e_));
        int d = 0;
        float* p[4];
        check(gymrs_state_ptrs(e_, p, &d));
        state_dim_ = d;
    }
    ~VecEnv() { gymrs_engine_destroy(e_); }
    // `Env: Clone` (core.rs:25): a deep copy on the device, including the RNG position (seed, tick)
    VecEnv(const VecEnv& other) : kind_(other.kind_), n_(other.n_), state_dim_(other.state_dim_)
    {
        check(gymrs_engine_clone(other.e_, &e_));
    }
    VecEnv& operator=(const VecEnv&) = delete;

    std::uint64_t reset(std::optional<std::uint64_t> seed, const float* bounds_low_high = nullptr)
    {
        std::uint64_t used = 0;
        check(gymrs_reset(e_, seed.has_value(), seed.value_or(0), bounds_low_high, &used));
        return used;
    }
    // The same reset drawn from the reference's own generator chain (Pcg64::seed_from_u64 + Uniform over f64,
    // seeding.rs:21-26): lane i = the reference's reset(Some(seed + offset + i)) rounded to f32 (gymrs_reset_pcg64).
    std::uint64_t reset_pcg64(std::optional<std::uint64_t> seed, const double* bounds_low_high = nullptr,
                              const std::uint64_t* seeds_dev = nullptr)
    {
        std::uint64_t used = 0;
        check(gymrs_reset_pcg64(e_, seed.has_value(), seed.value_or(0), seeds_dev, bounds_low_high, &used));
        return used;
    }
    void step_device(const void* actions_dev) { check(gymrs_step(e_, actions_dev)); } // async
    void step_host(const void* actions_host)
    {
        check(gymrs_step_host(e_, actions_host));
        check(gymrs_sync(e_));
    }
    // n_steps consecutive steps, step t with the actions of buffer t % n_buffers of a ring of device buffers stride_bytes apart; one
    // asynchronous call (8 steps and more: one chain through the engine's own HSA queue)
    void step_many(const void* actions_dev, std::uint64_t stride_bytes, std::uint32_t n_buffers, std::uint32_t n_steps, bool use_graph = false)
    {
        check(gymrs_step_many(e_, actions_dev, stride_bytes, n_buffers, n_steps, use_graph ? 1 : 0));
    }
    void sync() { check(gymrs_sync(e_)); }
    // the loop of examples/cartpole.rs:15-30 (random action, step, reset on done) for every lane, fused into one launch
    void rollout(std::uint32_t n_steps, std::uint64_t action_seed, std::uint64_t action_t0 = 0)
    {
        check(gymrs_rollout(e_, n_steps, action_seed, action_t0));
    }
    // the same loop keeping every step's (observation, action, reward, done) in device buffers
    void rollout_record(std::uint32_t n_steps, std::uint64_t action_seed, std::uint64_t action_t0, const gymrs_trajectory& out)
    {
        check(gymrs_rollout_record(e_, n_steps, action_seed, action_t0, &out));
    }
    // GYMRS_FINAL_OBS engines: zero-copy device views of the observation each lane's last finished episode ended in
    // (obs_dim SoA rows, the layout of gymrs_obs_ptrs); throws on an engine created without the flag
    std::vector<float*> final_obs_views()
    {
        float* p[4];
        int d = 0;
        check(gymrs_final_obs_ptrs(e_, p, &d));
        return std::vector<float*>(p, p + d);
    }
    std::array<double, 4> stats() // {sum_return, sum_length, n_episodes, n_steps}
    {
        std::array<double, 4> out{};
        check(gymrs_stats(e_, out.data()));
        return out;
    }
    // `Env: Serialize` (core.rs:25): everything a step can observe, as an opaque blob
    std::vector<unsigned char> snapshot()
    {
        std::uint64_t bytes = 0;
        check(gymrs_snapshot_size(e_, &bytes));
        std::vector<unsigned char> blob(bytes);
        check(gymrs_snapshot_save(e_, blob.data(), bytes));
        return blob;
    }
    void restore(const std::vector<unsigned char>& blob) { check(gymrs_snapshot_load(e_, blob.data(), blob.size())); }
    std::vector<float> state(std::uint64_t first, std::uint64_t count)
    {
        std::vector<float> out(count * state_dim_);
        check(gymrs_get_state(e_, first, count, out.data()));
        return out;
    }
    void set_state(std::uint64_t first, std::uint64_t count, const float* soa) { check(gymrs_set_state(e_, first, count, soa)); }
    void result(std::uint64_t first, std::uint64_t count, float* reward, std::uint8_t* done, std::uint8_t* truncated)
    {
        check(gymrs_get_step_result(e_, first, count, reward, done, truncated));
    }
    // the pub physics fields after construction (cartpole.rs:53-82): only the constants change, the episode carries on
    void set_params(const void* params) { check(gymrs_set_params(e_, params)); }
    void get_params(void* params_out) { check(gymrs_get_params(e_, params_out)); }
    // per-lane physics (gymrs_set_param_table): lane i steps with rows[index[i]]; set_param_table(nullptr, 0) switches it off
    void set_param_table(const void* rows, std::uint32_t k) { check(gymrs_set_param_table(e_, rows, k)); }
    std::uint32_t param_table(void* rows_out, std::uint32_t capacity)
    {
        std::uint32_t k = 0;
        check(gymrs_get_param_table(e_, rows_out, capacity, &k));
        return k;
    }
    std::uint16_t* param_index_view()
    {
        std::uint16_t* p = nullptr;
        check(gymrs_param_index_ptr(e_, &p));
        return p;
    }
    void set_param_index(std::uint64_t first, std::uint64_t count, const std::uint16_t* index) { check(gymrs_set_param_index(e_, first, count, index)); }
    std::vector<std::uint16_t> param_index(std::uint64_t first, std::uint64_t count)
    {
        std::vector<std::uint16_t> out(count);
        check(gymrs_get_param_index(e_, first, count, out.data()));
        return out;
    }
    void lane_params(std::uint64_t lane, void* params_out) { check(gymrs_get_lane_params(e_, lane, params_out)); }
    // closed-loop rollouts (gymrs_set_policy): n_policies policies of policy_size(kind, hidden) floats back to back; lane i uses
    // policy ((global_env_offset + i) / lanes_per_policy) % n_policies; clear_policy() removes the set
    static std::uint64_t policy_size(gymrs_env_kind kind, std::uint32_t hidden)
    {
        std::uint64_t n = 0;
        check(gymrs_policy_size(kind, hidden, &n));
        return n;
    }
    void set_policy(const float* weights_host, std::uint32_t hidden, std::uint32_t n_policies, std::uint64_t lanes_per_policy)
    {
        const gymrs_policy_desc d{hidden, n_policies, lanes_per_policy};
        check(gymrs_set_policy(e_, &d, weights_host));
    }
    void clear_policy() { check(gymrs_set_policy(e_, nullptr, nullptr)); }
    gymrs_policy_desc policy(float* weights_out = nullptr, std::uint64_t capacity_floats = 0)
    {
        gymrs_policy_desc d{};
        check(gymrs_get_policy(e_, &d, weights_out, capacity_floats));
        return d;
    }
    float* policy_weights_view(std::uint64_t* n_floats = nullptr)
    {
        float* p = nullptr;
        check(gymrs_policy_weights_ptr(e_, &p, n_floats));
        return p;
    }
    void policy_actions(void* actions_dev) { check(gymrs_policy_actions(e_, actions_dev)); }
    // n_steps of (policy_actions, step) fused into one launch; the second form keeps the trajectory
    void rollout_policy(std::uint32_t n_steps) { check(gymrs_rollout_policy(e_, n_steps)); }
    void rollout_policy_record(std::uint32_t n_steps, const gymrs_trajectory& out) { check(gymrs_rollout_policy_record(e_, n_steps, &out)); }
    // per-policy fitness: rollout_policy that also adds every step's reward / done / truncated to the record of the lane's policy
    void rollout_policy_fitness(std::uint32_t n_steps) { check(gymrs_rollout_policy_fitness(e_, n_steps)); }
    // the three calls above behind one descriptor with a flags word; lane_params (GYMRS_CLOSED_LOOP_LANE_PARAMS): under an active
    // parameter table every lane steps with its own row, n_steps steps in one launch (without a table: no change)
    void rollout_closed_loop(const gymrs_closed_loop_desc& d) { check(gymrs_rollout_closed_loop(e_, &d)); }
    void rollout_closed_loop(std::uint32_t n_steps, bool lane_params = false, bool fitness = false, const gymrs_trajectory* record = nullptr)
    {
        const gymrs_closed_loop_desc d{n_steps, (lane_params ? GYMRS_CLOSED_LOOP_LANE_PARAMS : 0u) | (fitness ? GYMRS_CLOSED_LOOP_FITNESS : 0u), record, 0};
        check(gymrs_rollout_closed_loop(e_, &d));
    }
    // epsilon-greedy exploration (gymrs_set_exploration): a step explores with probability threshold / 65536, drawing from a Philox
    // stream keyed (seed, global lane id, engine tick); launches play it with explore = true (GYMRS_CLOSED_LOOP_EXPLORE) only
    void set_exploration(std::uint64_t seed, std::uint32_t threshold)
    {
        const gymrs_exploration x{seed, threshold, 0};
        check(gymrs_set_exploration(e_, &x));
    }
    void clear_exploration() { check(gymrs_set_exploration(e_, nullptr)); }
    gymrs_exploration exploration() const
    {
        gymrs_exploration x{};
        check(gymrs_get_exploration(e_, &x));
        return x;
    }
    // policy_actions mixed with the draw at the engine's current tick: explore_actions + step_device, K times, is
    // rollout_closed_loop(K, .., explore = true)
    void explore_actions(void* actions_dev) { check(gymrs_explore_actions(e_, actions_dev)); }
    void rollout_closed_loop(std::uint32_t n_steps, bool lane_params, bool fitness, const gymrs_trajectory* record, bool explore)
    {
        const gymrs_closed_loop_desc d{n_steps,
                                       (lane_params ? GYMRS_CLOSED_LOOP_LANE_PARAMS : 0u) | (fitness ? GYMRS_CLOSED_LOOP_FITNESS : 0u) |
                                           (explore ? GYMRS_CLOSED_LOOP_EXPLORE : 0u),
                                       record, 0};
        check(gymrs_rollout_closed_loop(e_, &d));
    }
    // softmax sampling (gymrs_set_sampling): a ~ softmax(logits / temperature), scale = log2(e) / temperature, drawn from a Philox
    // stream keyed (seed, global lane id, engine tick); launches play it with sample = true (GYMRS_CLOSED_LOOP_SAMPLE) only
    void set_sampling(std::uint64_t seed, float scale)
    {
        const gymrs_sampling x{seed, scale, 0};
        check(gymrs_set_sampling(e_, &x));
    }
    void clear_sampling() { check(gymrs_set_sampling(e_, nullptr)); }
    gymrs_sampling sampling() const
    {
        gymrs_sampling x{};
        check(gymrs_get_sampling(e_, &x));
        return x;
    }
    // the sampled action at the engine's current tick (prob_dev, may be null: the probability of the action taken): sample_actions +
    // step_device, K times, is rollout_closed_loop(K, .., sample = true)
    void sample_actions(void* actions_dev, float* prob_dev = nullptr) { check(gymrs_sample_actions(e_, actions_dev, prob_dev)); }
    void rollout_closed_loop(std::uint32_t n_steps, bool lane_params, bool fitness, const gymrs_trajectory* record, bool explore, bool sample)
    {
        const gymrs_closed_loop_desc d{n_steps,
                                       (lane_params ? GYMRS_CLOSED_LOOP_LANE_PARAMS : 0u) | (fitness ? GYMRS_CLOSED_LOOP_FITNESS : 0u) |
                                           (explore ? GYMRS_CLOSED_LOOP_EXPLORE : 0u) | (sample ? GYMRS_CLOSED_LOOP_SAMPLE : 0u),
                                       record, 0};
        check(gymrs_rollout_closed_loop(e_, &d));
    }
    // gymrs_rollout_transitions: the recording closed-loop launch that also writes, per step, the pre-re-arm observation of every ended
    // lane into final_obs ([n_steps][D][record.lane_stride], only those elements) and, unless NULL, the launch's start observations
    // into start_obs ([D][record.lane_stride]): successor of step k = ended ? final_obs[k] : obs[k].  Engines with GYMRS_AUTO_RESET only.
    void rollout_transitions(const gymrs_transitions_desc& d) { check(gymrs_rollout_transitions(e_, &d)); }
    void rollout_transitions(std::uint32_t n_steps, const gymrs_trajectory& record, float* final_obs, float* start_obs = nullptr,
                             bool lane_params = false, bool explore = false)
    {
        const gymrs_transitions_desc d{n_steps, (lane_params ? GYMRS_CLOSED_LOOP_LANE_PARAMS : 0u) | (explore ? GYMRS_CLOSED_LOOP_EXPLORE : 0u),
                                       record, final_obs, start_obs, 0};
        check(gymrs_rollout_transitions(e_, &d));
    }
    // ... with sample = true: the action drawn under set_sampling (GYMRS_CLOSED_LOOP_SAMPLE)
    void rollout_transitions(std::uint32_t n_steps, const gymrs_trajectory& record, float* final_obs, float* start_obs, bool lane_params,
                             bool explore, bool sample)
    {
        const gymrs_transitions_desc d{n_steps,
                                       (lane_params ? GYMRS_CLOSED_LOOP_LANE_PARAMS : 0u) | (explore ? GYMRS_CLOSED_LOOP_EXPLORE : 0u) |
                                           (sample ? GYMRS_CLOSED_LOOP_SAMPLE : 0u),
                                       record, final_obs, start_obs, 0};
        check(gymrs_rollout_transitions(e_, &d));
    }
    // advantages (gymrs_advantages): the critic set -- n_critics critics of critic_size(kind, hidden) floats back to back, lane i uses
    // critic ((global_env_offset + i) / lanes_per_critic) % n_critics -- and the GAE(lambda) scan over a transitions record in one
    // launch on the engine's stream; critic = true (GYMRS_ADVANTAGES_CRITIC) evaluates the critic inside the kernel, else V = 0
    static std::uint64_t critic_size(gymrs_env_kind kind, std::uint32_t hidden)
    {
        std::uint64_t n = 0;
        check(gymrs_critic_size(kind, hidden, &n));
        return n;
    }
    static float critic_value(gymrs_env_kind kind, std::uint32_t hidden, const float* weights, const float* obs)
    {
        float v = 0.0f;
        check(gymrs_critic_value(kind, hidden, weights, obs, &v));
        return v;
    }
    void set_critic(const float* weights_host, std::uint32_t hidden, std::uint32_t n_critics, std::uint64_t lanes_per_critic)
    {
        const gymrs_policy_desc d{hidden, n_critics, lanes_per_critic};
        check(gymrs_set_critic(e_, &d, weights_host));
    }
    void clear_critic() { check(gymrs_set_critic(e_, nullptr, nullptr)); }
    gymrs_policy_desc critic(float* weights_out = nullptr, std::uint64_t capacity_floats = 0)
    {
        gymrs_policy_desc d{};
        check(gymrs_get_critic(e_, &d, weights_out, capacity_floats));
        return d;
    }
    float* critic_weights_view(std::uint64_t* n_floats = nullptr)
    {
        float* p = nullptr;
        check(gymrs_critic_weights_ptr(e_, &p, n_floats));
        return p;
    }
    void advantages(const gymrs_advantages_desc& d) { check(gymrs_advantages(e_, &d)); }
    void advantages(std::uint32_t n_steps, const gymrs_trajectory& record, const float* final_obs, const float* start_obs, float* advantages_out,
                    float* returns_out, float* values_out, float gamma, float lambda, bool critic)
    {
        const gymrs_advantages_desc d{n_steps, critic ? GYMRS_ADVANTAGES_CRITIC : 0u, gamma, lambda, record, final_obs, start_obs, advantages_out,
                                      returns_out, values_out, 0};
        check(gymrs_advantages(e_, &d));
    }
    // gradients (gymrs_policy_gradient): ADDS the fixed-point score-function gradient of the policy set over a transitions record --
    // or, critic = true (GYMRS_GRADIENT_CRITIC), the value gradient of the critic set -- to grad (device int64 [n_sets][S]; the
    // gradient is grad * 2^-24) and the (lane, parameter) pairs left out to excluded (device uint64 [n_sets]), in one launch on the
    // engine's stream; scale = log2(e) / temperature (policy head only), prob may be null
    void policy_gradient(const gymrs_gradient_desc& d) { check(gymrs_policy_gradient(e_, &d)); }
    void policy_gradient(std::uint32_t n_steps, const gymrs_trajectory& record, const float* start_obs, const float* coef, std::int64_t* grad,
                         std::uint64_t* excluded, float* prob, float scale, bool critic)
    {
        const gymrs_gradient_desc d{n_steps, critic ? GYMRS_GRADIENT_CRITIC : 0u, scale, 0u, record, start_obs, coef, prob, grad, excluded, 0};
        check(gymrs_policy_gradient(e_, &d));
    }
    // the clipped surrogate (gymrs_ppo_gradient): policy_gradient's policy head with the coefficient computed in the kernel from the
    // advantages row and the old-probability row under the clip range [clip_low, clip_high] (the caller's floats); ADDS PPO's
    // gradient (to ascend) to grad and excluded and, when counts (device uint64 [n_sets][2]) is not null, the lane-steps seen and cut
    void ppo_gradient(const gymrs_ppo_desc& d) { check(gymrs_ppo_gradient(e_, &d)); }
    void ppo_gradient(std::uint32_t n_steps, const gymrs_trajectory& record, const float* start_obs, const float* advantages, const float* old_prob,
                      std::int64_t* grad, std::uint64_t* excluded, std::uint64_t* counts, float* prob, float scale, float clip_low, float clip_high)
    {
        const gymrs_ppo_desc d{n_steps, 0u, scale, clip_low, clip_high, 0u, record, start_obs, advantages, old_prob, prob, grad, excluded, counts, 0};
        check(gymrs_ppo_gradient(e_, &d));
    }
    std::vector<gymrs_policy_fitness> policy_fitness(std::uint32_t first, std::uint32_t count)
    {
        std::vector<gymrs_policy_fitness> out(count);
        check(gymrs_get_policy_fitness(e_, first, count, out.data()));
        return out;
    }
    gymrs_policy_fitness* policy_fitness_view(std::uint32_t* n_policies = nullptr)
    {
        gymrs_policy_fitness* p = nullptr;
        check(gymrs_policy_fitness_ptr(e_, &p, n_policies));
        return p;
    }
    void policy_fitness_clear() { check(gymrs_policy_fitness_clear(e_)); }
    // episodic policy evaluation: E whole episodes per lane in one launch; the records are those of the latest call
    void evaluate_policy(const gymrs_eval_desc& d) { check(gymrs_evaluate_policy(e_, &d)); }
    void evaluate_policy(std::uint32_t episodes_per_lane, std::uint32_t max_episode_steps = 0, std::uint64_t seed = 0, bool common_starts = false,
                         std::uint32_t* lengths_dev = nullptr)
    {
        const gymrs_eval_desc d{episodes_per_lane, max_episode_steps, seed, common_starts ? GYMRS_EVAL_COMMON_STARTS : 0u, 0u, lengths_dev};
        check(gymrs_evaluate_policy(e_, &d));
    }
    // lane_params (GYMRS_EVAL_LANE_PARAMS): every lane plays with the row of the parameter table step() would use for it; without a
    // table it changes nothing.  Without it an engine with a table refuses the call.
    void evaluate_policy(std::uint32_t episodes_per_lane, std::uint32_t max_episode_steps, std::uint64_t seed, bool common_starts,
                         std::uint32_t* lengths_dev, bool lane_params)
    {
        const gymrs_eval_desc d{episodes_per_lane, max_episode_steps, seed,
                                (common_starts ? GYMRS_EVAL_COMMON_STARTS : 0u) | (lane_params ? GYMRS_EVAL_LANE_PARAMS : 0u), 0u, lengths_dev};
        check(gymrs_evaluate_policy(e_, &d));
    }
    std::vector<gymrs_policy_eval> policy_eval(std::uint32_t first, std::uint32_t count)
    {
        std::vector<gymrs_policy_eval> out(count);
        check(gymrs_get_policy_eval(e_, first, count, out.data()));
        return out;
    }
    gymrs_policy_eval* policy_eval_view(std::uint32_t* n_policies = nullptr)
    {
        gymrs_policy_eval* p = nullptr;
        check(gymrs_policy_eval_ptr(e_, &p, n_policies));
        return p;
    }
    // `#[derive(Serialize)]` view of the reference env lane `lane` stands for (core.rs:25)
    std::string to_json(std::uint64_t lane = 0)
    {
        std::uint64_t need = 0;
        std::string buf(2048, '\0');
        gymrs_status st = gymrs_env_json(e_, lane, buf.data(), buf.size(), &need);
        if (st != GYMRS_OK && need > buf.size()) {
            buf.assign(need, '\0');
            st = gymrs_env_json(e_, lane, buf.data(), buf.size(), &need);
        }
        check(st);
        buf.resize(need ? need - 1 : 0);
        return buf;
    }
    gymrs_engine* handle() { return e_; }
    std::uint64_t size() const { return n_; }
    int state_dim() const { return state_dim_; }

private:
    gymrs_env_kind kind_;
    std::uint64_t n_;
    gymrs_engine* e_ = nullptr;
    int state_dim_ = 0;
};

// ---- one batch over several GPUs, in one process (gymrs_sharded_*: one engine + one native host thread per block) ---------
// contiguous blocks of lanes, global lane ids, no exchange except the four statistics doubles (RCCL over xGMI on
// distinct devices, a host-side sum where blocks share a device).  Every result is bit-identical to ONE VecEnv of n_total lanes.
class ShardedVecEnv {
public:
    ShardedVecEnv(gymrs_env_kind kind, std::uint64_t n_total, const std::vector<int>& devices, std::uint32_t flags = 0, const void* params = nullptr,
                  std::uint64_t global_env_offset = 0)
        : n_(n_total), state_dim_(kind == GYMRS_CARTPOLE ? 4 : 2)
    {
        check(gymrs_sharded_create(kind, n_total, global_env_offset, (int)devices.size(), devices.data(), params, flags, &h_));
        int k = 0;
        check(gymrs_sharded_count(h_, &k));
        n_blocks_ = (std::size_t)k;
    }
    ~ShardedVecEnv() { gymrs_sharded_destroy(h_); }
    ShardedVecEnv(const ShardedVecEnv&) = delete;
    ShardedVecEnv& operator=(const ShardedVecEnv&) = delete;

    struct Block {
        gymrs_engine* engine; // for the zero-copy views (gymrs_obs_ptrs, gymrs_reward_ptr, ...); not to be stepped directly
        std::uint64_t first_lane, n_lanes;
        int device;
    };
    int n_blocks()
    {
        int k = 0;
        check(gymrs_sharded_count(h_, &k));
        return k;
    }
    Block block(int r)
    {
        Block b{};
        check(gymrs_sharded_shard(h_, r, &b.engine, &b.first_lane, &b.n_lanes, &b.device));
        return b;
    }
    std::uint64_t reset(std::optional<std::uint64_t> seed, const float* bounds_low_high = nullptr)
    {
        std::uint64_t used = 0;
        check(gymrs_sharded_reset(h_, seed.has_value(), seed.value_or(0), bounds_low_high, &used));
        return used;
    }
    // actions_dev[r]: block r's actions (ring) on ITS device
    // (the native side reads actions_dev[r] for EVERY block: a shorter vector would be an out-of-bounds read that ends as a wild device pointer)
    void step_device(const std::vector<const void*>& actions_dev) // async
    {
        one_pointer_per_block(actions_dev.size(), "step_device");
        check(gymrs_sharded_step(h_, actions_dev.data()));
    }
    void step_many(const std::vector<const void*>& actions_dev, std::uint64_t stride_bytes, std::uint32_t n_buffers, std::uint32_t n_steps)
    {
        one_pointer_per_block(actions_dev.size(), "step_many");
        check(gymrs_sharded_step_many(h_, actions_dev.data(), stride_bytes, n_buffers, n_steps, 0));
    }
    void fill_actions(const std::vector<void*>& actions_dev, std::uint64_t seed, std::uint64_t t)
    {
        one_pointer_per_block(actions_dev.size(), "fill_actions");
        check(gymrs_sharded_fill_actions(h_, actions_dev.data(), seed, t));
    }
    void rollout(std::uint32_t n_steps, std::uint64_t action_seed, std::uint64_t action_t0 = 0) { check(gymrs_sharded_rollout(h_, n_steps, action_seed, action_t0)); }
    // closed-loop rollouts and per-policy fitness on every block (the same policy set everywhere, keyed by global lane ids)
    void set_policy(const float* weights_host, std::uint32_t hidden, std::uint32_t n_policies, std::uint64_t lanes_per_policy)
    {
        const gymrs_policy_desc d{hidden, n_policies, lanes_per_policy};
        check(gymrs_sharded_set_policy(h_, &d, weights_host));
    }
    void clear_policy() { check(gymrs_sharded_set_policy(h_, nullptr, nullptr)); }
    void rollout_policy(std::uint32_t n_steps) { check(gymrs_sharded_rollout_policy(h_, n_steps)); }
    void rollout_policy_fitness(std::uint32_t n_steps) { check(gymrs_sharded_rollout_policy_fitness(h_, n_steps)); }
    // VecEnv::rollout_closed_loop on every block (record must stay NULL: the blocks live on several devices)
    void rollout_closed_loop(const gymrs_closed_loop_desc& d) { check(gymrs_sharded_rollout_closed_loop(h_, &d)); }
    void rollout_closed_loop(std::uint32_t n_steps, bool lane_params = false, bool fitness = false)
    {
        const gymrs_closed_loop_desc d{n_steps, (lane_params ? GYMRS_CLOSED_LOOP_LANE_PARAMS : 0u) | (fitness ? GYMRS_CLOSED_LOOP_FITNESS : 0u), nullptr, 0};
        check(gymrs_sharded_rollout_closed_loop(h_, &d));
    }
    // VecEnv::set_exploration on every block: the same settings everywhere (the draw is keyed by global lane ids)
    void set_exploration(std::uint64_t seed, std::uint32_t threshold)
    {
        const gymrs_exploration x{seed, threshold, 0};
        check(gymrs_sharded_set_exploration(h_, &x));
    }
    void clear_exploration() { check(gymrs_sharded_set_exploration(h_, nullptr)); }
    // VecEnv::set_sampling on every block
    void set_sampling(std::uint64_t seed, float scale)
    {
        const gymrs_sampling x{seed, scale, 0};
        check(gymrs_sharded_set_sampling(h_, &x));
    }
    void clear_sampling() { check(gymrs_sharded_set_sampling(h_, nullptr)); }
    void rollout_closed_loop(std::uint32_t n_steps, bool lane_params, bool fitness, bool explore, bool sample)
    {
        const gymrs_closed_loop_desc d{n_steps,
                                       (lane_params ? GYMRS_CLOSED_LOOP_LANE_PARAMS : 0u) | (fitness ? GYMRS_CLOSED_LOOP_FITNESS : 0u) |
                                           (explore ? GYMRS_CLOSED_LOOP_EXPLORE : 0u) | (sample ? GYMRS_CLOSED_LOOP_SAMPLE : 0u),
                                       nullptr, 0};
        check(gymrs_sharded_rollout_closed_loop(h_, &d));
    }
    void rollout_closed_loop(std::uint32_t n_steps, bool lane_params, bool fitness, bool explore)
    {
        const gymrs_closed_loop_desc d{n_steps,
                                       (lane_params ? GYMRS_CLOSED_LOOP_LANE_PARAMS : 0u) | (fitness ? GYMRS_CLOSED_LOOP_FITNESS : 0u) |
                                           (explore ? GYMRS_CLOSED_LOOP_EXPLORE : 0u),
                                       nullptr, 0};
        check(gymrs_sharded_rollout_closed_loop(h_, &d));
    }
    std::vector<gymrs_policy_fitness> policy_fitness(std::uint32_t first, std::uint32_t count) // the blocks' records, summed
    {
        std::vector<gymrs_policy_fitness> out(count);
        check(gymrs_sharded_get_policy_fitness(h_, first, count, out.data()));
        return out;
    }
    void policy_fitness_clear() { check(gymrs_sharded_policy_fitness_clear(h_)); }
    // episodic policy evaluation on every block (d.lengths_dev must be NULL); the blocks' records merged
    void evaluate_policy(const gymrs_eval_desc& d) { check(gymrs_sharded_evaluate_policy(h_, &d)); }
    std::vector<gymrs_policy_eval> policy_eval(std::uint32_t first, std::uint32_t count)
    {
        std::vector<gymrs_policy_eval> out(count);
        check(gymrs_sharded_get_policy_eval(h_, first, count, out.data()));
        return out;
    }
    void set_params(const void* params) { check(gymrs_sharded_set_params(h_, params)); }
    // per-lane physics on the batch: the same rows on every block (set_param_table(nullptr, 0) switches it off), the index in BATCH
    // lane numbering; evaluate_policy with GYMRS_EVAL_LANE_PARAMS in d.flags plays it
    void set_param_table(const void* rows, std::uint32_t k) { check(gymrs_sharded_set_param_table(h_, rows, k)); }
    std::uint32_t param_table(void* rows_out, std::uint32_t capacity) // K; rows_out (capacity >= K, or nullptr with 0) from block 0
    {
        std::uint32_t k = 0;
        check(gymrs_sharded_get_param_table(h_, rows_out, capacity, &k));
        return k;
    }
    void set_param_index(std::uint64_t first, std::uint64_t count, const std::uint16_t* index) { check(gymrs_sharded_set_param_index(h_, first, count, index)); }
    std::vector<std::uint16_t> param_index(std::uint64_t first, std::uint64_t count)
    {
        std::vector<std::uint16_t> out(count);
        check(gymrs_sharded_get_param_index(h_, first, count, out.data()));
        return out;
    }
    void sync() { check(gymrs_sharded_sync(h_)); }
    std::array<double, 4> stats() // {sum_return, sum_length, n_episodes, n_steps} of the whole batch
    {
        std::array<double, 4> out{};
        check(gymrs_sharded_stats(h_, out.data()));
        return out;
    }
    void stats_clear() { check(gymrs_sharded_stats_clear(h_)); }
    std::string reduce_path() { return gymrs_sharded_reduce_path(h_); } // "rccl" | "host" | "none"
    std::vector<float> state(std::uint64_t first, std::uint64_t count)
    {
        std::vector<float> out(count * state_dim_);
        check(gymrs_sharded_get_state(h_, first, count, out.data()));
        return out;
    }
    void result(std::uint64_t first, std::uint64_t count, float* reward, std::uint8_t* done, std::uint8_t* truncated)
    {
        check(gymrs_sharded_get_step_result(h_, first, count, reward, done, truncated));
    }
    std::uint64_t size() const { return n_; }

private:
    void one_pointer_per_block(std::size_t given, const char* who) const
    {
        if (given != n_blocks_)
            throw std::invalid_argument(std::string("ShardedVecEnv::") + who + ": " + std::to_string(given) + " action pointers for " + std::to_string(n_blocks_) + " blocks");
    }
    std::uint64_t n_;
    int state_dim_;
    std::size_t n_blocks_ = 0;
    gymrs_sharded* h_ = nullptr;
};

// ---- single envs with the reference's surface ------------------------------------------------------
class CartPoleEnv {
public:
    using Action = std::size_t;
    using Observation = CartPoleObservation;
    explicit CartPoleEnv(RenderMode mode = RenderMode::None) : env_(make(mode)) {}
    ResetRng reset_rng = ResetRng::Philox;

    ActionReward<Observation, Unit> step(Action action) // Env::step, cartpole.rs:398-483
    {
        if (!action_space().contains(action)) throw Panic(GYMRS_EACTION, std::to_string(action) + " usize invalid"); // :402-406
        const std::uint8_t a = static_cast<std::uint8_t>(action);
        env_.step_host(&a);
        float r;
        std::uint8_t d;
        env_.result(0, 1, &r, &d, nullptr);
        return {state(), r, d != 0, false, Unit{}}; // truncated: false, info: Some(()) (:480-481)
    }
    std::pair<Observation, std::optional<Unit>> reset(std::optional<std::uint64_t> seed, bool return_info,
                                                       std::optional<BoxR<Observation>> options) // :485-516
    {
        float b[8];
        double b64[8];
        if (options) {
            const auto lo = options->low.to_vec(), hi = options->high.to_vec();
            for (int j = 0; j < 4; ++j) {
                b[j] = static_cast<float>(b64[j] = lo[j]);
                b[4 + j] = static_cast<float>(b64[4 + j] = hi[j]);
            }
        }
        if (reset_rng == ResetRng::Pcg64)
            env_.reset_pcg64(seed, options ? b64 : nullptr);
        else
            env_.reset(seed, options ? b : nullptr);
        return {state(), return_info ? std::optional<Unit>(Unit{}) : std::nullopt};
    }
    void render(RenderMode) {} // renderer.rs:52-62: nothing is drawn under RenderMode::None
    void close() {}
    Observation state()
    {
        const auto s = env_.state(0, 1);
        return {s[0], s[1], s[2], s[3]};
    }
    void set_state(const Observation& o)
    {
        const float s[4] = {(float)o.x, (float)o.x_dot, (float)o.theta, (float)o.theta_dot};
        env_.set_state(0, 1, s);
    }
    // The reference's constants are pub fields (cartpole.rs:53-82): read them all, edit, assign them back.  Like the
    // assignment in Rust this changes nothing but the constants (state, steps_beyond_terminated, seed/tick carry on).
    gymrs_cartpole_params params()
    {
        gymrs_cartpole_params p;
        env_.get_params(&p);
        return p;
    }
    void set_params(const gymrs_cartpole_params& p) { env_.set_params(&p); }
    std::string to_json() { return env_.to_json(0); } // serde_json::to_string(&env)
    Discrete action_space() const { return Discrete{2}; } // cartpole.rs:114
    BoxR<Observation> observation_space()               // cartpole.rs:105-115
    {
        const double inf = std::numeric_limits<double>::infinity();
        const gymrs_cartpole_params p = params();
        const Observation high{p.x_threshold * 2., inf, p.theta_threshold_radians * 2., inf};
        return {-high, high};
    }
    RewardRange reward_range() const { return {}; }
    RenderMode render_mode() const { return RenderMode::None; }

private:
    static VecEnv make(RenderMode mode)
    {
        if (mode != RenderMode::None) throw Panic(GYMRS_EINVAL, "rendering is out of scope: use RenderMode::None");
        return VecEnv(GYMRS_CARTPOLE, 1);
    }
    VecEnv env_;
};

class MountainCarEnv {
public:
    using Action = std::size_t;
    using Observation = MountainCarObservation;
    explicit MountainCarEnv(RenderMode mode = RenderMode::None) : env_(make(mode)) {}
    ResetRng reset_rng = ResetRng::Philox;

    ActionReward<Observation, Unit> step(Action action) // mountain_car.rs:398-435
    {
        if (!action_space().contains(action)) throw Panic(GYMRS_EACTION, std::to_string(action) + " (usize) invalid");
        const std::uint8_t a = static_cast<std::uint8_t>(action);
        env_.step_host(&a);
        float r;
        std::uint8_t d;
        env_.result(0, 1, &r, &d, nullptr);
        return {state(), r, d != 0, false, std::nullopt}; // info: None (:433)
    }
    std::pair<Observation, std::optional<Unit>> reset(std::optional<std::uint64_t> seed, bool return_info,
                                                       std::optional<BoxR<Observation>> options) // :464-501
    {
        float b[4];
        double b64[4];
        if (options) {
            b[0] = (float)(b64[0] = options->low.position);
            b[1] = (float)(b64[1] = options->low.velocity);
            b[2] = (float)(b64[2] = options->high.position);
            b[3] = (float)(b64[3] = options->high.velocity);
        }
        if (reset_rng == ResetRng::Pcg64)
            env_.reset_pcg64(seed, options ? b64 : nullptr);
        else
            env_.reset(seed, options ? b : nullptr);
        return {state(), return_info ? std::optional<Unit>(Unit{}) : std::nullopt};
    }
    void render(RenderMode) {}
    void close() {}
    Observation state()
    {
        const auto s = env_.state(0, 1);
        return {s[0], s[1]};
    }
    void set_state(const Observation& o)
    {
        const float s[2] = {(float)o.position, (float)o.velocity};
        env_.set_state(0, 1, s);
    }
    gymrs_mountain_car_params params()
    {
        gymrs_mountain_car_params p;
        env_.get_params(&p);
        return p;
    }
    void set_params(const gymrs_mountain_car_params& p) { env_.set_params(&p); }
    std::string to_json() { return env_.to_json(0); }
    Discrete action_space() const { return Discrete{3}; }                                    // mountain_car.rs:362
    BoxR<Observation> observation_space() const { return {{-1.2, -0.07}, {0.6, 0.07}}; }      // :353-364

private:
    static VecEnv make(RenderMode mode)
    {
        if (mode != RenderMode::None) throw Panic(GYMRS_EINVAL, "rendering is out of scope: use RenderMode::None");
        return VecEnv(GYMRS_MOUNTAIN_CAR, 1);
    }
    VecEnv env_;
};

} // namespace gymrs
