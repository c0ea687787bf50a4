// gymrs_engine_learn.hip -- the learner surface of the C ABI (include/gymrs_amd.h): the policy and critic sets, the exploration and sampling
// settings with their per-step calls and host draws, advantages, gradients and the clipped surrogate over a transitions record with their
// host-only lanes, the per-policy fitness and evaluation tables.  Host code only: the kernels are behind gymrs_kernels.h.  The engine
// object and the refusals shared with the stepping paths: gymrs_engine_priv.h.
#include "gymrs_engine_priv.h"
#include "gymrs_evaluate.h"
#include "gymrs_sample.h"
#include "gymrs_advantages.h"
#include "gymrs_gradient.h"

namespace {
// ---- the checks more than one entry point words the same way --------------------------------------------------------------------
// Which envs take a small network, and how wide one may be.
gymrs_status check_network(gymrs_env_kind kind, uint32_t hidden, const std::string& who)
{
    if (gymrs_status st = check_discrete_env(kind, who)) return st;
    if (hidden > kMaxPolicyHidden) return fail(GYMRS_EINVAL, who + ": hidden must be <= 64");
    return GYMRS_OK;
}

bool finite_non_negative(float x) { return x >= 0.0f && x <= std::numeric_limits<float>::max(); } // (false for a NaN)

// 0 <= low <= 1 <= high, finite (false for a NaN)
bool ppo_bounds_ok(float low, float high) { return low >= 0.0f && low <= 1.0f && high >= 1.0f && high <= std::numeric_limits<float>::max(); }

// ---- a weight set: the policies of gymrs_set_policy, the critics of gymrs_set_critic -----------------------------------------------
// What differs between the two: where the engine keeps the set, the floats of one network and the words of the refusals.
struct WeightKind {
    WeightSet gymrs_engine::*set;
    uint64_t (*floats)(gymrs_env_kind, uint32_t hidden);
    const char* noun;     // also how the setter ends: gymrs_set_<noun>
    const char* networks; // what the refusals call gymrs_policy_desc::n_policies ...
    const char* lanes;    // ... and ::lanes_per_policy
};
const WeightKind kPolicyKind{&gymrs_engine::policy, policy_floats, "policy", "n_policies", "lanes_per_policy"};
const WeightKind kCriticKind{&gymrs_engine::critic, critic_floats, "critic", "n_policies (the number of critics)", "lanes_per_policy (lanes per critic)"};

// The buffer goes (launches already enqueued still read it: wait for them).
gymrs_status remove_weights(gymrs_engine* e, const WeightKind& k)
{
    WeightSet& set = e->*k.set;
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipFree(set.dev));
    set = WeightSet{};
    return GYMRS_OK;
}

// What a setter refuses before it touches anything.
gymrs_status check_weights(const gymrs_engine* e, const WeightKind& k, const gymrs_policy_desc* d, const float* weights_host, const std::string& who)
{
    if (gymrs_status st = check_network(e->kind, d->hidden, who)) return st;
    if (d->n_policies == 0) return fail(GYMRS_EINVAL, who + ": " + k.networks + " must be >= 1");
    if (d->lanes_per_policy == 0) return fail(GYMRS_EINVAL, who + ": " + k.lanes + " must be >= 1");
    if (!weights_host) return fail(GYMRS_EINVAL, who + ": weights_host is NULL");
    return GYMRS_OK;
}

// A checked set takes the place of the old one (the engine's device is current).
gymrs_status install_weights(gymrs_engine* e, const WeightKind& k, const gymrs_policy_desc* d, const float* weights_host)
{
    WeightSet& set = e->*k.set;
    const uint64_t stride = k.floats(e->kind, d->hidden), total = stride * d->n_policies;
    if (total > set.capacity) { // a larger set: a new buffer (launches in flight still read the old one: wait for them)
        if (gymrs_status st = remove_weights(e, k)) return st;
        HIP_TRY(hipMalloc(&set.dev, (size_t)total * sizeof(float)));
        set.capacity = total;
    }
    // stream-ordered: launches enqueued before this call read the old set; the host weights are consumed before the call returns
    HIP_TRY(hipMemcpyAsync(set.dev, weights_host, (size_t)total * sizeof(float), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    set.args = PolicyArgs{set.dev, d->lanes_per_policy, d->n_policies, d->hidden, (uint32_t)stride, 0};
    return GYMRS_OK;
}

// The description, or with room for them the description and the weights (synchronising).
gymrs_status read_weights(gymrs_engine* e, const WeightKind& k, gymrs_policy_desc* d_out, float* weights_out, uint64_t capacity_floats, const std::string& who)
{
    if (!e || !d_out) return fail(GYMRS_EINVAL, who + ": NULL argument");
    const WeightSet& set = e->*k.set;
    if (gymrs_status st = check_weight_set(set, k.noun, who)) return st;
    d_out->hidden = set.args.hidden;
    d_out->n_policies = set.args.n_policies;
    d_out->lanes_per_policy = set.args.lanes_per_policy;
    if (!weights_out && capacity_floats == 0) return GYMRS_OK; // a query of the description
    const uint64_t total = (uint64_t)set.args.stride * set.args.n_policies;
    if (!weights_out || capacity_floats < total) return fail(GYMRS_EINVAL, who + ": capacity_floats is smaller than the " + k.noun + " set");
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipMemcpyAsync(weights_out, set.dev, (size_t)total * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    return stream_sync_checked(e);
}

gymrs_status weights_view(const gymrs_engine* e, const WeightKind& k, float** dev_out, uint64_t* n_floats, const std::string& who)
{
    if (!e || !dev_out) return fail(GYMRS_EINVAL, who + ": NULL argument");
    const WeightSet& set = e->*k.set;
    if (gymrs_status st = check_weight_set(set, k.noun, who)) return st;
    *dev_out = set.dev;
    if (n_floats) *n_floats = (uint64_t)set.args.stride * set.args.n_policies;
    return GYMRS_OK;
}

// ---- a per-policy table: policy.args.n_policies records on the device that appear at first use and go with the policy set -------------
// (the fitness counters, the episodic records).  `slot` is the engine's pointer to it, `init` fills a new table in stream order.
template <class Record>
struct PolicyTable {
    Record* gymrs_engine::*slot;
    hipError_t (*init)(Record* table, uint32_t n_policies, hipStream_t stream);

    // The table goes (launches already enqueued still add to it: wait for them).
    gymrs_status discard(gymrs_engine* e) const
    {
        if (!(e->*slot)) return GYMRS_OK;
        HIP_TRY(hipSetDevice(e->device));
        HIP_TRY(hipStreamSynchronize(e->stream));
        HIP_TRY(hipFree(e->*slot));
        e->*slot = nullptr;
        return GYMRS_OK;
    }

    // The table, made at the first use after a gymrs_set_policy (the caller has checked that there is a policy set).
    gymrs_status table(gymrs_engine* e) const
    {
        if (e->*slot) return GYMRS_OK;
        HIP_TRY(hipSetDevice(e->device));
        HIP_TRY(hipMalloc(&(e->*slot), (size_t)e->policy.args.n_policies * sizeof(Record)));
        if (hipError_t err = init(e->*slot, e->policy.args.n_policies, e->stream)) {
            (void)hipFree(e->*slot);
            e->*slot = nullptr;
            HIP_TRY(err);
        }
        return GYMRS_OK;
    }

    // The checks the calls over the table share, then the table.
    gymrs_status ensure(gymrs_engine* e, const std::string& who) const
    {
        if (gymrs_status st = check_discrete_env(e->kind, who)) return st;
        if (gymrs_status st = check_policy_set(e, who)) return st;
        return table(e);
    }

    gymrs_status view(gymrs_engine* e, Record** dev_out, uint32_t* n_policies, const std::string& who) const
    {
        if (!e || !dev_out) return fail(GYMRS_EINVAL, who + ": NULL argument");
        if (gymrs_status st = ensure(e, who)) return st;
        *dev_out = e->*slot;
        if (n_policies) *n_policies = e->policy.args.n_policies;
        return GYMRS_OK;
    }

    // Records [first, first + count) to the host (synchronising).
    gymrs_status read(gymrs_engine* e, uint32_t first, uint32_t count, Record* host_out, const std::string& who) const
    {
        if (!e || !host_out) return fail(GYMRS_EINVAL, who + ": NULL argument");
        if (gymrs_status st = ensure(e, who)) return st;
        if ((uint64_t)first + count > e->policy.args.n_policies) return fail(GYMRS_EINVAL, who + ": first + count is beyond n_policies");
        if (count == 0) return stream_sync_checked(e);
        HIP_TRY(hipMemcpyAsync(host_out, e->*slot + first, (size_t)count * sizeof(Record), hipMemcpyDeviceToHost, e->stream));
        return stream_sync_checked(e);
    }
};

hipError_t zero_fitness(gymrs_policy_fitness* table, uint32_t n_policies, hipStream_t stream)
{
    return hipMemsetAsync(table, 0, (size_t)n_policies * sizeof(gymrs_policy_fitness), stream);
}
const PolicyTable<gymrs_policy_fitness> kFitness{&gymrs_engine::fitness_dev, zero_fitness};
const PolicyTable<gymrs_policy_eval> kEval{&gymrs_engine::eval_dev, launch_policy_eval_identity};

// ---- a call over a transitions record: the checks gymrs_advantages, gymrs_policy_gradient and gymrs_ppo_gradient share, worded once ----
// Each entry point lists its checks in its own order (the tests and callers depend on which refusal wins).
struct RecordCall {
    const gymrs_engine* e;
    const void* d;
    std::string who;

    struct Field {
        const void* p;
        const char* name;
        const char* why = ""; // what the message adds behind "<name> is NULL"
    };

    gymrs_status refuse(const std::string& what) const { return fail(GYMRS_EINVAL, who + ": " + what); }

    // NULL engine, NULL descriptor, Discrete envs only.  `subject`: how the call names what it computes ("gradients are").
    gymrs_status prologue(const char* subject) const
    {
        if (!e) return refuse("NULL engine");
        if (!d) return refuse("NULL desc");
        if (e->kind != GYMRS_CARTPOLE && e->kind != GYMRS_MOUNTAIN_CAR)
            return refuse(std::string(subject) + " for the Discrete envs (CartPole, MountainCar); Pendulum takes no policy and records no transitions");
        return GYMRS_OK;
    }

    gymrs_status scale(float s) const { return finite_non_negative(s) ? GYMRS_OK : refuse("scale must be finite and >= 0"); }

    // The first of `fields` that is NULL is refused by name.
    gymrs_status not_null(std::initializer_list<Field> fields) const
    {
        for (const Field& f : fields)
            if (!f.p) return refuse(std::string(f.name) + " is NULL" + f.why);
        return GYMRS_OK;
    }

    // Every one of `ptrs` (a NULL is aligned) is a multiple of `bytes`, or `message`.
    gymrs_status aligned(std::initializer_list<const void*> ptrs, uintptr_t bytes, const char* message) const
    {
        uintptr_t bits = 0;
        for (const void* p : ptrs) bits |= reinterpret_cast<uintptr_t>(p);
        return bits % bytes == 0 ? GYMRS_OK : refuse(message);
    }

    gymrs_status lane_stride(uint64_t stride) const
    {
        return stride >= e->n && stride % 16 == 0 ? GYMRS_OK : refuse("lane_stride must be >= n_envs and a multiple of 16");
    }
};

// The descriptor of a gradient launch as its kernel gets it.  `actions`: NULL for the critic head; `coef`: the advantages row for the clipped surrogate.
GradientArgs gradient_args(const gymrs_engine* e, const gymrs_trajectory& rec, const void* actions, uint32_t n_steps, float scale, const float* start_obs,
                           const float* coef, float* prob, int64_t* grad, uint64_t* excluded)
{
    return GradientArgs{rec.obs, static_cast<const uint8_t*>(actions), start_obs, coef, prob, reinterpret_cast<unsigned long long*>(grad),
                        reinterpret_cast<unsigned long long*>(excluded), /*stride, n, gid0*/ rec.lane_stride, e->n, e->gid0, n_steps, scale};
}

// ---- the host-only lanes (gymrs_critic_value, gymrs_gradient_lane, gymrs_ppo_lane): the kernels' shared text over host memory -------------
struct HostWeights { // w(k, i) of critic_values and the gymrs_gradient.h templates over one network in host memory
    const float* w;
    float operator()(int, uint32_t i) const { return w[i]; }
};

// What "clipped surrogate" adds to a lane: coef is then the advantages row
struct PpoLane {
    const float* old_prob;
    float clip_low, clip_high;
    uint64_t* counts; // [2], SET
};

// One lane by the shared text: the kernels' walk with VEC = 1, chunk after chunk.
template <int D, int A, bool CRITIC>
void gradient_lane(uint32_t H, float scale, const float* weights, uint32_t K, const float* x, const uint8_t* actions, const float* coef, int64_t* q,
                   uint64_t* excluded, float* prob, const PpoLane* ppo = nullptr)
{
    uint64_t seen = 0, ncut = 0;
    const HostWeights w{weights};
    uint64_t excl = 0;
    auto emit = [&](uint32_t s, const float (&L)[1]) {
        long long v;
        if (!gradient_fixed(L[0], v)) excl += 1;
        q[s] = v;
    };
    const uint32_t chunks = H == 0 ? 1 : (H + kGradientChunk - 1) / kGradientChunk;
    for (uint32_t chunk = 0; chunk < chunks; ++chunk) {
        const uint32_t h0 = chunk * kGradientChunk;
        GradientAffine<D, A, 1> aff{};
        GradientChunk<D, A, 1> chk{};
        float db2[A][1] = {};
        for (uint32_t k = 0; k < K; ++k) {
            float xs[D][1], g[A][1];
            bool on[1] = {true};
            for (int j = 0; j < D; ++j) xs[j][0] = x[(size_t)k * D + j];
            if constexpr (CRITIC) {
                g[0][0] = coef[k];
            } else {
                float y[A][1], pa[1];
                const float c[1] = {coef[k]};
                const uint8_t act[1] = {actions[k]};
                gradient_logits<D, A, 1, 1>(w, H, xs, y);
                if (ppo) {
                    const float po[1] = {ppo->old_prob[k]};
                    bool cut[1];
                    gradient_ppo_head<A, 1>(y, act, c, po, scale, ppo->clip_low, ppo->clip_high, g, on, pa, cut);
                    if (chunk == 0) {
                        seen += on[0] ? 1 : 0;
                        ncut += cut[0] ? 1 : 0;
                    }
                } else {
                    gradient_policy_head<A, 1>(y, act, c, scale, g, on, pa);
                }
                if (prob && chunk == 0) prob[k] = pa[0];
            }
            if (H == 0) {
                gradient_affine_step<D, A, 1, !CRITIC>(xs, g, on, aff);
            } else {
                gradient_chunk_step<D, A, 1, !CRITIC>(w, H, h0, xs, g, on, chk);
                if (chunk == 0) gradient_bias_step<A, 1, !CRITIC>(g, on, db2);
            }
        }
        if (H == 0) {
            gradient_affine_each<D, A, 1>(aff, emit);
        } else {
            gradient_chunk_each<D, A, 1>(H, h0, chk, emit);
            if (chunk == 0) gradient_bias_each<D, A, 1>(H, db2, emit);
        }
    }
    *excluded = excl;
    if (ppo && ppo->counts) {
        ppo->counts[0] = seen;
        ppo->counts[1] = ncut;
    }
}
} // namespace

GYMRS_HOST_INTERNAL gymrs_status policy_fitness_table(gymrs_engine* e) { return kFitness.table(e); }

extern "C" {

// ---- closed-loop rollouts: the policy set --------------------------------------------------------------------------------
gymrs_status gymrs_policy_size(gymrs_env_kind kind, uint32_t hidden, uint64_t* n_floats)
{
    if (!n_floats) return fail(GYMRS_EINVAL, "gymrs_policy_size: n_floats is NULL");
    if (gymrs_status st = check_network(kind, hidden, "gymrs_policy_size")) return st;
    *n_floats = policy_floats(kind, hidden);
    return GYMRS_OK;
}

gymrs_status gymrs_set_policy(gymrs_engine* e, const gymrs_policy_desc* d, const float* weights_host)
{
    if (!e) return fail(GYMRS_EINVAL, "gymrs_set_policy: NULL engine");
    if (!d) { // remove the policy, and the tables with it
        if (gymrs_status st = remove_weights(e, kPolicyKind)) return st;
        if (gymrs_status st = kEval.discard(e)) return st;
        return kFitness.discard(e);
    }
    if (gymrs_status st = check_weights(e, kPolicyKind, d, weights_host, "gymrs_set_policy")) return st;
    HIP_TRY(hipSetDevice(e->device));
    // a new set starts from zero counters: a table of another size goes (allocated again at its first use), one of the same
    // size -- a search's next generation -- is kept and zeroed in stream order, after the launches that still add to it
    if (e->fitness_dev && d->n_policies == e->policy.args.n_policies) {
        HIP_TRY(zero_fitness(e->fitness_dev, d->n_policies, e->stream));
    } else if (gymrs_status st = kFitness.discard(e)) {
        return st;
    }
    if (gymrs_status st = kEval.discard(e)) return st; // the episodic records belong to the set they were played with
    return install_weights(e, kPolicyKind, d, weights_host);
}

gymrs_status gymrs_get_policy(gymrs_engine* e, gymrs_policy_desc* d_out, float* weights_out, uint64_t capacity_floats)
{
    return read_weights(e, kPolicyKind, d_out, weights_out, capacity_floats, "gymrs_get_policy");
}

gymrs_status gymrs_policy_weights_ptr(gymrs_engine* e, float** dev_out, uint64_t* n_floats)
{
    return weights_view(e, kPolicyKind, dev_out, n_floats, "gymrs_policy_weights_ptr");
}

gymrs_status gymrs_policy_actions(gymrs_engine* e, void* actions_dev)
{
    if (!e || !actions_dev) return fail(GYMRS_EINVAL, "gymrs_policy_actions: NULL argument");
    if (gymrs_status st = check_policy_set(e, "gymrs_policy_actions")) return st;
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(launch_policy_actions(e->kind, e->s, actions_dev, e->n, e->gid0, e->policy.args, e->stream));
    return GYMRS_OK;
}

// ---- epsilon-greedy exploration: the settings, the per-step call and the host-side draw ------------------------------------------
static gymrs_status check_exploration(const gymrs_exploration* x, const std::string& who)
{
    if (x->threshold > kExploreOne) return fail(GYMRS_EINVAL, who + ": threshold must be <= 65536 (epsilon = threshold / 65536)");
    if (x->reserved != 0) return fail(GYMRS_EINVAL, who + ": reserved must be 0");
    return GYMRS_OK;
}

gymrs_status gymrs_set_exploration(gymrs_engine* e, const gymrs_exploration* x)
{
    if (!e) return fail(GYMRS_EINVAL, "gymrs_set_exploration: NULL engine");
    if (e->kind != GYMRS_CARTPOLE && e->kind != GYMRS_MOUNTAIN_CAR)
        return fail(GYMRS_EINVAL, "gymrs_set_exploration: exploration is for the Discrete envs (CartPole, MountainCar); Pendulum takes a Box action");
    if (!x) { // (launches already enqueued carry their own copy of the settings)
        e->explore = ExploreArgs{};
        e->explore_set = false;
        return GYMRS_OK;
    }
    if (gymrs_status st = check_exploration(x, "gymrs_set_exploration")) return st;
    e->explore = ExploreArgs{x->seed, x->threshold, 0};
    e->explore_set = true;
    return GYMRS_OK;
}

gymrs_status gymrs_get_exploration(gymrs_engine* e, gymrs_exploration* x_out)
{
    if (!e || !x_out) return fail(GYMRS_EINVAL, "gymrs_get_exploration: NULL argument");
    if (!e->explore_set) return fail(GYMRS_EINVAL, "gymrs_get_exploration: the engine has no exploration settings (gymrs_set_exploration)");
    *x_out = gymrs_exploration{e->explore.seed, e->explore.threshold, 0};
    return GYMRS_OK;
}

gymrs_status gymrs_explore_actions(gymrs_engine* e, void* actions_dev)
{
    if (!e || !actions_dev) return fail(GYMRS_EINVAL, "gymrs_explore_actions: NULL argument");
    if (gymrs_status st = check_policy_set(e, "gymrs_explore_actions")) return st;
    if (!e->explore_set) return fail(GYMRS_EINVAL, "gymrs_explore_actions: the engine has no exploration settings (gymrs_set_exploration)");
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(launch_explore_actions(e->kind, e->s, actions_dev, e->n, e->gid0, e->tick, e->policy.args, e->explore, e->stream));
    return GYMRS_OK;
}

gymrs_status gymrs_explore_draw(const gymrs_exploration* x, uint32_t n_actions, uint64_t global_id, uint64_t tick, uint8_t* explored,
                                uint8_t* random_action)
{
    if (!x) return fail(GYMRS_EINVAL, "gymrs_explore_draw: NULL settings");
    if (gymrs_status st = check_exploration(x, "gymrs_explore_draw")) return st;
    if (n_actions == 0 || n_actions > 256) return fail(GYMRS_EINVAL, "gymrs_explore_draw: n_actions must be in 1 .. 256");
    const uint32_t w = explore_word(x->seed, global_id, tick);
    if (explored) *explored = explore_decides(w, x->threshold) ? 1 : 0;
    if (random_action) *random_action = explore_random(w, n_actions);
    return GYMRS_OK;
}

// ---- softmax sampling: the settings, the per-step call and the host-side draw (include/gymrs_amd.h, "sampling") ------------------
static gymrs_status check_sampling(const gymrs_sampling* x, const std::string& who)
{
    if (!finite_non_negative(x->scale))
        return fail(GYMRS_EINVAL, who + ": scale must be finite and >= 0 (scale = log2(e) / temperature; 0 is the uniform policy)");
    if (x->reserved != 0) return fail(GYMRS_EINVAL, who + ": reserved must be 0");
    return GYMRS_OK;
}

gymrs_status gymrs_set_sampling(gymrs_engine* e, const gymrs_sampling* x)
{
    if (!e) return fail(GYMRS_EINVAL, "gymrs_set_sampling: NULL engine");
    if (e->kind != GYMRS_CARTPOLE && e->kind != GYMRS_MOUNTAIN_CAR)
        return fail(GYMRS_EINVAL, "gymrs_set_sampling: sampling is for the Discrete envs (CartPole, MountainCar); Pendulum takes a Box action");
    if (!x) { // (launches already enqueued carry their own copy of the settings)
        e->sample = SampleArgs{};
        e->sample_set = false;
        return GYMRS_OK;
    }
    if (gymrs_status st = check_sampling(x, "gymrs_set_sampling")) return st;
    e->sample = SampleArgs{x->seed, x->scale, 0};
    e->sample_set = true;
    return GYMRS_OK;
}

gymrs_status gymrs_get_sampling(gymrs_engine* e, gymrs_sampling* x_out)
{
    if (!e || !x_out) return fail(GYMRS_EINVAL, "gymrs_get_sampling: NULL argument");
    if (!e->sample_set) return fail(GYMRS_EINVAL, "gymrs_get_sampling: the engine has no sampling settings (gymrs_set_sampling)");
    *x_out = gymrs_sampling{e->sample.seed, e->sample.scale, 0};
    return GYMRS_OK;
}

gymrs_status gymrs_sample_actions(gymrs_engine* e, void* actions_dev, float* prob_dev)
{
    if (!e || !actions_dev) return fail(GYMRS_EINVAL, "gymrs_sample_actions: NULL argument");
    if (gymrs_status st = check_policy_set(e, "gymrs_sample_actions")) return st;
    if (!e->sample_set) return fail(GYMRS_EINVAL, "gymrs_sample_actions: the engine has no sampling settings (gymrs_set_sampling)");
    if (reinterpret_cast<uintptr_t>(prob_dev) % sizeof(float) != 0) return fail(GYMRS_EINVAL, "gymrs_sample_actions: prob_dev must be 4-byte aligned");
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(launch_sample_actions(e->kind, e->s, actions_dev, prob_dev, e->n, e->gid0, e->tick, e->policy.args, e->sample, e->stream));
    return GYMRS_OK;
}

gymrs_status gymrs_sample_draw(const gymrs_sampling* x, uint32_t n_actions, const float* logits, uint64_t global_id, uint64_t tick, uint8_t* action,
                               float* probs)
{
    if (!x) return fail(GYMRS_EINVAL, "gymrs_sample_draw: NULL settings");
    if (gymrs_status st = check_sampling(x, "gymrs_sample_draw")) return st;
    if (n_actions < 2 || n_actions > kMaxSampleActions) return fail(GYMRS_EINVAL, "gymrs_sample_draw: n_actions must be in 2 .. 8");
    if (!logits) return fail(GYMRS_EINVAL, "gymrs_sample_draw: NULL logits");
    const uint32_t a = sample_action(logits, n_actions, x->scale, sample_word(x->seed, global_id, tick), probs);
    if (action) *action = (uint8_t)a;
    return GYMRS_OK;
}

// ---- advantages: the critic set, the host-side value and the launch (include/gymrs_amd.h, "advantages") --------------------------
gymrs_status gymrs_critic_size(gymrs_env_kind kind, uint32_t hidden, uint64_t* n_floats)
{
    if (!n_floats) return fail(GYMRS_EINVAL, "gymrs_critic_size: n_floats is NULL");
    if (gymrs_status st = check_network(kind, hidden, "gymrs_critic_size")) return st;
    *n_floats = critic_floats(kind, hidden);
    return GYMRS_OK;
}

gymrs_status gymrs_set_critic(gymrs_engine* e, const gymrs_policy_desc* d, const float* weights_host)
{
    if (!e) return fail(GYMRS_EINVAL, "gymrs_set_critic: NULL engine");
    if (!d) return remove_weights(e, kCriticKind);
    if (gymrs_status st = check_weights(e, kCriticKind, d, weights_host, "gymrs_set_critic")) return st;
    HIP_TRY(hipSetDevice(e->device));
    return install_weights(e, kCriticKind, d, weights_host);
}

gymrs_status gymrs_get_critic(gymrs_engine* e, gymrs_policy_desc* d_out, float* weights_out, uint64_t capacity_floats)
{
    return read_weights(e, kCriticKind, d_out, weights_out, capacity_floats, "gymrs_get_critic");
}

gymrs_status gymrs_critic_weights_ptr(gymrs_engine* e, float** dev_out, uint64_t* n_floats)
{
    return weights_view(e, kCriticKind, dev_out, n_floats, "gymrs_critic_weights_ptr");
}

gymrs_status gymrs_critic_value(gymrs_env_kind kind, uint32_t hidden, const float* weights, const float* obs, float* v)
{
    if (!weights || !obs || !v) return fail(GYMRS_EINVAL, "gymrs_critic_value: NULL argument");
    if (gymrs_status st = check_network(kind, hidden, "gymrs_critic_value")) return st;
    const HostWeights w{weights};
    float out[1];
    if (kind == GYMRS_CARTPOLE) {
        const float x[4][1] = {{obs[0]}, {obs[1]}, {obs[2]}, {obs[3]}};
        critic_values<4, 1, 1>(w, hidden, x, out);
    } else {
        const float x[2][1] = {{obs[0]}, {obs[1]}};
        critic_values<2, 1, 1>(w, hidden, x, out);
    }
    *v = out[0];
    return GYMRS_OK;
}

gymrs_status gymrs_advantages(gymrs_engine* e, const gymrs_advantages_desc* d)
{
    const RecordCall c{e, d, "gymrs_advantages"};
    if (gymrs_status st = c.prologue("advantages are")) return st;
    if (d->reserved != 0) return c.refuse("reserved must be 0");
    if (d->flags & ~GYMRS_ADVANTAGES_CRITIC) return c.refuse("unknown flag bits (GYMRS_ADVANTAGES_CRITIC is the only one)");
    const bool critic = (d->flags & GYMRS_ADVANTAGES_CRITIC) != 0;
    if (critic && !e->critic.dev) return c.refuse("GYMRS_ADVANTAGES_CRITIC without a critic set on the engine (gymrs_set_critic)");
    if (!(d->gamma >= 0.0f && d->gamma <= 1.0f)) return c.refuse("gamma must be in [0, 1]");
    if (!(d->lambda >= 0.0f && d->lambda <= 1.0f)) return c.refuse("lambda must be in [0, 1]");
    const gymrs_trajectory& rec = d->record;
    if (gymrs_status st = c.not_null({{rec.obs, "record.obs"}, {rec.reward, "record.reward"}, {rec.done, "record.done"}, {d->start_obs, "start_obs"},
                                      {d->advantages, "advantages"}}))
        return st;
    if (gymrs_status st = c.aligned({rec.obs, rec.reward, rec.done, rec.truncated, d->final_obs, d->start_obs, d->advantages, d->returns, d->values}, 16,
                                    "every buffer must be 16-byte aligned"))
        return st;
    if (gymrs_status st = c.lane_stride(rec.lane_stride)) return st;
    if (d->n_steps == 0) return GYMRS_OK;
    const AdvantageArgs a{rec.obs, rec.reward, rec.done, rec.truncated, d->final_obs, d->start_obs, d->advantages, d->returns, d->values,
                          /*stride, n, gid0*/ rec.lane_stride, e->n, e->gid0, d->n_steps, d->gamma, /*gl*/ d->gamma * d->lambda, /*pad_*/ 0};
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(launch_advantages(e->kind, a, critic ? &e->critic.args : nullptr, e->stream));
    return GYMRS_OK;
}

// ---- gradients: the host-side lane and the launch (include/gymrs_amd.h, "gradients") ------------------------------------------------
gymrs_status gymrs_gradient_lane(gymrs_env_kind kind, uint32_t hidden, uint32_t flags, float scale, const float* weights, uint32_t n_steps,
                                 const float* x, const uint8_t* actions, const float* coef, int64_t* q, uint64_t* excluded, float* prob)
{
    const std::string who = "gymrs_gradient_lane";
    if (gymrs_status st = check_network(kind, hidden, who)) return st;
    if (flags & ~GYMRS_GRADIENT_CRITIC) return fail(GYMRS_EINVAL, who + ": unknown flag bits (GYMRS_GRADIENT_CRITIC is the only one)");
    const bool critic = (flags & GYMRS_GRADIENT_CRITIC) != 0;
    if (!weights || !coef || !q || !excluded || (n_steps != 0 && !x)) return fail(GYMRS_EINVAL, who + ": NULL argument");
    if (!critic && n_steps != 0 && !actions) return fail(GYMRS_EINVAL, who + ": actions is NULL (the policy head reads them)");
    if (critic && prob) return fail(GYMRS_EINVAL, who + ": prob with GYMRS_GRADIENT_CRITIC (the critic head has no probabilities)");
    if (!critic && !finite_non_negative(scale)) return fail(GYMRS_EINVAL, who + ": scale must be finite and >= 0");
    if (kind == GYMRS_CARTPOLE) {
        if (critic)
            gradient_lane<4, 1, true>(hidden, scale, weights, n_steps, x, actions, coef, q, excluded, prob);
        else
            gradient_lane<4, 2, false>(hidden, scale, weights, n_steps, x, actions, coef, q, excluded, prob);
    } else {
        if (critic)
            gradient_lane<2, 1, true>(hidden, scale, weights, n_steps, x, actions, coef, q, excluded, prob);
        else
            gradient_lane<2, 3, false>(hidden, scale, weights, n_steps, x, actions, coef, q, excluded, prob);
    }
    return GYMRS_OK;
}

gymrs_status gymrs_policy_gradient(gymrs_engine* e, const gymrs_gradient_desc* d)
{
    const RecordCall c{e, d, "gymrs_policy_gradient"};
    if (gymrs_status st = c.prologue("gradients are")) return st;
    if (d->reserved != 0 || d->pad_ != 0) return c.refuse("reserved must be 0");
    if (d->flags & ~GYMRS_GRADIENT_CRITIC) return c.refuse("unknown flag bits (GYMRS_GRADIENT_CRITIC is the only one)");
    const bool critic = (d->flags & GYMRS_GRADIENT_CRITIC) != 0;
    if (critic && !e->critic.dev) return c.refuse("GYMRS_GRADIENT_CRITIC without a critic set on the engine (gymrs_set_critic)");
    if (!critic) {
        if (gymrs_status st = check_policy_set(e, c.who)) return st;
        if (gymrs_status st = c.scale(d->scale)) return st;
    }
    const gymrs_trajectory& rec = d->record;
    const void* actions = critic ? nullptr : rec.actions;
    if (gymrs_status st = c.not_null({{rec.obs, "record.obs"}})) return st;
    if (!critic)
        if (gymrs_status st = c.not_null({{actions, "record.actions", " (the policy head reads them)"}})) return st;
    if (gymrs_status st = c.not_null({{d->start_obs, "start_obs"}, {d->coef, "coef"}, {d->grad, "grad"}, {d->excluded, "excluded"}})) return st;
    if (critic && d->prob) return c.refuse("prob with GYMRS_GRADIENT_CRITIC (the critic head has no probabilities)");
    if (gymrs_status st = c.aligned({rec.obs, actions, d->start_obs, d->coef, d->prob}, 16, "every row buffer must be 16-byte aligned")) return st;
    if (gymrs_status st = c.aligned({d->grad, d->excluded}, 8, "grad and excluded must be 8-byte aligned")) return st;
    if (gymrs_status st = c.lane_stride(rec.lane_stride)) return st;
    if (d->n_steps == 0) return GYMRS_OK;
    const GradientArgs a = gradient_args(e, rec, actions, d->n_steps, critic ? 0.0f : d->scale, d->start_obs, d->coef, d->prob, d->grad, d->excluded);
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(launch_policy_gradient(e->kind, critic, a, critic ? e->critic.args : e->policy.args, e->stream));
    return GYMRS_OK;
}

// ---- clipped surrogate: the host-side lane and the launch (include/gymrs_amd.h, "clipped surrogate") -------------------------------
gymrs_status gymrs_ppo_lane(gymrs_env_kind kind, uint32_t hidden, float scale, float clip_low, float clip_high, const float* weights, uint32_t n_steps,
                            const float* x, const uint8_t* actions, const float* advantages, const float* old_prob, int64_t* q, uint64_t* excluded,
                            uint64_t counts[2], float* prob)
{
    const std::string who = "gymrs_ppo_lane";
    if (gymrs_status st = check_network(kind, hidden, who)) return st;
    if (!weights || !advantages || !old_prob || !q || !excluded || (n_steps != 0 && (!x || !actions))) return fail(GYMRS_EINVAL, who + ": NULL argument");
    if (prob && prob == old_prob) return fail(GYMRS_EINVAL, who + ": prob and old_prob may not alias");
    if (!finite_non_negative(scale)) return fail(GYMRS_EINVAL, who + ": scale must be finite and >= 0");
    if (!ppo_bounds_ok(clip_low, clip_high)) return fail(GYMRS_EINVAL, who + ": clip bounds must be finite with 0 <= clip_low <= 1 <= clip_high");
    const PpoLane ppo{old_prob, clip_low, clip_high, counts};
    if (kind == GYMRS_CARTPOLE)
        gradient_lane<4, 2, false>(hidden, scale, weights, n_steps, x, actions, advantages, q, excluded, prob, &ppo);
    else
        gradient_lane<2, 3, false>(hidden, scale, weights, n_steps, x, actions, advantages, q, excluded, prob, &ppo);
    return GYMRS_OK;
}

gymrs_status gymrs_ppo_gradient(gymrs_engine* e, const gymrs_ppo_desc* d)
{
    const RecordCall c{e, d, "gymrs_ppo_gradient"};
    if (gymrs_status st = c.prologue("gradients are")) return st;
    if (d->reserved != 0 || d->pad_ != 0) return c.refuse("reserved and pad_ must be 0");
    if (d->flags != 0) return c.refuse("unknown flag bits (flags must be 0)");
    if (gymrs_status st = check_policy_set(e, c.who)) return st;
    if (gymrs_status st = c.scale(d->scale)) return st;
    if (!ppo_bounds_ok(d->clip_low, d->clip_high)) return c.refuse("clip bounds must be finite with 0 <= clip_low <= 1 <= clip_high");
    const gymrs_trajectory& rec = d->record;
    if (gymrs_status st = c.not_null({{rec.obs, "record.obs"}, {rec.actions, "record.actions", " (the policy head reads them)"}, {d->start_obs, "start_obs"},
                                      {d->advantages, "advantages"}, {d->old_prob, "old_prob"}, {d->grad, "grad"}, {d->excluded, "excluded"}}))
        return st;
    if (d->prob == d->old_prob) return c.refuse("prob and old_prob may not alias");
    if (gymrs_status st = c.aligned({rec.obs, rec.actions, d->start_obs, d->advantages, d->old_prob, d->prob}, 16, "every row buffer must be 16-byte aligned"))
        return st;
    if (gymrs_status st = c.aligned({d->grad, d->excluded, d->counts}, 8, "grad, excluded and counts must be 8-byte aligned")) return st;
    if (gymrs_status st = c.lane_stride(rec.lane_stride)) return st;
    if (d->n_steps == 0) return GYMRS_OK;
    const PpoArgs a{gradient_args(e, rec, rec.actions, d->n_steps, d->scale, d->start_obs, d->advantages, d->prob, d->grad, d->excluded), d->old_prob,
                    reinterpret_cast<unsigned long long*>(d->counts), d->clip_low, d->clip_high};
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(launch_ppo_gradient(e->kind, a, e->policy.args, e->stream));
    return GYMRS_OK;
}

// ---- per-policy fitness: the table behind gymrs_rollout_policy_fitness -----------------------------------------------------
gymrs_status gymrs_policy_fitness_ptr(gymrs_engine* e, gymrs_policy_fitness** dev_out, uint32_t* n_policies)
{
    return kFitness.view(e, dev_out, n_policies, "gymrs_policy_fitness_ptr");
}

gymrs_status gymrs_get_policy_fitness(gymrs_engine* e, uint32_t first, uint32_t count, gymrs_policy_fitness* host_out)
{
    return kFitness.read(e, first, count, host_out, "gymrs_get_policy_fitness");
}

gymrs_status gymrs_policy_fitness_clear(gymrs_engine* e)
{
    if (!e) return fail(GYMRS_EINVAL, "gymrs_policy_fitness_clear: NULL engine");
    const bool fresh = e->fitness_dev == nullptr; // (a table that comes into being here is already zero)
    if (gymrs_status st = kFitness.ensure(e, "gymrs_policy_fitness_clear")) return st;
    if (fresh) return GYMRS_OK;
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(zero_fitness(e->fitness_dev, e->policy.args.n_policies, e->stream));
    return GYMRS_OK;
}

// ---- episodic policy evaluation: gymrs_evaluate_policy and its table ------------------------------------------------------------
gymrs_status gymrs_evaluate_policy(gymrs_engine* e, const gymrs_eval_desc* d)
{
    const std::string who = "gymrs_evaluate_policy";
    if (!e) return fail(GYMRS_EINVAL, who + ": NULL engine");
    if (!d) return fail(GYMRS_EINVAL, who + ": NULL desc");
    if (gymrs_status st = check_discrete_env(e->kind, who)) return st;
    if (gymrs_status st = check_policy_set(e, who)) return st;
    if (gymrs_status st = check_table_opt_in(e, (d->flags & GYMRS_EVAL_LANE_PARAMS) != 0, who, // (a plain descriptor never plays a table engine with one set of parameters)
                                             ": set GYMRS_EVAL_LANE_PARAMS in flags and every lane plays with its own row, or use gymrs_policy_actions + gymrs_step"))
        return st;
    if (d->episodes_per_lane == 0) return fail(GYMRS_EINVAL, who + ": episodes_per_lane must be >= 1");
    if (d->reserved != 0) return fail(GYMRS_EINVAL, who + ": reserved must be 0");
    if (d->flags & ~(GYMRS_EVAL_COMMON_STARTS | GYMRS_EVAL_LANE_PARAMS))
        return fail(GYMRS_EINVAL, who + ": unknown flag bits (GYMRS_EVAL_COMMON_STARTS and GYMRS_EVAL_LANE_PARAMS are the only ones)");
    if (reinterpret_cast<uintptr_t>(d->lengths_dev) % alignof(uint32_t) != 0) return fail(GYMRS_EINVAL, who + ": lengths_dev must be 4-byte aligned");
    const uint32_t dflt = e->kind == GYMRS_CARTPOLE ? e->consts.cp.max_steps : e->consts.mc.max_steps; // the params' max_episode_steps (500 / 200 by default; a table: the limit its rows share)
    const uint32_t m = d->max_episode_steps ? d->max_episode_steps : dflt;
    if ((uint64_t)d->episodes_per_lane * m > kMaxEvalSteps)
        return fail(GYMRS_EINVAL, who + ": episodes_per_lane * max_episode_steps is above GYMRS_POLICY_EVAL_MAX_STEPS (it bounds the launch's running "
                                        "time and keeps a lane's step count in 32 bits); split the evaluation");
    if (gymrs_status st = kEval.ensure(e, who)) return st;
    HIP_TRY(hipSetDevice(e->device));
    // the latest call's results: identities first, in stream order, then this launch's episodes
    HIP_TRY(launch_policy_eval_identity(e->eval_dev, e->policy.args.n_policies, e->stream));
    EvalArgs a;
    std::memset(&a, 0, sizeof(a));
    a.n = e->n;
    a.gid0 = e->gid0;
    a.seed = d->seed;
    a.episodes = d->episodes_per_lane;
    a.max_steps = m;
    a.flags = d->flags & GYMRS_EVAL_COMMON_STARTS; // (GYMRS_EVAL_LANE_PARAMS chooses the kernel; without a table it changes nothing)
    a.lengths = d->lengths_dev;
    a.table = e->eval_dev;
    a.box = make_sample_box(e->dflt_lo, e->dflt_hi, e->state_dim); // gymrs_reset without bounds
    HIP_TRY(launch_evaluate_policy(e->kind, e->table_k ? kFlagTable : 0u, a, launch_consts(e), e->policy.args, e->stream));
    return GYMRS_OK;
}

gymrs_status gymrs_policy_eval_ptr(gymrs_engine* e, gymrs_policy_eval** dev_out, uint32_t* n_policies)
{
    return kEval.view(e, dev_out, n_policies, "gymrs_policy_eval_ptr");
}

gymrs_status gymrs_get_policy_eval(gymrs_engine* e, uint32_t first, uint32_t count, gymrs_policy_eval* host_out)
{
    return kEval.read(e, first, count, host_out, "gymrs_get_policy_eval");
}

} // extern "C"
