// gymrs_engine_learn.hip -- the learner surface of the C ABI (include/gymrs_amd.h): the policy and critic sets, the exploration and sampling
// settings with their per-step calls and host draws, advantages, gradients, the clipped surrogate, the entropy bonus and Q-learning (with its target set) over a
// transitions record, prioritized replay (push, sample, update and the host-only rules) with their host-only lanes, the optimizer with its Adam state and host-only set, the per-policy fitness and evaluation
// tables.  Host code only: the kernels are behind gymrs_kernels.h.  The engine
// object and the refusals shared with the stepping paths: gymrs_engine_priv.h.
#include "gymrs_engine_priv.h"
#include "gymrs_evaluate.h"
#include "gymrs_sample.h"
#include "gymrs_advantages.h"
#include "gymrs_gradient.h"
#include "gymrs_vtrace.h"
#include "gymrs_entropy.h"
#include "gymrs_value.h"
#include "gymrs_normalize.h"
#include "gymrs_qlearn.h"
#include "gymrs_replay.h"
#include "gymrs_optimizer.h"
#include "gymrs_es.h"

#include <algorithm>

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
    // (weights_host == NULL: the caller writes the set on the device, gymrs_es_init)
    if (weights_host) {
        HIP_TRY(hipMemcpyAsync(set.dev, weights_host, (size_t)total * sizeof(float), hipMemcpyHostToDevice, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
    }
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

// ---- the target set of gymrs_q_gradient: a copy of the policy set the engine owns ----------------------------------------------------
// The target goes with its buffer (launches already enqueued still read it: wait for them).
gymrs_status discard_q_target(gymrs_engine* e)
{
    if (!e->q_target.dev) return GYMRS_OK;
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipFree(e->q_target.dev));
    e->q_target = WeightSet{};
    return GYMRS_OK;
}

// A new policy set of the target's shape keeps the target.
bool q_target_fits(const gymrs_engine* e, const gymrs_policy_desc* d)
{
    const PolicyArgs& t = e->q_target.args;
    return e->q_target.dev && t.hidden == d->hidden && t.n_policies == d->n_policies && t.lanes_per_policy == d->lanes_per_policy;
}

// ---- the Adam state of gymrs_apply_gradient, per head: under the target's lifetime rule ------------------------------------------------
// The state goes with its buffer (launches already enqueued still read it: wait for them).
gymrs_status discard_opt_state(gymrs_engine* e, uint32_t head)
{
    OptimizerState& st = e->opt_state[head];
    if (!st.dev) return GYMRS_OK;
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipFree(st.dev));
    st = OptimizerState{};
    return GYMRS_OK;
}

// A new weight set of the state's shape keeps the state; any other discards it.
gymrs_status keep_or_discard_opt_state(gymrs_engine* e, uint32_t head, const gymrs_policy_desc* d)
{
    const PolicyArgs& t = e->opt_state[head].shape;
    if (t.hidden == d->hidden && t.n_policies == d->n_policies && t.lanes_per_policy == d->lanes_per_policy) return GYMRS_OK;
    return discard_opt_state(e, head);
}

// The state of a head, made fresh at the first Adam call on it (the caller has checked that the head has a set).
gymrs_status opt_state_of(gymrs_engine* e, uint32_t head, const WeightSet& set)
{
    OptimizerState& st = e->opt_state[head];
    if (st.dev) return GYMRS_OK;
    HIP_TRY(hipSetDevice(e->device));
    st.shape = set.args;
    HIP_TRY(hipMalloc(&st.dev, (size_t)(2 * st.words() + 2 * (uint64_t)st.shape.n_policies) * sizeof(float)));
    if (hipError_t err = launch_optimizer_fresh(st.m(), st.v(), st.pw(), st.shape.n_policies, st.shape.stride, e->stream)) {
        (void)hipFree(st.dev);
        st = OptimizerState{};
        HIP_TRY(err);
    }
    return GYMRS_OK;
}

// ---- the evolution-strategies state of gymrs_es_init: under the target's lifetime rule ---------------------------------------------------
// The state goes with its buffers (launches already enqueued still use them: wait for them).
gymrs_status discard_es(gymrs_engine* e)
{
    EsState& es = e->es;
    if (!es.dev) return GYMRS_OK;
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipFree(es.dev));
    HIP_TRY(hipFree(es.u));
    HIP_TRY(hipFree(es.fitness));
    es = EsState{};
    return GYMRS_OK;
}

// A new policy set of the state's shape keeps the state; any other discards it.
bool es_fits(const gymrs_engine* e, const gymrs_policy_desc* d)
{
    const PolicyArgs& t = e->es.shape;
    return e->es.dev && t.hidden == d->hidden && t.n_policies == d->n_policies && t.lanes_per_policy == d->lanes_per_policy;
}

// The state for the policy set that was just installed: the buffers of a kept state are reused (the caller discarded any other).
gymrs_status es_state_for(gymrs_engine* e)
{
    EsState& es = e->es;
    if (es.dev) return GYMRS_OK;
    const size_t P = e->policy.args.n_policies;
    hipError_t err = hipMalloc(&es.dev, sizeof(EsDeviceState));
    if (!err) err = hipMalloc(&es.u, P * sizeof(float));
    if (!err) err = hipMalloc(&es.fitness, P * sizeof(double));
    if (err) {
        (void)hipFree(es.dev);
        (void)hipFree(es.u);
        (void)hipFree(es.fitness);
        es = EsState{};
        HIP_TRY(err);
    }
    return GYMRS_OK;
}

// What the ES kernels get by value, without the step's own values.
EsArgs es_args(const gymrs_engine* e)
{
    const EsState& es = e->es;
    EsArgs a;
    std::memset(&a, 0, sizeof(a));
    a.st = es.dev;
    a.weights = e->policy.dev;
    a.u = es.u;
    a.fitness = es.fitness;
    a.seed = es.seed;
    a.gen = es.gen;
    a.P = es.shape.n_policies;
    a.S = es.shape.stride;
    a.sigma = a.sigma_new = es.sigma;
    return a;
}

bool es_sigma_ok(float sigma) { return sigma > 0.0f && sigma <= std::numeric_limits<float>::max(); } // (false for a NaN)

// slot[0] of the butterfly mask = 512 .. 1 over 1024 slots, as written in the header
double es_fold(double* slot)
{
    double next[kEsChunk];
    for (uint32_t mask = kEsChunk / 2; mask >= 1; mask >>= 1) {
        for (uint32_t l = 0; l < kEsChunk; ++l) next[l] = slot[l] + slot[l ^ mask];
        std::copy(next, next + kEsChunk, slot);
    }
    return slot[0];
}

// The two-level sum of value(p) over p < P: chunks of 1024, then the chunk sums.
template <class Value>
double es_sum(uint32_t P, Value value)
{
    double slot[kEsChunk], top[kEsChunk];
    std::fill(top, top + kEsChunk, 0.0);
    for (uint32_t c = 0; c * kEsChunk < P; ++c) {
        for (uint32_t l = 0; l < kEsChunk; ++l) slot[l] = c * kEsChunk + l < P ? value(c * kEsChunk + l) : 0.0;
        top[c] = es_fold(slot);
    }
    return es_fold(top);
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

// The evaluation table goes, and with it the scratch of gymrs_es_ranks (launches already enqueued still use it: wait for them).
gymrs_status discard_eval(gymrs_engine* e)
{
    if (gymrs_status st = kEval.discard(e)) return st;
    if (!e->rank_scratch) return GYMRS_OK;
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipFree(e->rank_scratch));
    e->rank_scratch = nullptr;
    return GYMRS_OK;
}

// A checked policy set takes the place of the old one, and everything that belongs to a set follows its lifetime rule: what
// gymrs_set_policy and gymrs_es_init (weights_host == NULL: it writes the set on the device) share.  The ES state is the caller's.
gymrs_status replace_policy_set(gymrs_engine* e, const gymrs_policy_desc* d, const float* weights_host)
{
    HIP_TRY(hipSetDevice(e->device));
    if (!q_target_fits(e, d))
        if (gymrs_status st = discard_q_target(e)) return st; // a target of another shape belongs to the set it was copied from
    if (gymrs_status st = keep_or_discard_opt_state(e, GYMRS_OPT_HEAD_POLICY, d)) return st; // so do the moments
    // a new set starts from zero counters: a table of another size goes (allocated again at its first use), one of the same
    // size -- a search's next generation -- is kept and zeroed in stream order, after the launches that still add to it
    if (e->fitness_dev && d->n_policies == e->policy.args.n_policies) {
        HIP_TRY(zero_fitness(e->fitness_dev, d->n_policies, e->stream));
    } else if (gymrs_status st = kFitness.discard(e)) {
        return st;
    }
    if (gymrs_status st = discard_eval(e)) return st; // the episodic records belong to the set they were played with
    e->es.evaluated = false;
    return install_weights(e, kPolicyKind, d, weights_host);
}

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

// One lane of "Entropy" by the shared text: the kernel's walk with VEC = 1, chunk after chunk.  old_prob == NULL: no KL estimate.
template <int D, int A>
void entropy_lane(uint32_t H, float scale, float coef, const float* weights, uint32_t K, const float* x, const uint8_t* actions, const float* old_prob,
                  int64_t* q, uint64_t* excluded, int64_t* sums_out, uint64_t* counts)
{
    const HostWeights w{weights};
    uint64_t excl = 0;
    EntropySums<1> sums{};
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
            float xs[D][1], y[A][1], g[A][1], hn[1], pr[A][1];
            bool on[1];
            for (int j = 0; j < D; ++j) xs[j][0] = x[(size_t)k * D + j];
            gradient_logits<D, A, 1, 1>(w, H, xs, y);
            entropy_head<A, 1>(y, scale, coef, g, on, hn, pr);
            if (chunk == 0) {
                const uint8_t act[1] = {old_prob ? actions[k] : uint8_t(0)};
                const float po[1] = {old_prob ? old_prob[k] : 0.0f};
                if (old_prob)
                    entropy_sums_step<A, 1, true>(on, hn, pr, act, po, sums);
                else
                    entropy_sums_step<A, 1, false>(on, hn, pr, act, po, sums);
            }
            if (H == 0) {
                gradient_affine_step<D, A, 1, true>(xs, g, on, aff);
            } else {
                gradient_chunk_step<D, A, 1, true>(w, H, h0, xs, g, on, chk);
                if (chunk == 0) gradient_bias_step<A, 1, true>(g, on, db2);
            }
        }
        if (H == 0) {
            gradient_affine_each<D, A, 1>(aff, emit);
        } else {
            gradient_chunk_each<D, A, 1>(H, h0, chk, emit);
            if (chunk == 0) gradient_bias_each<D, A, 1>(H, db2, emit);
        }
    }
    long long v;
    if (!gradient_fixed(sums.h[0], v)) excl += 1;
    sums_out[0] = v;
    if (!gradient_fixed(sums.kl[0], v)) excl += 1;
    sums_out[1] = v;
    *excluded = excl;
    if (counts) {
        counts[0] = sums.n_h[0];
        counts[1] = sums.n_kl[0];
    }
}

// One lane of "Q-learning" by the shared text: the TD kernel's walk, then the gradient kernel's, with VEC = 1, chunk after chunk.
template <int D, int A>
void q_lane(uint32_t H, uint32_t flags, float gamma, float kappa, const float* weights, const float* target_weights, uint32_t K, const float* x,
            const float* x_next, const uint8_t* actions, const float* reward, const uint8_t* done, int64_t* q, uint64_t* excluded, float* td,
            uint64_t* counts)
{
    const HostWeights w{weights}, wt{target_weights};
    std::vector<float> delta(K);
    uint64_t seen = 0, ncut = 0;
    for (uint32_t k = 0; k < K; ++k) {
        float xs[D][1], xn[D][1], y[A][1], yt[A][1], ysel[A][1], dl[1];
        for (int j = 0; j < D; ++j) {
            xs[j][0] = x[(size_t)k * D + j];
            xn[j][0] = x_next[(size_t)k * D + j];
        }
        gradient_logits<D, A, 1, 1>(w, H, xs, y);
        gradient_logits<D, A, 1, 1>(wt, H, xn, yt);
        if (flags & GYMRS_Q_DOUBLE)
            gradient_logits<D, A, 1, 1>(w, H, xn, ysel);
        else
            for (int b = 0; b < A; ++b) ysel[b][0] = yt[b][0];
        const uint8_t act[1] = {actions[k]};
        const float r[1] = {reward[k]};
        const bool dn[1] = {done[k] != 0};
        bool on[1];
        q_td_step<A, 1>(y, yt, ysel, act, r, dn, gamma, dl, on);
        delta[k] = dl[0];
        seen += on[0] ? 1 : 0;
        ncut += (on[0] && q_clamped(dl[0], kappa)) ? 1 : 0;
    }
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
            bool on[1];
            for (int j = 0; j < D; ++j) xs[j][0] = x[(size_t)k * D + j];
            const float dl[1] = {delta[k]};
            const uint8_t act[1] = {actions[k]};
            q_head<A, 1>(dl, act, kappa, g, on);
            if (H == 0) {
                gradient_affine_step<D, A, 1, true>(xs, g, on, aff);
            } else {
                gradient_chunk_step<D, A, 1, true>(w, H, h0, xs, g, on, chk);
                if (chunk == 0) gradient_bias_step<A, 1, true>(g, on, db2);
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
    if (td) std::copy(delta.begin(), delta.end(), td);
    if (counts) {
        counts[0] = seen;
        counts[1] = ncut;
    }
}

// One lane of "Value loss" by the shared text: the forward walk (v, c, sums, counts), then the critic head's lane fed c.
template <int D>
void value_lane(uint32_t H, float clip, const float* weights, uint32_t K, const float* x, const float* returns, const float* old_values, int64_t* q,
                       uint64_t* excluded, int64_t* sums_out, uint64_t* counts, float* values)
{
    const HostWeights w{weights};
    std::vector<float> c(K);
    ValueSums<1> sums{};
    for (uint32_t k = 0; k < K; ++k) {
        float xs[D][1], v[1], g[1][1];
        for (int j = 0; j < D; ++j) xs[j][0] = x[(size_t)k * D + j];
        critic_values<D, 1, 1>(w, H, xs, v);
        const float R[1] = {returns[k]}, vo[1] = {old_values ? old_values[k] : 0.0f};
        value_head<1, true>(v, R, vo, clip, old_values != nullptr, g, sums);
        c[k] = g[0][0];
        if (values) values[k] = v[0];
    }
    gradient_lane<D, 1, true>(H, 0.0f, weights, K, x, nullptr, c.data(), q, excluded, nullptr);
    if (sums_out) {
        long long f;
        if (!gradient_fixed(sums.s0[0], f)) *excluded += 1;
        sums_out[0] = f;
        if (!gradient_fixed(sums.s1[0], f)) *excluded += 1;
        sums_out[1] = f;
    }
    if (counts) {
        counts[0] = sums.seen[0];
        counts[1] = sums.cut[0];
    }
}

// ---- "V-trace": the scalars both entry points refuse in the same words, and the lane
struct VtraceScalars {
    float gamma, lambda, scale, rho_bar, c_bar, pg_rho_bar;
};
bool vtrace_bar_ok(float bar) { return bar > 0.0f; } // (false for a NaN; +inf is no clipping)
// what the lane and the launch refuse in the same words; "" = fine
const char* vtrace_scalars_refused(const VtraceScalars& s)
{
    if (!(s.gamma >= 0.0f && s.gamma <= 1.0f)) return "gamma must be in [0, 1]";
    if (!(s.lambda >= 0.0f && s.lambda <= 1.0f)) return "lambda must be in [0, 1]";
    if (!finite_non_negative(s.scale)) return "scale must be finite and >= 0";
    if (!vtrace_bar_ok(s.rho_bar) || !vtrace_bar_ok(s.c_bar) || !vtrace_bar_ok(s.pg_rho_bar)) return "rho_bar, c_bar and pg_rho_bar must be > 0 (+inf: no clipping)";
    return "";
}

// One lane of "V-trace" by the shared text: the kernel's forward phase and scan with one lane, row K-1 down to row 0.
template <int D, int A>
void vtrace_lane(uint32_t Hp, uint32_t Hc, const float* wp_, const float* wc_, uint32_t K, const float* x, const float* x_next, const uint8_t* actions,
                 const float* reward, const uint8_t* done, const uint8_t* ended, const float* old_prob, const VtraceScalars& s, float* vs, float* pg,
                 float* values, float* prob, uint64_t* counts)
{
    const HostWeights wp{wp_}, wc{wc_};
    uint64_t cnt[3] = {0, 0, 0};
    float acc = 0.0f;
    for (uint32_t k = K; k-- > 0;) {
        float xs[D][1], xn[D][1], y[A][1], v_cur[1], v_succ[1], yl[A];
        for (int j = 0; j < D; ++j) {
            xs[j][0] = x[(size_t)k * D + j];
            xn[j][0] = x_next[(size_t)k * D + j];
        }
        gradient_logits<D, A, 1, 1>(wp, Hp, xs, y);
        critic_values<D, 1, 1>(wc, Hc, xs, v_cur);
        critic_values<D, 1, 1>(wc, Hc, xn, v_succ);
        for (int b = 0; b < A; ++b) yl[b] = y[b][0];
        const float pa = vtrace_prob<A>(yl, actions[k], s.scale);
        const bool valid = actions[k] < (uint8_t)A;
        const VtraceWeights w = vtrace_weights(pa, old_prob[k], valid, s.gamma, s.lambda, s.rho_bar, s.c_bar, s.pg_rho_bar);
        vtrace_step(s.gamma, reward[k], done[k] != 0, ended[k] != 0, v_succ[0], v_cur[0], w.rho, w.gc, w.rho_pg, acc, vs[k], pg[k]);
        if (values) values[k] = v_cur[0];
        if (prob) prob[k] = pa;
        cnt[0] += valid ? 1 : 0;
        cnt[1] += w.over_rho ? 1 : 0;
        cnt[2] += w.over_c ? 1 : 0;
    }
    if (counts)
        for (int c = 0; c < 3; ++c) counts[c] = cnt[c];
}

bool q_gamma_ok(float gamma) { return gamma >= 0.0f && gamma <= 1.0f; } // (false for a NaN)
bool q_kappa_ok(float kappa) { return kappa > 0.0f; }                   // (false for a NaN; +inf is the squared loss)
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
        if (gymrs_status st = discard_q_target(e)) return st;
        if (gymrs_status st = discard_opt_state(e, GYMRS_OPT_HEAD_POLICY)) return st;
        if (gymrs_status st = discard_es(e)) return st;
        if (gymrs_status st = discard_eval(e)) return st;
        return kFitness.discard(e);
    }
    if (gymrs_status st = check_weights(e, kPolicyKind, d, weights_host, "gymrs_set_policy")) return st;
    if (!es_fits(e, d))
        if (gymrs_status st = discard_es(e)) return st; // an ES state of another shape belongs to the population it wrote
    return replace_policy_set(e, d, weights_host);
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
    if (!d) {
        if (gymrs_status st = remove_weights(e, kCriticKind)) return st;
        return discard_opt_state(e, GYMRS_OPT_HEAD_CRITIC);
    }
    if (gymrs_status st = check_weights(e, kCriticKind, d, weights_host, "gymrs_set_critic")) return st;
    HIP_TRY(hipSetDevice(e->device));
    if (gymrs_status st = keep_or_discard_opt_state(e, GYMRS_OPT_HEAD_CRITIC, d)) return st; // the moments belong to a set of their shape
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

// ---- V-trace: the host-side lane and the launch (include/gymrs_amd.h, "V-trace") ----------------------------------------------------
static_assert(sizeof(gymrs_vtrace_desc) == 152, "descriptor size");

gymrs_status gymrs_vtrace_lane(gymrs_env_kind kind, uint32_t policy_hidden, uint32_t critic_hidden, const float* policy_weights,
                               const float* critic_weights, uint32_t n_steps, const float* x, const float* x_next, const uint8_t* actions,
                               const float* reward, const uint8_t* done, const uint8_t* ended, const float* old_prob, float gamma, float lambda,
                               float scale, float rho_bar, float c_bar, float pg_rho_bar, float* vs, float* pg_advantages, float* values, float* prob,
                               uint64_t counts[3])
{
    const std::string who = "gymrs_vtrace_lane";
    if (gymrs_status st = check_network(kind, policy_hidden, who)) return st;
    if (gymrs_status st = check_network(kind, critic_hidden, who)) return st;
    if (!policy_weights || !critic_weights || (n_steps != 0 && (!x || !x_next || !actions || !reward || !done || !ended || !old_prob || !vs || !pg_advantages)))
        return fail(GYMRS_EINVAL, who + ": NULL argument");
    if (prob && prob == old_prob) return fail(GYMRS_EINVAL, who + ": prob and old_prob may not alias");
    const VtraceScalars s{gamma, lambda, scale, rho_bar, c_bar, pg_rho_bar};
    if (const char* why = vtrace_scalars_refused(s); *why) return fail(GYMRS_EINVAL, who + ": " + why);
    if (kind == GYMRS_CARTPOLE)
        vtrace_lane<4, 2>(policy_hidden, critic_hidden, policy_weights, critic_weights, n_steps, x, x_next, actions, reward, done, ended, old_prob, s, vs,
                          pg_advantages, values, prob, counts);
    else
        vtrace_lane<2, 3>(policy_hidden, critic_hidden, policy_weights, critic_weights, n_steps, x, x_next, actions, reward, done, ended, old_prob, s, vs,
                          pg_advantages, values, prob, counts);
    return GYMRS_OK;
}

gymrs_status gymrs_vtrace(gymrs_engine* e, const gymrs_vtrace_desc* d)
{
    const RecordCall c{e, d, "gymrs_vtrace"};
    if (gymrs_status st = c.prologue("V-trace targets are")) return st;
    if (d->reserved != 0) return c.refuse("reserved must be 0");
    if (d->flags != 0) return c.refuse("unknown flag bits (flags must be 0)");
    if (gymrs_status st = check_policy_set(e, c.who)) return st;
    if (!e->critic.dev) return c.refuse("the engine has no critic set (gymrs_set_critic)");
    if (const char* why = vtrace_scalars_refused({d->gamma, d->lambda, d->scale, d->rho_bar, d->c_bar, d->pg_rho_bar}); *why) return c.refuse(why);
    const gymrs_trajectory& rec = d->record;
    if (gymrs_status st = c.not_null({{rec.obs, "record.obs"}, {rec.actions, "record.actions"}, {rec.reward, "record.reward"}, {rec.done, "record.done"},
                                      {d->start_obs, "start_obs"}, {d->old_prob, "old_prob"}, {d->vs, "vs"}, {d->pg_advantages, "pg_advantages"}}))
        return st;
    if (d->prob == d->old_prob) return c.refuse("prob and old_prob may not alias");
    if (gymrs_status st = c.aligned({rec.obs, rec.actions, rec.reward, rec.done, rec.truncated, d->final_obs, d->start_obs, d->old_prob, d->vs,
                                     d->pg_advantages, d->values, d->prob},
                                    16, "every row buffer must be 16-byte aligned"))
        return st;
    if (gymrs_status st = c.aligned({d->counts}, 8, "counts must be 8-byte aligned")) return st;
    if (gymrs_status st = c.lane_stride(rec.lane_stride)) return st;
    if (d->n_steps == 0) return GYMRS_OK;
    const VtraceArgs a{rec.obs, static_cast<const uint8_t*>(rec.actions), rec.reward, rec.done, rec.truncated, d->final_obs, d->start_obs, d->old_prob,
                       d->vs, d->pg_advantages, d->values, d->prob, reinterpret_cast<unsigned long long*>(d->counts),
                       /*stride, n, gid0*/ rec.lane_stride, e->n, e->gid0, d->n_steps, d->gamma, d->lambda, d->scale, d->rho_bar, d->c_bar, d->pg_rho_bar,
                       /*pad_*/ 0};
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(launch_vtrace(e->kind, a, e->policy.args, e->critic.args, e->stream));
    return GYMRS_OK;
}

// ---- entropy bonus and KL estimate: the logarithm, the host-side lane and the launch (include/gymrs_amd.h, "Entropy") ---------------
static bool finite_f(float x) { return x >= -std::numeric_limits<float>::max() && x <= std::numeric_limits<float>::max(); } // (false for a NaN)

gymrs_status gymrs_entropy_log2(float v, float* out)
{
    const std::string who = "gymrs_entropy_log2";
    if (!out) return fail(GYMRS_EINVAL, who + ": NULL argument");
    if (!(v >= 0x1p-126f && finite_f(v))) return fail(GYMRS_EINVAL, who + ": v must be finite and >= 2^-126");
    *out = entropy_log2(v);
    return GYMRS_OK;
}

gymrs_status gymrs_entropy_lane(gymrs_env_kind kind, uint32_t hidden, float scale, float coef, const float* weights, uint32_t n_steps, const float* x,
                                const uint8_t* actions, const float* old_prob, int64_t* q, uint64_t* excluded, int64_t sums[2], uint64_t counts[2])
{
    const std::string who = "gymrs_entropy_lane";
    if (gymrs_status st = check_network(kind, hidden, who)) return st;
    if (!weights || !q || !excluded || !sums || (n_steps != 0 && !x)) return fail(GYMRS_EINVAL, who + ": NULL argument");
    if (old_prob && n_steps != 0 && !actions) return fail(GYMRS_EINVAL, who + ": actions is NULL (the KL estimate reads them)");
    if (!finite_non_negative(scale)) return fail(GYMRS_EINVAL, who + ": scale must be finite and >= 0");
    if (!finite_f(coef)) return fail(GYMRS_EINVAL, who + ": coef must be finite");
    if (kind == GYMRS_CARTPOLE)
        entropy_lane<4, 2>(hidden, scale, coef, weights, n_steps, x, actions, old_prob, q, excluded, sums, counts);
    else
        entropy_lane<2, 3>(hidden, scale, coef, weights, n_steps, x, actions, old_prob, q, excluded, sums, counts);
    return GYMRS_OK;
}

gymrs_status gymrs_entropy_gradient(gymrs_engine* e, const gymrs_entropy_desc* d)
{
    const RecordCall c{e, d, "gymrs_entropy_gradient"};
    if (gymrs_status st = c.prologue("gradients are")) return st;
    if (d->reserved != 0) return c.refuse("reserved must be 0");
    if (d->flags != 0) return c.refuse("unknown flag bits (flags must be 0)");
    if (gymrs_status st = check_policy_set(e, c.who)) return st;
    if (gymrs_status st = c.scale(d->scale)) return st;
    if (!finite_f(d->coef)) return c.refuse("coef must be finite");
    const gymrs_trajectory& rec = d->record;
    if (gymrs_status st = c.not_null({{rec.obs, "record.obs"}, {d->start_obs, "start_obs"}, {d->grad, "grad"}, {d->excluded, "excluded"}, {d->sums, "sums"}}))
        return st;
    if (d->old_prob)
        if (gymrs_status st = c.not_null({{rec.actions, "record.actions", " (the KL estimate reads them with old_prob)"}})) return st;
    const void* actions = d->old_prob ? rec.actions : nullptr;
    if (gymrs_status st = c.aligned({rec.obs, actions, d->start_obs, d->old_prob}, 16, "every row buffer must be 16-byte aligned")) return st;
    if (gymrs_status st = c.aligned({d->grad, d->excluded, d->sums, d->counts}, 8, "grad, excluded, sums and counts must be 8-byte aligned")) return st;
    if (gymrs_status st = c.lane_stride(rec.lane_stride)) return st;
    if (d->n_steps == 0) return GYMRS_OK;
    const EntropyArgs a{rec.obs, d->start_obs, static_cast<const uint8_t*>(actions), d->old_prob, reinterpret_cast<unsigned long long*>(d->grad),
                        reinterpret_cast<unsigned long long*>(d->excluded), reinterpret_cast<unsigned long long*>(d->sums),
                        reinterpret_cast<unsigned long long*>(d->counts), /*stride, n, gid0*/ rec.lane_stride, e->n, e->gid0, d->n_steps, d->scale, d->coef};
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(launch_entropy_gradient(e->kind, a, e->policy.args, e->stream));
    return GYMRS_OK;
}

// ---- value loss: the host-side lane and the launch (include/gymrs_amd.h, "Value loss") -----------------------------------------------
static_assert(sizeof(gymrs_value_desc) == 136 && sizeof(gymrs_normalize_desc) == 64 && sizeof(gymrs_advantage_stats) == 40, "descriptor sizes");

static bool value_clip_ok(float clip) { return clip > 0.0f && clip <= std::numeric_limits<float>::max(); } // (false for a NaN)

gymrs_status gymrs_value_lane(gymrs_env_kind kind, uint32_t hidden, float clip, const float* weights, uint32_t n_steps, const float* x,
                              const float* returns, const float* old_values, int64_t* q, uint64_t* excluded, int64_t sums[2], uint64_t counts[2],
                              float* values)
{
    const std::string who = "gymrs_value_lane";
    if (gymrs_status st = check_network(kind, hidden, who)) return st;
    if (!weights || !q || !excluded || (n_steps != 0 && (!x || !returns))) return fail(GYMRS_EINVAL, who + ": NULL argument");
    if (old_values && !value_clip_ok(clip)) return fail(GYMRS_EINVAL, who + ": clip must be finite and > 0 with old_values");
    if (kind == GYMRS_CARTPOLE)
        value_lane<4>(hidden, clip, weights, n_steps, x, returns, old_values, q, excluded, sums, counts, values);
    else
        value_lane<2>(hidden, clip, weights, n_steps, x, returns, old_values, q, excluded, sums, counts, values);
    return GYMRS_OK;
}

gymrs_status gymrs_value_gradient(gymrs_engine* e, const gymrs_value_desc* d)
{
    const RecordCall c{e, d, "gymrs_value_gradient"};
    if (gymrs_status st = c.prologue("gradients are")) return st;
    if (d->reserved != 0 || d->pad_ != 0) return c.refuse("reserved and pad_ must be 0");
    if (d->flags & ~GYMRS_VALUE_CLIP) return c.refuse("unknown flag bits (GYMRS_VALUE_CLIP is the only one)");
    const bool clipped = (d->flags & GYMRS_VALUE_CLIP) != 0;
    if (!e->critic.dev) return c.refuse("the engine has no critic set (gymrs_set_critic)");
    if (clipped && !value_clip_ok(d->clip)) return c.refuse("clip must be finite and > 0 with GYMRS_VALUE_CLIP");
    const gymrs_trajectory& rec = d->record;
    if (gymrs_status st = c.not_null({{rec.obs, "record.obs"}, {d->start_obs, "start_obs"}, {d->returns, "returns"}, {d->grad, "grad"},
                                      {d->excluded, "excluded"}}))
        return st;
    if (clipped)
        if (gymrs_status st = c.not_null({{d->old_values, "old_values", " (GYMRS_VALUE_CLIP reads it)"}})) return st;
    if (!clipped && d->old_values) return c.refuse("old_values without GYMRS_VALUE_CLIP");
    if (d->values && (d->values == d->returns || d->values == d->old_values)) return c.refuse("values may not alias returns or old_values");
    if (gymrs_status st = c.aligned({rec.obs, d->start_obs, d->returns, d->old_values, d->values}, 16, "every row buffer must be 16-byte aligned")) return st;
    if (gymrs_status st = c.aligned({d->grad, d->excluded, d->sums, d->counts}, 8, "grad, excluded, sums and counts must be 8-byte aligned")) return st;
    if (gymrs_status st = c.lane_stride(rec.lane_stride)) return st;
    if (d->n_steps == 0) return GYMRS_OK;
    HIP_TRY(hipSetDevice(e->device));
    float* v_row = d->values;
    if (!v_row && e->critic.args.hidden != 0) { // the chunks of hidden units read V from a row: the engine's
        const uint64_t need = (uint64_t)d->n_steps * rec.lane_stride;
        if (need > e->value_scratch_floats) { // (launches already enqueued still use the old one: wait for them)
            HIP_TRY(hipStreamSynchronize(e->stream));
            HIP_TRY(hipFree(e->value_scratch));
            e->value_scratch = nullptr;
            e->value_scratch_floats = 0;
            HIP_TRY(hipMalloc(&e->value_scratch, (size_t)need * sizeof(float)));
            e->value_scratch_floats = need;
        }
        v_row = e->value_scratch;
    }
    const ValueArgs a{rec.obs, d->start_obs, d->returns, d->old_values, v_row, reinterpret_cast<unsigned long long*>(d->grad),
                      reinterpret_cast<unsigned long long*>(d->excluded), reinterpret_cast<unsigned long long*>(d->sums),
                      reinterpret_cast<unsigned long long*>(d->counts), /*stride, n, gid0*/ rec.lane_stride, e->n, e->gid0, d->n_steps, d->clip};
    HIP_TRY(launch_value_gradient(e->kind, a, e->critic.args, e->stream));
    return GYMRS_OK;
}

// ---- advantage normalisation: the host-side set and the launch (include/gymrs_amd.h, "Advantage normalisation") ------------------------
static bool normalize_eps_ok(float eps) { return eps > 0.0f && eps <= std::numeric_limits<float>::max(); } // (false for a NaN)

gymrs_status gymrs_normalize_host(const float* a, uint64_t count, float eps, float* out, gymrs_advantage_stats* st)
{
    const std::string who = "gymrs_normalize_host";
    if (!st || (count != 0 && (!a || !out))) return fail(GYMRS_EINVAL, who + ": NULL argument");
    if (!normalize_eps_ok(eps)) return fail(GYMRS_EINVAL, who + ": eps must be finite and > 0");
    unsigned long long s1 = 0, s2 = 0, n = 0, non_members = 0; // modulo 2^64, as the device adds
    for (uint64_t j = 0; j < count; ++j) {
        if (normalize_member(a[j])) {
            s1 += (unsigned long long)normalize_q1(a[j]);
            n += 1;
        } else {
            non_members += 1;
        }
    }
    const float mean = normalize_mean((long long)s1, n);
    for (uint64_t j = 0; j < count; ++j)
        if (normalize_member(a[j])) s2 += normalize_q2(a[j], mean);
    const float inv = normalize_inv(s2, n, eps);
    for (uint64_t j = 0; j < count; ++j) out[j] = normalize_out(a[j], mean, inv);
    *st = gymrs_advantage_stats{(long long)s1, n, s2, non_members, mean, inv};
    return GYMRS_OK;
}

gymrs_status gymrs_normalize_advantages(gymrs_engine* e, const gymrs_normalize_desc* d)
{
    const RecordCall c{e, d, "gymrs_normalize_advantages"};
    if (!e) return c.refuse("NULL engine");
    if (!d) return c.refuse("NULL desc");
    if (d->reserved != 0) return c.refuse("reserved must be 0");
    if (d->flags != 0) return c.refuse("unknown flag bits (flags must be 0)");
    if (!normalize_eps_ok(d->eps)) return c.refuse("eps must be finite and > 0");
    if (d->n_sets == 0) return c.refuse("n_sets must be >= 1");
    if (d->lanes_per_policy == 0) return c.refuse("lanes_per_policy must be >= 1");
    if (gymrs_status st = c.not_null({{d->adv, "adv"}, {d->out, "out"}, {d->stats, "stats"}})) return st;
    if (gymrs_status st = c.aligned({d->adv, d->out}, 16, "adv and out must be 16-byte aligned")) return st;
    if (gymrs_status st = c.aligned({d->stats}, 8, "stats must be 8-byte aligned")) return st;
    if (gymrs_status st = c.lane_stride(d->lane_stride)) return st;
    if (d->n_steps == 0) return GYMRS_OK;
    const NormalizeArgs a{d->adv, d->out, d->stats, /*stride, n, gid0*/ d->lane_stride, e->n, e->gid0, d->lanes_per_policy, d->n_sets, d->n_steps, d->eps, 0};
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(launch_normalize(a, e->stream));
    return GYMRS_OK;
}

// ---- Q-learning: the target set, the host-side lane and the launch (include/gymrs_amd.h, "Q-learning") -----------------------------
gymrs_status gymrs_q_target_sync(gymrs_engine* e)
{
    const std::string who = "gymrs_q_target_sync";
    if (!e) return fail(GYMRS_EINVAL, who + ": NULL engine");
    if (gymrs_status st = check_discrete_env(e->kind, who)) return st;
    if (gymrs_status st = check_policy_set(e, who)) return st;
    const PolicyArgs& p = e->policy.args;
    const uint64_t total = (uint64_t)p.stride * p.n_policies;
    WeightSet& t = e->q_target;
    HIP_TRY(hipSetDevice(e->device));
    if (total > t.capacity) { // (a kept target has the policy's shape: only a first use gets here)
        if (gymrs_status st = discard_q_target(e)) return st;
        HIP_TRY(hipMalloc(&t.dev, (size_t)total * sizeof(float)));
        t.capacity = total;
    }
    // stream-ordered, device to device: launches enqueued before this call read the old target
    HIP_TRY(hipMemcpyAsync(t.dev, e->policy.dev, (size_t)total * sizeof(float), hipMemcpyDeviceToDevice, e->stream));
    t.args = p;
    t.args.weights = t.dev;
    return GYMRS_OK;
}

gymrs_status gymrs_q_target_ptr(gymrs_engine* e, float** dev_out, uint64_t* n_floats)
{
    const std::string who = "gymrs_q_target_ptr";
    if (!e || !dev_out) return fail(GYMRS_EINVAL, who + ": NULL argument");
    if (gymrs_status st = check_discrete_env(e->kind, who)) return st;
    if (gymrs_status st = check_policy_set(e, who)) return st;
    if (!e->q_target.dev) return fail(GYMRS_EINVAL, who + ": the engine has no target set (gymrs_q_target_sync)");
    *dev_out = e->q_target.dev;
    if (n_floats) *n_floats = (uint64_t)e->q_target.args.stride * e->q_target.args.n_policies;
    return GYMRS_OK;
}

gymrs_status gymrs_q_lane(gymrs_env_kind kind, uint32_t hidden, uint32_t flags, float gamma, float kappa, const float* weights,
                          const float* target_weights, uint32_t n_steps, const float* x, const float* x_next, const uint8_t* actions,
                          const float* reward, const uint8_t* done, int64_t* q, uint64_t* excluded, float* td, uint64_t* counts)
{
    const std::string who = "gymrs_q_lane";
    if (gymrs_status st = check_network(kind, hidden, who)) return st;
    if (flags & ~GYMRS_Q_DOUBLE) return fail(GYMRS_EINVAL, who + ": unknown flag bits (GYMRS_Q_DOUBLE is the only one)");
    if (!weights || !target_weights || !q || !excluded || (n_steps != 0 && (!x || !x_next || !actions || !reward || !done)))
        return fail(GYMRS_EINVAL, who + ": NULL argument");
    if (!q_gamma_ok(gamma)) return fail(GYMRS_EINVAL, who + ": gamma must be in [0, 1]");
    if (!q_kappa_ok(kappa)) return fail(GYMRS_EINVAL, who + ": kappa must be > 0 (+inf is the squared loss)");
    if (kind == GYMRS_CARTPOLE)
        q_lane<4, 2>(hidden, flags, gamma, kappa, weights, target_weights, n_steps, x, x_next, actions, reward, done, q, excluded, td, counts);
    else
        q_lane<2, 3>(hidden, flags, gamma, kappa, weights, target_weights, n_steps, x, x_next, actions, reward, done, q, excluded, td, counts);
    return GYMRS_OK;
}

gymrs_status gymrs_q_gradient(gymrs_engine* e, const gymrs_q_desc* d)
{
    const RecordCall c{e, d, "gymrs_q_gradient"};
    if (gymrs_status st = c.prologue("Q-gradients are")) return st;
    if (d->reserved != 0) return c.refuse("reserved must be 0");
    if (d->flags & ~GYMRS_Q_DOUBLE) return c.refuse("unknown flag bits (GYMRS_Q_DOUBLE is the only one)");
    if (gymrs_status st = check_policy_set(e, c.who)) return st;
    if (!e->q_target.dev) return c.refuse("the engine has no target set (gymrs_q_target_sync)");
    if (!q_gamma_ok(d->gamma)) return c.refuse("gamma must be in [0, 1]");
    if (!q_kappa_ok(d->kappa)) return c.refuse("kappa must be > 0 (+inf is the squared loss)");
    const gymrs_trajectory& rec = d->record;
    if (gymrs_status st = c.not_null({{rec.obs, "record.obs"}, {rec.actions, "record.actions"}, {rec.reward, "record.reward"}, {rec.done, "record.done"},
                                      {d->start_obs, "start_obs"}, {d->final_obs, "final_obs"}, {d->td, "td"}, {d->grad, "grad"},
                                      {d->excluded, "excluded"}}))
        return st;
    for (const void* in : {(const void*)rec.obs, (const void*)rec.actions, (const void*)rec.reward, (const void*)rec.done, (const void*)rec.truncated,
                           (const void*)d->start_obs, (const void*)d->final_obs})
        if (in == d->td) return c.refuse("td may not alias an input row");
    if (gymrs_status st = c.aligned({rec.obs, rec.actions, rec.reward, rec.done, rec.truncated, d->start_obs, d->final_obs, d->td}, 16,
                                    "every row buffer must be 16-byte aligned"))
        return st;
    if (gymrs_status st = c.aligned({d->grad, d->excluded, d->counts}, 8, "grad, excluded and counts must be 8-byte aligned")) return st;
    if (gymrs_status st = c.lane_stride(rec.lane_stride)) return st;
    if (d->n_steps == 0) return GYMRS_OK;
    const QArgs a{rec.obs, static_cast<const uint8_t*>(rec.actions), rec.reward, rec.done, rec.truncated, d->final_obs, d->start_obs, d->td,
                  reinterpret_cast<unsigned long long*>(d->grad), reinterpret_cast<unsigned long long*>(d->excluded),
                  reinterpret_cast<unsigned long long*>(d->counts), /*stride, n, gid0*/ rec.lane_stride, e->n, e->gid0, d->n_steps, d->flags, d->gamma,
                  d->kappa};
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(launch_q_gradient(e->kind, a, e->policy.args, e->q_target.args, e->stream));
    return GYMRS_OK;
}

// ---- prioritized replay: the checks, the host-only rules and the launches (include/gymrs_amd.h, "Replay") --------------------------
// What the three calls refuse in a store.  `rows`: the call reads or writes the transitions, not the priorities alone.
static gymrs_status check_replay_store(const RecordCall& c, const gymrs_replay& st, bool rows)
{
    if (rows)
        if (gymrs_status s = c.not_null({{st.s, "store.s"}, {st.s_next, "store.s_next"}, {st.action, "store.action"}, {st.reward, "store.reward"},
                                         {st.done, "store.done"}}))
            return s;
    if (gymrs_status s = c.not_null({{st.priority, "store.priority"}})) return s;
    if (st.capacity < 16 || st.capacity > kReplayMaxCapacity || st.capacity % 16 != 0)
        return c.refuse("store.capacity must be a multiple of 16 in 16 .. 2^26");
    if (rows) {
        if (gymrs_status s = c.aligned({st.s, st.s_next, st.reward, st.priority}, 16, "store.s, s_next, reward and priority must be 16-byte aligned")) return s;
        if (gymrs_status s = c.aligned({st.action, st.done}, 4, "store.action and done must be 4-byte aligned")) return s;
    }
    return c.aligned({st.priority}, 4, "store.priority must be 4-byte aligned");
}

static ReplayStore replay_store(const gymrs_replay& st) { return ReplayStore{st.s, st.s_next, st.action, st.reward, st.done, st.priority, st.capacity}; }

gymrs_status gymrs_replay_priority(float td, float alpha, float eps, float cap, uint32_t* out)
{
    const std::string who = "gymrs_replay_priority";
    if (!out) return fail(GYMRS_EINVAL, who + ": NULL argument");
    if (!replay_rule_ok(alpha, eps, cap)) return fail(GYMRS_EINVAL, who + ": needs 2^-126 <= eps <= cap < inf and 0 <= alpha <= 1");
    *out = replay_priority(td, alpha, eps, cap);
    return GYMRS_OK;
}

gymrs_status gymrs_replay_draw(const uint32_t* priority, uint64_t count, uint32_t n_samples, uint64_t seed, uint64_t draw, uint32_t* idx, uint64_t* total)
{
    const std::string who = "gymrs_replay_draw";
    if (!priority || !idx) return fail(GYMRS_EINVAL, who + ": NULL argument");
    if (count == 0 || count > kReplayMaxCapacity) return fail(GYMRS_EINVAL, who + ": count must be in 1 .. 2^26");
    if (n_samples == 0 || n_samples > kReplayMaxSamples) return fail(GYMRS_EINVAL, who + ": n_samples must be in 1 .. 2^24");
    replay_draw_host(priority, count, n_samples, seed, draw, idx, total);
    return GYMRS_OK;
}

gymrs_status gymrs_replay_push(gymrs_engine* e, const gymrs_replay_push_desc* d)
{
    const RecordCall c{e, d, "gymrs_replay_push"};
    if (gymrs_status st = c.prologue("replay stores are")) return st;
    if (d->reserved != 0 || d->pad_ != 0) return c.refuse("reserved must be 0");
    if (d->flags != 0) return c.refuse("unknown flag bits (flags must be 0)");
    const gymrs_trajectory& rec = d->record;
    if (gymrs_status st = c.not_null({{rec.obs, "record.obs"}, {rec.actions, "record.actions"}, {rec.reward, "record.reward"}, {rec.done, "record.done"},
                                      {d->start_obs, "start_obs"}, {d->final_obs, "final_obs"}}))
        return st;
    if (gymrs_status st = check_replay_store(c, d->store, true)) return st;
    if (gymrs_status st = c.aligned({rec.obs, rec.actions, rec.reward, rec.done, rec.truncated, d->start_obs, d->final_obs}, 16,
                                    "every row buffer must be 16-byte aligned"))
        return st;
    if (gymrs_status st = c.lane_stride(rec.lane_stride)) return st;
    if (d->head >= d->store.capacity) return c.refuse("head must be below store.capacity");
    if (e->n > d->store.capacity || d->n_steps > d->store.capacity / e->n) return c.refuse("n_steps * n_envs must not exceed store.capacity");
    if (d->priority > kReplayMaxPriority) return c.refuse("priority must be <= 2^24");
    if (d->n_steps == 0) return GYMRS_OK;
    const ReplayPushArgs a{replay_store(d->store), rec.obs, static_cast<const uint8_t*>(rec.actions), rec.reward, rec.done, rec.truncated, d->start_obs,
                           d->final_obs, /*stride, n, head*/ rec.lane_stride, e->n, d->head, d->n_steps, d->priority};
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(launch_replay_push(e->kind, a, e->stream));
    return GYMRS_OK;
}

gymrs_status gymrs_replay_sample(gymrs_engine* e, const gymrs_replay_sample_desc* d)
{
    const RecordCall c{e, d, "gymrs_replay_sample"};
    if (gymrs_status st = c.prologue("replay stores are")) return st;
    if (d->reserved != 0) return c.refuse("reserved must be 0");
    if (d->flags != 0) return c.refuse("unknown flag bits (flags must be 0)");
    const gymrs_trajectory& b = d->batch;
    if (gymrs_status st = c.not_null({{b.obs, "batch.obs"}, {b.actions, "batch.actions"}, {b.reward, "batch.reward"}, {b.done, "batch.done"},
                                      {d->start_obs, "start_obs"}, {d->idx, "idx"}, {d->total, "total"}}))
        return st;
    if (gymrs_status st = check_replay_store(c, d->store, true)) return st;
    if (d->count == 0 || d->count > d->store.capacity) return c.refuse("count must be in 1 .. store.capacity");
    if (d->n_samples == 0 || d->n_samples > kReplayMaxSamples) return c.refuse("n_samples must be in 1 .. 2^24");
    if (gymrs_status st = c.aligned({b.obs, b.actions, b.reward, b.done, d->start_obs}, 16, "every row buffer must be 16-byte aligned")) return st;
    if (gymrs_status st = c.aligned({d->idx, d->prio}, 4, "idx and prio must be 4-byte aligned")) return st;
    if (gymrs_status st = c.aligned({d->total}, 8, "total must be 8-byte aligned")) return st;
    if (b.lane_stride < d->n_samples || b.lane_stride % 16 != 0) return c.refuse("batch.lane_stride must be >= n_samples and a multiple of 16");
    HIP_TRY(hipSetDevice(e->device));
    if (d->store.capacity > kReplayTile && !e->replay_scratch) HIP_TRY(hipMalloc(&e->replay_scratch, kReplayScratchBytes)); // (a store of one tile needs none)
    const ReplaySampleArgs a{replay_store(d->store), d->count, d->seed, d->draw, b.obs, static_cast<uint8_t*>(b.actions), b.reward, b.done, d->start_obs,
                             d->idx, d->prio, reinterpret_cast<unsigned long long*>(d->total),
                             d->store.capacity > kReplayTile ? static_cast<unsigned long long*>(e->replay_scratch) : nullptr, b.lane_stride, d->n_samples};
    HIP_TRY(launch_replay_sample(e->kind, a, e->stream));
    return GYMRS_OK;
}

gymrs_status gymrs_replay_update(gymrs_engine* e, const gymrs_replay_update_desc* d)
{
    const RecordCall c{e, d, "gymrs_replay_update"};
    if (gymrs_status st = c.prologue("replay stores are")) return st;
    if (d->reserved != 0 || f2u(d->pad_) != 0) return c.refuse("reserved must be 0");
    if (d->flags != 0) return c.refuse("unknown flag bits (flags must be 0)");
    if (gymrs_status st = c.not_null({{d->idx, "idx"}, {d->td, "td"}})) return st;
    if (gymrs_status st = check_replay_store(c, d->store, false)) return st;
    if (d->n_samples > kReplayMaxSamples) return c.refuse("n_samples must be <= 2^24");
    if (gymrs_status st = c.aligned({d->idx, d->td}, 4, "idx and td must be 4-byte aligned")) return st;
    if (!replay_rule_ok(d->alpha, d->eps, d->cap)) return c.refuse("needs 2^-126 <= eps <= cap < inf and 0 <= alpha <= 1");
    const ReplayUpdateArgs a{d->store.priority, d->store.capacity, d->idx, d->td, d->n_samples, d->alpha, d->eps, d->cap};
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(launch_replay_update(a, e->stream));
    return GYMRS_OK;
}

// ---- the optimizer: the checks, the host-side set and the launch (include/gymrs_amd.h, "Optimizer") -------------------------------
// What gymrs_apply_gradient and gymrs_optimizer_set refuse in the values of a descriptor.
static gymrs_status check_optimizer_values(const gymrs_optimizer_desc* d, const std::string& who)
{
    if (d->kind != GYMRS_OPT_SGD && d->kind != GYMRS_OPT_ADAM) return fail(GYMRS_EINVAL, who + ": unknown kind (GYMRS_OPT_SGD or GYMRS_OPT_ADAM)");
    if (d->flags & ~(GYMRS_OPT_ASCEND | GYMRS_OPT_ZERO_GRAD))
        return fail(GYMRS_EINVAL, who + ": unknown flag bits (GYMRS_OPT_ASCEND and GYMRS_OPT_ZERO_GRAD are the only ones)");
    if (d->reserved != 0) return fail(GYMRS_EINVAL, who + ": reserved must be 0");
    if (!finite_f(d->lr)) return fail(GYMRS_EINVAL, who + ": lr must be finite");
    if (!finite_f(d->grad_scale)) return fail(GYMRS_EINVAL, who + ": grad_scale must be finite");
    if (!finite_non_negative(d->eps)) return fail(GYMRS_EINVAL, who + ": eps must be finite and >= 0");
    if (!(d->beta1 >= 0.0f && d->beta1 < 1.0f)) return fail(GYMRS_EINVAL, who + ": beta1 must be in [0, 1)");
    if (!(d->beta2 >= 0.0f && d->beta2 < 1.0f)) return fail(GYMRS_EINVAL, who + ": beta2 must be in [0, 1)");
    if (!(d->max_norm > 0.0f)) return fail(GYMRS_EINVAL, who + ": max_norm must be > 0 (+inf turns the clip off)");
    if (!(d->tau >= 0.0f && d->tau <= 1.0f)) return fail(GYMRS_EINVAL, who + ": tau must be in [0, 1]");
    return GYMRS_OK;
}

static gymrs_status check_optimizer_head(const gymrs_engine* e, uint32_t head, const std::string& who)
{
    if (gymrs_status st = check_discrete_env(e->kind, who)) return st;
    if (head != GYMRS_OPT_HEAD_POLICY && head != GYMRS_OPT_HEAD_CRITIC)
        return fail(GYMRS_EINVAL, who + ": unknown head (GYMRS_OPT_HEAD_POLICY or GYMRS_OPT_HEAD_CRITIC)");
    return GYMRS_OK;
}

gymrs_status gymrs_optimizer_set(const gymrs_optimizer_desc* d, uint64_t n_params, const int64_t* q, float* w, float* m, float* v, float* pw,
                                 float* target)
{
    const std::string who = "gymrs_optimizer_set";
    if (!d || !q || !w) return fail(GYMRS_EINVAL, who + ": NULL argument");
    if (n_params == 0) return fail(GYMRS_EINVAL, who + ": n_params must be >= 1");
    if (gymrs_status st = check_optimizer_values(d, who)) return st;
    const bool adam = d->kind == GYMRS_OPT_ADAM, ascend = (d->flags & GYMRS_OPT_ASCEND) != 0;
    if (adam && (!m || !v || !pw)) return fail(GYMRS_EINVAL, who + ": GYMRS_OPT_ADAM needs m, v and pw");
    if (d->tau > 0.0f && !target) return fail(GYMRS_EINVAL, who + ": tau > 0 needs target");
    std::vector<float> g(n_params);
    for (uint64_t s = 0; s < n_params; ++s) g[s] = opt_gradient(q[s], d->grad_scale);
    if (d->max_norm < std::numeric_limits<float>::infinity()) { // the 64 slots and the butterfly, as written
        double slot[64], next[64];
        for (uint64_t l = 0; l < 64; ++l) {
            slot[l] = 0.0;
            for (uint64_t s = l; s < n_params; s += 64) slot[l] = slot[l] + opt_square(g[s]);
        }
        for (int mask = 32; mask >= 1; mask >>= 1) {
            for (int l = 0; l < 64; ++l) next[l] = slot[l] + slot[l ^ mask];
            std::copy(next, next + 64, slot);
        }
        bool clipped;
        const float cs = opt_clip_scale(slot[0], d->max_norm, clipped);
        if (clipped)
            for (uint64_t s = 0; s < n_params; ++s) g[s] = g[s] * cs;
    }
    float c1 = 1.0f, c2 = 1.0f;
    if (adam) opt_adam_advance(d->beta1, d->beta2, pw[0], pw[1], c1, c2);
    for (uint64_t s = 0; s < n_params; ++s) {
        const float step = adam ? opt_adam_step(g[s], d->lr, d->beta1, d->beta2, d->eps, c1, c2, m[s], v[s]) : opt_sgd_step(g[s], d->lr);
        w[s] = opt_apply(w[s], step, ascend);
        if (d->tau > 0.0f) target[s] = opt_target(d->tau, w[s], target[s]);
    }
    return GYMRS_OK;
}

gymrs_status gymrs_apply_gradient(gymrs_engine* e, const gymrs_optimizer_desc* d)
{
    const std::string who = "gymrs_apply_gradient";
    if (!e) return fail(GYMRS_EINVAL, who + ": NULL engine");
    if (!d) return fail(GYMRS_EINVAL, who + ": NULL desc");
    if (gymrs_status st = check_optimizer_head(e, d->head, who)) return st;
    if (gymrs_status st = check_optimizer_values(d, who)) return st;
    const bool critic = d->head == GYMRS_OPT_HEAD_CRITIC;
    const WeightSet& set = critic ? e->critic : e->policy;
    if (gymrs_status st = check_weight_set(set, critic ? "critic" : "policy", who)) return st;
    if (d->tau > 0.0f) {
        if (critic) return fail(GYMRS_EINVAL, who + ": tau > 0 is for the policy head (the critic has no target set)");
        if (!e->q_target.dev) return fail(GYMRS_EINVAL, who + ": tau > 0 but the engine has no target set (gymrs_q_target_sync)");
    }
    if (!d->grad) return fail(GYMRS_EINVAL, who + ": grad is NULL");
    if (!d->excluded) return fail(GYMRS_EINVAL, who + ": excluded is NULL");
    for (const void* p : {(const void*)d->grad, (const void*)d->excluded, (const void*)d->skipped})
        if (reinterpret_cast<uintptr_t>(p) % 8 != 0) return fail(GYMRS_EINVAL, who + ": grad, excluded and skipped must be 8-byte aligned");
    if (set.args.stride > kMaxOptimizerParams) return fail(GYMRS_EINVAL, who + ": the set has more parameters per network than the kernel holds");
    const bool adam = d->kind == GYMRS_OPT_ADAM;
    if (adam)
        if (gymrs_status st = opt_state_of(e, d->head, set)) return st;
    const OptimizerState& state = e->opt_state[d->head];
    const OptimizerArgs a{set.dev,
                          adam ? state.m() : nullptr,
                          adam ? state.v() : nullptr,
                          adam ? state.pw() : nullptr,
                          d->tau > 0.0f ? e->q_target.dev : nullptr,
                          reinterpret_cast<unsigned long long*>(d->grad),
                          reinterpret_cast<unsigned long long*>(d->excluded),
                          reinterpret_cast<unsigned long long*>(d->skipped),
                          set.args.n_policies,
                          set.args.stride,
                          d->kind,
                          d->flags,
                          d->lr,
                          d->grad_scale,
                          d->beta1,
                          d->beta2,
                          d->eps,
                          d->max_norm,
                          d->tau};
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(launch_apply_gradient(a, e->stream));
    return GYMRS_OK;
}

gymrs_status gymrs_optimizer_reset(gymrs_engine* e, uint32_t head)
{
    const std::string who = "gymrs_optimizer_reset";
    if (!e) return fail(GYMRS_EINVAL, who + ": NULL engine");
    if (gymrs_status st = check_optimizer_head(e, head, who)) return st;
    const OptimizerState& state = e->opt_state[head];
    if (!state.dev) return GYMRS_OK; // fresh already
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(launch_optimizer_fresh(state.m(), state.v(), state.pw(), state.shape.n_policies, state.shape.stride, e->stream));
    return GYMRS_OK;
}

gymrs_status gymrs_get_optimizer_state(gymrs_engine* e, uint32_t head, float* m_out, float* v_out, float* pw_out)
{
    const std::string who = "gymrs_get_optimizer_state";
    if (!e) return fail(GYMRS_EINVAL, who + ": NULL engine");
    if (gymrs_status st = check_optimizer_head(e, head, who)) return st;
    const OptimizerState& state = e->opt_state[head];
    if (!state.dev) return fail(GYMRS_EINVAL, who + ": the head has no optimizer state (gymrs_apply_gradient with GYMRS_OPT_ADAM)");
    HIP_TRY(hipSetDevice(e->device));
    const size_t bytes = (size_t)state.words() * sizeof(float);
    if (m_out) HIP_TRY(hipMemcpyAsync(m_out, state.m(), bytes, hipMemcpyDeviceToHost, e->stream));
    if (v_out) HIP_TRY(hipMemcpyAsync(v_out, state.v(), bytes, hipMemcpyDeviceToHost, e->stream));
    if (pw_out) HIP_TRY(hipMemcpyAsync(pw_out, state.pw(), (size_t)state.shape.n_policies * 2 * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    return stream_sync_checked(e);
}

// ---- evolution strategies: the state, the step and the host-only definitions (include/gymrs_amd.h, "Evolution strategies") -----------
gymrs_status gymrs_es_init(gymrs_engine* e, const gymrs_es_desc* d, const float* centre_host)
{
    const std::string who = "gymrs_es_init";
    if (!e) return fail(GYMRS_EINVAL, who + ": NULL engine");
    if (!d) return fail(GYMRS_EINVAL, who + ": NULL desc");
    if (gymrs_status st = check_network(e->kind, d->hidden, who)) return st;
    if (d->n_policies < 2 || d->n_policies % 2 != 0 || d->n_policies > kEsMaxPolicies)
        return fail(GYMRS_EINVAL, who + ": n_policies must be even, >= 2 and <= GYMRS_ES_MAX_POLICIES (antithetic pairs)");
    if (d->lanes_per_policy == 0) return fail(GYMRS_EINVAL, who + ": lanes_per_policy must be >= 1");
    if (!es_sigma_ok(d->sigma)) return fail(GYMRS_EINVAL, who + ": sigma must be finite and > 0");
    if (d->reserved != 0) return fail(GYMRS_EINVAL, who + ": reserved must be 0");
    if (!centre_host) return fail(GYMRS_EINVAL, who + ": centre_host is NULL");
    const gymrs_policy_desc pd{d->hidden, d->n_policies, d->lanes_per_policy};
    if (policy_floats(e->kind, d->hidden) > kEsSlots) return fail(GYMRS_EINVAL, who + ": the network has more parameters than the kernels hold");
    if (!es_fits(e, &pd))
        if (gymrs_status st = discard_es(e)) return st;
    if (gymrs_status st = replace_policy_set(e, &pd, nullptr)) return st; // the weights: written below, on the device
    if (gymrs_status st = es_state_for(e)) return st;
    EsState& es = e->es;
    es.shape = e->policy.args;
    es.seed = d->seed;
    es.gen = 0;
    es.sigma = d->sigma;
    es.evaluated = false;
    // the centre is consumed before the call returns: the one wait of this call
    HIP_TRY(hipMemcpyAsync(&es.dev->theta[0][0], centre_host, (size_t)es.shape.stride * sizeof(float), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(launch_es_init(es_args(e), e->stream));
    return GYMRS_OK;
}

gymrs_status gymrs_es_step(gymrs_engine* e, const gymrs_es_step_desc* d)
{
    const std::string who = "gymrs_es_step";
    if (!e) return fail(GYMRS_EINVAL, who + ": NULL engine");
    if (!d) return fail(GYMRS_EINVAL, who + ": NULL desc");
    if (gymrs_status st = check_discrete_env(e->kind, who)) return st;
    if (d->flags & ~GYMRS_OPT_ASCEND) return fail(GYMRS_EINVAL, who + ": unknown flag bits (GYMRS_OPT_ASCEND is the only one)");
    gymrs_optimizer_desc od;
    std::memset(&od, 0, sizeof(od));
    od.kind = d->kind, od.flags = d->flags, od.lr = d->lr, od.grad_scale = d->grad_scale, od.beta1 = d->beta1, od.beta2 = d->beta2;
    od.eps = d->eps, od.max_norm = d->max_norm, od.reserved = d->reserved;
    if (gymrs_status st = check_optimizer_values(&od, who)) return st;
    if (d->sigma_next != 0.0f && !es_sigma_ok(d->sigma_next))
        return fail(GYMRS_EINVAL, who + ": sigma_next must be 0 (sigma stays) or finite and > 0");
    if (reinterpret_cast<uintptr_t>(d->utilities) % alignof(float) != 0) return fail(GYMRS_EINVAL, who + ": utilities must be 4-byte aligned");
    if (reinterpret_cast<uintptr_t>(d->skipped) % 8 != 0) return fail(GYMRS_EINVAL, who + ": skipped must be 8-byte aligned");
    EsState& es = e->es;
    if (!es.dev || !e->policy.dev) return fail(GYMRS_EINVAL, who + ": the engine has no evolution-strategies state (gymrs_es_init)");
    if (!d->utilities && !(es.evaluated && e->eval_dev))
        return fail(GYMRS_EINVAL, who + ": no evaluation ran since the population was written (gymrs_evaluate_policy), and no utilities were given");
    EsArgs a = es_args(e);
    a.records = d->utilities ? nullptr : e->eval_dev;
    a.u_in = d->utilities;
    a.skipped = reinterpret_cast<unsigned long long*>(d->skipped);
    a.kind = d->kind, a.flags = d->flags, a.lr = d->lr, a.grad_scale = d->grad_scale, a.beta1 = d->beta1, a.beta2 = d->beta2;
    a.eps = d->eps, a.max_norm = d->max_norm;
    if (d->sigma_next > 0.0f) a.sigma_new = d->sigma_next;
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(launch_es_step(a, e->stream));
    es.gen += 1; // the policy buffer holds the next generation (in stream order), which nothing has played yet
    es.sigma = a.sigma_new;
    es.evaluated = false;
    return GYMRS_OK;
}

gymrs_status gymrs_get_es(gymrs_engine* e, gymrs_es_desc* d_out, uint64_t* generation, float* centre_out, uint64_t capacity_floats)
{
    const std::string who = "gymrs_get_es";
    if (!e || !d_out) return fail(GYMRS_EINVAL, who + ": NULL argument");
    const EsState& es = e->es;
    if (!es.dev) return fail(GYMRS_EINVAL, who + ": the engine has no evolution-strategies state (gymrs_es_init)");
    *d_out = gymrs_es_desc{es.shape.hidden, es.shape.n_policies, es.shape.lanes_per_policy, es.seed, es.sigma, 0};
    if (generation) *generation = es.gen;
    if (!centre_out && capacity_floats == 0) return GYMRS_OK; // a query of the description
    if (!centre_out || capacity_floats < es.shape.stride) return fail(GYMRS_EINVAL, who + ": capacity_floats is smaller than the centre");
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipMemcpyAsync(centre_out, &es.dev->centre[0], (size_t)es.shape.stride * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    return stream_sync_checked(e);
}

gymrs_status gymrs_es_centre_ptr(gymrs_engine* e, float** dev_out, uint64_t* n_floats)
{
    const std::string who = "gymrs_es_centre_ptr";
    if (!e || !dev_out) return fail(GYMRS_EINVAL, who + ": NULL argument");
    if (!e->es.dev) return fail(GYMRS_EINVAL, who + ": the engine has no evolution-strategies state (gymrs_es_init)");
    *dev_out = &e->es.dev->centre[0];
    if (n_floats) *n_floats = e->es.shape.stride;
    return GYMRS_OK;
}

gymrs_status gymrs_es_utilities_ptr(gymrs_engine* e, float** dev_out, uint32_t* n_policies)
{
    const std::string who = "gymrs_es_utilities_ptr";
    if (!e || !dev_out) return fail(GYMRS_EINVAL, who + ": NULL argument");
    if (!e->es.dev) return fail(GYMRS_EINVAL, who + ": the engine has no evolution-strategies state (gymrs_es_init)");
    *dev_out = e->es.u;
    if (n_policies) *n_policies = e->es.shape.n_policies;
    return GYMRS_OK;
}

gymrs_status gymrs_get_es_optimizer_state(gymrs_engine* e, float* m_out, float* v_out, float* pw_out)
{
    const std::string who = "gymrs_get_es_optimizer_state";
    if (!e) return fail(GYMRS_EINVAL, who + ": NULL engine");
    const EsState& es = e->es;
    if (!es.dev) return fail(GYMRS_EINVAL, who + ": the engine has no evolution-strategies state (gymrs_es_init)");
    HIP_TRY(hipSetDevice(e->device));
    const uint32_t half = (uint32_t)es.gen & 1u; // the half the next step reads
    const size_t bytes = (size_t)es.shape.stride * sizeof(float);
    if (m_out) HIP_TRY(hipMemcpyAsync(m_out, &es.dev->m[half][0], bytes, hipMemcpyDeviceToHost, e->stream));
    if (v_out) HIP_TRY(hipMemcpyAsync(v_out, &es.dev->v[half][0], bytes, hipMemcpyDeviceToHost, e->stream));
    if (pw_out) HIP_TRY(hipMemcpyAsync(pw_out, &es.dev->pw[half][0], 2 * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    return stream_sync_checked(e);
}

gymrs_status gymrs_es_noise(uint64_t seed, uint64_t generation, uint64_t pair, uint32_t s, float* eps_out)
{
    if (!eps_out) return fail(GYMRS_EINVAL, "gymrs_es_noise: eps_out is NULL");
    if (s >= kEsSlots) return fail(GYMRS_EINVAL, "gymrs_es_noise: s must be < 512 (nine bits of the key)");
    *eps_out = es_noise(seed, generation, pair, s);
    return GYMRS_OK;
}

gymrs_status gymrs_es_utilities(const gymrs_policy_eval* records, uint32_t n_policies, float* u_out)
{
    const std::string who = "gymrs_es_utilities";
    if (!records || !u_out) return fail(GYMRS_EINVAL, who + ": NULL argument");
    if (n_policies == 0 || n_policies > kEsMaxPolicies) return fail(GYMRS_EINVAL, who + ": n_policies must be in 1 .. GYMRS_ES_MAX_POLICIES");
    const uint32_t P = n_policies;
    auto valid = [&](uint32_t p) { return records[p].episodes > 0; };
    auto F = [&](uint32_t p) { return es_fitness(records[p].return_sum, records[p].episodes); };
    const double total = es_sum(P, [&](uint32_t p) { return valid(p) ? F(p) : 0.0; });
    const double n_valid = es_sum(P, [&](uint32_t p) { return valid(p) ? 1.0 : 0.0; });
    const double mean = total / n_valid;
    const double total2 = es_sum(P, [&](uint32_t p) {
        const double dev = F(p) - mean;
        return valid(p) ? dev * dev : 0.0;
    });
    const double sd = es_sd(total2, n_valid);
    for (uint32_t p = 0; p < P; ++p) u_out[p] = es_utility(valid(p), valid(p) ? F(p) : 0.0, mean, sd);
    return GYMRS_OK;
}

gymrs_status gymrs_es_ranks(gymrs_engine* e, const gymrs_es_ranks_desc* d)
{
    const std::string who = "gymrs_es_ranks";
    if (!e) return fail(GYMRS_EINVAL, who + ": NULL engine");
    if (!d) return fail(GYMRS_EINVAL, who + ": NULL desc");
    if (gymrs_status st = check_discrete_env(e->kind, who)) return st;
    if (gymrs_status st = check_policy_set(e, who)) return st;
    if (d->flags != 0) return fail(GYMRS_EINVAL, who + ": unknown flag bits (flags must be 0)");
    if (d->reserved != 0) return fail(GYMRS_EINVAL, who + ": reserved must be 0");
    if (!d->utilities) return fail(GYMRS_EINVAL, who + ": utilities is NULL");
    if (reinterpret_cast<uintptr_t>(d->utilities) % alignof(float) != 0) return fail(GYMRS_EINVAL, who + ": utilities must be 4-byte aligned");
    if (reinterpret_cast<uintptr_t>(d->rank2) % alignof(uint32_t) != 0) return fail(GYMRS_EINVAL, who + ": rank2 must be 4-byte aligned");
    const uint32_t P = e->policy.args.n_policies;
    if (P > kEsMaxPolicies) return fail(GYMRS_EINVAL, who + ": the policy set has more than GYMRS_ES_MAX_POLICIES policies");
    if (!e->eval_dev) return fail(GYMRS_EINVAL, who + ": the engine has no evaluation table yet (gymrs_evaluate_policy)");
    HIP_TRY(hipSetDevice(e->device));
    EsRanksArgs a;
    std::memset(&a, 0, sizeof(a));
    a.records = e->eval_dev;
    a.u = d->utilities;
    a.rank2 = d->rank2;
    a.P = P;
    if (P > kEsRankTile) { // (a set of one tile is one launch and needs no scratch)
        if (!e->rank_scratch) HIP_TRY(hipMalloc(&e->rank_scratch, es_rank_scratch_bytes(P)));
        es_rank_scratch_rows(a, e->rank_scratch);
    }
    HIP_TRY(launch_es_ranks(a, e->stream));
    return GYMRS_OK;
}

gymrs_status gymrs_es_rank_utilities(const gymrs_policy_eval* records, uint32_t n_policies, float* u_out, uint32_t* rank2_out)
{
    const std::string who = "gymrs_es_rank_utilities";
    if (!records || !u_out) return fail(GYMRS_EINVAL, who + ": NULL argument");
    if (n_policies == 0 || n_policies > kEsMaxPolicies) return fail(GYMRS_EINVAL, who + ": n_policies must be in 1 .. GYMRS_ES_MAX_POLICIES");
    auto valid = [&](uint32_t p) { return records[p].episodes > 0; };
    auto F = [&](uint32_t p) { return es_fitness(records[p].return_sum, records[p].episodes); };
    std::vector<double> sorted;
    for (uint32_t p = 0; p < n_policies; ++p)
        if (valid(p)) sorted.push_back(F(p));
    std::sort(sorted.begin(), sorted.end()); // (no NaN among them: a strict weak order)
    const uint32_t n = (uint32_t)sorted.size();
    for (uint32_t p = 0; p < n_policies; ++p) {
        uint32_t rank2 = GYMRS_ES_RANK_INVALID;
        if (valid(p)) {
            const auto range = std::equal_range(sorted.begin(), sorted.end(), F(p));
            const uint32_t less = (uint32_t)(range.first - sorted.begin()), equal = (uint32_t)(range.second - range.first);
            rank2 = 2u * less + equal - 1u;
        }
        u_out[p] = es_rank_utility(valid(p), n, (long long)rank2 - (long long)(n - 1u));
        if (rank2_out) rank2_out[p] = rank2;
    }
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
    e->es.evaluated = true; // (an ES population, if that is the set: gymrs_es_step may read the table)
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
