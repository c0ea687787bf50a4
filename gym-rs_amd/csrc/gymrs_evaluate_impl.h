// gymrs_evaluate_impl.h -- the episodic evaluation kernel (gymrs_evaluate_policy, include/gymrs_amd.h "episodic policy
// evaluation"), gfx950: included by gymrs_evaluate.hip (the uniform envs) and by gymrs_table_<env>.hip (TableT: every lane plays
// with the parameter row gymrs_step would give it, GYMRS_EVAL_LANE_PARAMS).
// Every lane plays E whole episodes under its policy in ONE launch, and every policy gets exact episodic statistics.  Not
// rollout_block's shared step clock: a lane carries its own episode index and step count, records an episode the moment it ends
// and starts the next one at once; a wave leaves the loop as soon as none of its lanes has an episode left.  State, counters and
// accumulators live in registers: memory sees the weights (in), the optional per-episode lengths and, once per wave, the integer
// atomics of the records.  4 lanes per work-item.  Both envs pay a constant per step, so a return is +-L and everything is counted
// in integers of L.
#pragma once
#include "gymrs_evaluate.h"
#include "gymrs_policy.h"

namespace gymrs {

constexpr int kEvalVec = 4;

// One record's worth of accumulators, in episode lengths.  A lane plays at most E * M <= kMaxEvalSteps (2^24) steps, so 32 bits
// hold the steps, episodes and flags of a work-item's four lanes; the squares need 64.
struct EvalAcc {
    uint32_t steps = 0, episodes = 0, done = 0, trunc = 0, lmin = 0xffffffffu, lmax = 0;
    unsigned long long sq = 0;
    __device__ __forceinline__ void record(uint32_t len, bool dn, bool tr)
    {
        steps += len;
        sq += (unsigned long long)len * len;
        episodes += 1;
        done += dn ? 1u : 0u;
        trunc += tr ? 1u : 0u;
        lmin = min(lmin, len);
        lmax = max(lmax, len);
    }
    __device__ __forceinline__ void add(const EvalAcc& o)
    {
        steps += o.steps;
        sq += o.sq;
        episodes += o.episodes;
        done += o.done;
        trunc += o.trunc;
        lmin = min(lmin, o.lmin);
        lmax = max(lmax, o.lmax);
    }
};

// Adds what `episodes` (> 0) episodes of total length `steps` came to.  SIGN: the env's reward per step (+1 / -1).
template <int SIGN>
__device__ __forceinline__ void eval_commit(gymrs_policy_eval* rec, unsigned long long steps, unsigned long long sq, unsigned long long episodes,
                                            unsigned long long done, unsigned long long trunc, uint32_t lmin, uint32_t lmax)
{
    if (episodes == 0) return; // (the record keeps its identity)
    unsigned long long* w = reinterpret_cast<unsigned long long*>(rec); // {return_sum, return_sq_sum, episodes, done, truncated, steps, min, max}
    atomic_add_nonzero(w + 0, SIGN > 0 ? steps : 0ull - steps); // two's complement
    atomic_add_nonzero(w + 1, sq);
    atomic_add_nonzero(w + 2, episodes);
    atomic_add_nonzero(w + 3, done);
    atomic_add_nonzero(w + 4, trunc);
    atomic_add_nonzero(w + 5, steps);
    const long long lo = SIGN > 0 ? (long long)lmin : -(long long)lmax, hi = SIGN > 0 ? (long long)lmax : -(long long)lmin;
    (void)__hip_atomic_fetch_min(reinterpret_cast<long long*>(w + 6), lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    (void)__hip_atomic_fetch_max(reinterpret_cast<long long*>(w + 7), hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The episodes of the 4 lanes of a work-item.  UNI (wave-uniform): every lane of the wave plays pol[0] -- scalar weights, one
// accumulator set per work-item, a wave reduction at the end; else every lane gathers its own weights and keeps its own set.
// TableT: every lane fetches its row once (two dwordx4 gathers, the table sits in the L2) and keeps its constants in registers for
// all of its episodes; a lane whose index is not in the table plays nothing, like a lane beyond n.  Row and policy are
// independent: a wave that is uniform in its policy may mix rows.
template <class Env, bool UNI>
__device__ __forceinline__ void evaluate_lanes(const EvalArgs& a, const typename Env::Consts& c, const PolicyArgs& p, const uint32_t (&pol)[kEvalVec],
                                               uint64_t base)
{
    constexpr int V = kEvalVec, NS = Env::kState, NA = UNI ? 1 : V;
    constexpr int SIGN = Env::kReward > 0.0f ? 1 : -1;
    static_assert(Env::kConstReward && !Env::kNeverTerminates, "a return is +-length: CartPole and MountainCar");
    using Action = typename Env::Action;
    const PolicyWeights<V, UNI> W(p, pol);
    const uint32_t E = a.episodes, M = a.max_steps;

    Vec<float, V> st[NS]; // a parked lane (through with its episodes, or beyond n) holds zeros: inside the fast path's range
    uint32_t ep[V], len[V];
    uint64_t key[V]; // the global id in the key of the lane's reset draws
    EvalAcc acc[NA];
    const uint64_t g0 = a.gid0 + base;
    uint64_t r = (a.flags & GYMRS_EVAL_COMMON_STARTS) ? g0 % p.lanes_per_policy : 0;
    uint32_t need = 0; // bit k: lane k starts episode ep[k] and has not drawn its state yet
    [[maybe_unused]] typename TableLane<Env>::type lc[V];
    [[maybe_unused]] Vec<uint16_t, V> pidx;
    if constexpr (Env::kTable) {
        pidx = load_vec<uint16_t, V, false>(c.index, base, a.n, base + V <= a.n, uint16_t(0));
#pragma unroll
        for (int k = 0; k < V; ++k) lc[k] = Env::lane_consts(c, c.rows[pidx.v[k] < c.k ? pidx.v[k] : 0u]);
    }
#pragma unroll
    for (int k = 0; k < V; ++k) {
        if (a.flags & GYMRS_EVAL_COMMON_STARTS) {
            key[k] = r;
            if (++r == p.lanes_per_policy) r = 0;
        } else {
            key[k] = g0 + k;
        }
        bool live = base + k < a.n;
        if constexpr (Env::kTable) live = live && pidx.v[k] < c.k;
        ep[k] = live ? 0u : E;
        len[k] = 0;
        need |= live ? (1u << k) : 0u;
#pragma unroll
        for (int j = 0; j < NS; ++j) st[j].v[k] = 0.0f;
    }

    // A counted loop: a lane with an episode left steps on every trip and an episode takes at most M steps, so E * M trips see every
    // lane through.  The host refuses E * M > kMaxEvalSteps.
    const uint32_t trips = E * M;
    for (uint32_t t = 0;; ++t) {
        // ---- start states: one Philox block per pass serves whichever lane of the work-item needs one (inline, under the lane mask) ----
        while (need != 0) {
            const uint32_t s = (uint32_t)__builtin_ctz(need);
            need &= need - 1u;
            uint32_t e_s = ep[0];
            uint64_t k_s = key[0];
#pragma unroll
            for (int k = 1; k < V; ++k) {
                e_s = s == (uint32_t)k ? ep[k] : e_s;
                k_s = s == (uint32_t)k ? key[k] : k_s;
            }
            const u32x4 rnd = draw4(a.seed + e_s, k_s, 0, kStreamReset); // gymrs_reset(seed + ep): tick 0
            float ns[NS];
            Env::sample(rnd, a.box, ns);
#pragma unroll
            for (int k = 0; k < V; ++k) {
#pragma unroll
                for (int j = 0; j < NS; ++j) st[j].v[k] = s == (uint32_t)k ? ns[j] : st[j].v[k];
            }
        }
        bool busy = false;
#pragma unroll
        for (int k = 0; k < V; ++k) busy = busy || ep[k] < E;
        if (t >= trips || !__any(busy)) break; // wave-uniform

        // ---- action and physics of one step, as advance_tile does them ----
        Vec<Action, V> act;
        policy_eval<Env, V, UNI>(W, p.hidden, st, act);
        float ls[NS][V];
        Action la[V];
        uint32_t rkey = 0;
#pragma unroll
        for (int k = 0; k < V; ++k) {
            la[k] = act.v[k];
            float lane_st[NS];
#pragma unroll
            for (int j = 0; j < NS; ++j) lane_st[j] = ls[j][k] = st[j].v[k];
            const uint32_t kk = Env::range_key(lane_st);
            rkey = rkey > kk ? rkey : kk;
        }
        float rw[V];
        bool dn[V];
        if (__all(rkey <= Env::kRangeMax)) { // wave-uniform: the branch-free physics
            if constexpr (Env::kTable) {
                if (Env::kVariants == 1 || Env::variant(c) == 0)
                    advance_fast_rows<Env, V, 0>(lc, ls, la, rw, dn);
                else
                    advance_fast_rows<Env, V, 1>(lc, ls, la, rw, dn);
            } else {
                if (Env::kVariants == 1 || Env::variant(c) == 0)
                    advance_fast_all<Env, V, 0>(c, ls, la, rw, dn);
                else
                    advance_fast_all<Env, V, 1>(c, ls, la, rw, dn);
            }
        } else { // angles outside the fast range, NaN states
#pragma unroll
            for (int k = 0; k < V; ++k) {
                float lane_st[NS];
#pragma unroll
                for (int j = 0; j < NS; ++j) lane_st[j] = ls[j][k];
                if constexpr (Env::kTable)
                    Env::advance(lc[k], lane_st, la[k], rw[k], dn[k]);
                else
                    Env::advance(c, lane_st, la[k], rw[k], dn[k]);
#pragma unroll
                for (int j = 0; j < NS; ++j) ls[j][k] = lane_st[j];
            }
        }
        // ---- the lanes' own clocks ----
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const bool playing = ep[k] < E;
            const uint32_t l = len[k] + 1u;
            const bool tr = l == M;
            const bool ended = playing && (dn[k] || tr);
            if (ended) {
                acc[UNI ? 0 : k].record(l, dn[k], tr);
                if (a.lengths) a.lengths[(uint64_t)ep[k] * a.n + base + k] = l | (dn[k] ? 0x80000000u : 0u);
                ep[k] += 1u;
                need |= ep[k] < E ? (1u << k) : 0u;
            }
            len[k] = ended ? 0u : l;
            const bool keep = playing && !ended; // an ended lane draws afresh or parks; a parked lane stays where it is
#pragma unroll
            for (int j = 0; j < NS; ++j) st[j].v[k] = keep ? ls[j][k] : 0.0f;
        }
    }

    // ---- the records ----
    if constexpr (UNI) {
        const unsigned long long steps = wave_sum_u64(acc[0].steps), sq = wave_sum_u64(acc[0].sq), episodes = wave_sum_u64(acc[0].episodes),
                                 done = wave_sum_u64(acc[0].done), trunc = wave_sum_u64(acc[0].trunc);
        const uint32_t lmin = wave_min_u32(acc[0].lmin), lmax = wave_max_u32(acc[0].lmax);
        if ((threadIdx.x & 63u) == 0) eval_commit<SIGN>(a.table + __builtin_amdgcn_readfirstlane(pol[0]), steps, sq, episodes, done, trunc, lmin, lmax);
    } else {
        EvalAcc run;
#pragma unroll
        for (int k = 0; k < V; ++k) {
            run.add(acc[UNI ? 0 : k]);
            if (k + 1 == V || pol[k + 1] != pol[k]) { // consecutive lanes of one policy are added together (a lane beyond n played nothing)
                eval_commit<SIGN>(a.table + pol[k], run.steps, run.sq, run.episodes, run.done, run.trunc, run.lmin, run.lmax);
                run = EvalAcc();
            }
        }
    }
}

template <class Env>
__global__ __launch_bounds__(kBlock) void evaluate_policy_kernel(const EvalArgs a, const typename Env::Consts c, const PolicyArgs p)
{
    const uint64_t base = (uint64_t)blockIdx.x * (kBlock * kEvalVec) + (uint64_t)threadIdx.x * kEvalVec;
    uint32_t pol[kEvalVec];
    bool uniform;
    policy_select<kEvalVec>(p, a.gid0 + base, pol, uniform); // (every work-item of the wave is active: nothing returns early)
    if (uniform)
        evaluate_lanes<Env, true>(a, c, p, pol, base);
    else
        evaluate_lanes<Env, false>(a, c, p, pol, base);
}

} // namespace gymrs
