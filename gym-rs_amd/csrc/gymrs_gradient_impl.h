// gymrs_gradient_impl.h -- the kernels of gymrs_policy_gradient (include/gymrs_amd.h, "gradients"): the score-function gradient of
// the policy set (or the value gradient of the critic set) over a transitions record in one launch.  gfx950.  The kernel steps no
// env.  Four kernels per env (head: policy / critic, network: affine / hidden); inside, the wave-uniform choices uniform / gathered
// weights and full / ragged wave, as in advantages_kernel.
//
// One work-item owns 4 consecutive lanes and walks their column from row 0 up to row K-1, one f32 accumulator per (lane,
// parameter) in registers.  Rows are 16-byte aligned with a stride that is a multiple of 16 lanes, so every row access of a full
// wave is one 16-byte load or store per component (4 bytes for the action row).  The loads of row k+1 are issued before the
// arithmetic of row k.  An affine network is one pass (A*(D+1) accumulators per lane).  A hidden layer is taken kGradientChunk
// units at a time, one chunk per blockIdx.y of the same launch: every chunk recomputes the forward pass of its lane-steps (the
// policy head needs all logits for g; the critic head needs none) and owns the sums of its units; chunk 0 also owns db2 and writes
// `prob`.  After the walk every sum becomes its fixed-point integer (gradient_fixed) and is added to the table: a wave whose lanes
// share one set sums in integers first (wave_sum_u64) and issues one atomic per parameter, a gathered wave one per lane and
// parameter.  Integer adds commute: the table does not depend on the order.
//
// gymrs_ppo_gradient ("clipped surrogate") is the policy head with PPO = true: the coefficient of a lane-step comes from the
// advantages row (in the `coef` slot), one more row (old_prob) and the p[a] the head already holds, and chunk 0 counts the lane-steps
// and the cut ones per set.  The eight kernels above are compiled without any of it (if constexpr).
#pragma once
#include "gymrs_gradient.h"
#include "gymrs_policy.h"

namespace gymrs {

// Where the sums of a work-item go.  live[k]: lane k exists (ragged waves); a lane that does not adds and counts nothing.
template <int VEC, bool UNI>
struct GradientSink {
    unsigned long long* grad; // the table, [n_sets][S]
    uint32_t S;
    uint32_t pol[VEC];
    bool live[VEC];
    uint32_t excl[VEC];
    __device__ __forceinline__ void operator()(uint32_t s, const float (&L)[VEC])
    {
        unsigned long long q[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            long long v;
            const bool ok = gradient_fixed(L[k], v);
            q[k] = live[k] ? (unsigned long long)v : 0ull;
            excl[k] += (live[k] && !ok) ? 1u : 0u;
        }
        if constexpr (UNI) {
            unsigned long long sum = q[0];
#pragma unroll
            for (int k = 1; k < VEC; ++k) sum += q[k];
            const unsigned long long total = wave_sum_u64(sum);
            if ((threadIdx.x & 63u) == 0) atomic_add_nonzero(grad + (uint64_t)pol[0] * S + s, total);
        } else {
#pragma unroll
            for (int k = 0; k < VEC; ++k) atomic_add_nonzero(grad + (uint64_t)pol[k] * S + s, q[k]);
        }
    }
    __device__ __forceinline__ void finish(unsigned long long* excluded)
    {
        if constexpr (UNI) {
            uint32_t sum = excl[0];
#pragma unroll
            for (int k = 1; k < VEC; ++k) sum += excl[k];
            const uint32_t total = wave_sum_u32(sum);
            if ((threadIdx.x & 63u) == 0) atomic_add_nonzero(excluded + pol[0], (unsigned long long)total);
        } else {
#pragma unroll
            for (int k = 0; k < VEC; ++k) atomic_add_nonzero(excluded + pol[k], (unsigned long long)excl[k]);
        }
    }
    // counts[set][0] += the lane-steps seen, counts[set][1] += the cut ones: per lane at most K < 2^32 each, the wave's sum in 64 bits
    __device__ __forceinline__ void count(unsigned long long* counts, const uint32_t (&seen)[VEC], const uint32_t (&cut)[VEC])
    {
        if constexpr (UNI) {
            unsigned long long s = 0, c = 0;
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                s += live[k] ? seen[k] : 0u;
                c += live[k] ? cut[k] : 0u;
            }
            const unsigned long long ts = wave_sum_u64(s), tc = wave_sum_u64(c);
            if ((threadIdx.x & 63u) == 0) {
                atomic_add_nonzero(counts + (uint64_t)pol[0] * 2, ts);
                atomic_add_nonzero(counts + (uint64_t)pol[0] * 2 + 1, tc);
            }
        } else {
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                atomic_add_nonzero(counts + (uint64_t)pol[k] * 2, live[k] ? (unsigned long long)seen[k] : 0ull);
                atomic_add_nonzero(counts + (uint64_t)pol[k] * 2 + 1, live[k] ? (unsigned long long)cut[k] : 0ull);
            }
        }
    }
};

// PPO: x != NULL holds what "clipped surrogate" adds to the policy head (a.coef is its advantages row)
template <class Env, bool CRITIC, bool HID, bool UNI, bool FULL, bool PPO>
__device__ __forceinline__ void gradient_block(const GradientArgs& a, const PolicyArgs& p, const uint32_t (&pol)[4], uint64_t base,
                                               [[maybe_unused]] const PpoArgs* x_)
{
    static_assert(!(PPO && CRITIC), "the clipped surrogate is a policy head");
    constexpr int VEC = 4, D = Env::kState, A = CRITIC ? 1 : (int)Env::kActions;
    constexpr bool NT = !HID; // an affine launch reads every row once; the chunks of a hidden one read them again
    constexpr bool MASK = !CRITIC;
    const uint64_t stride = a.stride, n = a.n;
    const PolicyWeights<VEC, UNI> w(p, pol);
    const uint32_t H = p.hidden, K = a.n_steps;
    const uint32_t h0 = HID ? blockIdx.y * (uint32_t)kGradientChunk : 0u;
    const bool first = !HID || blockIdx.y == 0; // wave-uniform: this pass owns db2 and `prob`

    [[maybe_unused]] GradientAffine<D, A, VEC> aff{};
    [[maybe_unused]] GradientChunk<D, A, VEC> chk{};
    [[maybe_unused]] float db2[A][VEC] = {};

    Vec<float, VEC> x[D], cf;
    Vec<uint8_t, VEC> ac{};
    [[maybe_unused]] Vec<float, VEC> op{};
    [[maybe_unused]] uint32_t seen[VEC] = {}, ncut[VEC] = {};
#pragma unroll
    for (int j = 0; j < D; ++j) x[j] = load_vec<float, VEC, NT>(a.start_obs + (uint64_t)j * stride, base, n, FULL, 0.0f);
    cf = load_vec<float, VEC, NT>(a.coef, base, n, FULL, 0.0f);
    if constexpr (!CRITIC) ac = load_vec<uint8_t, VEC, NT>(a.actions, base, n, FULL, uint8_t(0));
    if constexpr (PPO) op = load_vec<float, VEC, NT>(x_->old_prob, base, n, FULL, 0.0f);

    for (uint32_t k = 0; k < K; ++k) {
        // row k + 1 (its observation is obs[k]), before the arithmetic of row k
        Vec<float, VEC> xn[D], cn{};
        Vec<uint8_t, VEC> an{};
        [[maybe_unused]] Vec<float, VEC> opn{};
#pragma unroll
        for (int j = 0; j < D; ++j) xn[j] = Vec<float, VEC>{};
        if (k + 1 < K) {
#pragma unroll
            for (int j = 0; j < D; ++j) xn[j] = load_vec<float, VEC, NT>(a.obs + ((uint64_t)k * D + j) * stride, base, n, FULL, 0.0f);
            cn = load_vec<float, VEC, NT>(a.coef + (uint64_t)(k + 1) * stride, base, n, FULL, 0.0f);
            if constexpr (!CRITIC) an = load_vec<uint8_t, VEC, NT>(a.actions + (uint64_t)(k + 1) * stride, base, n, FULL, uint8_t(0));
            if constexpr (PPO) opn = load_vec<float, VEC, NT>(x_->old_prob + (uint64_t)(k + 1) * stride, base, n, FULL, 0.0f);
        }

        float xs[D][VEC], g[A][VEC];
        bool on[VEC];
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            on[i] = true;
#pragma unroll
            for (int j = 0; j < D; ++j) xs[j][i] = x[j].v[i];
        }
        if constexpr (CRITIC) {
#pragma unroll
            for (int i = 0; i < VEC; ++i) g[0][i] = cf.v[i];
        } else {
            float y[A][VEC], c[VEC], pa[VEC];
            uint8_t act[VEC];
#pragma unroll
            for (int i = 0; i < VEC; ++i) {
                c[i] = cf.v[i];
                act[i] = ac.v[i];
            }
            // gathered: one unit's weights per lane in flight, not four units' (policy_logits)
            gradient_logits<D, A, VEC, UNI ? 4 : 1>(w, H, xs, y);
            if constexpr (PPO) {
                float po[VEC];
                bool cut[VEC];
#pragma unroll
                for (int i = 0; i < VEC; ++i) po[i] = op.v[i];
                gradient_ppo_head<A, VEC>(y, act, c, po, a.scale, x_->clip_low, x_->clip_high, g, on, pa, cut);
#pragma unroll
                for (int i = 0; i < VEC; ++i) {
                    seen[i] += on[i] ? 1u : 0u;
                    ncut[i] += cut[i] ? 1u : 0u;
                }
            } else {
                gradient_policy_head<A, VEC>(y, act, c, a.scale, g, on, pa);
            }
            if (a.prob && first) {
                Vec<float, VEC> pr;
#pragma unroll
                for (int i = 0; i < VEC; ++i) pr.v[i] = pa[i];
                store_vec<float, VEC, true>(a.prob + (uint64_t)k * stride, base, n, FULL, pr);
            }
        }
        if constexpr (HID) {
            gradient_chunk_step<D, A, VEC, MASK>(w, H, h0, xs, g, on, chk);
            if (first) gradient_bias_step<A, VEC, MASK>(g, on, db2);
        } else {
            gradient_affine_step<D, A, VEC, MASK>(xs, g, on, aff);
        }
#pragma unroll
        for (int j = 0; j < D; ++j) x[j] = xn[j];
        cf = cn;
        ac = an;
        if constexpr (PPO) op = opn;
    }

    GradientSink<VEC, UNI> sink;
    sink.grad = a.grad;
    sink.S = p.stride;
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
        sink.pol[i] = UNI ? (uint32_t)__builtin_amdgcn_readfirstlane(pol[0]) : pol[i];
        sink.live[i] = FULL || base + i < n;
        sink.excl[i] = 0;
    }
    if constexpr (HID) {
        gradient_chunk_each<D, A, VEC>(H, h0, chk, sink);
        if (first) gradient_bias_each<D, A, VEC>(H, db2, sink);
    } else {
        gradient_affine_each<D, A, VEC>(aff, sink);
    }
    sink.finish(a.excluded);
    if constexpr (PPO) {
        if (x_->counts && first) sink.count(x_->counts, seen, ncut); // wave-uniform
    }
}

template <class Env, bool CRITIC, bool HID>
__global__ __launch_bounds__(kBlock) void gradient_kernel(const GradientArgs a, const PolicyArgs p)
{
    constexpr int VEC = 4, LPB = kBlock * VEC;
    const uint64_t base = (uint64_t)blockIdx.x * LPB + (uint64_t)threadIdx.x * VEC;
    const bool full = (uint64_t)blockIdx.x * LPB + (uint64_t)((threadIdx.x >> 6) + 1) * (64 * VEC) <= a.n; // wave-uniform, see step_kernel
    uint32_t pol[VEC] = {0, 0, 0, 0};
    bool uniform = true;
    policy_select<VEC>(p, a.gid0 + base, pol, uniform);
    if (uniform) {
        if (full)
            gradient_block<Env, CRITIC, HID, true, true, false>(a, p, pol, base, nullptr);
        else
            gradient_block<Env, CRITIC, HID, true, false, false>(a, p, pol, base, nullptr);
    } else {
        if (full)
            gradient_block<Env, CRITIC, HID, false, true, false>(a, p, pol, base, nullptr);
        else
            gradient_block<Env, CRITIC, HID, false, false, false>(a, p, pol, base, nullptr);
    }
}

// The same four copies of the clipped surrogate's policy head
template <class Env, bool HID>
__global__ __launch_bounds__(kBlock) void gradient_ppo_kernel(const PpoArgs x, const PolicyArgs p)
{
    const GradientArgs& a = x.g;
    constexpr int VEC = 4, LPB = kBlock * VEC;
    const uint64_t base = (uint64_t)blockIdx.x * LPB + (uint64_t)threadIdx.x * VEC;
    const bool full = (uint64_t)blockIdx.x * LPB + (uint64_t)((threadIdx.x >> 6) + 1) * (64 * VEC) <= a.n; // wave-uniform, see step_kernel
    uint32_t pol[VEC] = {0, 0, 0, 0};
    bool uniform = true;
    policy_select<VEC>(p, a.gid0 + base, pol, uniform);
    if (uniform) {
        if (full)
            gradient_block<Env, false, HID, true, true, true>(a, p, pol, base, &x);
        else
            gradient_block<Env, false, HID, true, false, true>(a, p, pol, base, &x);
    } else {
        if (full)
            gradient_block<Env, false, HID, false, true, true>(a, p, pol, base, &x);
        else
            gradient_block<Env, false, HID, false, false, true>(a, p, pol, base, &x);
    }
}

// The launch for one env type.  The caller's checks (gymrs_policy_gradient) are what makes every access safe: rows of `stride` >= n
// lanes, every row touched at lanes < n only (full waves: whole 4-lane groups below n); a table of n_sets * S words, S = p.stride.
template <class Env, bool CRITIC>
static hipError_t gradient_env(const GradientArgs& a, const PolicyArgs& p, hipStream_t stream)
{
    launch_begin();
    const uint32_t blocks = step_grid(a.n, 4);
    if (p.hidden == 0) {
        hipLaunchKernelGGL((gradient_kernel<Env, CRITIC, false>), dim3(blocks), dim3(kBlock), 0, stream, a, p);
    } else {
        const uint32_t chunks = (p.hidden + kGradientChunk - 1) / kGradientChunk;
        hipLaunchKernelGGL((gradient_kernel<Env, CRITIC, true>), dim3(blocks, chunks), dim3(kBlock), 0, stream, a, p);
    }
    return hipGetLastError();
}

// The same for gymrs_ppo_gradient (gymrs_gradient_ppo.hip); its checks are gymrs_ppo_gradient's.
template <class Env>
static hipError_t gradient_ppo_env(const PpoArgs& a, const PolicyArgs& p, hipStream_t stream)
{
    launch_begin();
    const uint32_t blocks = step_grid(a.g.n, 4);
    if (p.hidden == 0) {
        hipLaunchKernelGGL((gradient_ppo_kernel<Env, false>), dim3(blocks), dim3(kBlock), 0, stream, a, p);
    } else {
        const uint32_t chunks = (p.hidden + kGradientChunk - 1) / kGradientChunk;
        hipLaunchKernelGGL((gradient_ppo_kernel<Env, true>), dim3(blocks, chunks), dim3(kBlock), 0, stream, a, p);
    }
    return hipGetLastError();
}

} // namespace gymrs
