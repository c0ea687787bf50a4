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
};

template <class Env, bool CRITIC, bool HID, bool UNI, bool FULL>
__device__ __forceinline__ void gradient_block(const GradientArgs& a, const PolicyArgs& p, const uint32_t (&pol)[4], uint64_t base)
{
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
#pragma unroll
    for (int j = 0; j < D; ++j) x[j] = load_vec<float, VEC, NT>(a.start_obs + (uint64_t)j * stride, base, n, FULL, 0.0f);
    cf = load_vec<float, VEC, NT>(a.coef, base, n, FULL, 0.0f);
    if constexpr (!CRITIC) ac = load_vec<uint8_t, VEC, NT>(a.actions, base, n, FULL, uint8_t(0));

    for (uint32_t k = 0; k < K; ++k) {
        // row k + 1 (its observation is obs[k]), before the arithmetic of row k
        Vec<float, VEC> xn[D], cn{};
        Vec<uint8_t, VEC> an{};
#pragma unroll
        for (int j = 0; j < D; ++j) xn[j] = Vec<float, VEC>{};
        if (k + 1 < K) {
#pragma unroll
            for (int j = 0; j < D; ++j) xn[j] = load_vec<float, VEC, NT>(a.obs + ((uint64_t)k * D + j) * stride, base, n, FULL, 0.0f);
            cn = load_vec<float, VEC, NT>(a.coef + (uint64_t)(k + 1) * stride, base, n, FULL, 0.0f);
            if constexpr (!CRITIC) an = load_vec<uint8_t, VEC, NT>(a.actions + (uint64_t)(k + 1) * stride, base, n, FULL, uint8_t(0));
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
            gradient_policy_head<A, VEC>(y, act, c, a.scale, g, on, pa);
            if (a.prob && first) {
                Vec<float, VEC> pr;
#pragma unroll
                for (int i = 0; i < VEC; ++i) pr.v[i] = pa[i];
                store_vec<float, VEC, 1>(a.prob + (uint64_t)k * stride, base, n, FULL, pr);
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
            gradient_block<Env, CRITIC, HID, true, true>(a, p, pol, base);
        else
            gradient_block<Env, CRITIC, HID, true, false>(a, p, pol, base);
    } else {
        if (full)
            gradient_block<Env, CRITIC, HID, false, true>(a, p, pol, base);
        else
            gradient_block<Env, CRITIC, HID, false, false>(a, p, pol, base);
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

} // namespace gymrs
