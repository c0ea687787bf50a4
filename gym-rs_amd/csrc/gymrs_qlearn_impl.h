// gymrs_qlearn_impl.h -- the two kernels of gymrs_q_gradient (include/gymrs_amd.h, "Q-learning"), launched back to back on the
// engine's stream.  gfx950.  Neither steps an env.
//
// The gradient kernels re-walk the record once per kGradientChunk units of the hidden layer.  The TD error needs two forward passes
// per lane-step (three where an episode was truncated), which folded into every chunk would be paid ceil(H / 4) times.  So the
// forward-heavy part runs once and hands the chunked part one row:
//
//   q_td_kernel<Env, DOUBLE>   one work-item owns 4 consecutive lanes and walks their column from row K-1 down to row 0, as
//     advantages_block does.  In registers across the walk: obs[k] and the online logits of obs[k], which are the y of step k+1 --
//     the online net is evaluated once per lane-step plus once for start_obs, and GYMRS_Q_DOUBLE costs no forward pass on
//     lane-steps that went on.  The target net is evaluated once per lane-step, at obs[k].  The logits of final_obs[k] are needed
//     on truncated-only lane-steps alone: they are evaluated behind a wave-level "any lane needs it" branch and selected per lane,
//     so the unwritten bytes of that buffer reach no output.  The loads of row k-1 are issued before the arithmetic of row k;
//     read-once rows and the td store carry the non-temporal hint.  Writes td and, when given, counts.
//   q_gradient_kernel<Env, HID>   walks upward like gradient_block, reading x, a and td[k]; forms d and the one-hot g; an affine
//     net needs no forward pass at all, a hidden one is taken kGradientChunk units per blockIdx.y.  Sums go through GradientSink.
//
// Inside both, the wave-uniform choices uniform / gathered weights and full / ragged wave, as everywhere else.  Both sets share the
// key, so one policy_select serves both PolicyWeights of the TD kernel.
#pragma once
#include "gymrs_gradient_impl.h"
#include "gymrs_qlearn.h"

namespace gymrs {

template <class Env, int VEC, bool UNI>
__device__ __forceinline__ void q_logits(const PolicyWeights<VEC, UNI>& w, uint32_t H, const Vec<float, VEC> (&x)[Env::kState],
                                         float (&y)[Env::kActions][VEC])
{
    float xs[Env::kState][VEC];
#pragma unroll
    for (int j = 0; j < Env::kState; ++j) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) xs[j][k] = x[j].v[k];
    }
    // gathered: one unit's weights per lane in flight, not four units' (policy_logits)
    gradient_logits<Env::kState, (int)Env::kActions, VEC, UNI ? 4 : 1>(w, H, xs, y);
}

template <class Env, bool DOUBLE, bool UNI, bool FULL>
__device__ __forceinline__ void q_td_block(const QArgs& a, const PolicyArgs& p, const PolicyArgs& pt, const uint32_t (&pol)[4], uint64_t base)
{
    constexpr int VEC = 4, D = Env::kState, A = (int)Env::kActions;
    constexpr bool NT = true; // every row is read once here; td is written once and read by the next kernel
    const uint64_t stride = a.stride, n = a.n;
    const PolicyWeights<VEC, UNI> w(p, pol), wt(pt, pol);
    const uint32_t H = p.hidden;
    const bool has_trunc = a.truncated != nullptr; // wave-uniform

    // row K-1
    uint32_t k = a.n_steps - 1;
    Vec<float, VEC> x_obs[D]; // obs[k]
#pragma unroll
    for (int j = 0; j < D; ++j) x_obs[j] = load_vec<float, VEC, NT>(a.obs + ((uint64_t)k * D + j) * stride, base, n, FULL, 0.0f);
    Vec<float, VEC> rew = load_vec<float, VEC, NT>(a.reward + (uint64_t)k * stride, base, n, FULL, 0.0f);
    Vec<uint8_t, VEC> dn = load_vec<uint8_t, VEC, NT>(a.done + (uint64_t)k * stride, base, n, FULL, uint8_t(0));
    Vec<uint8_t, VEC> ac = load_vec<uint8_t, VEC, NT>(a.actions + (uint64_t)k * stride, base, n, FULL, uint8_t(0));
    Vec<uint8_t, VEC> tr{};
    if (has_trunc) tr = load_vec<uint8_t, VEC, NT>(a.truncated + (uint64_t)k * stride, base, n, FULL, uint8_t(0));
    float y_obs[A][VEC] = {}; // the online logits of obs[k]: the bootstrap action's choice (DOUBLE), and y of step k + 1
    if constexpr (DOUBLE) q_logits<Env, VEC, UNI>(w, H, x_obs, y_obs);
    uint32_t seen[VEC] = {}, ncut[VEC] = {};

    for (;; --k) {
        // row k - 1 (start_obs for k == 0), before the arithmetic of row k
        Vec<float, VEC> xp[D], rew_p{};
        Vec<uint8_t, VEC> dn_p{}, tr_p{}, ac_p{};
        const float* prev = k ? a.obs + (uint64_t)(k - 1) * D * stride : a.start_obs;
#pragma unroll
        for (int j = 0; j < D; ++j) xp[j] = load_vec<float, VEC, NT>(prev + (uint64_t)j * stride, base, n, FULL, 0.0f);
        if (k) {
            rew_p = load_vec<float, VEC, NT>(a.reward + (uint64_t)(k - 1) * stride, base, n, FULL, 0.0f);
            dn_p = load_vec<uint8_t, VEC, NT>(a.done + (uint64_t)(k - 1) * stride, base, n, FULL, uint8_t(0));
            ac_p = load_vec<uint8_t, VEC, NT>(a.actions + (uint64_t)(k - 1) * stride, base, n, FULL, uint8_t(0));
            if (has_trunc) tr_p = load_vec<uint8_t, VEC, NT>(a.truncated + (uint64_t)(k - 1) * stride, base, n, FULL, uint8_t(0));
        }

        bool done[VEC], ended[VEC], need = false; // need: truncated only -- the successor is the observation the episode ended in
        float r[VEC];
        uint8_t act[VEC];
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            done[i] = dn.v[i] != 0;
            ended[i] = done[i] || tr.v[i] != 0;
            need = need || (ended[i] && !done[i]);
            r[i] = rew.v[i];
            act[i] = ac.v[i];
        }
        float yt[A][VEC], ysel[A][VEC];
        q_logits<Env, VEC, UNI>(wt, H, x_obs, yt);
#pragma unroll
        for (int b = 0; b < A; ++b) {
#pragma unroll
            for (int i = 0; i < VEC; ++i) ysel[b][i] = DOUBLE ? y_obs[b][i] : yt[b][i];
        }
        if (__any(need)) {
            Vec<float, VEC> xf[D];
#pragma unroll
            for (int j = 0; j < D; ++j) xf[j] = load_vec<float, VEC, NT>(a.final_obs + ((uint64_t)k * D + j) * stride, base, n, FULL, 0.0f);
            float yf[A][VEC];
            q_logits<Env, VEC, UNI>(wt, H, xf, yf);
#pragma unroll
            for (int b = 0; b < A; ++b) {
#pragma unroll
                for (int i = 0; i < VEC; ++i) {
                    yt[b][i] = ended[i] ? yf[b][i] : yt[b][i];
                    if constexpr (!DOUBLE) ysel[b][i] = yt[b][i];
                }
            }
            if constexpr (DOUBLE) {
                float yo[A][VEC];
                q_logits<Env, VEC, UNI>(w, H, xf, yo);
#pragma unroll
                for (int b = 0; b < A; ++b) {
#pragma unroll
                    for (int i = 0; i < VEC; ++i) ysel[b][i] = ended[i] ? yo[b][i] : ysel[b][i];
                }
            }
        }
        float y[A][VEC], delta[VEC];
        bool on[VEC];
        q_logits<Env, VEC, UNI>(w, H, xp, y);
        q_td_step<A, VEC>(y, yt, ysel, act, r, done, a.gamma, delta, on);
        Vec<float, VEC> td;
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            td.v[i] = delta[i];
            seen[i] += on[i] ? 1u : 0u;
            ncut[i] += (on[i] && q_clamped(delta[i], a.kappa)) ? 1u : 0u;
        }
        store_vec<float, VEC, NT>(a.td + (uint64_t)k * stride, base, n, FULL, td);
        if (k == 0) break;
#pragma unroll
        for (int j = 0; j < D; ++j) x_obs[j] = xp[j];
#pragma unroll
        for (int b = 0; b < A; ++b) {
#pragma unroll
            for (int i = 0; i < VEC; ++i) y_obs[b][i] = y[b][i];
        }
        rew = rew_p;
        dn = dn_p;
        tr = tr_p;
        ac = ac_p;
    }

    if (a.counts) { // wave-uniform
        GradientSink<VEC, UNI> sink;
        sink.grad = nullptr;
        sink.S = 0;
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            sink.pol[i] = UNI ? (uint32_t)__builtin_amdgcn_readfirstlane(pol[0]) : pol[i];
            sink.live[i] = FULL || base + i < n;
            sink.excl[i] = 0;
        }
        sink.count(a.counts, seen, ncut);
    }
}

template <class Env, bool DOUBLE>
__global__ __launch_bounds__(kBlock) void q_td_kernel(const QArgs a, const PolicyArgs p, const PolicyArgs pt)
{
    constexpr int VEC = 4, LPB = kBlock * VEC;
    const uint64_t base = (uint64_t)blockIdx.x * LPB + (uint64_t)threadIdx.x * VEC;
    const bool full = (uint64_t)blockIdx.x * LPB + (uint64_t)((threadIdx.x >> 6) + 1) * (64 * VEC) <= a.n; // wave-uniform, see step_kernel
    uint32_t pol[VEC] = {0, 0, 0, 0};
    bool uniform = true;
    policy_select<VEC>(p, a.gid0 + base, pol, uniform);
    if (uniform) {
        if (full)
            q_td_block<Env, DOUBLE, true, true>(a, p, pt, pol, base);
        else
            q_td_block<Env, DOUBLE, true, false>(a, p, pt, pol, base);
    } else {
        if (full)
            q_td_block<Env, DOUBLE, false, true>(a, p, pt, pol, base);
        else
            q_td_block<Env, DOUBLE, false, false>(a, p, pt, pol, base);
    }
}

template <class Env, bool HID, bool UNI, bool FULL>
__device__ __forceinline__ void q_gradient_block(const QArgs& a, const PolicyArgs& p, const uint32_t (&pol)[4], uint64_t base)
{
    constexpr int VEC = 4, D = Env::kState, A = (int)Env::kActions;
    constexpr bool NT = !HID; // an affine launch reads every row once; the chunks of a hidden one read them again
    const uint64_t stride = a.stride, n = a.n;
    const PolicyWeights<VEC, UNI> w(p, pol);
    const uint32_t H = p.hidden, K = a.n_steps;
    const uint32_t h0 = HID ? blockIdx.y * (uint32_t)kGradientChunk : 0u;
    const bool first = !HID || blockIdx.y == 0; // wave-uniform: this pass owns db2

    [[maybe_unused]] GradientAffine<D, A, VEC> aff{};
    [[maybe_unused]] GradientChunk<D, A, VEC> chk{};
    [[maybe_unused]] float db2[A][VEC] = {};

    Vec<float, VEC> x[D], td;
    Vec<uint8_t, VEC> ac;
#pragma unroll
    for (int j = 0; j < D; ++j) x[j] = load_vec<float, VEC, NT>(a.start_obs + (uint64_t)j * stride, base, n, FULL, 0.0f);
    td = load_vec<float, VEC, NT>(a.td, base, n, FULL, 0.0f);
    ac = load_vec<uint8_t, VEC, NT>(a.actions, base, n, FULL, uint8_t(0));

    for (uint32_t k = 0; k < K; ++k) {
        // row k + 1 (its observation is obs[k]), before the arithmetic of row k
        Vec<float, VEC> xn[D], tn{};
        Vec<uint8_t, VEC> an{};
#pragma unroll
        for (int j = 0; j < D; ++j) xn[j] = Vec<float, VEC>{};
        if (k + 1 < K) {
#pragma unroll
            for (int j = 0; j < D; ++j) xn[j] = load_vec<float, VEC, NT>(a.obs + ((uint64_t)k * D + j) * stride, base, n, FULL, 0.0f);
            tn = load_vec<float, VEC, NT>(a.td + (uint64_t)(k + 1) * stride, base, n, FULL, 0.0f);
            an = load_vec<uint8_t, VEC, NT>(a.actions + (uint64_t)(k + 1) * stride, base, n, FULL, uint8_t(0));
        }
        float xs[D][VEC], g[A][VEC], delta[VEC];
        uint8_t act[VEC];
        bool on[VEC];
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            delta[i] = td.v[i];
            act[i] = ac.v[i];
#pragma unroll
            for (int j = 0; j < D; ++j) xs[j][i] = x[j].v[i];
        }
        q_head<A, VEC>(delta, act, a.kappa, g, on);
        if constexpr (HID) {
            gradient_chunk_step<D, A, VEC, true>(w, H, h0, xs, g, on, chk);
            if (first) gradient_bias_step<A, VEC, true>(g, on, db2);
        } else {
            gradient_affine_step<D, A, VEC, true>(xs, g, on, aff);
        }
#pragma unroll
        for (int j = 0; j < D; ++j) x[j] = xn[j];
        td = tn;
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

template <class Env, bool HID>
__global__ __launch_bounds__(kBlock) void q_gradient_kernel(const QArgs a, const PolicyArgs p)
{
    constexpr int VEC = 4, LPB = kBlock * VEC;
    const uint64_t base = (uint64_t)blockIdx.x * LPB + (uint64_t)threadIdx.x * VEC;
    const bool full = (uint64_t)blockIdx.x * LPB + (uint64_t)((threadIdx.x >> 6) + 1) * (64 * VEC) <= a.n; // wave-uniform, see step_kernel
    uint32_t pol[VEC] = {0, 0, 0, 0};
    bool uniform = true;
    policy_select<VEC>(p, a.gid0 + base, pol, uniform);
    if (uniform) {
        if (full)
            q_gradient_block<Env, HID, true, true>(a, p, pol, base);
        else
            q_gradient_block<Env, HID, true, false>(a, p, pol, base);
    } else {
        if (full)
            q_gradient_block<Env, HID, false, true>(a, p, pol, base);
        else
            q_gradient_block<Env, HID, false, false>(a, p, pol, base);
    }
}

// The two launches for one env type.  The caller's checks (gymrs_q_gradient) are what makes every access safe: rows of `stride` >= n
// lanes, every row touched at lanes < n only (full waves: whole 4-lane groups below n); tables of n_sets * S, n_sets and n_sets * 2
// words.  The second launch reads the td row the first one wrote: stream order.
template <class Env>
static hipError_t q_gradient_env(const QArgs& a, const PolicyArgs& p, const PolicyArgs& pt, hipStream_t stream)
{
    launch_begin();
    const uint32_t blocks = step_grid(a.n, 4);
    if (a.flags & GYMRS_Q_DOUBLE)
        hipLaunchKernelGGL((q_td_kernel<Env, true>), dim3(blocks), dim3(kBlock), 0, stream, a, p, pt);
    else
        hipLaunchKernelGGL((q_td_kernel<Env, false>), dim3(blocks), dim3(kBlock), 0, stream, a, p, pt);
    if (hipError_t err = hipGetLastError()) return err;
    if (p.hidden == 0) {
        hipLaunchKernelGGL((q_gradient_kernel<Env, false>), dim3(blocks), dim3(kBlock), 0, stream, a, p);
    } else {
        const uint32_t chunks = (p.hidden + kGradientChunk - 1) / kGradientChunk;
        hipLaunchKernelGGL((q_gradient_kernel<Env, true>), dim3(blocks, chunks), dim3(kBlock), 0, stream, a, p);
    }
    return hipGetLastError();
}

} // namespace gymrs
