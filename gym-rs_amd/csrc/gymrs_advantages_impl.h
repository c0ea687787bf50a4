// gymrs_advantages_impl.h -- the kernel of gymrs_advantages (include/gymrs_amd.h, "advantages"): GAE(lambda) advantages, returns and
// values over a transitions record in one pass.  gfx950.  The kernel steps no env: it has no flag-set, TableT, explore or sample
// axis.  Two kernels per env (critic on / off); inside, the wave-uniform choices uniform / gathered critic weights and full / ragged
// wave, as in the recording kernels: eight code copies per env pair.
//
// One work-item owns 4 consecutive lanes and walks their column from row K-1 down to row 0.  Rows are 16-byte aligned with a stride
// that is a multiple of 16 lanes, so every row access of a full wave is one 16-byte load or store per component (4 bytes for the
// flag rows).  In registers across the walk: the carry A[k+1] and V(obs[k]) -- v_next of step k is v_cur of step k+1, so the critic
// is evaluated once per lane-step plus once for start_obs.  The loads of row k-1 are issued before the arithmetic of row k.
// V(final_obs[k]) is needed on truncated-only steps alone: it is evaluated behind a wave-level "any lane needs it" branch and
// selected per lane, so the unwritten bytes of that buffer reach no output.
#pragma once
#include "gymrs_advantages.h"
#include "gymrs_policy.h"

namespace gymrs {

// The critic's weights through the policy's accessors: PolicyWeights<VEC, UNI> is w(k, i).
template <class Env, int VEC, bool UNI>
__device__ __forceinline__ void critic_eval(const PolicyWeights<VEC, UNI>& w, uint32_t H, const Vec<float, VEC> (&x)[Env::kState], float (&v)[VEC])
{
    float xs[Env::kState][VEC];
#pragma unroll
    for (int j = 0; j < Env::kState; ++j) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) xs[j][k] = x[j].v[k];
    }
    // gathered: one unit's 2 + D vector loads per lane in flight, not four units' (policy_logits)
    critic_values<Env::kState, VEC, UNI ? 4 : 1>(w, H, xs, v);
}

template <class Env, bool CRITIC, bool UNI, bool FULL>
__device__ __forceinline__ void advantages_block(const AdvantageArgs& a, const PolicyArgs& p, const uint32_t (&pol)[4], uint64_t base)
{
    constexpr int VEC = 4, D = Env::kState;
    constexpr bool NT = true; // read-once rows and write-once outputs carry the non-temporal hint (plain measured slower: profiles/advantages.md)
    const uint64_t stride = a.stride, n = a.n;
    const PolicyWeights<VEC, UNI> w(p, pol);
    const bool has_trunc = a.truncated != nullptr, has_final = a.final_obs != nullptr; // wave-uniform

    // row K-1
    uint32_t k = a.n_steps - 1;
    Vec<float, VEC> rew = load_vec<float, VEC, NT>(a.reward + (uint64_t)k * stride, base, n, FULL, 0.0f);
    Vec<uint8_t, VEC> dn = load_vec<uint8_t, VEC, NT>(a.done + (uint64_t)k * stride, base, n, FULL, uint8_t(0));
    Vec<uint8_t, VEC> tr{};
    if (has_trunc) tr = load_vec<uint8_t, VEC, NT>(a.truncated + (uint64_t)k * stride, base, n, FULL, uint8_t(0));
    float v_obs[VEC], carry[VEC]; // V(obs[k]), A[k + 1]
#pragma unroll
    for (int i = 0; i < VEC; ++i) v_obs[i] = carry[i] = 0.0f;
    if constexpr (CRITIC) {
        Vec<float, VEC> x[D];
#pragma unroll
        for (int j = 0; j < D; ++j) x[j] = load_vec<float, VEC, NT>(a.obs + ((uint64_t)k * D + j) * stride, base, n, FULL, 0.0f);
        critic_eval<Env, VEC, UNI>(w, p.hidden, x, v_obs);
    }

    for (;; --k) {
        // row k - 1 (start_obs for k == 0), before the arithmetic of row k
        Vec<float, VEC> xp[D], rew_p{};
        Vec<uint8_t, VEC> dn_p{}, tr_p{};
        if constexpr (CRITIC) {
            const float* prev = k ? a.obs + (uint64_t)(k - 1) * D * stride : a.start_obs;
#pragma unroll
            for (int j = 0; j < D; ++j) xp[j] = load_vec<float, VEC, NT>(prev + (uint64_t)j * stride, base, n, FULL, 0.0f);
        }
        if (k) {
            rew_p = load_vec<float, VEC, NT>(a.reward + (uint64_t)(k - 1) * stride, base, n, FULL, 0.0f);
            dn_p = load_vec<uint8_t, VEC, NT>(a.done + (uint64_t)(k - 1) * stride, base, n, FULL, uint8_t(0));
            if (has_trunc) tr_p = load_vec<uint8_t, VEC, NT>(a.truncated + (uint64_t)(k - 1) * stride, base, n, FULL, uint8_t(0));
        }

        bool done[VEC], ended[VEC];
        float v_succ[VEC], v_cur[VEC];
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            done[i] = dn.v[i] != 0;
            ended[i] = done[i] || tr.v[i] != 0;
            v_succ[i] = v_obs[i];
            v_cur[i] = 0.0f;
        }
        if constexpr (CRITIC) {
            if (has_final) {
                bool need = false; // truncated only: the successor is the observation the episode ended in
#pragma unroll
                for (int i = 0; i < VEC; ++i) need = need || (ended[i] && !done[i]);
                if (__any(need)) {
                    Vec<float, VEC> xf[D];
#pragma unroll
                    for (int j = 0; j < D; ++j)
                        xf[j] = load_vec<float, VEC, NT>(a.final_obs + ((uint64_t)k * D + j) * stride, base, n, FULL, 0.0f);
                    float v_fin[VEC];
                    critic_eval<Env, VEC, UNI>(w, p.hidden, xf, v_fin);
#pragma unroll
                    for (int i = 0; i < VEC; ++i) v_succ[i] = ended[i] ? v_fin[i] : v_obs[i];
                }
            }
            critic_eval<Env, VEC, UNI>(w, p.hidden, xp, v_cur);
        }
        Vec<float, VEC> adv, ret, val;
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            advantage_step(a.gamma, a.gl, rew.v[i], done[i], ended[i], v_succ[i], v_cur[i], carry[i], adv.v[i], ret.v[i]);
            val.v[i] = v_cur[i];
            carry[i] = adv.v[i];
            v_obs[i] = v_cur[i];
        }
        store_vec<float, VEC, NT>(a.advantages + (uint64_t)k * stride, base, n, FULL, adv);
        if (a.returns) store_vec<float, VEC, NT>(a.returns + (uint64_t)k * stride, base, n, FULL, ret);
        if (a.values) store_vec<float, VEC, NT>(a.values + (uint64_t)k * stride, base, n, FULL, val);
        if (k == 0) break;
        rew = rew_p;
        dn = dn_p;
        tr = tr_p;
    }
}

template <class Env, bool CRITIC>
__global__ __launch_bounds__(kBlock) void advantages_kernel(const AdvantageArgs a, const PolicyArgs p)
{
    constexpr int VEC = 4, LPB = kBlock * VEC;
    const uint64_t base = (uint64_t)blockIdx.x * LPB + (uint64_t)threadIdx.x * VEC;
    const bool full = (uint64_t)blockIdx.x * LPB + (uint64_t)((threadIdx.x >> 6) + 1) * (64 * VEC) <= a.n; // wave-uniform, see step_kernel
    uint32_t pol[VEC] = {0, 0, 0, 0};
    bool uniform = true;
    if constexpr (CRITIC) policy_select<VEC>(p, a.gid0 + base, pol, uniform);
    if (uniform) {
        if (full)
            advantages_block<Env, CRITIC, true, true>(a, p, pol, base);
        else
            advantages_block<Env, CRITIC, true, false>(a, p, pol, base);
    } else if constexpr (CRITIC) {
        if (full)
            advantages_block<Env, CRITIC, false, true>(a, p, pol, base);
        else
            advantages_block<Env, CRITIC, false, false>(a, p, pol, base);
    }
}

// The launch for one env type.  The caller's checks (gymrs_advantages) are what makes every access safe: rows of `stride` >= n
// lanes, every row touched at lanes < n only (full waves: whole 4-lane groups below n).
template <class Env>
static hipError_t advantages_env(const AdvantageArgs& a, const PolicyArgs* critic, hipStream_t stream)
{
    launch_begin();
    if (critic)
        hipLaunchKernelGGL((advantages_kernel<Env, true>), dim3(step_grid(a.n, 4)), dim3(kBlock), 0, stream, a, *critic);
    else
        hipLaunchKernelGGL((advantages_kernel<Env, false>), dim3(step_grid(a.n, 4)), dim3(kBlock), 0, stream, a, PolicyArgs{});
    return hipGetLastError();
}

} // namespace gymrs
