// gymrs_entropy_impl.h -- the kernels of gymrs_entropy_gradient (include/gymrs_amd.h, "Entropy"): the gradient of coef * the policy's
// entropy over a transitions record, the entropy itself and the k3 estimate of the KL divergence from the recorded policy, in one
// launch.  gfx950.  The kernel steps no env.  Four kernels per env (network: affine / hidden; with / without old_prob); inside, the
// wave-uniform choices uniform / gathered weights and full / ragged wave, as in gradient_kernel (gymrs_gradient_impl.h), whose
// GradientSink, accumulators and policy_select are used as they are.
//
// What is this head's own.  It has no coefficient row: the coefficient is one scalar of the descriptor.  Without old_prob it reads
// no action row either: a lane-step is its D observation components, 16 bytes per component and work-item of a full wave, and the
// loads of row k+1 are issued before the arithmetic of row k.  With old_prob two more rows travel with them (4 + 16 bytes).  Besides
// the parameter sums a lane carries two f32 running sums (entropy, KL estimate) and two counters; after the walk they are fixed to
// integers (gradient_fixed) like every parameter sum, BEFORE any lane is added to another: the sink is pointed at `sums` (a table
// of two words per set) and takes them as parameters 0 and 1, so a uniform wave issues one atomic per word and the outputs do not
// depend on any order.  Chunk 0 (blockIdx.y == 0) alone owns db2, sums and counts.
//
// The hidden layer keeps the chunks of kGradientChunk = 4 units of the gradient kernels.  Reason, from the compiled kernels: with
// chunks of 4 the hidden kernels already take 366 .. 412 of the 512 registers of a work-item (VGPR + AGPR; gradient_ppo_kernel: 380
// .. 392), one wave per SIMD, without scratch.  The accumulators are GradientChunk's, (4 * (D + 1) + 4 * A) * VEC = 112 (CartPole)
// / 96 (MountainCar) of them; a chunk of 8 needs as many again and would spill.  Every chunk pays the forward pass again (H * (D +
// 1 + A) fma per lane-step) and now the weights, the divide and the log2 as well (about 60 operations, an eighth of the forward
// pass at H = 64), so a wider chunk at 2 lanes per work-item could still win: that form was not built or timed.
// profiles/entropy.md has the registers and the timings of this one.
#pragma once
#include "gymrs_entropy.h"
#include "gymrs_gradient_impl.h"

namespace gymrs {

template <class Env, bool HID, bool UNI, bool FULL, bool KL>
__device__ __forceinline__ void entropy_block(const EntropyArgs& a, const PolicyArgs& p, const uint32_t (&pol)[4], uint64_t base)
{
    constexpr int VEC = 4, D = Env::kState, A = (int)Env::kActions;
    constexpr bool NT = !HID; // an affine launch reads every row once; the chunks of a hidden one read them again
    const uint64_t stride = a.stride, n = a.n;
    const PolicyWeights<VEC, UNI> w(p, pol);
    const uint32_t H = p.hidden, K = a.n_steps;
    const uint32_t h0 = HID ? blockIdx.y * (uint32_t)kGradientChunk : 0u;
    const bool first = !HID || blockIdx.y == 0; // wave-uniform: this pass owns db2, sums and counts

    [[maybe_unused]] GradientAffine<D, A, VEC> aff{};
    [[maybe_unused]] GradientChunk<D, A, VEC> chk{};
    [[maybe_unused]] float db2[A][VEC] = {};
    EntropySums<VEC> sums{};

    Vec<float, VEC> x[D];
    [[maybe_unused]] Vec<uint8_t, VEC> ac{};
    [[maybe_unused]] Vec<float, VEC> op{};
#pragma unroll
    for (int j = 0; j < D; ++j) x[j] = load_vec<float, VEC, NT>(a.start_obs + (uint64_t)j * stride, base, n, FULL, 0.0f);
    if constexpr (KL) {
        ac = load_vec<uint8_t, VEC, NT>(a.actions, base, n, FULL, uint8_t(0));
        op = load_vec<float, VEC, NT>(a.old_prob, base, n, FULL, 0.0f);
    }

    for (uint32_t k = 0; k < K; ++k) {
        // row k + 1 (its observation is obs[k]), before the arithmetic of row k
        Vec<float, VEC> xn[D];
        [[maybe_unused]] Vec<uint8_t, VEC> an{};
        [[maybe_unused]] Vec<float, VEC> opn{};
#pragma unroll
        for (int j = 0; j < D; ++j) xn[j] = Vec<float, VEC>{};
        if (k + 1 < K) {
#pragma unroll
            for (int j = 0; j < D; ++j) xn[j] = load_vec<float, VEC, NT>(a.obs + ((uint64_t)k * D + j) * stride, base, n, FULL, 0.0f);
            if constexpr (KL) {
                an = load_vec<uint8_t, VEC, NT>(a.actions + (uint64_t)(k + 1) * stride, base, n, FULL, uint8_t(0));
                opn = load_vec<float, VEC, NT>(a.old_prob + (uint64_t)(k + 1) * stride, base, n, FULL, 0.0f);
            }
        }

        float xs[D][VEC], y[A][VEC], g[A][VEC], hn[VEC], pr[A][VEC];
        bool on[VEC];
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
#pragma unroll
            for (int j = 0; j < D; ++j) xs[j][i] = x[j].v[i];
        }
        // gathered: one unit's weights per lane in flight, not four units' (policy_logits)
        gradient_logits<D, A, VEC, UNI ? 4 : 1>(w, H, xs, y);
        entropy_head<A, VEC>(y, a.scale, a.coef, g, on, hn, pr);
        if (first) {
            uint8_t act[VEC] = {};
            float po[VEC] = {};
            if constexpr (KL) {
#pragma unroll
                for (int i = 0; i < VEC; ++i) {
                    act[i] = ac.v[i];
                    po[i] = op.v[i];
                }
            }
            entropy_sums_step<A, VEC, KL>(on, hn, pr, act, po, sums);
        }
        if constexpr (HID) {
            gradient_chunk_step<D, A, VEC, true>(w, H, h0, xs, g, on, chk);
            if (first) gradient_bias_step<A, VEC, true>(g, on, db2);
        } else {
            gradient_affine_step<D, A, VEC, true>(xs, g, on, aff);
        }
#pragma unroll
        for (int j = 0; j < D; ++j) x[j] = xn[j];
        if constexpr (KL) {
            ac = an;
            op = opn;
        }
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
    if (first) { // wave-uniform
        sink.grad = a.sums; // the two sums are parameters 0 and 1 of a table of two words per set
        sink.S = 2;
        sink(0u, sums.h);
        if constexpr (KL) sink(1u, sums.kl);
        if (a.counts) sink.count(a.counts, sums.n_h, sums.n_kl);
    }
    sink.finish(a.excluded);
}

template <class Env, bool HID, bool KL>
__global__ __launch_bounds__(kBlock) void entropy_kernel(const EntropyArgs a, const PolicyArgs p)
{
    constexpr int VEC = 4, LPB = kBlock * VEC;
    const uint64_t base = (uint64_t)blockIdx.x * LPB + (uint64_t)threadIdx.x * VEC;
    const bool full = (uint64_t)blockIdx.x * LPB + (uint64_t)((threadIdx.x >> 6) + 1) * (64 * VEC) <= a.n; // wave-uniform, see step_kernel
    uint32_t pol[VEC] = {0, 0, 0, 0};
    bool uniform = true;
    policy_select<VEC>(p, a.gid0 + base, pol, uniform);
    if (uniform) {
        if (full)
            entropy_block<Env, HID, true, true, KL>(a, p, pol, base);
        else
            entropy_block<Env, HID, true, false, KL>(a, p, pol, base);
    } else {
        if (full)
            entropy_block<Env, HID, false, true, KL>(a, p, pol, base);
        else
            entropy_block<Env, HID, false, false, KL>(a, p, pol, base);
    }
}

// The launch for one env type.  The caller's checks (gymrs_entropy_gradient) are what makes every access safe: rows of `stride` >= n
// lanes, every row touched at lanes < n only (full waves: whole 4-lane groups below n); tables of n_sets * S and n_sets * 2 words.
template <class Env, bool KL>
static hipError_t entropy_env(const EntropyArgs& a, const PolicyArgs& p, hipStream_t stream)
{
    launch_begin();
    const uint32_t blocks = step_grid(a.n, 4);
    if (p.hidden == 0) {
        hipLaunchKernelGGL((entropy_kernel<Env, false, KL>), dim3(blocks), dim3(kBlock), 0, stream, a, p);
    } else {
        const uint32_t chunks = (p.hidden + kGradientChunk - 1) / kGradientChunk;
        hipLaunchKernelGGL((entropy_kernel<Env, true, KL>), dim3(blocks, chunks), dim3(kBlock), 0, stream, a, p);
    }
    return hipGetLastError();
}

} // namespace gymrs
