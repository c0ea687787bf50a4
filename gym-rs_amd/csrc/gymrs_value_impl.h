// gymrs_value_impl.h -- the kernels of gymrs_value_gradient (include/gymrs_amd.h, "value loss"): the critic head of
// gymrs_policy_gradient with its coefficient computed here, from the critic's own V(x), a returns row and (GYMRS_VALUE_CLIP) an
// old-values row.  gfx950.  The kernel steps no env.  Siblings of gradient_kernel (gymrs_gradient_impl.h), whose GradientSink,
// accumulators, policy_select and walk (one work-item owns 4 consecutive lanes, row k + 1 is loaded before the arithmetic of row k,
// 16-byte row accesses in a full wave) are used as they are; that file is not touched, so its twelve kernels keep their code.
//
// What is new against the critic head.  There the coefficient is a row, and a chunk of hidden units needs no forward pass beyond
// its own units.  Here every chunk needs the complete V(x) to form c.  Of the two ways to get it
//   (a) every chunk recomputes the forward pass, as the policy head does for its logits;
//   (b) V is computed once into a row and the chunks read it, two kernels back to back (as gymrs_q_gradient does for td);
// (b) is taken.  A chunk's own work is 4 units; the forward pass is H of them, so at H = 64 way (a) multiplies the arithmetic of
// the sixteen chunks by about five ((64 + 4 * 2.5) / (4 * 2.5) in unit-passes, a backward unit costing about 1.5 forward ones),
// where (b) adds one forward pass (the cost of the forward half of gymrs_advantages for one observation per step) and one more row
// of traffic per chunk: 4 bytes per lane-step beside the 4 * D + 4 (+ 4) the chunk reads anyway.  The row is `values` when the caller
// asks for it, else a scratch row of the engine; the chunks recompute c from v, R and vo (six operations), so that there is one
// path whether or not `values` is given.
//
// Three passes, one kernel each per env:
//   Affine   H == 0, the whole call: v, c, values, sums, counts, dW and db.
//   Forward  H  > 0, first launch:   v, c, the v row, sums, counts, db2 (which does not depend on the unit).
//   Chunk    H  > 0, second launch, one chunk of kGradientChunk units per blockIdx.y: c from the v row, dW1, db1 and dW2.
// Inside each, the wave-uniform choices uniform / gathered weights and full / ragged wave.  Sums and counters go through the sink
// like entropy_kernel's: fixed per lane (gradient_fixed) before any lane is added to another.
// Registers (the compiler's resource report for gfx950) are recorded in profiles/value_gradient.md.
#pragma once
#include "gymrs_value.h"
#include "gymrs_gradient_impl.h"

namespace gymrs {

enum class ValuePass { Affine, Forward, Chunk };

template <class Env, ValuePass PASS, bool UNI, bool FULL>
__device__ __forceinline__ void value_block(const ValueArgs& a, const PolicyArgs& p, const uint32_t (&pol)[4], uint64_t base)
{
    constexpr int VEC = 4, D = Env::kState;
    constexpr bool OWNER = PASS != ValuePass::Chunk; // computes v itself: owns the v row, sums, counts and the bias of the output
    constexpr bool NT = PASS == ValuePass::Affine;   // an affine launch reads every row once; the two launches of a hidden one read them again
    const uint64_t stride = a.stride, n = a.n;
    const PolicyWeights<VEC, UNI> w(p, pol);
    const uint32_t H = p.hidden, K = a.n_steps;
    const uint32_t h0 = PASS == ValuePass::Chunk ? blockIdx.y * (uint32_t)kGradientChunk : 0u;
    const bool clipped = a.old_values != nullptr; // wave-uniform (GYMRS_VALUE_CLIP)

    [[maybe_unused]] GradientAffine<D, 1, VEC> aff{};
    [[maybe_unused]] GradientChunk<D, 1, VEC> chk{};
    [[maybe_unused]] float db2[1][VEC] = {};
    ValueSums<VEC> sums{};

    Vec<float, VEC> x[D], rt, vo{}, vr{};
#pragma unroll
    for (int j = 0; j < D; ++j) x[j] = load_vec<float, VEC, NT>(a.start_obs + (uint64_t)j * stride, base, n, FULL, 0.0f);
    rt = load_vec<float, VEC, NT>(a.returns, base, n, FULL, 0.0f);
    if (clipped) vo = load_vec<float, VEC, NT>(a.old_values, base, n, FULL, 0.0f);
    if constexpr (!OWNER) vr = load_vec<float, VEC, false>(a.v_row, base, n, FULL, 0.0f);

    for (uint32_t k = 0; k < K; ++k) {
        // row k + 1 (its observation is obs[k]), before the arithmetic of row k
        Vec<float, VEC> xn[D], rn{}, von{}, vrn{};
#pragma unroll
        for (int j = 0; j < D; ++j) xn[j] = Vec<float, VEC>{};
        if (k + 1 < K) {
#pragma unroll
            for (int j = 0; j < D; ++j) xn[j] = load_vec<float, VEC, NT>(a.obs + ((uint64_t)k * D + j) * stride, base, n, FULL, 0.0f);
            rn = load_vec<float, VEC, NT>(a.returns + (uint64_t)(k + 1) * stride, base, n, FULL, 0.0f);
            if (clipped) von = load_vec<float, VEC, NT>(a.old_values + (uint64_t)(k + 1) * stride, base, n, FULL, 0.0f);
            if constexpr (!OWNER) vrn = load_vec<float, VEC, false>(a.v_row + (uint64_t)(k + 1) * stride, base, n, FULL, 0.0f);
        }

        float xs[D][VEC], g[1][VEC], v[VEC], R[VEC], o[VEC];
        bool on[VEC];
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            on[i] = true;
            R[i] = rt.v[i];
            o[i] = vo.v[i];
#pragma unroll
            for (int j = 0; j < D; ++j) xs[j][i] = x[j].v[i];
        }
        if constexpr (OWNER) {
            // gathered: one unit's weights per lane in flight, not four units' (policy_logits)
            critic_values<D, VEC, UNI ? 4 : 1>(w, H, xs, v);
            if (a.v_row) {
                Vec<float, VEC> out;
#pragma unroll
                for (int i = 0; i < VEC; ++i) out.v[i] = v[i];
                store_vec<float, VEC, NT>(a.v_row + (uint64_t)k * stride, base, n, FULL, out);
            }
        } else {
#pragma unroll
            for (int i = 0; i < VEC; ++i) v[i] = vr.v[i];
        }
        value_head<VEC, OWNER>(v, R, o, a.clip, clipped, g, sums);
        if constexpr (PASS == ValuePass::Affine) gradient_affine_step<D, 1, VEC, false>(xs, g, on, aff);
        if constexpr (PASS == ValuePass::Forward) gradient_bias_step<1, VEC, false>(g, on, db2);
        if constexpr (PASS == ValuePass::Chunk) gradient_chunk_step<D, 1, VEC, false>(w, H, h0, xs, g, on, chk);
#pragma unroll
        for (int j = 0; j < D; ++j) x[j] = xn[j];
        rt = rn;
        vo = von;
        if constexpr (!OWNER) vr = vrn;
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
    if constexpr (PASS == ValuePass::Affine) gradient_affine_each<D, 1, VEC>(aff, sink);
    if constexpr (PASS == ValuePass::Forward) gradient_bias_each<D, 1, VEC>(H, db2, sink);
    if constexpr (PASS == ValuePass::Chunk) gradient_chunk_each<D, 1, VEC>(H, h0, chk, sink);
    if constexpr (OWNER) {
        if (a.sums) {           // wave-uniform
            sink.grad = a.sums; // the two sums are parameters 0 and 1 of a table of two words per set
            sink.S = 2;
            sink(0u, sums.s0);
            sink(1u, sums.s1);
        }
        if (a.counts) sink.count(a.counts, sums.seen, sums.cut);
    }
    sink.finish(a.excluded);
}

template <class Env, ValuePass PASS>
__global__ __launch_bounds__(kBlock) void value_kernel(const ValueArgs a, const PolicyArgs p)
{
    constexpr int VEC = 4, LPB = kBlock * VEC;
    const uint64_t base = (uint64_t)blockIdx.x * LPB + (uint64_t)threadIdx.x * VEC;
    const bool full = (uint64_t)blockIdx.x * LPB + (uint64_t)((threadIdx.x >> 6) + 1) * (64 * VEC) <= a.n; // wave-uniform, see step_kernel
    uint32_t pol[VEC] = {0, 0, 0, 0};
    bool uniform = true;
    policy_select<VEC>(p, a.gid0 + base, pol, uniform);
    if (uniform) {
        if (full)
            value_block<Env, PASS, true, true>(a, p, pol, base);
        else
            value_block<Env, PASS, true, false>(a, p, pol, base);
    } else {
        if (full)
            value_block<Env, PASS, false, true>(a, p, pol, base);
        else
            value_block<Env, PASS, false, false>(a, p, pol, base);
    }
}

// The launches for one env type.  The caller's checks (gymrs_value_gradient) are what makes every access safe: rows of `stride` >= n
// lanes, every row touched at lanes < n only (full waves: whole 4-lane groups below n); a table of n_sets * S words, S = p.stride,
// tables of n_sets * 2 words; with a hidden layer a v row of n_steps * stride floats.
template <class Env>
static hipError_t value_env(const ValueArgs& a, const PolicyArgs& p, hipStream_t stream)
{
    launch_begin();
    const uint32_t blocks = step_grid(a.n, 4);
    if (p.hidden == 0) {
        hipLaunchKernelGGL((value_kernel<Env, ValuePass::Affine>), dim3(blocks), dim3(kBlock), 0, stream, a, p);
    } else {
        const uint32_t chunks = (p.hidden + kGradientChunk - 1) / kGradientChunk;
        hipLaunchKernelGGL((value_kernel<Env, ValuePass::Forward>), dim3(blocks), dim3(kBlock), 0, stream, a, p);
        if (hipError_t err = hipGetLastError()) return err;
        hipLaunchKernelGGL((value_kernel<Env, ValuePass::Chunk>), dim3(blocks, chunks), dim3(kBlock), 0, stream, a, p); // reads the v row: stream order
    }
    return hipGetLastError();
}

} // namespace gymrs
