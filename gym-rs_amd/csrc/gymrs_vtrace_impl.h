// gymrs_vtrace_impl.h -- the kernel of gymrs_vtrace (include/gymrs_amd.h, "V-trace"): V-trace targets and policy-gradient advantages
// over a transitions record in one launch.  gfx950.  Unlike the other scans of the library (advantages_block, q_td_block) this one is
// not a column walker: only the recurrence is sequential in k, the two forward passes per lane-step are not, so they are spread over k.
//
// A workgroup of 256 work-items owns a tile of kVtraceTile = 64 consecutive lanes and walks the K rows from the top down in passes of
// kVtraceRows = 16 rows.
//   Forward phase.  Work-item t takes the 4 consecutive lanes 4 * (t % 16) of ONE row, slot t / 16 of the pass (row k_top - slot): the
//   16-byte row accesses of the other kernels are kept.  It evaluates the policy's logits and pa, V(x_cur) and -- behind the wave-level
//   "any lane truncated only" branch of advantages_block -- V(final_obs[k]), and parks what the recurrence needs in LDS as [slot][64] f32
//   planes: consecutive lanes in consecutive banks.  prob is written from here.
//   Scan phase.  After a barrier wavefront 0 scans the slots in sequence, one lane per work-item: acc and V(obs[k]) stay in registers
//   across passes (v_next of a row that went on is v_cur of the row above: the slot before, or the carry between passes; it is
//   evaluated on its own once, for obs[K-1]); every plane read is conflict-free; vs, pg_advantages and values leave as 256-byte row
//   segments.  A second barrier hands the planes back.
// The planes are single-buffered: 7 planes x 16 slots x 256 B = 28 KB per workgroup (profiles/vtrace.md says why).
// Code copies per env: uniform / gathered weights (over the tile's 64 lanes and BOTH keys: policy_select_tile) x full / ragged tile.
#pragma once
#include "gymrs_advantages_impl.h"
#include "gymrs_vtrace.h"

namespace gymrs {

struct alignas(16) VtraceLds {
    float rho[kVtraceRows][kVtraceTile], gc[kVtraceRows][kVtraceTile], rho_pg[kVtraceRows][kVtraceTile];
    float v_cur[kVtraceRows][kVtraceTile], v_fin[kVtraceRows][kVtraceTile], reward[kVtraceRows][kVtraceTile];
    uint32_t flags[kVtraceRows][kVtraceTile]; // bit 0: ended, bit 1: done, bit 2: the successor is final_obs[k] (v_fin was evaluated)
    float v_top[kVtraceTile];                 // V(obs[K - 1])
    uint32_t counts[3][kVtraceTile], set[kVtraceTile]; // per lane of the tile: the three counters, the policy set
};

template <class Env, bool UNI, bool FULL>
__device__ __forceinline__ void vtrace_block(const VtraceArgs& a, const PolicyArgs& pp, const PolicyArgs& pc, const uint32_t (&pol_p)[4],
                                             const uint32_t (&pol_c)[4], uint64_t tile0, VtraceLds& lds)
{
    constexpr int VEC = 4, D = Env::kState, A = (int)Env::kActions;
    constexpr uint32_t R = kVtraceRows;
    constexpr bool NT = true; // read-once rows and write-once outputs carry the non-temporal hint, as in advantages_block
    typedef float f4 __attribute__((ext_vector_type(4)));
    typedef uint32_t u4 __attribute__((ext_vector_type(4)));
    const uint32_t t = threadIdx.x, slot = t >> 4, lane0 = (t & 15u) * VEC;
    const uint64_t stride = a.stride, n = a.n, base = tile0 + lane0;
    const PolicyWeights<VEC, UNI> wp(pp, pol_p), wc(pc, pol_c);
    const bool has_trunc = a.truncated != nullptr, has_final = a.final_obs != nullptr;
    const bool scan = t < (uint32_t)kVtraceTile; // wavefront 0: work-item t scans lane t of the tile
    const uint64_t mine = tile0 + t;
    const bool mine_live = FULL || mine < n;

    if (t < 16) { // V(obs[K - 1]): the one successor value no row of the walk evaluates as its v_cur
        Vec<float, VEC> x[D];
#pragma unroll
        for (int j = 0; j < D; ++j) x[j] = load_vec<float, VEC, NT>(a.obs + ((uint64_t)(a.n_steps - 1) * D + j) * stride, base, n, FULL, 0.0f);
        float v[VEC];
        critic_eval<Env, VEC, UNI>(wc, pc.hidden, x, v);
        *reinterpret_cast<f4*>(&lds.v_top[lane0]) = f4{v[0], v[1], v[2], v[3]};
    }
    if (scan) {
#pragma unroll
        for (int c = 0; c < 3; ++c) lds.counts[c][t] = 0;
        lds.set[t] = (uint32_t)(((a.gid0 + mine) / pp.lanes_per_policy) % pp.n_policies);
    }
    __syncthreads();
    float acc = 0.0f, v_above = scan ? lds.v_top[t] : 0.0f; // acc[k + 1], V(obs[k])
    uint32_t cnt[3][VEC] = {};

    for (uint32_t k_top = a.n_steps - 1;; k_top -= R) {
        const uint32_t rows = k_top + 1 < R ? k_top + 1 : R; // of this pass: k_top down to k_top - rows + 1
        // ---- forward phase: slot `slot` is row k_top - slot.  A wavefront whose four slots all lie past the record's first row skips the phase
        // (wave-uniform); in a wavefront that has a row, a slot past it evaluates row 0 again: it parks planes the scan never reads (s < rows) and
        // writes neither prob nor counts
        if ((slot & ~3u) < rows) {
            const bool row_on = slot < rows;
            const uint32_t k = row_on ? k_top - slot : 0u;
            const float* prev = k ? a.obs + (uint64_t)(k - 1) * D * stride : a.start_obs;
            Vec<float, VEC> x[D];
#pragma unroll
            for (int j = 0; j < D; ++j) x[j] = load_vec<float, VEC, NT>(prev + (uint64_t)j * stride, base, n, FULL, 0.0f);
            const Vec<uint8_t, VEC> act = load_vec<uint8_t, VEC, NT>(a.actions + (uint64_t)k * stride, base, n, FULL, uint8_t(0));
            const Vec<float, VEC> po = load_vec<float, VEC, NT>(a.old_prob + (uint64_t)k * stride, base, n, FULL, 0.0f);
            const Vec<float, VEC> rew = load_vec<float, VEC, NT>(a.reward + (uint64_t)k * stride, base, n, FULL, 0.0f);
            const Vec<uint8_t, VEC> dn = load_vec<uint8_t, VEC, NT>(a.done + (uint64_t)k * stride, base, n, FULL, uint8_t(0));
            Vec<uint8_t, VEC> tr{};
            if (has_trunc) tr = load_vec<uint8_t, VEC, NT>(a.truncated + (uint64_t)k * stride, base, n, FULL, uint8_t(0));

            float y[A][VEC], v_cur[VEC], v_fin[VEC];
            policy_logits<Env, VEC, UNI>(wp, pp.hidden, x, y);
            critic_eval<Env, VEC, UNI>(wc, pc.hidden, x, v_cur);
            bool ended[VEC], fin = false;
#pragma unroll
            for (int i = 0; i < VEC; ++i) {
                ended[i] = dn.v[i] != 0 || tr.v[i] != 0;
                v_fin[i] = 0.0f;
            }
            if (has_final) {
                bool need = false; // truncated only: the successor is the observation the episode ended in
#pragma unroll
                for (int i = 0; i < VEC; ++i) need = need || (ended[i] && dn.v[i] == 0);
                if (__any(need)) { // (a done step selects +0.0f whether v_fin was evaluated or not)
                    Vec<float, VEC> xf[D];
#pragma unroll
                    for (int j = 0; j < D; ++j) xf[j] = load_vec<float, VEC, NT>(a.final_obs + ((uint64_t)k * D + j) * stride, base, n, FULL, 0.0f);
                    critic_eval<Env, VEC, UNI>(wc, pc.hidden, xf, v_fin);
                    fin = true;
                }
            }
            f4 p_rho, p_gc, p_pg, p_vc, p_vf, p_rw;
            u4 p_fl;
            Vec<float, VEC> pr;
#pragma unroll
            for (int i = 0; i < VEC; ++i) {
                float yl[A];
#pragma unroll
                for (int b = 0; b < A; ++b) yl[b] = y[b][i];
                const float pa = vtrace_prob<A>(yl, act.v[i], a.scale);
                const bool valid = act.v[i] < (uint8_t)A;
                const VtraceWeights w = vtrace_weights(pa, po.v[i], valid, a.gamma, a.lambda, a.rho_bar, a.c_bar, a.pg_rho_bar);
                pr.v[i] = pa; // (+0.0f where the action is none of the A)
                p_rho[i] = w.rho;
                p_gc[i] = w.gc;
                p_pg[i] = w.rho_pg;
                p_vc[i] = v_cur[i];
                p_vf[i] = v_fin[i];
                p_rw[i] = rew.v[i];
                p_fl[i] = (ended[i] ? 1u : 0u) | (dn.v[i] != 0 ? 2u : 0u) | (fin && ended[i] ? 4u : 0u);
                const bool counted = row_on && (FULL || base + i < n);
                cnt[0][i] += counted && valid ? 1u : 0u;
                cnt[1][i] += counted && w.over_rho ? 1u : 0u;
                cnt[2][i] += counted && w.over_c ? 1u : 0u;
            }
            *reinterpret_cast<f4*>(&lds.rho[slot][lane0]) = p_rho;
            *reinterpret_cast<f4*>(&lds.gc[slot][lane0]) = p_gc;
            *reinterpret_cast<f4*>(&lds.rho_pg[slot][lane0]) = p_pg;
            *reinterpret_cast<f4*>(&lds.v_cur[slot][lane0]) = p_vc;
            *reinterpret_cast<f4*>(&lds.v_fin[slot][lane0]) = p_vf;
            *reinterpret_cast<f4*>(&lds.reward[slot][lane0]) = p_rw;
            *reinterpret_cast<u4*>(&lds.flags[slot][lane0]) = p_fl;
            if (a.prob && row_on) store_vec<float, VEC, NT>(a.prob + (uint64_t)k * stride, base, n, FULL, pr);
        }
        __syncthreads();

        // ---- scan phase: the recurrence, one lane per work-item of wavefront 0
        if (scan) {
            for (uint32_t s = 0; s < rows; ++s) {
                const uint32_t fl = lds.flags[s][t];
                const float vc = lds.v_cur[s][t];
                const float v_succ = (fl & 4u) ? lds.v_fin[s][t] : v_above;
                float vs, pg;
                vtrace_step(a.gamma, lds.reward[s][t], (fl & 2u) != 0, (fl & 1u) != 0, v_succ, vc, lds.rho[s][t], lds.gc[s][t], lds.rho_pg[s][t], acc, vs,
                            pg);
                v_above = vc;
                if (mine_live) {
                    const uint64_t at = (uint64_t)(k_top - s) * stride + mine;
                    __builtin_nontemporal_store(vs, a.vs + at);
                    __builtin_nontemporal_store(pg, a.pg + at);
                    if (a.values) __builtin_nontemporal_store(vc, a.values + at);
                }
            }
        }
        __syncthreads(); // the planes are free for the next pass
        if (k_top < R) break;
    }

    // ---- counts: per lane of the tile in LDS, then one atomic per counter and set the tile touches: the first lane of a set collects its lanes
    if (a.counts) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
#pragma unroll
            for (int i = 0; i < VEC; ++i)
                if (cnt[c][i]) (void)__hip_atomic_fetch_add(&lds.counts[c][lane0 + i], cnt[c][i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        __syncthreads();
        if (scan) {
            const uint32_t set = lds.set[t];
            bool first = true;
            for (uint32_t j = 0; j < t; ++j) first = first && lds.set[j] != set;
            if (first) {
                unsigned long long sum[3] = {0, 0, 0};
                for (uint32_t j = t; j < (uint32_t)kVtraceTile; ++j) {
                    const bool same = lds.set[j] == set;
#pragma unroll
                    for (int c = 0; c < 3; ++c) sum[c] += same ? lds.counts[c][j] : 0u;
                }
#pragma unroll
                for (int c = 0; c < 3; ++c) atomic_add_nonzero(a.counts + (uint64_t)set * 3 + c, sum[c]);
            }
        }
    }
}

template <class Env>
__global__ __launch_bounds__(kBlock) void vtrace_kernel(const VtraceArgs a, const PolicyArgs pp, const PolicyArgs pc)
{
    __shared__ VtraceLds lds;
    const uint64_t tile0 = (uint64_t)blockIdx.x * kVtraceTile, base = tile0 + (threadIdx.x & 15u) * 4;
    const bool full = tile0 + kVtraceTile <= a.n; // workgroup-uniform
    uint32_t pol_p[4], pol_c[4];
    bool uni_p, uni_c;
    policy_select_tile<4, kVtraceTile>(pp, a.gid0 + base, a.gid0 + tile0, pol_p, uni_p);
    policy_select_tile<4, kVtraceTile>(pc, a.gid0 + base, a.gid0 + tile0, pol_c, uni_c);
    if (uni_p && uni_c) {
        if (full)
            vtrace_block<Env, true, true>(a, pp, pc, pol_p, pol_c, tile0, lds);
        else
            vtrace_block<Env, true, false>(a, pp, pc, pol_p, pol_c, tile0, lds);
    } else {
        if (full)
            vtrace_block<Env, false, true>(a, pp, pc, pol_p, pol_c, tile0, lds);
        else
            vtrace_block<Env, false, false>(a, pp, pc, pol_p, pol_c, tile0, lds);
    }
}

// The launch for one env type.  The caller's checks (gymrs_vtrace) are what makes every access safe: rows of `stride` >= n lanes,
// every row touched at lanes < n only (full tiles: whole 4-lane groups below n).
template <class Env>
static hipError_t vtrace_env(const VtraceArgs& a, const PolicyArgs& policy, const PolicyArgs& critic, hipStream_t stream)
{
    static_assert(kBlock == 4 * kVtraceTile && kBlock / 16 == (int)kVtraceRows, "16 work-items per row, one pass per trip of the workgroup");
    launch_begin();
    hipLaunchKernelGGL((vtrace_kernel<Env>), dim3((uint32_t)((a.n + kVtraceTile - 1) / kVtraceTile)), dim3(kBlock), 0, stream, a, policy, critic);
    return hipGetLastError();
}

} // namespace gymrs
