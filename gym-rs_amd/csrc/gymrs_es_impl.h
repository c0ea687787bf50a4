// gymrs_es_impl.h -- the kernels of gymrs_es_init and gymrs_es_step (include/gymrs_amd.h, "Evolution strategies"): the utilities of a
// population from its evaluation records, the gradient of the centre from the utilities and the regenerated noise, and the update of
// the centre fused with the population of the next generation.  gfx950.  The noise is never stored: both kernels that need eps(gen, j, s)
// evaluate its Philox block again (one block per pair and parameter, 82 VALU instructions of rounds against 8 bytes of traffic each way).
//
// Utilities (es_utilities_kernel<PASS>, three launches of one block of 1024 work-items per chunk).  The rule's butterfly over the 1024
// slots of a chunk runs mask = 512 .. 64 FIRST, so the exchanges between waves come before those inside one.  es_butterfly therefore
// parks the 1024 values in LDS, every wave reads the 16 values of its lane position and folds them in the order wave 0 meets them
// (IEEE addition commutes, so every wave would end with the same bits; taking wave 0's order makes that literal), and masks 32 .. 1 are
// __shfl_xor exchanges of the double in registers.  Every work-item ends with slot[0].  Pass 0 reads the records (two 16-byte
// non-temporal loads of the 64: return_sum and episodes), leaves F[p] (NaN = not valid) in an engine-owned f64 row so that the 64-byte
// records are read once instead of three times, and writes the chunk's sum and count.  Passes 1 and 2 start by folding the at most
// 1024 chunk entries with the same function.  DEVIATION from "a final block reduces the scratch": every block folds the chunk entries
// itself (1024 loads that hit L2) -- the same bits in every block, and two launches of a single block less per step.
//
// Gradient (es_gradient_kernel; the hot one: P/2 * S Philox blocks).  A block of 256 work-items owns 256 consecutive pairs, lane =
// pair: d = u[2j] - u[2j+1] is loaded once and stays in a register while the block walks s.  Per s: one Philox4x32-10 block per
// lane, the integer halves-sum, one multiply, the fixed-point conversion, and an exact 64-bit wave sum in three DPP limbs
// (wave_sum_i64).  Each wave writes its sum to a row of its own in LDS (every (wave, s) is written exactly once: no LDS atomics),
// and after the walk the block adds the four rows and issues one 64-bit global atomic per parameter with a non-zero sum.  Integer
// adds commute: G does not depend on the order.  A population with few pairs is also cut along s (blockIdx.y) so that the grid
// still fills the device; a wave wholly past the last pair writes zeros and evaluates nothing, a ragged lane multiplies by d = +0.0f.
//
// Update and population (es_population_kernel<UPDATE, ADAM, CLIP>).  Block b owns the pairs [b * tile, (b + 1) * tile) and with them
// the contiguous floats [2 * b * tile * S, ..) of the policy set (tile is even: the range starts 16-byte aligned).  Every block
// computes theta' into LDS from the read-only half (gen & 1) of the state -- S <= 450 is two parameters per work-item, and the norm
// is the optimizer's 64 slots: squares parked in LDS, folded in ascending s per lane position, then the __shfl_xor butterfly.
// Block 0 alone stores theta', m', v', pw' into the OTHER half and zeroes that half's G and excluded for the next step, so no block
// reads what another writes in the same launch (G is a ping-pong pair for this reason too: the step's own half is still being read).
// A skipped step copies the old bytes across.  Then every block draws eps(gen + 1, j, s) for its pairs, forms both signs, stages the
// rows in LDS and stores them as 16-byte writes.  UPDATE = false is gymrs_es_init: theta comes from half 0 as the host left it.
#pragma once
#include <hip/hip_runtime.h>

#include "gymrs_es.h"
#include "gymrs_kernels.h"
#include "gymrs_optimizer.h"
#include "gymrs_tile.h"

namespace gymrs {

constexpr int kEsBlock = 256;        // four waves: the gradient and the population kernels
constexpr int kEsMaxTilePairs = 256; // pairs per block of the population kernel, at most
constexpr uint32_t kEsTileItems = 4096; // (pair, parameter) draws per block of the population kernel, about: 2 * 4096 staged floats
static_assert(kEsChunk == 1024 && kEsSlots == 2 * kEsBlock, "a chunk is one block of 1024; a work-item of the update holds two parameters");

typedef unsigned long long es_ull2 __attribute__((ext_vector_type(2)));

// slot[0] of `slot[l] += slot[l ^ mask]`, mask = 512 .. 1, over the values of the block's 1024 work-items; every work-item gets it.
__device__ __forceinline__ double es_butterfly(double v, double* lds)
{
    const uint32_t lane = threadIdx.x & 63u;
    __syncthreads(); // (the previous round's reads are over)
    lds[threadIdx.x] = v;
    __syncthreads();
    double x[16];
#pragma unroll
    for (int w = 0; w < 16; ++w) x[w] = lds[w * 64 + lane];
#pragma unroll
    for (int half = 8; half >= 1; half >>= 1) { // masks 512, 256, 128, 64 as wave 0 meets them
#pragma unroll
        for (int w = 0; w < half; ++w) x[w] = x[w] + x[w ^ half];
    }
    double s = x[0];
#pragma unroll
    for (int mask = 32; mask >= 1; mask >>= 1) s = s + __shfl_xor(s, mask, 64);
    return s;
}

template <int PASS>
__global__ __launch_bounds__(kEsChunk) void es_utilities_kernel(const EsArgs a)
{
    __shared__ double lds[kEsChunk];
    const uint32_t l = threadIdx.x, c = blockIdx.x, n_chunks = gridDim.x;
    const uint32_t p = c * kEsChunk + l; // (P <= 2^20: no overflow)
    const bool live = p < a.P;
    EsDeviceState& st = *a.st;
    if constexpr (PASS == 0) {
        bool valid = false;
        double F = 0.0;
        if (live) {
            const es_ull2* rec = reinterpret_cast<const es_ull2*>(static_cast<const char*>(a.records) + (size_t)p * 64u);
            const es_ull2 r0 = __builtin_nontemporal_load(rec), r1 = __builtin_nontemporal_load(rec + 1); // {return_sum, ..}, {episodes, ..}
            valid = r1.x != 0ull;
            if (valid) F = es_fitness((long long)r0.x, r1.x);
            a.fitness[p] = valid ? F : __builtin_nan("");
        }
        const double sum = es_butterfly(valid ? F : 0.0, lds);
        const double count = es_butterfly(valid ? 1.0 : 0.0, lds);
        if (l == 0) {
            st.chunk_sum[c] = sum;
            st.chunk_count[c] = count;
        }
    } else {
        const double F = live ? a.fitness[p] : __builtin_nan("");
        const bool valid = F == F;
        const double total = es_butterfly(l < n_chunks ? st.chunk_sum[l] : 0.0, lds);
        const double n_valid = es_butterfly(l < n_chunks ? st.chunk_count[l] : 0.0, lds); // (integers below 2^53: exact)
        const double mean = total / n_valid;
        if constexpr (PASS == 1) {
            const double dev = F - mean;
            const double sq = es_butterfly(valid ? dev * dev : 0.0, lds);
            if (l == 0) st.chunk_sq[c] = sq;
        } else {
            const double total2 = es_butterfly(l < n_chunks ? st.chunk_sq[l] : 0.0, lds);
            const double sd = es_sd(total2, n_valid);
            if (live) a.u[p] = es_utility(valid, F, mean, sd);
        }
    }
}

__global__ __launch_bounds__(kEsBlock) void es_gradient_kernel(const EsArgs a, const uint32_t s_per_block)
{
    __shared__ unsigned long long rows[kEsBlock / 64][kEsSlots];
    const uint32_t t = threadIdx.x, wave = t >> 6, lane = t & 63u;
    const uint32_t pairs = a.P >> 1;
    const uint32_t j = blockIdx.x * kEsBlock + t;
    const bool live = j < pairs;
    const bool wave_live = blockIdx.x * kEsBlock + wave * 64u < pairs; // wave-uniform
    const uint32_t s0 = blockIdx.y * s_per_block, s1 = min(a.S, s0 + s_per_block);
    EsDeviceState& st = *a.st;
    const uint32_t half = (uint32_t)a.gen & 1u;

    float d = 0.0f;
    if (live) {
        const float* src = a.u_in ? a.u_in : a.u;
        const float u0 = src[2u * j], u1 = src[2u * j + 1u];
        d = u0 - u1;
        if (a.u_in && blockIdx.y == 0) { // what the step used, kept for gymrs_es_utilities_ptr
            a.u[2u * j] = u0;
            a.u[2u * j + 1u] = u1;
        }
    }
    uint32_t excl = 0;
    if (wave_live) {
        for (uint32_t s = s0; s < s1; ++s) {
            long long q;
            const bool ok = es_term(d, es_noise(a.seed, a.gen, j, s), q);
            excl += (live && !ok) ? 1u : 0u;
            const long long total = wave_sum_i64(live ? q : 0ll);
            if (lane == 0) rows[wave][s - s0] = (unsigned long long)total;
        }
    } else {
        for (uint32_t s = s0 + lane; s < s1; s += 64u) rows[wave][s - s0] = 0ull;
    }
    __syncthreads();
    for (uint32_t s = s0 + t; s < s1; s += kEsBlock) {
        unsigned long long sum = rows[0][s - s0];
#pragma unroll
        for (int w = 1; w < kEsBlock / 64; ++w) sum += rows[w][s - s0];
        atomic_add_nonzero(&st.grad[half][s], sum);
    }
    const uint32_t wave_excl = wave_sum_u32(excl);
    if (lane == 0) atomic_add_nonzero(&st.excluded[half][0], (unsigned long long)wave_excl);
}

template <bool UPDATE, bool ADAM, bool CLIP>
__global__ __launch_bounds__(kEsBlock) void es_population_kernel(const EsArgs a, const uint32_t tile_pairs)
{
    __shared__ float theta_s[kEsSlots];
    __shared__ double sq[kEsSlots];
    extern __shared__ float4 stage4[]; // 2 * tile_pairs * S floats, rounded up to 16 bytes
    float* const stage = reinterpret_cast<float*>(stage4);
    const uint32_t t = threadIdx.x, lane = t & 63u, S = a.S;
    EsDeviceState& st = *a.st;
    const bool lead = blockIdx.x == 0;
    const uint32_t cur = UPDATE ? ((uint32_t)a.gen & 1u) : 0u, nxt = cur ^ 1u;
    const uint64_t gen_new = UPDATE ? a.gen + 1 : a.gen;

    if constexpr (UPDATE) {
        const bool skip = st.excluded[cur][0] != 0ull, ascend = (a.flags & GYMRS_OPT_ASCEND) != 0;
        // (the Adam state crosses to the other half under SGD as well, unchanged: a later Adam step finds it where it looks)
        float p1 = st.pw[cur][0], p2 = st.pw[cur][1], c1 = 1.0f, c2 = 1.0f;
        const float p1_old = p1, p2_old = p2;
        float g[2], th[2], mo[2], vo[2];
        bool on[2];
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const uint32_t s = t + (uint32_t)(kEsBlock * k);
            on[k] = s < S;
            const uint32_t at = on[k] ? s : 0u;
            g[k] = opt_gradient(on[k] ? (long long)st.grad[cur][at] : 0ll, a.grad_scale);
            th[k] = st.theta[cur][at];
            mo[k] = st.m[cur][at];
            vo[k] = st.v[cur][at];
        }
        if constexpr (CLIP) {
            sq[t] = opt_square(g[0]);
            sq[t + kEsBlock] = opt_square(g[1]);
            __syncthreads();
            double sum = 0.0;
#pragma unroll
            for (int k = 0; k < (int)kEsSlots / 64; ++k) sum = sum + sq[lane + 64u * k]; // slot[lane]: ascending s
#pragma unroll
            for (int mask = 32; mask >= 1; mask >>= 1) sum = sum + __shfl_xor(sum, mask, 64);
            bool clipped;
            const float cs = opt_clip_scale(sum, a.max_norm, clipped);
#pragma unroll
            for (int k = 0; k < 2; ++k) g[k] = clipped ? g[k] * cs : g[k];
        }
        if constexpr (ADAM) opt_adam_advance(a.beta1, a.beta2, p1, p2, c1, c2);
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const uint32_t s = t + (uint32_t)(kEsBlock * k);
            const float m_old = mo[k], v_old = vo[k];
            float step;
            if constexpr (ADAM)
                step = opt_adam_step(g[k], a.lr, a.beta1, a.beta2, a.eps, c1, c2, mo[k], vo[k]);
            else
                step = opt_sgd_step(g[k], a.lr);
            const float wn = skip ? th[k] : opt_apply(th[k], step, ascend);
            if (on[k]) {
                theta_s[s] = wn;
                if (lead) {
                    st.theta[nxt][s] = wn;
                    st.centre[s] = wn;
                    st.m[nxt][s] = (ADAM && !skip) ? mo[k] : m_old;
                    st.v[nxt][s] = (ADAM && !skip) ? vo[k] : v_old;
                    st.grad[nxt][s] = 0ull;
                }
            }
        }
        if (lead && t == 0) {
            st.pw[nxt][0] = (ADAM && !skip) ? p1 : p1_old;
            st.pw[nxt][1] = (ADAM && !skip) ? p2 : p2_old;
            st.excluded[nxt][0] = 0ull;
            if (skip && a.skipped) atomic_add_nonzero(a.skipped, 1ull);
        }
    } else {
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const uint32_t s = t + (uint32_t)(kEsBlock * k);
            const float w = st.theta[0][s]; // (a slot at or past S holds whatever it holds: read, never used)
            if (s < S) theta_s[s] = w;
            if (lead) { // the whole state, fresh: every slot
                st.centre[s] = s < S ? w : 0.0f;
                st.m[0][s] = 0.0f;
                st.v[0][s] = 0.0f;
                st.grad[0][s] = 0ull;
                st.grad[1][s] = 0ull;
            }
        }
        if (lead && t == 0) {
            st.pw[0][0] = 1.0f;
            st.pw[0][1] = 1.0f;
            st.excluded[0][0] = 0ull;
            st.excluded[1][0] = 0ull;
        }
    }
    __syncthreads(); // theta_s is whole

    const uint32_t pairs = a.P >> 1, j0 = blockIdx.x * tile_pairs;
    const uint32_t nj = min(tile_pairs, pairs - j0), items = nj * S; // (the grid has no block past the last pair)
    uint32_t jl = t / S, s = t - jl * S;
    const uint32_t dj = (uint32_t)kEsBlock / S, ds = (uint32_t)kEsBlock - dj * S; // item i + 256 from item i without a division
    for (uint32_t i = t; i < items; i += kEsBlock) {
        float plus, minus;
        es_members(a.sigma_new, es_noise(a.seed, gen_new, (uint64_t)(j0 + jl), s), theta_s[s], plus, minus);
        stage[(2u * jl) * S + s] = plus;
        stage[(2u * jl + 1u) * S + s] = minus;
        jl += dj;
        s += ds;
        if (s >= S) {
            s -= S;
            jl += 1u;
        }
    }
    __syncthreads();
    const uint64_t base = (uint64_t)2u * j0 * S; // a multiple of 4 floats: tile_pairs is even
    const uint32_t n_floats = 2u * items, n4 = n_floats / 4u;
    float4* const out4 = reinterpret_cast<float4*>(a.weights + base);
    for (uint32_t i = t; i < n4; i += kEsBlock) out4[i] = stage4[i];
    for (uint32_t i = n4 * 4u + t; i < n_floats; i += kEsBlock) a.weights[base + i] = stage[i]; // the last block's tail of up to 3 floats
}

// the tile of the population kernel: an even number of pairs with about kEsTileItems draws
inline uint32_t es_tile_pairs(uint32_t S)
{
    uint32_t tile = (kEsTileItems / S) & ~1u;
    tile = tile < 2u ? 2u : tile;
    return tile > (uint32_t)kEsMaxTilePairs ? (uint32_t)kEsMaxTilePairs : tile;
}

template <bool UPDATE, bool ADAM, bool CLIP>
static hipError_t es_launch_population(const EsArgs& a, hipStream_t stream)
{
    const uint32_t tile = es_tile_pairs(a.S), pairs = a.P >> 1;
    const size_t lds = (((size_t)2 * tile * a.S * sizeof(float)) + 15) & ~(size_t)15;
    launch_begin();
    hipLaunchKernelGGL((es_population_kernel<UPDATE, ADAM, CLIP>), dim3((pairs + tile - 1) / tile), dim3(kEsBlock), lds, stream, a, tile);
    return hipGetLastError();
}

} // namespace gymrs
