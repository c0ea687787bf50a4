// gymrs_replay_impl.h -- the kernels of include/gymrs_amd.h, "Replay": push, the draw with its gather, and the priority update.
// gfx950.  Everything the draw computes is an integer, so the result depends neither on scheduling nor on the tiling.
//
// The draw over a store of more than one tile of T = 4096 priorities is three launches in stream order, workgroups of 256:
//   replay_sum_kernel     one workgroup per tile.  A work-item takes 16 entries as four 16-byte loads (entry 4 (l + 256 k) + c: the
//                         lanes of a wave read 1 KB in a row), entries >= count weigh 0; the sums fold inside the wave with cross-lane
//                         swaps and across the four waves through 32 bytes of LDS.  One uint64 per tile.
//   replay_base_kernel    ONE workgroup turns the at most 2^14 tile sums into exclusive bases and the total.  DEVIATION from "scan them
//                         in LDS": a work-item folds a run of ceil(tiles / 256) <= 64 sums from global memory, the 256 run totals are
//                         scanned (cross-lane, then the four wave totals), and the run is walked again for the bases.  2^14 uint64 are
//                         128 KB, twice what a workgroup declares statically, and the common store (2^22: 1024 tiles) has runs of four.
//   replay_locate_kernel  one workgroup per tile again.  A work-item reloads 16 CONSECUTIVE entries (four 16-byte loads from its own
//                         64 bytes), the workgroup scans the 256 totals as above and every work-item writes its 16 inclusive prefixes
//                         to LDS as uint64 (32 KB: 4096 priorities of 2^24 sum to 2^36).  The strata ascend, so the samples of a tile
//                         are ONE run of j: from the stratum that holds `base` to the one that holds `base + sum - 1` (closed form,
//                         replay_stratum_of; the tile that ends the mass takes everything up to B - 1, which is where the empty strata
//                         of T < B land).  Work-items stride over that run in groups of four samples -- one Philox block serves
//                         j = 4g .. 4g + 3 --, recompute u_j, drop what is outside [base, base + sum), find the entry with 12
//                         branch-free probes of the LDS prefix and gather the transition's 2 D + 3 values into lane j of the batch:
//                         writes coalesced in j, reads scattered.  A tile that holds all the mass walks all B samples this way.
//                         The searched sum is the one the workgroup has just rebuilt, not the scratch's: a probe can then only stop at
//                         an entry of non-zero priority, which is below count.
// A store of one tile is ONE launch of replay_locate_kernel<.., true>: base 0, the total from its own scan, no scratch.
// NOT DONE: the 16 LDS prefix stores of a work-item are 128 bytes apart from its neighbour's and collide in the banks; a transposed
// ownership would cost the coalesced reload.  The kernel moves 4 B per entry and is bound by its launch and the scattered gather.
//
// replay_push_kernel<D>: a work-item takes four lanes of one step.  Where the ring position is a multiple of four (then the four
// slots do not wrap: the capacity is a multiple of 16) and the four lanes exist, every row moves as one 16-byte (4-byte for the u8
// rows) access; otherwise lane by lane with the wrap.  replay_update_kernel: one work-item per sample.
#pragma once
#include <hip/hip_runtime.h>

#include "gymrs_kernels.h"
#include "gymrs_replay.h"

namespace gymrs {

constexpr uint32_t kReplayBlock = 256;
constexpr uint32_t kReplayPer = kReplayTile / kReplayBlock; // priorities per work-item
static_assert(kReplayPer == 16 && kReplayBlock == 4 * 64, "four 16-byte loads per work-item, four waves per workgroup");

typedef uint32_t replay_u4 __attribute__((ext_vector_type(4)));
typedef float replay_f4 __attribute__((ext_vector_type(4)));

// Four priorities at entry `at` (a multiple of 4), those at or beyond count as 0.  at < count <= capacity and the capacity is a multiple
// of 16, so the 16 bytes are inside the row.
__device__ __forceinline__ replay_u4 replay_load4(const uint32_t* priority, uint64_t at, uint64_t count)
{
    replay_u4 v = {0u, 0u, 0u, 0u};
    if (at < count) v = *reinterpret_cast<const replay_u4*>(priority + at);
    v.y = at + 1u < count ? v.y : 0u;
    v.z = at + 2u < count ? v.z : 0u;
    v.w = at + 3u < count ? v.w : 0u;
    return v;
}

// The inclusive scan of one value per work-item over the workgroup (wave_tot: 4 words of LDS; one barrier); all = the workgroup's sum.
__device__ __forceinline__ unsigned long long replay_block_scan(unsigned long long v, unsigned long long* wave_tot, unsigned long long& all)
{
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    unsigned long long inc = v;
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const unsigned long long o = __shfl_up(inc, d, 64);
        inc += lane >= d ? o : 0ull;
    }
    if (lane == 63u) wave_tot[w] = inc;
    __syncthreads();
    unsigned long long before = 0ull;
    all = 0ull;
#pragma unroll
    for (uint32_t i = 0; i < kReplayBlock / 64u; ++i) {
        const unsigned long long t = wave_tot[i];
        before += i < w ? t : 0ull;
        all += t;
    }
    return inc + before;
}

__global__ __launch_bounds__(kReplayBlock) void replay_sum_kernel(const ReplaySampleArgs a)
{
    __shared__ unsigned long long wave_tot[kReplayBlock / 64u];
    const uint32_t l = threadIdx.x;
    const uint64_t base = (uint64_t)blockIdx.x * kReplayTile;
    unsigned long long sum = 0ull;
#pragma unroll
    for (uint32_t k = 0; k < kReplayPer / 4u; ++k) {
        const replay_u4 v = replay_load4(a.st.priority, base + 4u * (l + kReplayBlock * k), a.count);
        sum += (unsigned long long)v.x + v.y + v.z + v.w;
    }
#pragma unroll
    for (uint32_t d = 32; d >= 1u; d >>= 1) sum += __shfl_xor(sum, d, 64);
    if ((l & 63u) == 0u) wave_tot[l >> 6] = sum;
    __syncthreads();
    if (l == 0) a.scratch[blockIdx.x] = wave_tot[0] + wave_tot[1] + wave_tot[2] + wave_tot[3];
}

// sums [tiles] -> bases [tiles] (exclusive) and the total, by one workgroup
__global__ __launch_bounds__(kReplayBlock) void replay_base_kernel(const ReplaySampleArgs a, const uint32_t tiles)
{
    __shared__ unsigned long long wave_tot[kReplayBlock / 64u];
    const unsigned long long* sums = a.scratch;
    unsigned long long* bases = a.scratch + kReplayMaxTiles;
    const uint32_t run = (tiles + kReplayBlock - 1u) / kReplayBlock, first = threadIdx.x * run;
    unsigned long long mine = 0ull;
    for (uint32_t t = first; t < first + run && t < tiles; ++t) mine += sums[t];
    unsigned long long all;
    unsigned long long at = replay_block_scan(mine, wave_tot, all) - mine;
    for (uint32_t t = first; t < first + run && t < tiles; ++t) {
        bases[t] = at;
        at += sums[t];
    }
    if (threadIdx.x == 0) {
        a.scratch[2u * kReplayMaxTiles] = all;
        *a.total = all;
    }
}

// a draw from a store without mass: every idx is kReplayNone, every prio 0, the batch keeps its bytes
__device__ __forceinline__ void replay_no_mass(const ReplaySampleArgs& a)
{
    for (uint32_t j = threadIdx.x; j < a.B; j += kReplayBlock) {
        a.idx[j] = kReplayNone;
        if (a.prio) a.prio[j] = 0u;
    }
}

template <int D, bool SINGLE>
__global__ __launch_bounds__(kReplayBlock) void replay_locate_kernel(const ReplaySampleArgs a)
{
    __shared__ unsigned long long pre[kReplayTile];
    __shared__ unsigned long long wave_tot[kReplayBlock / 64u];
    const uint32_t l = threadIdx.x;
    const uint64_t first = (uint64_t)blockIdx.x * kReplayTile; // the tile's first entry
    unsigned long long base = 0ull, T = 0ull;
    if constexpr (!SINGLE) {
        T = a.scratch[2u * kReplayMaxTiles];
        if (T == 0ull) { // (uniform)
            if (blockIdx.x == 0) replay_no_mass(a);
            return;
        }
        if (a.scratch[blockIdx.x] == 0ull) return; // nothing is drawn from an empty tile
        base = a.scratch[kReplayMaxTiles + blockIdx.x];
    }

    uint32_t p[kReplayPer];
    unsigned long long mine = 0ull;
#pragma unroll
    for (uint32_t k = 0; k < kReplayPer / 4u; ++k) {
        const replay_u4 v = replay_load4(a.st.priority, first + kReplayPer * l + 4u * k, a.count);
        p[4u * k] = v.x, p[4u * k + 1u] = v.y, p[4u * k + 2u] = v.z, p[4u * k + 3u] = v.w;
        mine += (unsigned long long)v.x + v.y + v.z + v.w;
    }
    unsigned long long sum;
    unsigned long long at = replay_block_scan(mine, wave_tot, sum) - mine;
#pragma unroll
    for (uint32_t k = 0; k < kReplayPer; ++k) {
        at += p[k];
        pre[kReplayPer * l + k] = at;
    }
    if constexpr (SINGLE) {
        T = sum;
        if (l == 0) *a.total = T;
        if (T == 0ull) {
            replay_no_mass(a);
            return;
        }
    }
    __syncthreads();
    if (sum == 0ull) return;

    const ReplayStrata strata = replay_strata(T, a.B);
    const uint32_t j_first = replay_stratum_of(strata, base < T ? base : T - 1u);
    const uint32_t j_last = base + sum >= T ? a.B - 1u : replay_stratum_of(strata, base + sum - 1u);
    for (uint32_t g = (j_first >> 2) + l; g <= (j_last >> 2); g += kReplayBlock) {
        const u32x4 words = replay_block(a.seed, a.draw, g);
#pragma unroll
        for (uint32_t c = 0; c < 4u; ++c) {
            const uint32_t j = 4u * g + c;
            if (j >= a.B) continue;
            const unsigned long long u = replay_point(strata, words.v[c], j);
            if (u < base || u - base >= sum) continue; // another tile's
            const unsigned long long t = u - base;
            uint32_t pos = 0; // the smallest entry with pre > t; t < sum = pre[T - 1], so 12 probes end on it
#pragma unroll
            for (uint32_t s = kReplayTile / 2u; s >= 1u; s >>= 1) pos += pre[pos + s - 1u] <= t ? s : 0u;
            const uint64_t e = first + pos;
            if (e >= a.count) continue; // (cannot be: the entry has a non-zero priority)
            a.idx[j] = (uint32_t)e;
            if (a.prio) a.prio[j] = a.st.priority[e];
#pragma unroll
            for (int d = 0; d < D; ++d) {
                a.start_obs[(uint64_t)d * a.stride + j] = a.st.s[(uint64_t)d * a.st.capacity + e];
                a.obs[(uint64_t)d * a.stride + j] = a.st.s_next[(uint64_t)d * a.st.capacity + e];
            }
            a.actions[j] = a.st.action[e];
            a.reward[j] = a.st.reward[e];
            a.done[j] = a.st.done[e];
        }
    }
}

template <int D>
__global__ __launch_bounds__(kReplayBlock) void replay_push_kernel(const ReplayPushArgs a, const uint32_t groups)
{
    const uint64_t gid = (uint64_t)blockIdx.x * kReplayBlock + threadIdx.x;
    const uint64_t k = gid / groups, i = 4u * (gid % groups);
    if (k >= a.n_steps) return;
    const uint64_t cap = a.st.capacity, row = k * a.stride + i;
    uint64_t pos = a.head + k * a.n + i; // head < cap and k * n + i < K * n <= cap: one subtraction wraps
    pos = pos >= cap ? pos - cap : pos;
    const float* x = k == 0 ? a.start_obs : a.obs + (k - 1u) * D * a.stride; // [D][stride]: the observation before step k
    const float* xn = a.obs + k * D * a.stride;
    const float* xf = a.final_obs + k * D * a.stride;

    if (i + 3u < a.n && (pos & 3u) == 0u) {
        const uint32_t dn = *reinterpret_cast<const uint32_t*>(a.done + row);
        const uint32_t ended = dn | (a.truncated ? *reinterpret_cast<const uint32_t*>(a.truncated + row) : 0u);
#pragma unroll
        for (int d = 0; d < D; ++d) {
            *reinterpret_cast<replay_f4*>(a.st.s + (uint64_t)d * cap + pos) = *reinterpret_cast<const replay_f4*>(x + (uint64_t)d * a.stride + i);
            replay_f4 o = *reinterpret_cast<const replay_f4*>(xn + (uint64_t)d * a.stride + i);
            if (ended != 0u) {
                const replay_f4 f = *reinterpret_cast<const replay_f4*>(xf + (uint64_t)d * a.stride + i);
                o.x = (ended & 0x000000ffu) ? f.x : o.x;
                o.y = (ended & 0x0000ff00u) ? f.y : o.y;
                o.z = (ended & 0x00ff0000u) ? f.z : o.z;
                o.w = (ended & 0xff000000u) ? f.w : o.w;
            }
            *reinterpret_cast<replay_f4*>(a.st.s_next + (uint64_t)d * cap + pos) = o;
        }
        *reinterpret_cast<uint32_t*>(a.st.action + pos) = *reinterpret_cast<const uint32_t*>(a.actions + row);
        *reinterpret_cast<replay_f4*>(a.st.reward + pos) = *reinterpret_cast<const replay_f4*>(a.reward + row);
        *reinterpret_cast<uint32_t*>(a.st.done + pos) =
            ((dn & 0x000000ffu) ? 0x00000001u : 0u) | ((dn & 0x0000ff00u) ? 0x00000100u : 0u) | ((dn & 0x00ff0000u) ? 0x00010000u : 0u) |
            ((dn & 0xff000000u) ? 0x01000000u : 0u);
        const replay_u4 pr = {a.priority, a.priority, a.priority, a.priority};
        *reinterpret_cast<replay_u4*>(a.st.priority + pos) = pr;
        return;
    }
    for (uint32_t c = 0; c < 4u && i + c < a.n; ++c) {
        uint64_t e = pos + c;
        e = e >= cap ? e - cap : e;
        const uint64_t at = row + c;
        const bool ended = a.done[at] != 0 || (a.truncated && a.truncated[at] != 0);
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const uint64_t col = (uint64_t)d * a.stride + i + c;
            a.st.s[(uint64_t)d * cap + e] = x[col];
            a.st.s_next[(uint64_t)d * cap + e] = ended ? xf[col] : xn[col];
        }
        a.st.action[e] = a.actions[at];
        a.st.reward[e] = a.reward[at];
        a.st.done[e] = a.done[at] != 0 ? 1 : 0;
        a.st.priority[e] = a.priority;
    }
}

__global__ __launch_bounds__(kReplayBlock) void replay_update_kernel(const ReplayUpdateArgs a)
{
    const uint32_t j = blockIdx.x * kReplayBlock + threadIdx.x;
    if (j >= a.B) return;
    const uint32_t e = a.idx[j];
    if (e >= a.capacity) return; // kReplayNone of an empty draw among them
    a.priority[e] = replay_priority(a.td[j], a.alpha, a.eps, a.cap);
}

} // namespace gymrs
