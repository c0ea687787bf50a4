// gymrs_normalize_impl.h -- the kernels of gymrs_normalize_advantages (include/gymrs_amd.h, "advantage normalisation"): out = (A -
// mean) * inv per set, with mean and inv from integer sums (gymrs_normalize.h).  gfx950.  No env is stepped and no weight is read:
// the set of a lane is the policy's key computed from the descriptor's lanes_per_policy and n_sets (policy_select).
//
// Three phases depend on each other grid-wide: the sum of the members, the sum of their centred squares, the write.  A phase
// boundary is a kernel boundary in stream order; a small kernel in front zeroes the statistics (no memset node: the call may be
// captured into a graph).  In every phase one work-item owns 4 consecutive lanes and walks rows k0 .. k1 of its column with one
// 16-byte load per row (row k + 1 before the arithmetic of row k), summing in registers: per lane one 64-bit integer and two
// counters.  blockIdx.y cuts the K rows into slices so that a short batch with a deep record still fills the device.  After the walk
// a wave whose lanes share one set (wave-uniform, policy_select) adds its 4 lanes, sums over the wave (wave_sum_u64) and issues one
// atomic per word; a gathered wave issues one per lane and word (a zero is skipped).  Phase 2 and 3 take mean (and inv) from the
// integers of `stats`: every work-item recomputes them for its set(s), once per launch, which costs two f64 divides and a square
// root against K rows; work-items < n_sets of workgroup (0, 0) of phase 3 also write them into stats[set].mean / .inv (other
// bytes than the ones the phase reads).  Traffic: three reads and one write of the row; whether the second and third read come
// from the memory-side cache is measured in profiles/normalize.md.
//
// One launch instead of four when the record is small: at most kNormalizeSmallItems = 512 row items of 4 lanes (2048 elements: 2
// items per work-item of ONE workgroup of 256) and at most kNormalizeSmallSets = 64 sets, whose sums live in LDS (ds 64-bit atomics,
// one per element and word) with __syncthreads between the phases.  Above either bound the four launches are taken.  The bound
// comes from a measurement (profiles/normalize.md): at 4096 items the one workgroup took 71 us where the four launches take 16.
#pragma once
#include "gymrs_normalize.h"
#include "gymrs_policy.h"

namespace gymrs {

__device__ __forceinline__ PolicyArgs normalize_key(const NormalizeArgs& a) { return PolicyArgs{nullptr, a.lanes_per_policy, a.n_sets, 0u, 0u, 0u}; }

__device__ __forceinline__ unsigned long long* stats_word(gymrs_advantage_stats* s, size_t offset)
{
    return reinterpret_cast<unsigned long long*>(reinterpret_cast<char*>(s) + offset);
}

__global__ __launch_bounds__(kBlock) void normalize_zero_kernel(gymrs_advantage_stats* stats, uint32_t n_sets)
{
    const uint32_t s = blockIdx.x * kBlock + threadIdx.x;
    if (s < n_sets) stats[s] = gymrs_advantage_stats{0, 0, 0, 0, 0.0f, 0.0f};
}

// PHASE 1: s1, n, non_members; PHASE 2: s2.  The walk: the per-lane sums of rows [k0, k1) in registers.
template <int PHASE, bool FULL>
__device__ __forceinline__ void normalize_sum_block(const NormalizeArgs& a, const uint32_t (&pol)[4], bool uniform, uint64_t base, uint32_t k0, uint32_t k1,
                                                    unsigned long long (&sum)[4], uint32_t (&cnt)[4], uint32_t (&out)[4])
{
    constexpr int VEC = 4;
    const uint64_t stride = a.stride, n = a.n;
    float mean[VEC] = {};
    bool live[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
        live[i] = FULL || base + i < n;
        if constexpr (PHASE == 2) {
            const gymrs_advantage_stats& s = a.stats[uniform ? pol[0] : pol[i]];
            mean[i] = normalize_mean(s.s1, s.n);
        }
    }
    Vec<float, VEC> r{};
    if (k0 < k1) r = load_vec<float, VEC, false>(a.adv + (uint64_t)k0 * stride, base, n, FULL, 0.0f);
    for (uint32_t k = k0; k < k1; ++k) {
        Vec<float, VEC> rn{};
        if (k + 1 < k1) rn = load_vec<float, VEC, false>(a.adv + (uint64_t)(k + 1) * stride, base, n, FULL, 0.0f);
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            const float A = r.v[i];
            const bool member = live[i] && normalize_member(A);
            if constexpr (PHASE == 1) {
                sum[i] += member ? (unsigned long long)normalize_q1(A) : 0ull;
                cnt[i] += member ? 1u : 0u;
                out[i] += (live[i] && !member) ? 1u : 0u;
            } else {
                sum[i] += member ? normalize_q2(A, mean[i]) : 0ull;
            }
        }
        r = rn;
    }
}

// Where the sums of a work-item go (every work-item of the workgroup gets here: one text behind the full and the ragged walk).
template <int PHASE>
__device__ __forceinline__ void normalize_sum_reduce(const NormalizeArgs& a, const uint32_t (&pol)[4], bool uniform, const unsigned long long (&sum)[4],
                                                     const uint32_t (&cnt)[4], const uint32_t (&out)[4])
{
    constexpr int VEC = 4;
    static_assert(kBlock == 256, "four waves per workgroup");
    constexpr size_t word = PHASE == 1 ? offsetof(gymrs_advantage_stats, s1) : offsetof(gymrs_advantage_stats, s2);
    // A wave with one set sums over itself; a workgroup whose four waves all have the SAME set adds the four through LDS and issues
    // one atomic per word: with one set for a million lanes every wave of the launch adds to the same three words, and the time of
    // the launch was the queue of those atomics at the L2 (profiles/normalize.md), not the row's bytes.
    __shared__ unsigned long long part[kBlock / 64][3];
    __shared__ uint32_t part_set[kBlock / 64];
    const uint32_t wave = threadIdx.x >> 6, set0 = __builtin_amdgcn_readfirstlane(pol[0]);
    unsigned long long total = 0, tc = 0, to = 0;
    if (uniform) { // wave-uniform
        total = wave_sum_u64(sum[0] + sum[1] + sum[2] + sum[3]);
        if constexpr (PHASE == 1) {
            tc = wave_sum_u64((unsigned long long)cnt[0] + cnt[1] + cnt[2] + cnt[3]);
            to = wave_sum_u64((unsigned long long)out[0] + out[1] + out[2] + out[3]);
        }
    }
    if ((threadIdx.x & 63u) == 0) {
        part[wave][0] = total;
        part[wave][1] = tc;
        part[wave][2] = to;
        part_set[wave] = uniform ? set0 : 0xffffffffu; // a gathered wave matches nobody
    }
    __syncthreads();
    bool together = part_set[0] != 0xffffffffu;
#pragma unroll
    for (int w = 1; w < kBlock / 64; ++w) together = together && part_set[w] == part_set[0];
    if (together) { // workgroup-uniform
        if (threadIdx.x == 0) {
            gymrs_advantage_stats* s = a.stats + set0;
            atomic_add_nonzero(stats_word(s, word), part[0][0] + part[1][0] + part[2][0] + part[3][0]);
            if constexpr (PHASE == 1) {
                atomic_add_nonzero(stats_word(s, offsetof(gymrs_advantage_stats, n)), part[0][1] + part[1][1] + part[2][1] + part[3][1]);
                atomic_add_nonzero(stats_word(s, offsetof(gymrs_advantage_stats, non_members)), part[0][2] + part[1][2] + part[2][2] + part[3][2]);
            }
        }
    } else if (uniform) { // wave-uniform
        if ((threadIdx.x & 63u) == 0) {
            gymrs_advantage_stats* s = a.stats + set0;
            atomic_add_nonzero(stats_word(s, word), total);
            if constexpr (PHASE == 1) {
                atomic_add_nonzero(stats_word(s, offsetof(gymrs_advantage_stats, n)), tc);
                atomic_add_nonzero(stats_word(s, offsetof(gymrs_advantage_stats, non_members)), to);
            }
        }
    } else {
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            gymrs_advantage_stats* s = a.stats + pol[i];
            atomic_add_nonzero(stats_word(s, word), sum[i]);
            if constexpr (PHASE == 1) {
                atomic_add_nonzero(stats_word(s, offsetof(gymrs_advantage_stats, n)), (unsigned long long)cnt[i]);
                atomic_add_nonzero(stats_word(s, offsetof(gymrs_advantage_stats, non_members)), (unsigned long long)out[i]);
            }
        }
    }
}

// The rows [k0, k1) of slice blockIdx.y
__device__ __forceinline__ void normalize_slice(const NormalizeArgs& a, uint32_t& k0, uint32_t& k1)
{
    const uint32_t per = (a.n_steps + gridDim.y - 1) / gridDim.y;
    k0 = min(a.n_steps, blockIdx.y * per);
    k1 = min(a.n_steps, k0 + per);
}

template <int PHASE>
__global__ __launch_bounds__(kBlock) void normalize_sum_kernel(const NormalizeArgs a)
{
    constexpr int VEC = 4, LPB = kBlock * VEC;
    const uint64_t base = (uint64_t)blockIdx.x * LPB + (uint64_t)threadIdx.x * VEC;
    const bool full = (uint64_t)blockIdx.x * LPB + (uint64_t)((threadIdx.x >> 6) + 1) * (64 * VEC) <= a.n; // wave-uniform, see step_kernel
    uint32_t pol[VEC] = {0, 0, 0, 0}, k0, k1;
    bool uniform = true;
    policy_select<VEC>(normalize_key(a), a.gid0 + base, pol, uniform);
    normalize_slice(a, k0, k1);
    unsigned long long sum[VEC] = {};
    uint32_t cnt[VEC] = {}, out[VEC] = {};
    if (full)
        normalize_sum_block<PHASE, true>(a, pol, uniform, base, k0, k1, sum, cnt, out);
    else
        normalize_sum_block<PHASE, false>(a, pol, uniform, base, k0, k1, sum, cnt, out);
    normalize_sum_reduce<PHASE>(a, pol, uniform, sum, cnt, out);
}

template <bool FULL>
__device__ __forceinline__ void normalize_write_block(const NormalizeArgs& a, const uint32_t (&pol)[4], bool uniform, uint64_t base, uint32_t k0, uint32_t k1)
{
    constexpr int VEC = 4;
    const uint64_t stride = a.stride, n = a.n;
    float mean[VEC], inv[VEC];
    if (uniform) { // wave-uniform: one set, its two numbers once
        const gymrs_advantage_stats& s = a.stats[__builtin_amdgcn_readfirstlane(pol[0])];
        const float m = normalize_mean(s.s1, s.n), v = normalize_inv(s.s2, s.n, a.eps);
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            mean[i] = m;
            inv[i] = v;
        }
    } else {
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            const gymrs_advantage_stats& s = a.stats[pol[i]];
            mean[i] = normalize_mean(s.s1, s.n);
            inv[i] = normalize_inv(s.s2, s.n, a.eps);
        }
    }
    Vec<float, VEC> r{};
    if (k0 < k1) r = load_vec<float, VEC, false>(a.adv + (uint64_t)k0 * stride, base, n, FULL, 0.0f);
    for (uint32_t k = k0; k < k1; ++k) {
        Vec<float, VEC> rn{}, o;
        if (k + 1 < k1) rn = load_vec<float, VEC, false>(a.adv + (uint64_t)(k + 1) * stride, base, n, FULL, 0.0f);
#pragma unroll
        for (int i = 0; i < VEC; ++i) o.v[i] = normalize_out(r.v[i], mean[i], inv[i]);
        store_vec<float, VEC, true>(a.out + (uint64_t)k * stride, base, n, FULL, o); // the next reader is another kernel
        r = rn;
    }
}

__global__ __launch_bounds__(kBlock) void normalize_write_kernel(const NormalizeArgs a)
{
    constexpr int VEC = 4, LPB = kBlock * VEC;
    const uint64_t base = (uint64_t)blockIdx.x * LPB + (uint64_t)threadIdx.x * VEC;
    const bool full = (uint64_t)blockIdx.x * LPB + (uint64_t)((threadIdx.x >> 6) + 1) * (64 * VEC) <= a.n; // wave-uniform, see step_kernel
    uint32_t pol[VEC] = {0, 0, 0, 0}, k0, k1;
    bool uniform = true;
    policy_select<VEC>(normalize_key(a), a.gid0 + base, pol, uniform);
    normalize_slice(a, k0, k1);
    if (full)
        normalize_write_block<true>(a, pol, uniform, base, k0, k1);
    else
        normalize_write_block<false>(a, pol, uniform, base, k0, k1);
    // The two numbers of every set, for the learner's diagnostics.  Deliberate: these plain stores go to stats[s].mean / .inv while
    // other workgroups of this launch still read s1, n and s2 of the same 40-byte record.  Different bytes, and the readers only
    // ever load the three 8-byte words they name, so there is no race as long as nobody turns those reads into a copy of the record.
    if (blockIdx.x == 0 && blockIdx.y == 0) {
        for (uint32_t s = threadIdx.x; s < a.n_sets; s += kBlock) {
            gymrs_advantage_stats& st = a.stats[s];
            st.mean = normalize_mean(st.s1, st.n);
            st.inv = normalize_inv(st.s2, st.n, a.eps);
        }
    }
}

// The one-launch path: ONE workgroup, the sums of at most kNormalizeSmallSets sets in LDS.  Item t * kBlock + threadIdx.x is row
// item / groups, lanes 4 * (item % groups) ..; the trip count is the same for every work-item (an item past the end has no live lane).
__global__ __launch_bounds__(kBlock) void normalize_small_kernel(const NormalizeArgs a)
{
    constexpr int VEC = 4;
    __shared__ unsigned long long s1[kNormalizeSmallSets], cnt[kNormalizeSmallSets], s2[kNormalizeSmallSets], nm[kNormalizeSmallSets];
    __shared__ float mean_s[kNormalizeSmallSets], inv_s[kNormalizeSmallSets];
    const uint64_t stride = a.stride, n = a.n;
    const uint32_t groups = (uint32_t)((n + VEC - 1) / VEC), items = groups * a.n_steps, trips = (items + kBlock - 1) / kBlock;
    const PolicyArgs key = normalize_key(a);
    if (threadIdx.x < kNormalizeSmallSets) s1[threadIdx.x] = cnt[threadIdx.x] = s2[threadIdx.x] = nm[threadIdx.x] = 0;
    __syncthreads();
    for (int phase = 1; phase <= 3; ++phase) {
        for (uint32_t t = 0; t < trips; ++t) {
            const uint32_t item = t * kBlock + threadIdx.x;
            const bool valid = item < items;
            const uint32_t k = valid ? item / groups : 0u;
            const uint64_t base = valid ? (uint64_t)(item - k * groups) * VEC : (uint64_t)groups * VEC; // past the end: no live lane
            uint32_t pol[VEC];
            bool uniform;
            policy_select<VEC>(key, a.gid0 + base, pol, uniform);
            const Vec<float, VEC> r = load_vec<float, VEC, false>(a.adv + (uint64_t)k * stride, base, n, false, 0.0f);
            Vec<float, VEC> o{};
#pragma unroll
            for (int i = 0; i < VEC; ++i) {
                const float A = r.v[i];
                const bool live = base + i < n, member = live && normalize_member(A);
                const uint32_t s = pol[i];
                if (phase == 1) {
                    if (member) {
                        atomicAdd(&s1[s], (unsigned long long)normalize_q1(A));
                        atomicAdd(&cnt[s], 1ull);
                    } else if (live) {
                        atomicAdd(&nm[s], 1ull);
                    }
                } else if (phase == 2) {
                    if (member) atomicAdd(&s2[s], normalize_q2(A, mean_s[s]));
                } else {
                    o.v[i] = normalize_out(A, mean_s[s], inv_s[s]);
                }
            }
            if (phase == 3) store_vec<float, VEC, true>(a.out + (uint64_t)k * stride, base, n, false, o);
        }
        __syncthreads();
        if (threadIdx.x < a.n_sets) {
            const uint32_t s = threadIdx.x;
            if (phase == 1) mean_s[s] = normalize_mean((long long)s1[s], cnt[s]);
            if (phase == 2) {
                inv_s[s] = normalize_inv(s2[s], cnt[s], a.eps);
                a.stats[s] = gymrs_advantage_stats{(long long)s1[s], cnt[s], s2[s], nm[s], mean_s[s], inv_s[s]};
            }
        }
        __syncthreads();
    }
}

// The caller's checks (gymrs_normalize_advantages) are what makes every access safe: rows of `stride` >= n lanes, touched at lanes
// < n only (full waves: whole 4-lane groups below n); n_sets records of statistics.
static hipError_t normalize_launch(const NormalizeArgs& a, hipStream_t stream)
{
    launch_begin();
    const uint64_t groups = (a.n + 3) / 4;
    if (groups * a.n_steps <= kNormalizeSmallItems && a.n_sets <= kNormalizeSmallSets) {
        hipLaunchKernelGGL(normalize_small_kernel, dim3(1), dim3(kBlock), 0, stream, a);
        return hipGetLastError();
    }
    const uint32_t blocks = step_grid(a.n, 4);
    // slices of the K rows: about 1024 workgroups (4 per CU) where the batch alone gives fewer
    const uint32_t slices = std::max(1u, std::min(a.n_steps, 1024u / std::min(blocks, 1024u)));
    hipLaunchKernelGGL(normalize_zero_kernel, dim3((a.n_sets + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, a.stats, a.n_sets);
    if (hipError_t err = hipGetLastError()) return err;
    hipLaunchKernelGGL(normalize_sum_kernel<1>, dim3(blocks, slices), dim3(kBlock), 0, stream, a);
    if (hipError_t err = hipGetLastError()) return err;
    hipLaunchKernelGGL(normalize_sum_kernel<2>, dim3(blocks, slices), dim3(kBlock), 0, stream, a);
    if (hipError_t err = hipGetLastError()) return err;
    hipLaunchKernelGGL(normalize_write_kernel, dim3(blocks, slices), dim3(kBlock), 0, stream, a);
    return hipGetLastError();
}

} // namespace gymrs
