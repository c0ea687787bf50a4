// gymrs_es_ranks_impl.h -- the kernels of gymrs_es_ranks (include/gymrs_amd.h, "Evolution strategies", centred ranks): the centred,
// tie-averaged rank utilities of a population from its evaluation records.  gfx950.  Everything up to the last line of the rule is an
// integer (positions in sorted rows, summed as u32), so the result depends neither on the order a sort leaves ties in nor on scheduling.
//
// Keys.  F[p] becomes the order-preserving u64 image of its bits (es_rank_key: a negative value has every bit flipped, a non-negative one
// its sign bit), so that `<` and `==` on keys are the IEEE `<` and `==` on F.  That needs F to be neither NaN nor -0.0, the two cases in
// which bits and IEEE order part.  Neither occurs: return_sum is an int64 (its double is finite, and 0 becomes +0.0), episodes of a valid
// policy is in 1 .. 2^64 (its double is finite and positive), so the one division has a finite numerator and a finite non-zero
// denominator -- never NaN -- and a negative quotient is at least 2^-64 in magnitude, far from underflow -- never -0.0.  A policy without
// an episode, and the padding of a ragged tile, get UINT64_MAX: the image of no finite double, so they sort last and no valid key ever
// counts them.  The pad's index is UINT32_MAX (nothing is written for it), an invalid policy keeps its own (it gets +0.0f / INVALID).
//
// Tile kernel (es_rank_tile_kernel<FINISH>, one block of 1024 work-items per tile of T = 4096 policies).  Every work-item reads four
// records, two 16-byte non-temporal loads each as es_utilities_kernel<0> does (policy l + 1024 k of the tile: consecutive lanes, consecutive
// records), and parks key and index in two LDS rows (32 KB + 16 KB: the key passes move 8-byte words only, and for a compare distance
// j >= 32 the 64 lanes of a wave touch 64 consecutive keys).  A bitonic network over n_sort = the tile's size rounded up to a power
// of two sorts the pairs by key: log2(n)(log2(n)+1)/2 passes (78 at 4096, 36 at 256), two compare-exchanges per work-item and pass.
//   FINISH (P <= T, the common ES population: ONE launch and no scratch): n = the position of the first UINT64_MAX; for the key at
//   position i, less = i when the left neighbour differs, else a lower_bound in [0, i); less + equal = i + 1 when the right neighbour
//   differs, else an upper_bound in (i, n_sort).  u and rank2 are scattered through the index.
//   Otherwise the sorted tile and its valid count go to the scratch (keys [tiles][T] u64, index [tiles][T] u32, counts [tiles] u32).
//
// Count kernel (es_rank_count_kernel, P > T: tiles x 1024 work-items).  Block a keeps its sorted tile A in registers, four consecutive
// keys per work-item, and streams every tile B (its own among them: a key counts itself in `equal`) through two 32 KB LDS buffers: the
// 16-byte loads of tile b + 1 are issued before the searches of tile b and stored after them, one barrier per tile.  Per tile a work-item
// finds lower_bound(a0) and upper_bound(a3) over the whole row with 13 unrolled branch-free probes each, and the six bounds between them
// inside that window (both rows are sorted, so the bounds are monotone: each search starts where the previous one ended, and an equal
// neighbour reuses its lower bound).  less and less + equal add up in u32 registers; n is the sum of the counts, folded by every block
// from at most 256 uniform loads.  At the end each work-item computes u and scatters u / rank2 through its four indices.
// DEVIATION from "branch-free with clamped indices" for the inner bounds: they are plain bisection loops over the window, which the wave
// runs as long as its widest lane needs.  With distinct keys a window holds about four entries (2 - 3 probes); with a quarter of the
// population on one value the lanes inside the tie meet windows of up to T (12 probes).
// TRIED AND DROPPED (profiles/es_ranks.md): the two row-wide searches once per wave (lane 0's first key, lane 63's last: 26 broadcast
// probes) with the work-item's outer bounds bisected inside the wave's window, and no inner search for a key equal to its right
// neighbour.  Fewer probes, but 24 % slower at P = 2^20 and 14 % at 2^16 (supposed, not isolated: the two unrolled searches interleave their
// probes, while every probe of a bisection loop waits for the one before it and the wave waits for its widest lane).
// Cost, from the design (not a timing): a (work-item, tile) pair is 26 fixed probes and 6 x 2..12 window probes, each an 8-byte LDS
// read, a 64-bit compare and two selects.  At P = 2^20: 2^16 tile pairs x 1024 work-items x 40 .. 100 probes = 2.7 .. 6.7 G LDS reads
// at scattered addresses (the first probes of a wave hit one word -- a broadcast -- the last ones spread over the row), against
// 2^16 x 32 KB = 2 GB of B tiles read from L2 (the 12 MB scratch stays resident) and as much written to LDS.  The kernel is bound
// by LDS issue, then by the L2 reads; profiles/es_ranks.md has the measured times.
#pragma once
#include <hip/hip_runtime.h>

#include "gymrs_es.h"
#include "gymrs_kernels.h"

namespace gymrs {

constexpr uint32_t kEsRankBlock = 1024;                        // sixteen waves: both kernels
constexpr uint32_t kEsRankPer = kEsRankTile / kEsRankBlock;    // keys per work-item
constexpr unsigned long long kEsRankNoKey = ~0ull;             // not valid, or padding
constexpr uint32_t kEsRankPad = 0xffffffffu;                   // the index of padding
static_assert(kEsRankPer == 4 && (kEsRankTile & (kEsRankTile - 1)) == 0, "four keys per work-item (two 16-byte loads); the network needs a power of two");

typedef unsigned long long es_rank_ull2 __attribute__((ext_vector_type(2)));
typedef uint32_t es_rank_u4 __attribute__((ext_vector_type(4)));

// the order-preserving image of a double that is neither NaN nor -0.0 (see the head comment)
__device__ __forceinline__ unsigned long long es_rank_key(double F)
{
    const unsigned long long b = (unsigned long long)__double_as_longlong(F);
    return (b >> 63) ? ~b : (b | (1ull << 63));
}

// lower_bound / upper_bound of `key` in the sorted k[lo, hi): bisection (hi <= the row's length: every probe is inside)
template <bool UPPER>
__device__ __forceinline__ uint32_t es_rank_bound(const unsigned long long* k, uint32_t lo, uint32_t hi, unsigned long long key)
{
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        const unsigned long long v = k[mid];
        const bool right = UPPER ? v <= key : v < key;
        lo = right ? mid + 1u : lo;
        hi = right ? hi : mid;
    }
    return lo;
}

// the same over a whole row of kEsRankTile keys: 13 probes, no branch (the walk covers [0, T - 1), the last probe the last key)
template <bool UPPER>
__device__ __forceinline__ uint32_t es_rank_bound_row(const unsigned long long* k, unsigned long long key)
{
    uint32_t pos = 0;
#pragma unroll
    for (uint32_t s = kEsRankTile / 2; s >= 1u; s >>= 1) {
        const unsigned long long v = k[pos + s - 1u];
        pos += (UPPER ? v <= key : v < key) ? s : 0u;
    }
    const unsigned long long v = k[pos]; // (pos <= T - 1)
    return pos + ((UPPER ? v <= key : v < key) ? 1u : 0u);
}

// u and rank2 of one policy from its two integer sums; le = less + equal
__device__ __forceinline__ void es_rank_store(const EsRanksArgs& a, uint32_t p, bool valid, uint32_t less, uint32_t le, uint32_t n)
{
    const uint32_t rank2 = less + le - 1u; // 2 * less + equal - 1 (equal >= 1 for a valid p)
    a.u[p] = es_rank_utility(valid, n, (long long)rank2 - (long long)(n - 1u));
    if (a.rank2) a.rank2[p] = valid ? rank2 : GYMRS_ES_RANK_INVALID;
}

template <bool FINISH>
__global__ __launch_bounds__(kEsRankBlock) void es_rank_tile_kernel(const EsRanksArgs a, const uint32_t n_sort)
{
    __shared__ unsigned long long keys[kEsRankTile];
    __shared__ uint32_t ids[kEsRankTile];
    const uint32_t l = threadIdx.x, base = blockIdx.x * kEsRankTile; // (P <= 2^20: no overflow)

#pragma unroll
    for (uint32_t k = 0; k < kEsRankPer; ++k) {
        const uint32_t i = l + k * kEsRankBlock, p = base + i;
        if (i >= n_sort) break;
        unsigned long long key = kEsRankNoKey;
        if (p < a.P) {
            const es_rank_ull2* rec = reinterpret_cast<const es_rank_ull2*>(static_cast<const char*>(a.records) + (size_t)p * 64u);
            const es_rank_ull2 r0 = __builtin_nontemporal_load(rec), r1 = __builtin_nontemporal_load(rec + 1); // {return_sum, ..}, {episodes, ..}
            if (r1.x != 0ull) key = es_rank_key(es_fitness((long long)r0.x, r1.x));
        }
        keys[i] = key;
        ids[i] = p < a.P ? p : kEsRankPad;
    }
    __syncthreads();

    // the bitonic network: compare-exchange t of a pass pairs i (bit j clear) with i + j, ascending where bit `size` of i is clear
    for (uint32_t size = 2; size <= n_sort; size <<= 1) {
        for (uint32_t j = size >> 1; j >= 1u; j >>= 1) {
#pragma unroll
            for (uint32_t k = 0; k < kEsRankPer / 2; ++k) {
                const uint32_t t = l + k * kEsRankBlock;
                if (t < (n_sort >> 1)) {
                    const uint32_t i = ((t & ~(j - 1u)) << 1) | (t & (j - 1u)), q = i + j;
                    const unsigned long long ki = keys[i], kq = keys[q];
                    const bool up = (i & size) == 0u;
                    if (up ? ki > kq : ki < kq) {
                        keys[i] = kq;
                        keys[q] = ki;
                        const uint32_t ii = ids[i];
                        ids[i] = ids[q];
                        ids[q] = ii;
                    }
                }
            }
            __syncthreads();
        }
    }

    // the valid keys are the first n: every work-item finds n (the same words for every lane: LDS broadcasts)
    const uint32_t n = es_rank_bound<false>(keys, 0u, n_sort, kEsRankNoKey);
    if constexpr (FINISH) {
#pragma unroll
        for (uint32_t k = 0; k < kEsRankPer; ++k) {
            const uint32_t i = l + k * kEsRankBlock;
            if (i >= n_sort) break;
            const unsigned long long key = keys[i];
            const uint32_t p = ids[i];
            if (p == kEsRankPad) continue;
            const bool tie_left = i > 0u && keys[i - 1u] == key, tie_right = i + 1u < n_sort && keys[i + 1u] == key;
            const uint32_t less = es_rank_bound<false>(keys, tie_left ? 0u : i, i, key);
            const uint32_t le = es_rank_bound<true>(keys, i + 1u, tie_right ? n_sort : i + 1u, key);
            es_rank_store(a, p, key != kEsRankNoKey, less, le, n);
        }
    } else {
        // (n_sort == T here) four consecutive entries per work-item: 16-byte stores
        const es_rank_ull2* k2 = reinterpret_cast<const es_rank_ull2*>(keys);
        es_rank_ull2* out = reinterpret_cast<es_rank_ull2*>(a.keys + base);
        out[2u * l] = k2[2u * l];
        out[2u * l + 1u] = k2[2u * l + 1u];
        reinterpret_cast<es_rank_u4*>(a.index + base)[l] = reinterpret_cast<const es_rank_u4*>(ids)[l];
        if (l == 0) a.counts[blockIdx.x] = n;
    }
}

__global__ __launch_bounds__(kEsRankBlock) void es_rank_count_kernel(const EsRanksArgs a)
{
    __shared__ es_rank_ull2 rows[2][kEsRankTile / 2]; // two rows of T keys: 64 KB
    const uint32_t l = threadIdx.x, tiles = gridDim.x;
    const es_rank_ull2* src = reinterpret_cast<const es_rank_ull2*>(a.keys); // [tiles][T / 2]
    const size_t own = (size_t)blockIdx.x * (kEsRankTile / 2) + 2u * l;
    const es_rank_ull2 a01 = src[own], a23 = src[own + 1u];
    const unsigned long long ak[kEsRankPer] = {a01.x, a01.y, a23.x, a23.y};
    const es_rank_u4 ap = reinterpret_cast<const es_rank_u4*>(a.index)[(size_t)blockIdx.x * (kEsRankTile / 4) + l];
    uint32_t less[kEsRankPer] = {0, 0, 0, 0}, le[kEsRankPer] = {0, 0, 0, 0};

    uint32_t n = 0;
    for (uint32_t b = 0; b < tiles; ++b) n += a.counts[b]; // (uniform loads)

    rows[0][2u * l] = src[2u * l];
    rows[0][2u * l + 1u] = src[2u * l + 1u];
    __syncthreads();
    for (uint32_t b = 0; b < tiles; ++b) {
        const bool more = b + 1u < tiles;
        es_rank_ull2 n01 = {0ull, 0ull}, n23 = {0ull, 0ull};
        if (more) { // the next tile's loads fly under this tile's searches
            const size_t at = (size_t)(b + 1u) * (kEsRankTile / 2) + 2u * l;
            n01 = src[at];
            n23 = src[at + 1u];
        }
        const unsigned long long* B = reinterpret_cast<const unsigned long long*>(rows[b & 1u]);
        const uint32_t first = es_rank_bound_row<false>(B, ak[0]), last = es_rank_bound_row<true>(B, ak[kEsRankPer - 1]);
        uint32_t lw = first;
#pragma unroll
        for (uint32_t k = 0; k < kEsRankPer; ++k) {
            const uint32_t up = k + 1u == kEsRankPer ? last : es_rank_bound<true>(B, lw, last, ak[k]);
            less[k] += lw;
            le[k] += up;
            if (k + 1u < kEsRankPer) lw = ak[k + 1u] == ak[k] ? lw : es_rank_bound<false>(B, up, last, ak[k + 1u]);
        }
        if (more) {
            rows[(b + 1u) & 1u][2u * l] = n01;
            rows[(b + 1u) & 1u][2u * l + 1u] = n23;
        }
        __syncthreads(); // the next row is whole, and nobody reads this one any more
    }
    const uint32_t p[kEsRankPer] = {ap.x, ap.y, ap.z, ap.w};
#pragma unroll
    for (uint32_t k = 0; k < kEsRankPer; ++k)
        if (p[k] != kEsRankPad) es_rank_store(a, p[k], ak[k] != kEsRankNoKey, less[k], le[k], n);
}

} // namespace gymrs
