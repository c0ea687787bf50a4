// gymrs_es_ranks.hip -- gymrs_es_ranks (include/gymrs_amd.h, "Evolution strategies", centred ranks): the launches of the kernels of
// gymrs_es_ranks_impl.h.  A population of at most one tile is ONE launch and touches no scratch; a larger one is the tile sort and the
// count, in stream order, with no host synchronisation and no memset between them.
#include "gymrs_es_ranks_impl.h"

namespace gymrs {

void es_rank_scratch_rows(EsRanksArgs& a, void* scratch)
{
    const size_t slots = (size_t)es_rank_tiles(a.P) * kEsRankTile;
    a.keys = static_cast<unsigned long long*>(scratch);
    a.index = reinterpret_cast<uint32_t*>(a.keys + slots);
    a.counts = a.index + slots;
}

hipError_t launch_es_ranks(const EsRanksArgs& a, hipStream_t stream)
{
    // every access of the kernels is addressed inside [P] rows and the [tiles][T] rows of the scratch: these checks (and gymrs_es_ranks's) are
    // what makes that safe
    if (!a.records || !a.u || a.P == 0 || a.P > kEsMaxPolicies) return hipErrorInvalidValue;
    launch_begin();
    if (a.P <= kEsRankTile) {
        uint32_t n_sort = 2; // the network's size: P rounded up to a power of two
        while (n_sort < a.P) n_sort <<= 1;
        hipLaunchKernelGGL(es_rank_tile_kernel<true>, dim3(1), dim3(kEsRankBlock), 0, stream, a, n_sort);
        return hipGetLastError();
    }
    if (!a.keys || !a.index || !a.counts) return hipErrorInvalidValue;
    const dim3 grid(es_rank_tiles(a.P)), block(kEsRankBlock);
    hipLaunchKernelGGL(es_rank_tile_kernel<false>, grid, block, 0, stream, a, kEsRankTile);
    hipLaunchKernelGGL(es_rank_count_kernel, grid, block, 0, stream, a);
    return hipGetLastError();
}

} // namespace gymrs
