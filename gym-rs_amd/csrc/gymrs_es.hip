// gymrs_es.hip -- gymrs_es_init and gymrs_es_step (include/gymrs_amd.h, "Evolution strategies"): the launches of the kernels of
// gymrs_es_impl.h.  A step is the three utilities passes (unless the caller brought utilities), the gradient and the fused update and
// population: five launches in stream order, no host synchronisation and no memset among them.
#include "gymrs_es_impl.h"

namespace gymrs {

namespace {
// every access of the kernels is addressed inside [P] rows, [P][S] weights and the fixed slots of the state: these checks (and the
// caller's, gymrs_es_init / gymrs_es_step) are what makes that safe
bool es_args_ok(const EsArgs& a)
{
    return a.st && a.weights && a.u && a.fitness && a.P >= 2 && a.P % 2 == 0 && a.P <= kEsMaxPolicies && a.S >= 1 && a.S <= kEsSlots;
}
} // namespace

hipError_t launch_es_init(const EsArgs& a, hipStream_t stream)
{
    if (!es_args_ok(a)) return hipErrorInvalidValue;
    return es_launch_population<false, false, false>(a, stream);
}

hipError_t launch_es_step(const EsArgs& a, hipStream_t stream)
{
    if (!es_args_ok(a) || (!a.u_in && !a.records)) return hipErrorInvalidValue;
    if (a.kind != GYMRS_OPT_SGD && a.kind != GYMRS_OPT_ADAM) return hipErrorInvalidValue;
    if (a.flags & ~GYMRS_OPT_ASCEND) return hipErrorInvalidValue;
    if (!a.u_in) {
        const dim3 grid((a.P + kEsChunk - 1) / kEsChunk), block(kEsChunk);
        launch_begin();
        hipLaunchKernelGGL(es_utilities_kernel<0>, grid, block, 0, stream, a);
        hipLaunchKernelGGL(es_utilities_kernel<1>, grid, block, 0, stream, a);
        hipLaunchKernelGGL(es_utilities_kernel<2>, grid, block, 0, stream, a);
        if (hipError_t err = hipGetLastError()) return err;
    }
    {
        // few pairs: cut the walk over s as well, towards about 1024 blocks
        const uint32_t pair_blocks = ((a.P >> 1) + kEsBlock - 1) / kEsBlock;
        uint32_t splits = (1024u + pair_blocks - 1) / pair_blocks;
        splits = splits > a.S ? a.S : splits;
        const uint32_t s_per_block = (a.S + splits - 1) / splits;
        launch_begin();
        hipLaunchKernelGGL(es_gradient_kernel, dim3(pair_blocks, (a.S + s_per_block - 1) / s_per_block), dim3(kEsBlock), 0, stream, a, s_per_block);
        if (hipError_t err = hipGetLastError()) return err;
    }
    const bool adam = a.kind == GYMRS_OPT_ADAM, clip = a.max_norm < __builtin_inff();
    if (adam) return clip ? es_launch_population<true, true, true>(a, stream) : es_launch_population<true, true, false>(a, stream);
    return clip ? es_launch_population<true, false, true>(a, stream) : es_launch_population<true, false, false>(a, stream);
}

} // namespace gymrs
