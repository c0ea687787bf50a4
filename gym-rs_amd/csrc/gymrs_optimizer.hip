// gymrs_optimizer.hip -- gymrs_apply_gradient (include/gymrs_amd.h, "Optimizer"): the launch of optimizer_kernel
// (gymrs_optimizer_impl.h) for the group width and the slots per lane that hold S, and the fill of a fresh Adam state.
#include "gymrs_optimizer_impl.h"

namespace gymrs {

hipError_t launch_apply_gradient(const OptimizerArgs& a, hipStream_t stream)
{
    // every access is addressed inside a table of n_sets * S words (pw: n_sets * 2, excluded: n_sets): the caller's checks
    // (gymrs_apply_gradient) are what makes that safe
    if (!a.weights || !a.grad || !a.excluded || a.n_sets == 0 || a.S == 0 || a.S > kMaxOptimizerParams) return hipErrorInvalidValue;
    if (a.kind != GYMRS_OPT_SGD && a.kind != GYMRS_OPT_ADAM) return hipErrorInvalidValue;
    if (a.kind == GYMRS_OPT_ADAM && (!a.m || !a.v || !a.pw)) return hipErrorInvalidValue;
    if (a.flags & ~(GYMRS_OPT_ASCEND | GYMRS_OPT_ZERO_GRAD)) return hipErrorInvalidValue;
    const uint32_t S = a.S;
    if (S <= 8) return apply_gradient_shape<8, 1>(a, stream);
    if (S <= 16) return apply_gradient_shape<16, 1>(a, stream);
    if (S <= 32) return apply_gradient_shape<32, 1>(a, stream);
    if (S <= 64) return apply_gradient_shape<64, 1>(a, stream);
    if (S <= 128) return apply_gradient_shape<64, 2>(a, stream);
    if (S <= 256) return apply_gradient_shape<64, 4>(a, stream);
    return apply_gradient_shape<64, 8>(a, stream);
}

hipError_t launch_optimizer_fresh(float* m, float* v, float* pw, uint32_t n_sets, uint32_t S, hipStream_t stream)
{
    if (!m || !v || !pw || n_sets == 0 || S == 0) return hipErrorInvalidValue;
    const uint64_t words = (uint64_t)n_sets * S, sets2 = (uint64_t)n_sets * 2, most = words > sets2 ? words : sets2;
    launch_begin();
    hipLaunchKernelGGL(optimizer_fresh_kernel, dim3((uint32_t)((most + kOptBlock - 1) / kOptBlock)), dim3(kOptBlock), 0, stream, m, v, pw, words, sets2);
    return hipGetLastError();
}

} // namespace gymrs
