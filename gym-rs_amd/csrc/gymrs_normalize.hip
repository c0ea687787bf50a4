// gymrs_normalize.hip -- gymrs_normalize_advantages (include/gymrs_amd.h, "advantage normalisation"): the launches of the kernels
// of gymrs_normalize_impl.h and the one entry the engine calls.
#include <algorithm>

#include "gymrs_normalize_impl.h"

namespace gymrs {

hipError_t launch_normalize(const NormalizeArgs& a, hipStream_t stream)
{
    if (a.n == 0 || a.n_steps == 0) return hipSuccess;
    // every access is addressed inside a row of `stride` lanes and n_sets records: the caller's checks are what makes that safe
    if (!a.adv || !a.out || !a.stats || a.stride < a.n || a.stride % 16 != 0) return hipErrorInvalidValue;
    if (a.n_sets == 0 || a.lanes_per_policy == 0) return hipErrorInvalidValue;
    return normalize_launch(a, stream);
}

} // namespace gymrs
