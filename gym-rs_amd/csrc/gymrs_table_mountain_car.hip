// gymrs_table_mountain_car.hip -- the per-step, rollout and episodic evaluation kernels of MountainCar with per-lane parameter tables (TableT,
// gymrs_tile.h): every flag set, hint variant, lanes-per-work-item and workgroup size of the uniform tables, in a translation
// unit of its own so that the build compiles it in parallel with the others.
#include "gymrs_evaluate_impl.h"
#include "gymrs_rollout_impl.h"
#include "gymrs_step_impl.h"

namespace gymrs {

hipError_t launch_step_table_mountain_car(int vec, uint32_t flags, const StepArgs& a, const void* consts, hipStream_t stream)
{
    return launch_vec<TableT<MountainCarT>>(vec, flags, a, consts, stream);
}

hipError_t launch_rollout_table_mountain_car(int vec, uint32_t flags, const StepArgs& a, const RolloutArgs& r, const void* consts, hipStream_t stream)
{
    return rollout_vec<TableT<MountainCarT>>(vec, flags, a, r, consts, stream);
}

hipError_t launch_evaluate_table_mountain_car(const EvalArgs& a, const TableConsts& c, const PolicyArgs& p, hipStream_t stream)
{
    hipLaunchKernelGGL((evaluate_policy_kernel<TableT<MountainCarT>>), dim3(step_grid(a.n, kEvalVec)), dim3(kBlock), 0, stream, a, c, p);
    return hipGetLastError();
}

} // namespace gymrs
