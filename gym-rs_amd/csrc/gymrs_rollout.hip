// gymrs_rollout.hip -- the fused multi-step (random-policy rollout) kernel of the uniform envs (gymrs_rollout_impl.h).
#include "gymrs_rollout_impl.h"

namespace gymrs {

// the table instantiations (kFlagTable) live in one translation unit per env type
hipError_t launch_rollout_table_cartpole(int vec, uint32_t flags, const StepArgs& a, const RolloutArgs& r, const void* consts, hipStream_t stream);
hipError_t launch_rollout_table_mountain_car(int vec, uint32_t flags, const StepArgs& a, const RolloutArgs& r, const void* consts, hipStream_t stream);

hipError_t launch_rollout(gymrs_env_kind kind, int vec, uint32_t flags, const StepArgs& a, const RolloutArgs& r,
                          const void* consts, hipStream_t stream)
{
    if (a.n == 0 || r.n_steps == 0) return hipSuccess;
    if (flags & kFlagTable) {
        switch (kind) {
        case GYMRS_CARTPOLE: return launch_rollout_table_cartpole(vec, flags, a, r, consts, stream);
        case GYMRS_MOUNTAIN_CAR: return launch_rollout_table_mountain_car(vec, flags, a, r, consts, stream);
        default: return hipErrorInvalidValue;
        }
    }
    switch (kind) {
    case GYMRS_CARTPOLE: return rollout_vec<CartPoleT>(vec, flags, a, r, consts, stream);
    case GYMRS_MOUNTAIN_CAR: return rollout_vec<MountainCarT>(vec, flags, a, r, consts, stream);
    case GYMRS_PENDULUM: return rollout_vec<PendulumT>(vec, flags, a, r, consts, stream);
    default: return hipErrorInvalidValue;
    }
}

} // namespace gymrs
