// gymrs_replay.hip -- gymrs_replay_push, gymrs_replay_sample and gymrs_replay_update (include/gymrs_amd.h, "Replay"): the launches of
// the kernels of gymrs_replay_impl.h.  A store of at most one tile is drawn from in ONE launch and touches no scratch; a larger one in
// three (tile sums, tile bases, locate and gather), in stream order, with no host synchronisation and no memset between them.
#include "gymrs_replay_impl.h"

namespace gymrs {

namespace {

bool store_ok(const ReplayStore& st)
{
    return st.s && st.s_next && st.action && st.reward && st.done && st.priority && st.capacity >= 16 && st.capacity <= kReplayMaxCapacity &&
           st.capacity % 16 == 0;
}

// CartPole observes 4 components, MountainCar 2
template <class Launch>
hipError_t with_obs_dim(gymrs_env_kind kind, Launch launch)
{
    if (kind == GYMRS_CARTPOLE) return launch(std::integral_constant<int, 4>{});
    if (kind == GYMRS_MOUNTAIN_CAR) return launch(std::integral_constant<int, 2>{});
    return hipErrorInvalidValue;
}

} // namespace

hipError_t launch_replay_push(gymrs_env_kind kind, const ReplayPushArgs& a, hipStream_t stream)
{
    if (a.n == 0 || a.n_steps == 0) return hipSuccess;
    // every access is addressed inside a row of `stride` lanes and the `capacity` entries of the store: these checks (and
    // gymrs_replay_push's) are what makes that safe
    if (!store_ok(a.st) || !a.obs || !a.actions || !a.reward || !a.done || !a.start_obs || !a.final_obs || a.stride < a.n || a.stride % 16 != 0)
        return hipErrorInvalidValue;
    if (a.head >= a.st.capacity || a.n > a.st.capacity || (uint64_t)a.n_steps > a.st.capacity / a.n || a.priority > kReplayMaxPriority)
        return hipErrorInvalidValue;
    const uint64_t groups = (a.n + 3u) / 4u, blocks = (groups * a.n_steps + kReplayBlock - 1u) / kReplayBlock; // groups * K <= capacity
    return with_obs_dim(kind, [&](auto dim) {
        launch_begin();
        hipLaunchKernelGGL(replay_push_kernel<decltype(dim)::value>, dim3((uint32_t)blocks), dim3(kReplayBlock), 0, stream, a, (uint32_t)groups);
        return hipGetLastError();
    });
}

hipError_t launch_replay_sample(gymrs_env_kind kind, const ReplaySampleArgs& a, hipStream_t stream)
{
    if (!store_ok(a.st) || a.count == 0 || a.count > a.st.capacity || a.B == 0 || a.B > kReplayMaxSamples) return hipErrorInvalidValue;
    if (!a.obs || !a.actions || !a.reward || !a.done || !a.start_obs || !a.idx || !a.total || a.stride < a.B || a.stride % 16 != 0)
        return hipErrorInvalidValue;
    const uint32_t tiles = (uint32_t)((a.st.capacity + kReplayTile - 1u) / kReplayTile);
    if (tiles > 1u && !a.scratch) return hipErrorInvalidValue;
    return with_obs_dim(kind, [&](auto dim) {
        constexpr int D = decltype(dim)::value;
        launch_begin();
        if (tiles == 1u) {
            hipLaunchKernelGGL((replay_locate_kernel<D, true>), dim3(1), dim3(kReplayBlock), 0, stream, a);
            return hipGetLastError();
        }
        hipLaunchKernelGGL(replay_sum_kernel, dim3(tiles), dim3(kReplayBlock), 0, stream, a);
        hipLaunchKernelGGL(replay_base_kernel, dim3(1), dim3(kReplayBlock), 0, stream, a, tiles);
        hipLaunchKernelGGL((replay_locate_kernel<D, false>), dim3(tiles), dim3(kReplayBlock), 0, stream, a);
        return hipGetLastError();
    });
}

hipError_t launch_replay_update(const ReplayUpdateArgs& a, hipStream_t stream)
{
    if (a.B == 0) return hipSuccess;
    if (!a.priority || !a.idx || !a.td || a.capacity == 0 || a.capacity > kReplayMaxCapacity || a.B > kReplayMaxSamples ||
        !replay_rule_ok(a.alpha, a.eps, a.cap))
        return hipErrorInvalidValue;
    launch_begin();
    hipLaunchKernelGGL(replay_update_kernel, dim3((a.B + kReplayBlock - 1u) / kReplayBlock), dim3(kReplayBlock), 0, stream, a);
    return hipGetLastError();
}

} // namespace gymrs
