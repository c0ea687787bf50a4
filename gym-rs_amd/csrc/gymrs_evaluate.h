// gymrs_evaluate.h -- launch interface of the episodic policy evaluation (gymrs_evaluate_policy, include/gymrs_amd.h "episodic
// policy evaluation"): between the engine (gymrs_engine_learn.hip) and its kernels (gymrs_evaluate_impl.h).
#pragma once
#include "gymrs_kernels.h"

namespace gymrs {

// What one evaluation launch needs besides the env's constants and the policy set.  The launch touches no lane array of the engine.
struct EvalArgs {
    uint64_t n;           // lanes in this engine
    uint64_t gid0;        // global id of lane 0
    uint64_t seed;        // episode ep starts from the reset draw of seed + ep
    uint32_t episodes;    // E >= 1
    uint32_t max_steps;   // M >= 1; E * M <= kMaxEvalSteps
    uint32_t flags;       // GYMRS_EVAL_COMMON_STARTS (the kernels read no other bit)
    uint32_t pad_;
    uint32_t* lengths;    // [E][n] or NULL
    gymrs_policy_eval* table; // [n_policies], holds identities when the launch starts
    SampleBox box;        // the env's default reset box
};
constexpr uint32_t kMaxEvalSteps = GYMRS_POLICY_EVAL_MAX_STEPS;

// table[0 .. n_policies) = the identity record {0, 0, 0, 0, 0, 0, INT64_MAX, INT64_MIN}
hipError_t launch_policy_eval_identity(gymrs_policy_eval* table, uint32_t n_policies, hipStream_t stream);
// E episodes of every lane, added to table[policy of the lane] (integer atomics, once per wave and launch).  `flags`: 0 and the
// env's Consts, or kFlagTable and a TableConsts (GYMRS_EVAL_LANE_PARAMS on an engine with a parameter table: lane i plays with
// rows[index[i]], read in stream order; a lane whose index is not in the table plays nothing).
hipError_t launch_evaluate_policy(gymrs_env_kind kind, uint32_t flags, const EvalArgs& a, const void* consts, const PolicyArgs& p, hipStream_t stream);

} // namespace gymrs
