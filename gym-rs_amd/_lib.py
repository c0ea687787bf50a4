"""ctypes loader for ``libgymrs_amd.so`` (the C ABI declared in ``include/gymrs_amd.h``).

Fails loudly when the library is missing: the product path has no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

_PKG = Path(__file__).resolve().parent
ABI_VERSION = 3  # GYMRS_ABI_VERSION of include/gymrs_amd.h
_LIB = None

u8p = C.POINTER(C.c_uint8)
f32p = C.POINTER(C.c_float)
f64p = C.POINTER(C.c_double)
u64p = C.POINTER(C.c_uint64)

# name -> (restype, argtypes); mirrors include/gymrs_amd.h one to one
SIGNATURES = {
    "gymrs_default_params": (C.c_int, [C.c_int, C.c_void_p]),
    "gymrs_action_space": (C.c_int, [C.c_int, C.POINTER(C.c_uint32), f64p, f64p]),
    "gymrs_observation_space": (C.c_int, [C.c_int, C.c_void_p, f64p, f64p, C.POINTER(C.c_int)]),
    "gymrs_discrete_contains": (C.c_int, [C.c_uint64, C.c_uint64]),
    "gymrs_engine_create": (C.c_int, [C.c_int, C.c_uint64, C.c_uint64, C.c_int, C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p)]),
    "gymrs_engine_destroy": (C.c_int, [C.c_void_p]),
    "gymrs_set_stream": (C.c_int, [C.c_void_p, C.c_void_p]),
    "gymrs_get_stream": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "gymrs_reset": (C.c_int, [C.c_void_p, C.c_int, C.c_uint64, f32p, u64p]),
    "gymrs_reset_pcg64": (C.c_int, [C.c_void_p, C.c_int, C.c_uint64, C.c_void_p, C.POINTER(C.c_double), u64p]),
    "gymrs_step": (C.c_int, [C.c_void_p, C.c_void_p]),
    "gymrs_step_host": (C.c_int, [C.c_void_p, C.c_void_p]),
    "gymrs_step_many": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_int]),
    "gymrs_sync": (C.c_int, [C.c_void_p]),
    "gymrs_obs_ptrs": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int)]),
    "gymrs_state_ptrs": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int)]),
    "gymrs_reward_ptr": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "gymrs_done_ptr": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "gymrs_truncated_ptr": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "gymrs_final_obs_ptrs": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int)]),
    "gymrs_get_obs": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]),
    "gymrs_get_final_obs": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]),
    "gymrs_get_state": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]),
    "gymrs_set_state": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]),
    "gymrs_get_step_result": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gymrs_stats": (C.c_int, [C.c_void_p, f64p]),
    "gymrs_stats_clear": (C.c_int, [C.c_void_p]),
    "gymrs_stats_device": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "gymrs_comm_unique_id": (C.c_int, [C.c_void_p]),
    "gymrs_comm_init": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "gymrs_allreduce_stats": (C.c_int, [C.c_void_p, f64p]),
    "gymrs_engine_clone": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "gymrs_snapshot_size": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "gymrs_snapshot_save": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64]),
    "gymrs_snapshot_load": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64]),
    "gymrs_rollout_record": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64, C.c_void_p]),
    "gymrs_rollout": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64]),
    "gymrs_fill_actions": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64]),
    "gymrs_get_tick": (C.c_int, [C.c_void_p, u64p, u64p]),
    "gymrs_set_tuning": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "gymrs_set_params": (C.c_int, [C.c_void_p, C.c_void_p]),
    "gymrs_get_params": (C.c_int, [C.c_void_p, C.c_void_p]),
    "gymrs_set_param_table": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32]),
    "gymrs_get_param_table": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]),
    "gymrs_param_index_ptr": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "gymrs_set_param_index": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]),
    "gymrs_get_param_index": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]),
    "gymrs_get_lane_params": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p]),
    # closed-loop rollouts (gymrs_policy_desc: {u32 hidden, u32 n_policies, u64 lanes_per_policy})
    "gymrs_policy_size": (C.c_int, [C.c_int, C.c_uint32, u64p]),
    "gymrs_set_policy": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "gymrs_get_policy": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]),
    "gymrs_policy_weights_ptr": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), u64p]),
    "gymrs_policy_actions": (C.c_int, [C.c_void_p, C.c_void_p]),
    "gymrs_rollout_policy": (C.c_int, [C.c_void_p, C.c_uint32]),
    "gymrs_rollout_policy_record": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p]),
    # per-policy fitness (gymrs_policy_fitness: {i64 reward_sum, u64 episodes, u64 done, u64 truncated})
    "gymrs_rollout_policy_fitness": (C.c_int, [C.c_void_p, C.c_uint32]),
    "gymrs_policy_fitness_ptr": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint32)]),
    "gymrs_get_policy_fitness": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]),
    "gymrs_policy_fitness_clear": (C.c_int, [C.c_void_p]),
    # the closed-loop calls behind one descriptor (gymrs_closed_loop_desc 24 B: {u32 n_steps, u32 flags, trajectory*, u64 reserved})
    "gymrs_rollout_closed_loop": (C.c_int, [C.c_void_p, C.c_void_p]),
    # the recording closed-loop launch with per-step final observations (gymrs_transitions_desc 80 B)
    "gymrs_rollout_transitions": (C.c_int, [C.c_void_p, C.c_void_p]),
    # epsilon-greedy exploration (gymrs_exploration 16 B: {u64 seed, u32 threshold, u32 reserved})
    "gymrs_set_exploration": (C.c_int, [C.c_void_p, C.c_void_p]),
    "gymrs_get_exploration": (C.c_int, [C.c_void_p, C.c_void_p]),
    "gymrs_explore_actions": (C.c_int, [C.c_void_p, C.c_void_p]),
    "gymrs_explore_draw": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint8), C.POINTER(C.c_uint8)]),
    # softmax sampling (gymrs_sampling 16 B: {u64 seed, f32 scale, u32 reserved})
    "gymrs_set_sampling": (C.c_int, [C.c_void_p, C.c_void_p]),
    "gymrs_get_sampling": (C.c_int, [C.c_void_p, C.c_void_p]),
    "gymrs_sample_actions": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "gymrs_sample_draw": (C.c_int, [C.c_void_p, C.c_uint32, f32p, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint8), f32p]),
    # advantages over a transitions record (gymrs_advantages_desc 112 B); the critic set is described by a gymrs_policy_desc
    "gymrs_critic_size": (C.c_int, [C.c_int, C.c_uint32, u64p]),
    "gymrs_set_critic": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "gymrs_get_critic": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]),
    "gymrs_critic_weights_ptr": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), u64p]),
    "gymrs_critic_value": (C.c_int, [C.c_int, C.c_uint32, f32p, f32p, f32p]),
    "gymrs_advantages": (C.c_int, [C.c_void_p, C.c_void_p]),
    # gradients over a transitions record (gymrs_gradient_desc 112 B) and the host-only lane
    "gymrs_policy_gradient": (C.c_int, [C.c_void_p, C.c_void_p]),
    "gymrs_gradient_lane": (C.c_int, [C.c_int, C.c_uint32, C.c_uint32, C.c_float, f32p, C.c_uint32, f32p, C.POINTER(C.c_uint8), f32p,
                                      C.POINTER(C.c_int64), u64p, f32p]),
    # the clipped surrogate over a transitions record (gymrs_ppo_desc 136 B) and the host-only lane
    "gymrs_ppo_gradient": (C.c_int, [C.c_void_p, C.c_void_p]),
    "gymrs_ppo_lane": (C.c_int, [C.c_int, C.c_uint32, C.c_float, C.c_float, C.c_float, f32p, C.c_uint32, f32p, C.POINTER(C.c_uint8), f32p, f32p,
                                 C.POINTER(C.c_int64), u64p, u64p, f32p]),
    # episodic policy evaluation (gymrs_eval_desc 32 B in, gymrs_policy_eval 64 B records out)
    "gymrs_evaluate_policy": (C.c_int, [C.c_void_p, C.c_void_p]),
    "gymrs_get_policy_eval": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]),
    "gymrs_policy_eval_ptr": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint32)]),
    "gymrs_env_json": (C.c_int, [C.c_void_p, C.c_uint64, C.c_char_p, C.c_uint64, u64p]),
    "gymrs_params_from_json": (C.c_int, [C.c_int, C.c_char_p, C.c_void_p, f64p, C.POINTER(C.c_int)]),
    # one batch over several GPUs in one process
    "gymrs_allreduce_stats_multi": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, f64p, C.POINTER(C.c_int)]),
    "gymrs_sharded_create": (C.c_int, [C.c_int, C.c_uint64, C.c_uint64, C.c_int, C.POINTER(C.c_int), C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p)]),
    "gymrs_sharded_destroy": (C.c_int, [C.c_void_p]),
    "gymrs_sharded_count": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "gymrs_sharded_shard": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), u64p, u64p, C.POINTER(C.c_int)]),
    "gymrs_sharded_reset": (C.c_int, [C.c_void_p, C.c_int, C.c_uint64, f32p, u64p]),
    "gymrs_sharded_step": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "gymrs_sharded_step_many": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_uint64, C.c_uint32, C.c_uint32, C.c_int]),
    "gymrs_sharded_fill_actions": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_uint64, C.c_uint64]),
    "gymrs_sharded_rollout": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64]),
    "gymrs_sharded_set_policy": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "gymrs_sharded_rollout_policy": (C.c_int, [C.c_void_p, C.c_uint32]),
    "gymrs_sharded_rollout_policy_fitness": (C.c_int, [C.c_void_p, C.c_uint32]),
    "gymrs_sharded_get_policy_fitness": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]),
    "gymrs_sharded_policy_fitness_clear": (C.c_int, [C.c_void_p]),
    "gymrs_sharded_rollout_closed_loop": (C.c_int, [C.c_void_p, C.c_void_p]),
    "gymrs_sharded_set_exploration": (C.c_int, [C.c_void_p, C.c_void_p]),
    "gymrs_sharded_set_sampling": (C.c_int, [C.c_void_p, C.c_void_p]),
    "gymrs_sharded_evaluate_policy": (C.c_int, [C.c_void_p, C.c_void_p]),
    "gymrs_sharded_get_policy_eval": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]),
    # per-lane physics on a sharded batch (the index in batch lane numbering)
    "gymrs_sharded_set_param_table": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32]),
    "gymrs_sharded_get_param_table": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]),
    "gymrs_sharded_set_param_index": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]),
    "gymrs_sharded_get_param_index": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]),
    "gymrs_sharded_set_params": (C.c_int, [C.c_void_p, C.c_void_p]),
    "gymrs_sharded_sync": (C.c_int, [C.c_void_p]),
    "gymrs_sharded_stats": (C.c_int, [C.c_void_p, f64p]),
    "gymrs_sharded_stats_clear": (C.c_int, [C.c_void_p]),
    "gymrs_sharded_reduce_path": (C.c_char_p, [C.c_void_p]),
    "gymrs_sharded_get_state": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]),
    "gymrs_sharded_get_step_result": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gymrs_last_error": (C.c_char_p, []),
    "gymrs_abi_version": (C.c_int, []),
}


def library_path() -> Path:
    return Path(os.environ.get("GYMRS_AMD_LIB", _PKG / "libgymrs_amd.so"))


def load_library() -> C.CDLL:
    """Load the HIP extension.  Raises if it has not been built (``python gym-rs_amd/build.py``)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = library_path()
    if not path.exists():
        raise RuntimeError(
            f"gym-rs_amd: native library {path} is missing — build it with "
            "`python gym-rs_amd/build.py` (or __graft_entry__.build()). There is no CPU fallback."
        )
    try:
        # If the host application already loaded a HIP runtime (e.g. `import torch` on ROCm), the
        # dynamic linker resolves libamdhip64.so.7 to that same instance, so device pointers and
        # streams are interchangeable.
        lib = C.CDLL(str(path), mode=C.RTLD_GLOBAL)
    except OSError as exc:  # missing libamdhip64 etc.
        raise RuntimeError(f"gym-rs_amd: cannot load {path}: {exc}") from exc
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError here = the header and the library disagree
        fn.restype = restype
        fn.argtypes = argtypes
    if lib.gymrs_abi_version() != ABI_VERSION:
        raise RuntimeError("gym-rs_amd: ABI version mismatch between the binding and the library")
    _LIB = lib
    return lib
