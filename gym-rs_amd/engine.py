"""BatchedEngine — N independent gym-rs envs stepped by one HIP kernel launch.

Thin ctypes binding over the C ABI (``include/gymrs_amd.h``).  The batched form of the reference
API: ``step(actions)`` fills device arrays ``obs`` / ``reward`` / ``done`` / ``truncated``
(``ActionReward``, core.rs:94-106) for every lane; ``reset(seed, options)`` is ``Env::reset``
(core.rs:45-50) for every lane.  numpy is used only to hand host buffers across the boundary.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence, Tuple

import numpy as np

from ._lib import load_library

CARTPOLE, MOUNTAIN_CAR, PENDULUM = 0, 1, 2
AUTO_RESET, TRACK_STATS, TIME_LIMIT, FINAL_OBS = 1, 2, 4, 8

_OK, _EINVAL, _EHIP, _ENCCL, _ENOMEM, _EACTION = range(6)


class GymrsError(RuntimeError):
    def __init__(self, status: int, message: str):
        super().__init__(f"gymrs status {status}: {message}")
        self.status = status


class InvalidActionError(GymrsError, AssertionError):
    """An action outside the action space: the reference's ``assert!`` panic (cartpole.rs:402-406)."""


class CartPoleParams(C.Structure):
    """The ``pub`` physics fields of ``CartPoleEnv`` (cartpole.rs:53-82)."""

    _fields_ = [
        ("gravity", C.c_double), ("masscart", C.c_double), ("masspole", C.c_double), ("length", C.c_double),
        ("force_mag", C.c_double), ("tau", C.c_double), ("theta_threshold_radians", C.c_double),
        ("x_threshold", C.c_double), ("kinematics_integrator", C.c_int32), ("max_episode_steps", C.c_uint32),
    ]


class MountainCarParams(C.Structure):
    """The ``pub`` physics fields of ``MountainCarEnv`` (mountain_car.rs:49-77)."""

    _fields_ = [
        ("min_position", C.c_double), ("max_position", C.c_double), ("max_speed", C.c_double),
        ("goal_position", C.c_double), ("goal_velocity", C.c_double), ("force", C.c_double),
        ("gravity", C.c_double), ("max_episode_steps", C.c_uint32), ("_pad", C.c_uint32),
    ]


class PendulumParams(C.Structure):
    """Gym Pendulum-v1 constants (spec-derived; not in the reference)."""

    _fields_ = [
        ("max_speed", C.c_double), ("max_torque", C.c_double), ("dt", C.c_double), ("g", C.c_double),
        ("m", C.c_double), ("l", C.c_double), ("max_episode_steps", C.c_uint32), ("_pad", C.c_uint32),
    ]


class Trajectory(C.Structure):
    """``gymrs_trajectory`` (include/gymrs_amd.h)."""
    _fields_ = [("obs", C.c_void_p), ("actions", C.c_void_p), ("reward", C.c_void_p), ("done", C.c_void_p),
                ("truncated", C.c_void_p), ("lane_stride", C.c_uint64)]


class PolicyFitness(C.Structure):
    """``gymrs_policy_fitness`` (include/gymrs_amd.h): one policy's counters, 32 bytes."""
    _fields_ = [("reward_sum", C.c_int64), ("episodes", C.c_uint64), ("done", C.c_uint64), ("truncated", C.c_uint64)]


class PolicyEval(C.Structure):
    """``gymrs_policy_eval`` (include/gymrs_amd.h): one policy's episodic record, 64 bytes."""
    _fields_ = [("return_sum", C.c_int64), ("return_sq_sum", C.c_uint64), ("episodes", C.c_uint64), ("done", C.c_uint64),
                ("truncated", C.c_uint64), ("steps", C.c_uint64), ("return_min", C.c_int64), ("return_max", C.c_int64)]


class EvalDesc(C.Structure):
    """``gymrs_eval_desc`` (include/gymrs_amd.h), 32 bytes."""
    _fields_ = [("episodes_per_lane", C.c_uint32), ("max_episode_steps", C.c_uint32), ("seed", C.c_uint64), ("flags", C.c_uint32),
                ("reserved", C.c_uint32), ("lengths_dev", C.c_void_p)]


EVAL_COMMON_STARTS = 1  # GYMRS_EVAL_COMMON_STARTS
EVAL_LANE_PARAMS = 4  # GYMRS_EVAL_LANE_PARAMS


class ClosedLoopDesc(C.Structure):
    """``gymrs_closed_loop_desc`` (include/gymrs_amd.h), 24 bytes."""
    _fields_ = [("n_steps", C.c_uint32), ("flags", C.c_uint32), ("record", C.POINTER(Trajectory)), ("reserved", C.c_uint64)]


CLOSED_LOOP_FITNESS = 1  # GYMRS_CLOSED_LOOP_FITNESS
CLOSED_LOOP_LANE_PARAMS = 4  # GYMRS_CLOSED_LOOP_LANE_PARAMS
CLOSED_LOOP_EXPLORE = 16  # GYMRS_CLOSED_LOOP_EXPLORE
CLOSED_LOOP_SAMPLE = 32  # GYMRS_CLOSED_LOOP_SAMPLE


class TransitionsDesc(C.Structure):
    """``gymrs_transitions_desc`` (include/gymrs_amd.h), 80 bytes: the record by value, then the two observation buffers."""
    _fields_ = [("n_steps", C.c_uint32), ("flags", C.c_uint32), ("record", Trajectory), ("final_obs", C.c_void_p),
                ("start_obs", C.c_void_p), ("reserved", C.c_uint64)]


class AdvantagesDesc(C.Structure):
    """``gymrs_advantages_desc`` (include/gymrs_amd.h), 112 bytes: the record by value, two observation buffers in, three rows out."""
    _fields_ = [("n_steps", C.c_uint32), ("flags", C.c_uint32), ("gamma", C.c_float), ("lam", C.c_float), ("record", Trajectory),
                ("final_obs", C.c_void_p), ("start_obs", C.c_void_p), ("advantages", C.c_void_p), ("returns", C.c_void_p),
                ("values", C.c_void_p), ("reserved", C.c_uint64)]


ADVANTAGES_CRITIC = 1  # GYMRS_ADVANTAGES_CRITIC


class GradientDesc(C.Structure):
    """``gymrs_gradient_desc`` (include/gymrs_amd.h), 112 bytes: the record by value, two rows in, one optional row out, two tables
    added to."""
    _fields_ = [("n_steps", C.c_uint32), ("flags", C.c_uint32), ("scale", C.c_float), ("pad_", C.c_uint32), ("record", Trajectory),
                ("start_obs", C.c_void_p), ("coef", C.c_void_p), ("prob", C.c_void_p), ("grad", C.c_void_p), ("excluded", C.c_void_p),
                ("reserved", C.c_uint64)]


GRADIENT_CRITIC = 1  # GYMRS_GRADIENT_CRITIC


class PpoDesc(C.Structure):
    """``gymrs_ppo_desc`` (include/gymrs_amd.h), 136 bytes: the record by value, three rows in, one optional row out, two tables and
    an optional pair of counters per set added to."""
    _fields_ = [("n_steps", C.c_uint32), ("flags", C.c_uint32), ("scale", C.c_float), ("clip_low", C.c_float), ("clip_high", C.c_float),
                ("pad_", C.c_uint32), ("record", Trajectory), ("start_obs", C.c_void_p), ("advantages", C.c_void_p), ("old_prob", C.c_void_p),
                ("prob", C.c_void_p), ("grad", C.c_void_p), ("excluded", C.c_void_p), ("counts", C.c_void_p), ("reserved", C.c_uint64)]


class VtraceDesc(C.Structure):
    """``gymrs_vtrace_desc`` (include/gymrs_amd.h), 152 bytes: six scalars, the record by value, three buffers in, two rows out, two
    optional rows out and an optional triple of counters per policy set added to."""
    _fields_ = [("n_steps", C.c_uint32), ("flags", C.c_uint32), ("gamma", C.c_float), ("lam", C.c_float), ("scale", C.c_float),
                ("rho_bar", C.c_float), ("c_bar", C.c_float), ("pg_rho_bar", C.c_float), ("record", Trajectory), ("final_obs", C.c_void_p),
                ("start_obs", C.c_void_p), ("old_prob", C.c_void_p), ("vs", C.c_void_p), ("pg_advantages", C.c_void_p), ("values", C.c_void_p),
                ("prob", C.c_void_p), ("counts", C.c_void_p), ("reserved", C.c_uint64)]


class EntropyDesc(C.Structure):
    """``gymrs_entropy_desc`` (include/gymrs_amd.h), 128 bytes: the record by value, one row in and one optional row in, three tables
    and an optional pair of counters per set added to."""
    _fields_ = [("n_steps", C.c_uint32), ("flags", C.c_uint32), ("scale", C.c_float), ("coef", C.c_float), ("record", Trajectory),
                ("start_obs", C.c_void_p), ("old_prob", C.c_void_p), ("grad", C.c_void_p), ("excluded", C.c_void_p), ("sums", C.c_void_p),
                ("counts", C.c_void_p), ("reserved", C.c_uint64)]


class ValueDesc(C.Structure):
    """``gymrs_value_desc`` (include/gymrs_amd.h), 136 bytes: the record by value, three rows in (one optional), one optional row out,
    two tables and two optional pairs per set added to."""
    _fields_ = [("n_steps", C.c_uint32), ("flags", C.c_uint32), ("clip", C.c_float), ("pad_", C.c_uint32), ("record", Trajectory),
                ("start_obs", C.c_void_p), ("returns", C.c_void_p), ("old_values", C.c_void_p), ("values", C.c_void_p), ("grad", C.c_void_p),
                ("excluded", C.c_void_p), ("sums", C.c_void_p), ("counts", C.c_void_p), ("reserved", C.c_uint64)]


VALUE_CLIP = 1  # GYMRS_VALUE_CLIP


class AdvantageStats(C.Structure):
    """``gymrs_advantage_stats`` (include/gymrs_amd.h), 40 bytes: one set's integer sums and the two numbers pass 3 used."""
    _fields_ = [("s1", C.c_int64), ("n", C.c_uint64), ("s2", C.c_uint64), ("non_members", C.c_uint64), ("mean", C.c_float), ("inv", C.c_float)]


ADVANTAGE_STATS_DTYPE = np.dtype([("s1", "<i8"), ("n", "<u8"), ("s2", "<u8"), ("non_members", "<u8"), ("mean", "<f4"), ("inv", "<f4")])


class NormalizeDesc(C.Structure):
    """``gymrs_normalize_desc`` (include/gymrs_amd.h), 64 bytes."""
    _fields_ = [("n_steps", C.c_uint32), ("flags", C.c_uint32), ("eps", C.c_float), ("n_sets", C.c_uint32), ("lanes_per_policy", C.c_uint64),
                ("lane_stride", C.c_uint64), ("adv", C.c_void_p), ("out", C.c_void_p), ("stats", C.c_void_p), ("reserved", C.c_uint64)]


class QDesc(C.Structure):
    """``gymrs_q_desc`` (include/gymrs_amd.h), 120 bytes: the record by value, two observation buffers in, the td row out, two tables
    and an optional pair of counters per set added to."""
    _fields_ = [("n_steps", C.c_uint32), ("flags", C.c_uint32), ("gamma", C.c_float), ("kappa", C.c_float), ("record", Trajectory),
                ("start_obs", C.c_void_p), ("final_obs", C.c_void_p), ("td", C.c_void_p), ("grad", C.c_void_p), ("excluded", C.c_void_p),
                ("counts", C.c_void_p), ("reserved", C.c_uint64)]


Q_DOUBLE = 1  # GYMRS_Q_DOUBLE


class Replay(C.Structure):
    """``gymrs_replay`` (include/gymrs_amd.h), 56 bytes: the store in caller-owned device memory.  ``s`` / ``s_next`` are
    [D][capacity] f32, the rest [capacity].  ``head`` and ``count`` (plain attributes, not part of the struct) are the ring position
    and the fill that the C caller advances itself: ``BatchedEngine.replay_push`` keeps them here."""
    _fields_ = [("s", C.c_void_p), ("s_next", C.c_void_p), ("action", C.c_void_p), ("reward", C.c_void_p), ("done", C.c_void_p),
                ("priority", C.c_void_p), ("capacity", C.c_uint64)]
    head = 0
    count = 0


class ReplayPushDesc(C.Structure):
    """``gymrs_replay_push_desc`` (include/gymrs_amd.h), 152 bytes."""
    _fields_ = [("n_steps", C.c_uint32), ("flags", C.c_uint32), ("record", Trajectory), ("start_obs", C.c_void_p), ("final_obs", C.c_void_p),
                ("store", Replay), ("head", C.c_uint64), ("priority", C.c_uint32), ("pad_", C.c_uint32), ("reserved", C.c_uint64)]


class ReplaySampleDesc(C.Structure):
    """``gymrs_replay_sample_desc`` (include/gymrs_amd.h), 176 bytes."""
    _fields_ = [("store", Replay), ("count", C.c_uint64), ("n_samples", C.c_uint32), ("flags", C.c_uint32), ("seed", C.c_uint64),
                ("draw", C.c_uint64), ("batch", Trajectory), ("start_obs", C.c_void_p), ("idx", C.c_void_p), ("prio", C.c_void_p),
                ("total", C.c_void_p), ("reserved", C.c_uint64)]


class ReplayUpdateDesc(C.Structure):
    """``gymrs_replay_update_desc`` (include/gymrs_amd.h), 104 bytes."""
    _fields_ = [("store", Replay), ("idx", C.c_void_p), ("td", C.c_void_p), ("n_samples", C.c_uint32), ("flags", C.c_uint32),
                ("alpha", C.c_float), ("eps", C.c_float), ("cap", C.c_float), ("pad_", C.c_float), ("reserved", C.c_uint64)]


REPLAY_MAX_PRIORITY = 1 << 24  # the priority of a fresh transition and of an unknown error
REPLAY_NONE = 0xFFFFFFFF       # idx of a draw from a store without mass


class OptimizerDesc(C.Structure):
    """``gymrs_optimizer_desc`` (include/gymrs_amd.h), 72 bytes: head, kind, flags, seven floats, two tables read (and zeroed with
    ``OPT_ZERO_GRAD``), one optional counter added to."""
    _fields_ = [("head", C.c_uint32), ("kind", C.c_uint32), ("flags", C.c_uint32), ("lr", C.c_float), ("grad_scale", C.c_float),
                ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float), ("max_norm", C.c_float), ("tau", C.c_float),
                ("grad", C.c_void_p), ("excluded", C.c_void_p), ("skipped", C.c_void_p), ("reserved", C.c_uint64)]


OPT_HEAD_POLICY, OPT_HEAD_CRITIC = 0, 1  # GYMRS_OPT_HEAD_*
OPT_SGD, OPT_ADAM = 0, 1                 # GYMRS_OPT_SGD / _ADAM
OPT_ASCEND, OPT_ZERO_GRAD = 1, 2         # GYMRS_OPT_ASCEND / _ZERO_GRAD


def _optimizer_desc(head, kind, lr, grad_scale, beta1, beta2, eps, max_norm, tau, ascend, zero_grad, flags, grad=0, excluded=0,
                    skipped=None) -> OptimizerDesc:
    f = ((OPT_ASCEND if ascend else 0) | (OPT_ZERO_GRAD if zero_grad else 0)) if flags is None else int(flags)
    return OptimizerDesc(int(head), int(kind), f, float(lr), float(grad_scale), float(beta1), float(beta2), float(eps), float(max_norm),
                         float(tau), C.c_void_p(grad or None), C.c_void_p(excluded or None), C.c_void_p(skipped or None), 0)


class EsDesc(C.Structure):
    """``gymrs_es_desc`` (include/gymrs_amd.h), 32 bytes."""
    _fields_ = [("hidden", C.c_uint32), ("n_policies", C.c_uint32), ("lanes_per_policy", C.c_uint64), ("seed", C.c_uint64),
                ("sigma", C.c_float), ("reserved", C.c_uint32)]


class EsStepDesc(C.Structure):
    """``gymrs_es_step_desc`` (include/gymrs_amd.h), 56 bytes: kind, flags, seven floats, the optional utilities row, one optional
    counter added to."""
    _fields_ = [("kind", C.c_uint32), ("flags", C.c_uint32), ("lr", C.c_float), ("grad_scale", C.c_float), ("beta1", C.c_float),
                ("beta2", C.c_float), ("eps", C.c_float), ("max_norm", C.c_float), ("sigma_next", C.c_float), ("reserved", C.c_uint32),
                ("utilities", C.c_void_p), ("skipped", C.c_void_p)]


ES_MAX_POLICIES = 1 << 20  # GYMRS_ES_MAX_POLICIES


class EsRanksDesc(C.Structure):
    """``gymrs_es_ranks_desc`` (include/gymrs_amd.h), 24 bytes: the utilities row, the optional rank2 row, two zero words."""
    _fields_ = [("utilities", C.c_void_p), ("rank2", C.c_void_p), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


ES_RANK_INVALID = 0xFFFFFFFF  # GYMRS_ES_RANK_INVALID


class Exploration(C.Structure):
    """``gymrs_exploration`` (include/gymrs_amd.h), 16 bytes: epsilon = threshold / 65536."""
    _fields_ = [("seed", C.c_uint64), ("threshold", C.c_uint32), ("reserved", C.c_uint32)]


def _exploration(seed, epsilon, threshold) -> Exploration:
    """Exactly one of ``epsilon`` (a float in [0, 1], rounded to the nearest 1 / 65536) and ``threshold`` (0 .. 65536)."""
    if (epsilon is None) == (threshold is None):
        raise ValueError("give exactly one of epsilon and threshold")
    if threshold is None:
        if not 0.0 <= float(epsilon) <= 1.0:
            raise ValueError(f"epsilon must be in [0, 1], got {epsilon}")
        threshold = int(round(float(epsilon) * 65536))
    if not 0 <= int(threshold) < 2**32:
        raise ValueError(f"threshold must be in 0 .. 65536, got {threshold}")
    return Exploration(int(seed) & (2**64 - 1), int(threshold), 0)


def explore_draw(seed: int, threshold: int, n_actions: int, global_id, tick):
    """``gymrs_explore_draw`` (host only, no GPU): (explored, random_action) of the epsilon-greedy draw that takes lane
    ``global_id`` from engine tick ``tick`` to ``tick + 1``.  ``global_id`` and ``tick`` broadcast against each other; scalars give
    a (bool, int) pair, arrays a (bool array, uint8 array) pair.  A recorded action of row k of a launch that started at tick t0
    was exploratory where ``explore_draw(seed, threshold, n_actions, offset + lane, t0 + k)[0]`` says so."""
    lib = load_library()
    x = Exploration(int(seed) & (2**64 - 1), int(threshold), 0)
    g, t = np.broadcast_arrays(np.asarray(global_id, dtype=np.uint64), np.asarray(tick, dtype=np.uint64))
    explored = np.empty(g.shape, np.bool_)
    action = np.empty(g.shape, np.uint8)
    e, a = C.c_uint8(), C.c_uint8()
    for i in np.ndindex(g.shape):
        _check(lib, lib.gymrs_explore_draw(C.byref(x), int(n_actions), int(g[i]), int(t[i]), C.byref(e), C.byref(a)))
        explored[i], action[i] = bool(e.value), a.value
    if g.shape == ():
        return bool(explored), int(action)
    return explored, action


class Sampling(C.Structure):
    """``gymrs_sampling`` (include/gymrs_amd.h), 16 bytes: scale = log2(e) / temperature."""
    _fields_ = [("seed", C.c_uint64), ("scale", C.c_float), ("reserved", C.c_uint32)]


LOG2E = 1.4426950408889634  # log2(e): the sampling rule works in base 2


def _sampling(seed, temperature, scale) -> Sampling:
    """Exactly one of ``temperature`` (> 0; scale = log2(e) / temperature rounded to f32) and ``scale`` (finite, >= 0)."""
    if (temperature is None) == (scale is None):
        raise ValueError("give exactly one of temperature and scale")
    if scale is None:
        if not float(temperature) > 0.0:
            raise ValueError(f"temperature must be > 0, got {temperature}")
        scale = LOG2E / float(temperature)
    return Sampling(int(seed) & (2**64 - 1), float(scale), 0)


def sample_draw(seed: int, scale: float, logits, global_id: int, tick: int):
    """``gymrs_sample_draw`` (host only, no GPU): (action, probs) of the softmax draw that takes lane ``global_id`` from engine
    tick ``tick`` to ``tick + 1`` under the f32 ``logits`` (2 .. 8 of them): the definition of include/gymrs_amd.h, "sampling", as
    code.  ``probs`` is a float32 array, one per action."""
    lib = load_library()
    x = Sampling(int(seed) & (2**64 - 1), float(scale), 0)
    y = np.ascontiguousarray(logits, dtype=np.float32).reshape(-1)
    probs = np.empty(y.shape, np.float32)
    a = C.c_uint8()
    _check(lib, lib.gymrs_sample_draw(C.byref(x), int(y.size), y.ctypes.data_as(C.POINTER(C.c_float)), int(global_id), int(tick), C.byref(a),
                                      probs.ctypes.data_as(C.POINTER(C.c_float))))
    return int(a.value), probs


def _closed_loop_desc(n_envs, n_steps, lane_params, fitness, record, flags=None, explore=False, sample=False) -> ClosedLoopDesc:
    """``record``: None, a ``Trajectory``, or a mapping with the keyword arguments of ``rollout_policy_record`` (device addresses
    ``obs``, ``actions``, ``reward``, ``done``, optionally ``truncated`` and ``lane_stride``).  The descriptor keeps it alive."""
    f = ((CLOSED_LOOP_FITNESS if fitness else 0) | (CLOSED_LOOP_LANE_PARAMS if lane_params else 0) |
         (CLOSED_LOOP_EXPLORE if explore else 0) | (CLOSED_LOOP_SAMPLE if sample else 0)) if flags is None else int(flags)
    traj = record
    if record is not None and not isinstance(record, Trajectory):
        stride = record.get("lane_stride")
        traj = Trajectory(C.c_void_p(record["obs"]), C.c_void_p(record["actions"]), C.c_void_p(record["reward"]), C.c_void_p(record["done"]),
                          C.c_void_p(record.get("truncated") or None), int(stride) if stride is not None else (n_envs + 15) // 16 * 16)
    return ClosedLoopDesc(int(n_steps), f, C.pointer(traj) if traj is not None else None, 0)


def _eval_desc(episodes_per_lane, max_episode_steps, seed, common_starts, lengths, flags, lane_params=False) -> EvalDesc:
    f = ((EVAL_COMMON_STARTS if common_starts else 0) | (EVAL_LANE_PARAMS if lane_params else 0)) if flags is None else int(flags)
    return EvalDesc(int(episodes_per_lane), int(max_episode_steps), int(seed) & (2**64 - 1), f, 0, C.c_void_p(lengths or None))


class PolicyDesc(C.Structure):
    """``gymrs_policy_desc`` (include/gymrs_amd.h)."""
    _fields_ = [("hidden", C.c_uint32), ("n_policies", C.c_uint32), ("lanes_per_policy", C.c_uint64)]


_PARAMS = {CARTPOLE: CartPoleParams, MOUNTAIN_CAR: MountainCarParams, PENDULUM: PendulumParams}
_STATE_DIM = {CARTPOLE: 4, MOUNTAIN_CAR: 2, PENDULUM: 2}
_OBS_DIM = {CARTPOLE: 4, MOUNTAIN_CAR: 2, PENDULUM: 3}
_ACTION_DTYPE = {CARTPOLE: np.uint8, MOUNTAIN_CAR: np.uint8, PENDULUM: np.float32}


def default_params(kind: int):
    lib = load_library()
    p = _PARAMS[kind]()
    _check(lib, lib.gymrs_default_params(kind, C.byref(p)))
    return p


def policy_size(kind: int, hidden: int = 0) -> int:
    """Floats of one policy of ``gymrs_set_policy``: affine (``hidden`` = 0) ``W[A][D], b[A]``, else ``W1[H][D], b1[H], W2[A][H],
    b2[A]`` (host only, no GPU).  Raises for Pendulum and ``hidden`` > 64."""
    lib = load_library()
    n = C.c_uint64()
    _check(lib, lib.gymrs_policy_size(int(kind), int(hidden), C.byref(n)))
    return n.value


def critic_size(kind: int, hidden: int = 0) -> int:
    """Floats of one critic of ``gymrs_set_critic``: affine (``hidden`` = 0) ``W[D], b``, else ``W1[H][D], b1[H], W2[H], b2``: the
    policy layout with one action (host only, no GPU).  Raises for Pendulum and ``hidden`` > 64."""
    lib = load_library()
    n = C.c_uint64()
    _check(lib, lib.gymrs_critic_size(int(kind), int(hidden), C.byref(n)))
    return n.value


def critic_value(kind: int, hidden: int, weights, obs) -> np.float32:
    """``gymrs_critic_value`` (host only, no GPU): V(obs) under one critic of ``critic_size(kind, hidden)`` f32 weights: the
    definition of include/gymrs_amd.h, "advantages", as code."""
    lib = load_library()
    w = np.ascontiguousarray(weights, dtype=np.float32).reshape(-1)
    x = np.ascontiguousarray(obs, dtype=np.float32).reshape(-1)
    if w.size != critic_size(kind, hidden) or x.size != _OBS_DIM[kind]:
        raise ValueError(f"critic_value needs {critic_size(kind, hidden)} weights and {_OBS_DIM[kind]} observation components")
    v = C.c_float()
    fp = C.POINTER(C.c_float)
    _check(lib, lib.gymrs_critic_value(int(kind), int(hidden), w.ctypes.data_as(fp), x.ctypes.data_as(fp), C.byref(v)))
    return np.float32(v.value)


def gradient_lane(kind: int, hidden: int, weights, x, actions, coef, *, critic: bool = False, temperature: Optional[float] = None,
                  scale: Optional[float] = None, prob: bool = False):
    """``gymrs_gradient_lane`` (host only, no GPU): one lane's contribution to ``gymrs_policy_gradient`` -- the definition of
    include/gymrs_amd.h, "gradients", as code.  ``weights``: ONE policy (``policy_size`` floats) or, with ``critic``, one critic
    (``critic_size``); ``x`` [K][D] the observation every step started from, ``actions`` [K] (ignored with ``critic``), ``coef`` [K].
    Returns (q, excluded) or, with ``prob``, (q, excluded, prob [K]): q is int64 [S], the gradient is q * 2**-24."""
    lib = load_library()
    w = np.ascontiguousarray(weights, dtype=np.float32).reshape(-1)
    size = critic_size(kind, hidden) if critic else policy_size(kind, hidden)
    c = np.ascontiguousarray(coef, dtype=np.float32).reshape(-1)
    xs = np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
    if w.size != size or xs.size != c.size * _OBS_DIM[kind]:
        raise ValueError(f"gradient_lane needs {size} weights and {_OBS_DIM[kind]} observation components per step")
    if prob and critic:
        raise ValueError("the critic head has no probabilities")
    a = None
    if not critic:
        a = np.ascontiguousarray(actions, dtype=np.uint8).reshape(-1)
        if a.size != c.size:
            raise ValueError("gradient_lane needs one action per step")
        scale = _sampling(0, temperature, scale).scale
    q = np.zeros(size, np.int64)
    excluded = C.c_uint64()
    pr = np.empty(c.size, np.float32) if prob else None
    fp = C.POINTER(C.c_float)
    _check(lib, lib.gymrs_gradient_lane(int(kind), int(hidden), GRADIENT_CRITIC if critic else 0, float(scale or 0.0), w.ctypes.data_as(fp), int(c.size),
                                        xs.ctypes.data_as(fp), a.ctypes.data_as(C.POINTER(C.c_uint8)) if a is not None else None, c.ctypes.data_as(fp),
                                        q.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(excluded), pr.ctypes.data_as(fp) if prob else None))
    return (q, excluded.value, pr) if prob else (q, excluded.value)


def _clip_bounds(clip, clip_low, clip_high):
    """(clip_low, clip_high) as f32: either ``clip`` (epsilon: 1 - clip and 1 + clip rounded to f32) or both bounds."""
    if (clip_low is None) != (clip_high is None):
        raise ValueError("give clip_low and clip_high together")
    if clip_low is None:
        if clip is None:
            raise ValueError("give clip, or clip_low and clip_high")
        return float(np.float32(1.0 - float(clip))), float(np.float32(1.0 + float(clip)))
    return float(np.float32(clip_low)), float(np.float32(clip_high))


def ppo_lane(kind: int, hidden: int, weights, x, actions, advantages, old_prob, *, clip: Optional[float] = 0.2, clip_low: Optional[float] = None,
             clip_high: Optional[float] = None, temperature: Optional[float] = None, scale: Optional[float] = None, prob: bool = False):
    """``gymrs_ppo_lane`` (host only, no GPU): one lane's contribution to ``gymrs_ppo_gradient`` -- the definition of
    include/gymrs_amd.h, "clipped surrogate", as code.  ``weights``: ONE policy; ``x`` [K][D], ``actions`` [K], ``advantages`` [K],
    ``old_prob`` [K].  Returns (q, excluded, counts) or, with ``prob``, (q, excluded, counts, prob [K]): q is int64 [S], counts is
    uint64 [2] = (lane-steps with an action in range, those that were cut)."""
    lib = load_library()
    w = np.ascontiguousarray(weights, dtype=np.float32).reshape(-1)
    size = policy_size(kind, hidden)
    adv = np.ascontiguousarray(advantages, dtype=np.float32).reshape(-1)
    po = np.ascontiguousarray(old_prob, dtype=np.float32).reshape(-1)
    xs = np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
    a = np.ascontiguousarray(actions, dtype=np.uint8).reshape(-1)
    if w.size != size or xs.size != adv.size * _OBS_DIM[kind]:
        raise ValueError(f"ppo_lane needs {size} weights and {_OBS_DIM[kind]} observation components per step")
    if a.size != adv.size or po.size != adv.size:
        raise ValueError("ppo_lane needs one action and one old probability per step")
    low, high = _clip_bounds(clip, clip_low, clip_high)
    s = _sampling(0, temperature, scale).scale
    q = np.zeros(size, np.int64)
    excluded = C.c_uint64()
    counts = np.zeros(2, np.uint64)
    pr = np.empty(adv.size, np.float32) if prob else None
    fp, up = C.POINTER(C.c_float), C.POINTER(C.c_uint64)
    _check(lib, lib.gymrs_ppo_lane(int(kind), int(hidden), float(s), low, high, w.ctypes.data_as(fp), int(adv.size), xs.ctypes.data_as(fp),
                                   a.ctypes.data_as(C.POINTER(C.c_uint8)), adv.ctypes.data_as(fp), po.ctypes.data_as(fp),
                                   q.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(excluded), counts.ctypes.data_as(up),
                                   pr.ctypes.data_as(fp) if prob else None))
    return (q, excluded.value, counts, pr) if prob else (q, excluded.value, counts)


def vtrace_lane(kind: int, policy_hidden: int, critic_hidden: int, policy_weights, critic_weights, x, x_next, actions, reward, done, ended,
                old_prob, *, gamma: float, lam: float, rho_bar: float = 1.0, c_bar: float = 1.0, pg_rho_bar: float = 1.0,
                temperature: Optional[float] = None, scale: Optional[float] = None):
    """``gymrs_vtrace_lane`` (host only, no GPU): one lane of ``gymrs_vtrace`` -- the definition of include/gymrs_amd.h, "V-trace", as
    code.  ONE policy and ONE critic; ``x`` [K][D] (the observation each action was drawn from), ``x_next`` [K][D] (the successor,
    already selected), ``actions``, ``reward``, ``done``, ``ended``, ``old_prob`` [K].  Exactly one of ``temperature`` / ``scale``.
    Returns (vs, pg_advantages, values, prob, counts): f32 [K] each, counts uint64 [3] = (lane-steps with an action in range, of those
    ratio > rho_bar, of those ratio > c_bar)."""
    lib = load_library()
    f32 = lambda v: np.ascontiguousarray(v, dtype=np.float32).reshape(-1)  # noqa: E731
    u8 = lambda v: np.ascontiguousarray(v, dtype=np.uint8).reshape(-1)  # noqa: E731
    wp, wc, xs, xn, r, po = f32(policy_weights), f32(critic_weights), f32(x), f32(x_next), f32(reward), f32(old_prob)
    a, dn, en = u8(actions), u8(done), u8(ended)
    if wp.size != policy_size(kind, policy_hidden) or wc.size != critic_size(kind, critic_hidden):
        raise ValueError("vtrace_lane needs one policy's and one critic's weights")
    if xs.size != r.size * _OBS_DIM[kind] or xn.size != xs.size or any(v.size != r.size for v in (po, a, dn, en)):
        raise ValueError(f"vtrace_lane needs {_OBS_DIM[kind]} observation components and one of every row per step")
    s = _sampling(0, temperature, scale).scale
    vs, pg, values, prob = (np.empty(r.size, np.float32) for _ in range(4))
    counts = np.zeros(3, np.uint64)
    fp, bp = C.POINTER(C.c_float), C.POINTER(C.c_uint8)
    _check(lib, lib.gymrs_vtrace_lane(int(kind), int(policy_hidden), int(critic_hidden), wp.ctypes.data_as(fp), wc.ctypes.data_as(fp), int(r.size),
                                      xs.ctypes.data_as(fp), xn.ctypes.data_as(fp), a.ctypes.data_as(bp), r.ctypes.data_as(fp), dn.ctypes.data_as(bp),
                                      en.ctypes.data_as(bp), po.ctypes.data_as(fp), float(gamma), float(lam), float(s), float(rho_bar), float(c_bar),
                                      float(pg_rho_bar), vs.ctypes.data_as(fp), pg.ctypes.data_as(fp), values.ctypes.data_as(fp),
                                      prob.ctypes.data_as(fp), counts.ctypes.data_as(C.POINTER(C.c_uint64))))
    return vs, pg, values, prob, counts


def entropy_log2(v: float) -> float:
    """``gymrs_entropy_log2`` (host only, no GPU): the bit-defined f32 log2 of include/gymrs_amd.h, "Entropy", for a finite
    ``v >= 2**-126``."""
    lib = load_library()
    out = C.c_float()
    _check(lib, lib.gymrs_entropy_log2(float(v), C.byref(out)))
    return out.value


def entropy_lane(kind: int, hidden: int, weights, x, actions=None, old_prob=None, *, coef: float, temperature: Optional[float] = None,
                 scale: Optional[float] = None):
    """``gymrs_entropy_lane`` (host only, no GPU): one lane's contribution to ``gymrs_entropy_gradient`` -- the definition of
    include/gymrs_amd.h, "Entropy", as code.  ``weights``: ONE policy; ``x`` [K][D]; ``actions`` [K] and ``old_prob`` [K] together, or
    neither (no KL estimate).  Returns (q, excluded, sums, counts): q is int64 [S], the gradient of coef * entropy is q * 2**-24; sums
    is int64 [2] = the fixed points of (the lane's entropy sum in nats, its k3 KL sum); counts is uint64 [2] = the lane-steps in each."""
    lib = load_library()
    w = np.ascontiguousarray(weights, dtype=np.float32).reshape(-1)
    size = policy_size(kind, hidden)
    xs = np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
    k = xs.size // _OBS_DIM[kind]
    if w.size != size or xs.size != k * _OBS_DIM[kind]:
        raise ValueError(f"entropy_lane needs {size} weights and {_OBS_DIM[kind]} observation components per step")
    a = po = None
    if old_prob is not None:
        if actions is None:
            raise ValueError("entropy_lane needs actions with old_prob")
        a = np.ascontiguousarray(actions, dtype=np.uint8).reshape(-1)
        po = np.ascontiguousarray(old_prob, dtype=np.float32).reshape(-1)
        if a.size != k or po.size != k:
            raise ValueError("entropy_lane needs one action and one old probability per step")
    s = _sampling(0, temperature, scale).scale
    q = np.zeros(size, np.int64)
    excluded = C.c_uint64()
    sums, counts = np.zeros(2, np.int64), np.zeros(2, np.uint64)
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int64)
    _check(lib, lib.gymrs_entropy_lane(int(kind), int(hidden), float(s), float(coef), w.ctypes.data_as(fp), int(k), xs.ctypes.data_as(fp),
                                       a.ctypes.data_as(C.POINTER(C.c_uint8)) if a is not None else None, po.ctypes.data_as(fp) if po is not None else None,
                                       q.ctypes.data_as(ip), C.byref(excluded), sums.ctypes.data_as(ip), counts.ctypes.data_as(C.POINTER(C.c_uint64))))
    return q, excluded.value, sums, counts


def value_lane(kind: int, hidden: int, weights, x, returns, old_values=None, *, clip: float = 0.0):
    """``gymrs_value_lane`` (host only, no GPU): one lane's contribution to ``gymrs_value_gradient`` -- the definition of
    include/gymrs_amd.h, "Value loss", as code.  ``weights``: ONE critic; ``x`` [K][D], ``returns`` [K]; ``old_values`` [K] with ``clip``
    is GYMRS_VALUE_CLIP, None the plain squared error.  Returns (q, excluded, sums, counts, values): q is int64 [S]; sums is int64 [2] =
    the fixed points of (sum e1^2, sum of the larger squares); counts is uint64 [2] = (lane-steps, cut ones); values is f32 [K]."""
    lib = load_library()
    w = np.ascontiguousarray(weights, dtype=np.float32).reshape(-1)
    size = critic_size(kind, hidden)
    r = np.ascontiguousarray(returns, dtype=np.float32).reshape(-1)
    xs = np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
    if w.size != size or xs.size != r.size * _OBS_DIM[kind]:
        raise ValueError(f"value_lane needs {size} weights and {_OBS_DIM[kind]} observation components per step")
    vo = None
    if old_values is not None:
        vo = np.ascontiguousarray(old_values, dtype=np.float32).reshape(-1)
        if vo.size != r.size:
            raise ValueError("value_lane needs one old value per step")
    q = np.zeros(size, np.int64)
    excluded = C.c_uint64()
    sums, counts, values = np.zeros(2, np.int64), np.zeros(2, np.uint64), np.empty(r.size, np.float32)
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int64)
    _check(lib, lib.gymrs_value_lane(int(kind), int(hidden), float(clip), w.ctypes.data_as(fp), int(r.size), xs.ctypes.data_as(fp), r.ctypes.data_as(fp),
                                     vo.ctypes.data_as(fp) if vo is not None else None, q.ctypes.data_as(ip), C.byref(excluded), sums.ctypes.data_as(ip),
                                     counts.ctypes.data_as(C.POINTER(C.c_uint64)), values.ctypes.data_as(fp)))
    return q, excluded.value, sums, counts, values


def normalize_host(a, *, eps: float = 1e-6):
    """``gymrs_normalize_host`` (host only, no GPU): the rule of include/gymrs_amd.h, "Advantage normalisation", for ONE set.
    Returns (out f32 [count], stats): stats is a numpy record of ``ADVANTAGE_STATS_DTYPE``."""
    lib = load_library()
    src = np.ascontiguousarray(a, dtype=np.float32).reshape(-1)
    out = np.empty(src.size, np.float32)
    st = np.zeros(1, ADVANTAGE_STATS_DTYPE)
    fp = C.POINTER(C.c_float)
    _check(lib, lib.gymrs_normalize_host(src.ctypes.data_as(fp), int(src.size), float(eps), out.ctypes.data_as(fp), C.c_void_p(st.ctypes.data)))
    return out, st[0]


def q_lane(kind: int, hidden: int, weights, target_weights, x, x_next, actions, reward, done, *, gamma: float, kappa: float = float("inf"),
           double: bool = False, flags: Optional[int] = None):
    """``gymrs_q_lane`` (host only, no GPU): one lane's contribution to ``gymrs_q_gradient`` -- the definition of include/gymrs_amd.h,
    "Q-learning", as code.  ``weights`` / ``target_weights``: ONE online and ONE target network (``policy_size`` floats each); ``x``
    [K][D] the observation every step started from, ``x_next`` [K][D] the already selected successor, ``actions`` [K], ``reward`` [K],
    ``done`` [K] (it alone decides the bootstrap).  Returns (q, excluded, td [K], counts): q is int64 [S], the gradient of the Huber
    loss is q * 2**-24; counts is uint64 [2] = (lane-steps with an action in range, those with |delta| > kappa)."""
    lib = load_library()
    size = policy_size(kind, hidden)
    w, wt, xs, xn, r = (np.ascontiguousarray(v, dtype=np.float32).reshape(-1) for v in (weights, target_weights, x, x_next, reward))
    a, dn = (np.ascontiguousarray(v, dtype=np.uint8).reshape(-1) for v in (actions, done))
    k, d = r.size, _OBS_DIM[kind]
    if w.size != size or wt.size != size or xs.size != k * d or xn.size != k * d or a.size != k or dn.size != k:
        raise ValueError(f"q_lane needs {size} weights per network and, per step, 2 x {d} observation components, an action, a reward and a done flag")
    q = np.zeros(size, np.int64)
    excluded = C.c_uint64()
    td = np.zeros(k, np.float32)
    counts = np.zeros(2, np.uint64)
    fp, bp = C.POINTER(C.c_float), C.POINTER(C.c_uint8)
    f = (Q_DOUBLE if double else 0) if flags is None else int(flags)
    _check(lib, lib.gymrs_q_lane(int(kind), int(hidden), f, float(gamma), float(kappa), w.ctypes.data_as(fp), wt.ctypes.data_as(fp), k, xs.ctypes.data_as(fp),
                                 xn.ctypes.data_as(fp), a.ctypes.data_as(bp), r.ctypes.data_as(fp), dn.ctypes.data_as(bp), q.ctypes.data_as(C.POINTER(C.c_int64)),
                                 C.byref(excluded), td.ctypes.data_as(fp), counts.ctypes.data_as(C.POINTER(C.c_uint64))))
    return q, excluded.value, td, counts


def optimizer_set(q, w, *, kind: int = OPT_SGD, lr: float, grad_scale: float, m=None, v=None, pw=None, target=None, beta1: float = 0.9,
                  beta2: float = 0.999, eps: float = 1e-8, max_norm: float = float("inf"), tau: float = 0.0, ascend: bool = False,
                  flags: Optional[int] = None):
    """``gymrs_optimizer_set`` (host only, no GPU): one set's update by the definition of include/gymrs_amd.h, "Optimizer", as code.
    ``q`` int64 [S] is one row of a gradient table, ``w`` f32 [S] the weights; ``OPT_ADAM`` needs ``m``, ``v`` [S] and ``pw`` [2],
    ``tau`` > 0 needs ``target`` [S].  Returns fresh arrays (w, m, v, pw, target); what was not given stays ``None``."""
    lib = load_library()
    qq = np.ascontiguousarray(q, dtype=np.int64).reshape(-1)
    out = [None if a is None else np.array(a, dtype=np.float32).reshape(-1) for a in (w, m, v, pw, target)]
    if out[0] is None or out[0].size != qq.size or any(a is not None and a.size != n for a, n in zip(out[1:], (qq.size, qq.size, 2, qq.size))):
        raise ValueError("optimizer_set needs S weights (and moments, target) for S table entries, and pw of 2 floats")
    desc = _optimizer_desc(OPT_HEAD_POLICY, kind, lr, grad_scale, beta1, beta2, eps, max_norm, tau, ascend, False, flags)
    fp = C.POINTER(C.c_float)
    _check(lib, lib.gymrs_optimizer_set(C.byref(desc), qq.size, qq.ctypes.data_as(C.POINTER(C.c_int64)),
                                        *(None if a is None else a.ctypes.data_as(fp) for a in out)))
    return tuple(out)


def es_noise(seed: int, generation: int, pair, s) -> np.ndarray:
    """``gymrs_es_noise`` (host only, no GPU): eps(generation, pair, s) of include/gymrs_amd.h, "Evolution strategies", as f32;
    ``pair`` and ``s`` broadcast against each other."""
    lib = load_library()
    pairs, ss = np.broadcast_arrays(np.asarray(pair, dtype=np.uint64), np.asarray(s, dtype=np.uint32))
    out = np.empty(pairs.shape, np.float32)
    eps = C.c_float()
    for i in np.ndindex(*pairs.shape):
        _check(lib, lib.gymrs_es_noise(int(seed) & (2**64 - 1), int(generation) & (2**64 - 1), int(pairs[i]), int(ss[i]), C.byref(eps)))
        out[i] = eps.value
    return out


def es_utilities(records) -> np.ndarray:
    """``gymrs_es_utilities`` (host only, no GPU): the f32 utilities of P policies from their episodic records, int64 (P, 8) as
    ``BatchedEngine.policy_eval`` returns them."""
    lib = load_library()
    rec = np.ascontiguousarray(records, dtype=np.int64).reshape(-1, 8)
    out = np.empty(rec.shape[0], np.float32)
    _check(lib, lib.gymrs_es_utilities(rec.ctypes.data_as(C.c_void_p), rec.shape[0], out.ctypes.data_as(C.POINTER(C.c_float))))
    return out


def replay_priority(td: float, *, alpha: float, eps: float, cap: float) -> int:
    """``gymrs_replay_priority`` (host only, no GPU): the integer priority in 1 .. 2**24 of a TD error, the rule of
    include/gymrs_amd.h, "Replay": round(2**24 * (min(|td| + eps, cap) / cap) ** alpha) in the bit-defined f32 arithmetic."""
    lib = load_library()
    out = C.c_uint32()
    _check(lib, lib.gymrs_replay_priority(float(td), float(alpha), float(eps), float(cap), C.byref(out)))
    return out.value


def replay_draw(priority, n_samples: int, *, seed: int, draw: int) -> Tuple[np.ndarray, int]:
    """``gymrs_replay_draw`` (host only, no GPU): (idx uint32 [n_samples], total) of the stratified proportional draw of
    include/gymrs_amd.h, "Replay", over the priorities ``priority`` [count]."""
    lib = load_library()
    p = np.ascontiguousarray(priority, dtype=np.uint32).reshape(-1)
    idx, total = np.empty(max(int(n_samples), 0), np.uint32), C.c_uint64()
    _check(lib, lib.gymrs_replay_draw(p.ctypes.data_as(C.POINTER(C.c_uint32)), p.size, int(n_samples), int(seed) & (2**64 - 1),
                                      int(draw) & (2**64 - 1), idx.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(total)))
    return idx, total.value


def es_rank_utilities(records) -> Tuple[np.ndarray, np.ndarray]:
    """``gymrs_es_rank_utilities`` (host only, no GPU): (u f32 [P], rank2 uint32 [P]), the centred, tie-averaged rank utilities of P
    policies from their episodic records, int64 (P, 8) as ``BatchedEngine.policy_eval`` returns them."""
    lib = load_library()
    rec = np.ascontiguousarray(records, dtype=np.int64).reshape(-1, 8)
    u, rank2 = np.empty(rec.shape[0], np.float32), np.empty(rec.shape[0], np.uint32)
    _check(lib, lib.gymrs_es_rank_utilities(rec.ctypes.data_as(C.c_void_p), rec.shape[0], u.ctypes.data_as(C.POINTER(C.c_float)),
                                            rank2.ctypes.data_as(C.POINTER(C.c_uint32))))
    return u, rank2


def params_from_json(kind: int, text: str, params=None):
    """Inverse of ``BatchedEngine.env_json`` for the physics fields: (params, state or None).  Missing keys keep the
    value in ``params`` (default: the env's defaults)."""
    lib = load_library()
    p = params if params is not None else default_params(kind)
    state = (C.c_double * 4)()
    dim = C.c_int()
    _check(lib, lib.gymrs_params_from_json(int(kind), text.encode("utf-8"), C.byref(p), state, C.byref(dim)))
    return p, ([state[j] for j in range(dim.value)] if dim.value else None)


def _check(lib, status: int) -> None:
    if status == _OK:
        return
    msg = lib.gymrs_last_error().decode("utf-8", "replace")
    if status == _EACTION:
        raise InvalidActionError(status, msg)
    raise GymrsError(status, msg)


def _set_weights(lib, setter, handle, kind, weights, hidden, lanes, size_of, plural) -> None:
    """``gymrs_set_policy`` / ``gymrs_set_critic`` / ``gymrs_sharded_set_policy``: ``weights`` (None removes the set) holds a whole
    number of networks of ``size_of(kind, hidden)`` floats."""
    if weights is None:
        _check(lib, setter(handle, None, None))
        return
    w = np.ascontiguousarray(weights, dtype=np.float32)
    size = size_of(kind, hidden)
    if w.size == 0 or w.size % size != 0:
        raise ValueError(f"weights must hold a whole number (>= 1) of {plural} of {size} floats, got {w.size}")
    desc = PolicyDesc(int(hidden), w.size // size, int(lanes))
    _check(lib, setter(handle, C.byref(desc), w.ctypes.data_as(C.c_void_p)))


def _describe(lib, getter, handle) -> PolicyDesc:
    """``gymrs_get_policy`` / ``gymrs_get_critic`` as a query of the description."""
    desc = PolicyDesc()
    _check(lib, getter(handle, C.byref(desc), None, 0))
    return desc


def _get_weights(lib, getter, handle, kind, size_of):
    """``gymrs_get_policy`` / ``gymrs_get_critic``: (weights of shape (n, size), hidden, lanes per network) (synchronising)."""
    desc = _describe(lib, getter, handle)
    w = np.empty((desc.n_policies, size_of(kind, desc.hidden)), dtype=np.float32)
    _check(lib, getter(handle, C.byref(desc), w.ctypes.data_as(C.c_void_p), w.size))
    return w, int(desc.hidden), int(desc.lanes_per_policy)


def _view(lib, fn, handle, count_type=C.c_uint64) -> Tuple[int, int]:
    """(device address, count) of a ``gymrs_*_ptr`` call."""
    p, n = C.c_void_p(), count_type()
    _check(lib, fn(handle, C.byref(p), C.byref(n)))
    return p.value, n.value


def _record(who, n_envs, n_steps, record, unread=()) -> Trajectory:
    """The by-value record of a descriptor from ``record``, a ``Trajectory`` or a mapping as in ``rollout_closed_loop`` that may
    leave out the names the call does not read (``unread``)."""
    if record is None:
        raise ValueError(f"{who} needs a record")
    if not isinstance(record, Trajectory):
        record = dict(record)
        for name in unread:
            record.setdefault(name, 0)
    return _closed_loop_desc(n_envs, n_steps, False, False, record).record.contents


def _policy_records(lib, getter, handle, policy_handle, first, count, columns) -> np.ndarray:
    """Records of policies [first, first + count) as int64 rows (synchronising); ``count`` defaults to the rest of the set the engine
    ``policy_handle`` holds."""
    if count is None:
        count = int(_describe(lib, lib.gymrs_get_policy, policy_handle).n_policies) - int(first)
    out = np.zeros((max(int(count), 0), columns), dtype=np.int64)
    _check(lib, getter(handle, int(first), int(count), out.ctypes.data_as(C.c_void_p)))
    return out


def shard_range(n_total: int, world_size: int, rank: int) -> Tuple[int, int]:
    """Contiguous lane shard of rank ``rank``: (global offset, count).  Lanes are independent, so
    the batch shards trivially; the global id keeps Philox draws identical for any world size."""
    if not (0 <= rank < world_size):
        raise ValueError("rank out of range")
    base, rem = divmod(n_total, world_size)
    count = base + (1 if rank < rem else 0)
    offset = rank * base + min(rank, rem)
    return offset, count


class BatchedEngine:
    """One engine = one shard of lanes on one GPU, driven by one host thread."""

    def __init__(self, kind: int, n_envs: int, *, global_env_offset: int = 0, device: int = 0, params=None,
                 flags: int = 0, lanes_per_thread: Optional[int] = None):
        self._lib = load_library()
        self._h = C.c_void_p()
        self.kind = int(kind)
        self.n_envs = int(n_envs)
        self.global_env_offset = int(global_env_offset)
        self.flags = int(flags)
        self.state_dim = _STATE_DIM[self.kind]
        self.obs_dim = _OBS_DIM[self.kind]
        self.action_dtype = _ACTION_DTYPE[self.kind]
        self.params = params if params is not None else default_params(self.kind)
        _check(self._lib, self._lib.gymrs_engine_create(self.kind, self.n_envs, self.global_env_offset, int(device),
                                                        C.byref(self.params), self.flags, C.byref(self._h)))
        if lanes_per_thread is not None:
            self.set_tuning(lanes_per_thread)

    # -- lifetime ---------------------------------------------------------------------------
    def close(self) -> None:
        """``Env::close`` (core.rs:56)."""
        if getattr(self, "_h", None) is not None and self._h:
            self._lib.gymrs_engine_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- Clone + Serialize (core.rs:25) ---------------------------------------------------------
    def clone(self) -> "BatchedEngine":
        """Deep copy (``Env: Clone``): lane state, episode bookkeeping, statistics, RNG position."""
        h = C.c_void_p()
        _check(self._lib, self._lib.gymrs_engine_clone(self._h, C.byref(h)))
        other = BatchedEngine.__new__(BatchedEngine)
        other.__dict__.update({k: v for k, v in self.__dict__.items() if k != "_h"})
        other.params = type(self.params).from_buffer_copy(self.params)
        other._h = h
        return other

    def snapshot(self) -> bytes:
        """Everything a step can observe as an opaque blob (``Env: Serialize``); see ``restore``."""
        size = C.c_uint64()
        _check(self._lib, self._lib.gymrs_snapshot_size(self._h, C.byref(size)))
        buf = (C.c_char * size.value)()
        _check(self._lib, self._lib.gymrs_snapshot_save(self._h, buf, size.value))
        return bytes(buf)

    def restore(self, blob: bytes) -> None:
        """Load a ``snapshot()`` taken from an engine of the same kind, n_envs and flags; stepping then
        continues bit-identically to the engine the snapshot came from."""
        buf = (C.c_char * len(blob)).from_buffer_copy(blob)
        _check(self._lib, self._lib.gymrs_snapshot_load(self._h, buf, len(blob)))

    # -- stream / tuning ----------------------------------------------------------------------
    @property
    def stream(self) -> int:
        p = C.c_void_p()
        _check(self._lib, self._lib.gymrs_get_stream(self._h, C.byref(p)))
        return p.value or 0

    def set_stream(self, hip_stream: int) -> None:
        _check(self._lib, self._lib.gymrs_set_stream(self._h, C.c_void_p(hip_stream)))

    def set_tuning(self, lanes_per_thread: int = 4, memory_hint: int = 0) -> None:
        """lanes_per_thread: 4 or 8.  memory_hint: 0 automatic, 1 every access non-temporal, 2 none, 3 only the stores nobody reads again."""
        _check(self._lib, self._lib.gymrs_set_tuning(self._h, int(lanes_per_thread), int(memory_hint)))

    # -- the pub physics fields after construction; the Serialize view -------------------------------
    def set_params(self, params) -> None:
        """Assign the pub physics fields (cartpole.rs:53-82) of every lane: only the launch constants change --
        state, steps_beyond_terminated, episode clocks, statistics, seed and tick carry on."""
        if not isinstance(params, _PARAMS[self.kind]):
            raise TypeError(f"expected {_PARAMS[self.kind].__name__}")
        _check(self._lib, self._lib.gymrs_set_params(self._h, C.byref(params)))
        self.params = type(params).from_buffer_copy(params)

    def get_params(self):
        p = _PARAMS[self.kind]()
        _check(self._lib, self._lib.gymrs_get_params(self._h, C.byref(p)))
        return p

    # -- per-lane physics: a parameter table and a row index per lane (gymrs_set_param_table) --------
    def set_param_table(self, rows) -> None:
        """Give lane i the physics of ``rows[index[i]]`` (a sequence of this kind's params; ``None`` or ``[]`` switches the table
        off, every lane then steps with row 0).  The first table starts every index at 0.  Only the launch constants change."""
        rows = list(rows or [])
        cls = _PARAMS[self.kind]
        if any(not isinstance(r, cls) for r in rows):
            raise TypeError(f"expected {cls.__name__} rows")
        arr = (cls * len(rows))(*rows) if rows else None
        _check(self._lib, self._lib.gymrs_set_param_table(self._h, arr, len(rows)))
        self.params = self.get_params()

    def param_table(self) -> list:
        """The rows of the active table in f64 exactly as set ([] without a table)."""
        k = C.c_uint32()
        _check(self._lib, self._lib.gymrs_get_param_table(self._h, None, 0, C.byref(k)))
        if k.value == 0:
            return []
        arr = (_PARAMS[self.kind] * k.value)()
        _check(self._lib, self._lib.gymrs_get_param_table(self._h, arr, k.value, C.byref(k)))
        return list(arr)

    def param_index_ptr(self) -> int:
        """Device address of the uint16 row index of every lane (zero-copy; the engine's stream orders writes to it)."""
        return self._ptr(self._lib.gymrs_param_index_ptr)

    def set_param_index(self, index, first: int = 0) -> None:
        idx = np.ascontiguousarray(index, dtype=np.uint16)
        _check(self._lib, self._lib.gymrs_set_param_index(self._h, int(first), idx.size, idx.ctypes.data_as(C.c_void_p)))

    def get_param_index(self, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        count = self.n_envs - first if count is None else count
        out = np.empty(count, dtype=np.uint16)
        _check(self._lib, self._lib.gymrs_get_param_index(self._h, int(first), int(count), out.ctypes.data_as(C.c_void_p)))
        return out

    def lane_params(self, lane: int):
        """The params lane ``lane`` steps with: row index[lane] of the table (without one, get_params())."""
        p = _PARAMS[self.kind]()
        _check(self._lib, self._lib.gymrs_get_lane_params(self._h, int(lane), C.byref(p)))
        return p

    def env_json(self, lane: int = 0) -> str:
        """What ``serde_json::to_string(&env)`` prints for the reference env lane ``lane`` stands for (core.rs:25)."""
        need = C.c_uint64()
        buf = C.create_string_buffer(2048)
        st = self._lib.gymrs_env_json(self._h, int(lane), buf, len(buf), C.byref(need))
        if st != _OK and need.value > len(buf):
            buf = C.create_string_buffer(need.value)
            st = self._lib.gymrs_env_json(self._h, int(lane), buf, len(buf), C.byref(need))
        _check(self._lib, st)
        return buf.value.decode("utf-8")

    # -- Env::reset ------------------------------------------------------------------------------
    def reset(self, seed: Optional[int] = None, options: Optional[Sequence[float]] = None) -> int:
        """``reset(seed, _, options)`` for every lane.  ``options`` = state_dim lows then state_dim
        highs.  Returns the seed number used (seeding.rs:21-26)."""
        bounds = None
        if options is not None:
            arr = np.ascontiguousarray(options, dtype=np.float32)
            if arr.size != 2 * self.state_dim:
                raise ValueError(f"options needs {2 * self.state_dim} floats (lows then highs)")
            bounds = arr.ctypes.data_as(C.POINTER(C.c_float))
        used = C.c_uint64()
        _check(self._lib, self._lib.gymrs_reset(self._h, 0 if seed is None else 1, 0 if seed is None else int(seed),
                                                bounds, C.byref(used)))
        return used.value

    def reset_pcg64(self, seed: Optional[int] = None, seeds_dev: Optional[int] = None,
                    options: Optional[Sequence[float]] = None) -> int:
        """``reset`` with the reference's own generator chain (``gymrs_reset_pcg64``): lane i gets, rounded once to f32,
        the state the reference's ``reset(Some(s), _, options)`` returns for ``s = seed + global_env_offset + i`` or, if
        ``seeds_dev`` (device address of n_envs u64) is given, ``s = seeds[i]``.  ``options`` = lows then highs, f64.
        CartPole / MountainCar only.  Returns the seed number used."""
        bounds = None
        if options is not None:
            arr = np.ascontiguousarray(options, dtype=np.float64)
            if arr.size != 2 * self.state_dim:
                raise ValueError(f"options needs {2 * self.state_dim} floats (lows then highs)")
            bounds = arr.ctypes.data_as(C.POINTER(C.c_double))
        used = C.c_uint64()
        _check(self._lib, self._lib.gymrs_reset_pcg64(self._h, 0 if seed is None else 1, 0 if seed is None else int(seed) & ((1 << 64) - 1),
                                                      C.c_void_p(seeds_dev) if seeds_dev else None, bounds, C.byref(used)))
        return used.value

    # -- Env::step ---------------------------------------------------------------------------------
    def step(self, actions_dev: int) -> None:
        """Asynchronous; ``actions_dev`` is a device address of n_envs actions."""
        _check(self._lib, self._lib.gymrs_step(self._h, C.c_void_p(actions_dev)))

    def step_host(self, actions) -> None:
        a = np.ascontiguousarray(actions, dtype=self.action_dtype)
        if a.size != self.n_envs:
            raise ValueError("one action per lane expected")
        _check(self._lib, self._lib.gymrs_step_host(self._h, a.ctypes.data_as(C.c_void_p)))
        self.sync()  # the host buffer must outlive the copy

    def step_many(self, actions_dev: int, stride_bytes: int, n_buffers: int, n_steps: int, use_graph: bool = False) -> None:
        _check(self._lib, self._lib.gymrs_step_many(self._h, C.c_void_p(actions_dev), int(stride_bytes), int(n_buffers),
                                                    int(n_steps), 1 if use_graph else 0))

    def sync(self) -> None:
        _check(self._lib, self._lib.gymrs_sync(self._h))

    # -- device views -----------------------------------------------------------------------------
    def obs_ptrs(self):
        ptrs = (C.c_void_p * 4)()
        dim = C.c_int()
        _check(self._lib, self._lib.gymrs_obs_ptrs(self._h, ptrs, C.byref(dim)))
        return [ptrs[j] for j in range(dim.value)]

    def final_obs_ptrs(self):
        """FINAL_OBS engines: device views of the observation each lane's last finished episode ended in (gymrs_final_obs_ptrs)."""
        ptrs = (C.c_void_p * 4)()
        dim = C.c_int()
        _check(self._lib, self._lib.gymrs_final_obs_ptrs(self._h, ptrs, C.byref(dim)))
        return [ptrs[j] for j in range(dim.value)]

    def state_ptrs(self):
        ptrs = (C.c_void_p * 4)()
        dim = C.c_int()
        _check(self._lib, self._lib.gymrs_state_ptrs(self._h, ptrs, C.byref(dim)))
        return [ptrs[j] for j in range(dim.value)]

    def _ptr(self, fn) -> int:
        p = C.c_void_p()
        _check(self._lib, fn(self._h, C.byref(p)))
        return p.value or 0

    @property
    def reward_ptr(self) -> int:
        return self._ptr(self._lib.gymrs_reward_ptr)

    @property
    def done_ptr(self) -> int:
        return self._ptr(self._lib.gymrs_done_ptr)

    @property
    def truncated_ptr(self) -> int:
        return self._ptr(self._lib.gymrs_truncated_ptr)

    # -- host copies ---------------------------------------------------------------------------------
    def get_obs(self, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        count = self.n_envs - first if count is None else count
        out = np.empty((self.obs_dim, count), dtype=np.float32)
        _check(self._lib, self._lib.gymrs_get_obs(self._h, first, count, out.ctypes.data_as(C.c_void_p)))
        return out

    def get_final_obs(self, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        """FINAL_OBS engines: host copy of the final observations, shape (obs_dim, count) like get_obs."""
        count = self.n_envs - first if count is None else count
        out = np.empty((self.obs_dim, count), dtype=np.float32)
        _check(self._lib, self._lib.gymrs_get_final_obs(self._h, first, count, out.ctypes.data_as(C.c_void_p)))
        return out

    def get_state(self, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        count = self.n_envs - first if count is None else count
        out = np.empty((self.state_dim, count), dtype=np.float32)
        _check(self._lib, self._lib.gymrs_get_state(self._h, first, count, out.ctypes.data_as(C.c_void_p)))
        return out

    def set_state(self, state, first: int = 0) -> None:
        arr = np.ascontiguousarray(state, dtype=np.float32)
        if arr.ndim != 2 or arr.shape[0] != self.state_dim:
            raise ValueError(f"state must have shape ({self.state_dim}, count)")
        _check(self._lib, self._lib.gymrs_set_state(self._h, first, arr.shape[1], arr.ctypes.data_as(C.c_void_p)))

    def get_step_result(self, first: int = 0, count: Optional[int] = None):
        count = self.n_envs - first if count is None else count
        reward = np.empty(count, dtype=np.float32)
        done = np.empty(count, dtype=np.uint8)
        trunc = np.empty(count, dtype=np.uint8)
        _check(self._lib, self._lib.gymrs_get_step_result(self._h, first, count, reward.ctypes.data_as(C.c_void_p),
                                                          done.ctypes.data_as(C.c_void_p), trunc.ctypes.data_as(C.c_void_p)))
        return reward, done, trunc

    # -- statistics ----------------------------------------------------------------------------------
    def stats(self) -> np.ndarray:
        """{sum_return, sum_length, n_episodes, n_steps} of this shard."""
        out = (C.c_double * 4)()
        _check(self._lib, self._lib.gymrs_stats(self._h, out))
        return np.array(out[:], dtype=np.float64)

    def stats_clear(self) -> None:
        _check(self._lib, self._lib.gymrs_stats_clear(self._h))

    def stats_device(self) -> int:
        """Device address of 4 doubles, valid after the engine stream reaches this point."""
        p = C.c_void_p()
        _check(self._lib, self._lib.gymrs_stats_device(self._h, C.byref(p)))
        return p.value or 0

    # RCCL, one process per GPU
    def comm_unique_id(self) -> bytes:
        buf = (C.c_uint8 * 128)()
        _check(self._lib, self._lib.gymrs_comm_unique_id(buf))
        return bytes(buf)

    def comm_init(self, n_ranks: int, rank: int, unique_id: bytes) -> None:
        buf = (C.c_uint8 * 128).from_buffer_copy(unique_id)
        _check(self._lib, self._lib.gymrs_comm_init(self._h, n_ranks, rank, buf))

    def allreduce_stats(self) -> np.ndarray:
        out = (C.c_double * 4)()
        _check(self._lib, self._lib.gymrs_allreduce_stats(self._h, out))
        return np.array(out[:], dtype=np.float64)

    # -- utilities -----------------------------------------------------------------------------------
    def rollout(self, n_steps: int, action_seed: int, action_t0: int = 0) -> None:
        """``n_steps`` random-policy steps of every lane in one kernel launch: the effect of
        ``fill_actions(buf, action_seed, action_t0 + k); step(buf)`` for k in range(n_steps), bit for bit
        (the caller loop of examples/cartpole.rs:15-30)."""
        _check(self._lib, self._lib.gymrs_rollout(self._h, int(n_steps), int(action_seed), int(action_t0)))

    def rollout_record(self, n_steps: int, action_seed: int, action_t0: int, *, obs: int, actions: int, reward: int,
                       done: int, truncated: int = 0, lane_stride: Optional[int] = None) -> None:
        """``rollout`` that also keeps the trajectory.  The arguments are device addresses of buffers laid out
        ``obs[n_steps][obs_dim][lane_stride]`` (f32), ``actions/reward/done/truncated[n_steps][lane_stride]``;
        ``lane_stride`` defaults to n_envs rounded up to a multiple of 16."""
        stride = int(lane_stride) if lane_stride is not None else (self.n_envs + 15) // 16 * 16
        traj = Trajectory(C.c_void_p(obs), C.c_void_p(actions), C.c_void_p(reward), C.c_void_p(done),
                          C.c_void_p(truncated or None), stride)
        _check(self._lib, self._lib.gymrs_rollout_record(self._h, int(n_steps), int(action_seed), int(action_t0), C.byref(traj)))

    def fill_actions(self, actions_dev: int, seed: int, t: int) -> None:
        _check(self._lib, self._lib.gymrs_fill_actions(self._h, C.c_void_p(actions_dev), int(seed), int(t)))

    # -- closed-loop rollouts: a small policy evaluated inside the kernel (gymrs_set_policy) -----------
    def set_policy(self, weights, hidden: int = 0, lanes_per_policy: int = 1) -> None:
        """Install a policy set: ``weights`` is an array of shape (n_policies, policy_size(kind, hidden)) (or one flat policy),
        f32, laid out as include/gymrs_amd.h says; lane i uses policy ((global_env_offset + i) // lanes_per_policy) % n_policies.
        ``None`` removes the policy.  Touches no lane state, tick or statistics."""
        _set_weights(self._lib, self._lib.gymrs_set_policy, self._h, self.kind, weights, hidden, lanes_per_policy, policy_size, "policies")

    def get_policy(self):
        """(weights of shape (n_policies, policy_size), hidden, lanes_per_policy) as set (synchronising)."""
        return _get_weights(self._lib, self._lib.gymrs_get_policy, self._h, self.kind, policy_size)

    def policy_weights_ptr(self) -> Tuple[int, int]:
        """(device address, number of floats) of the policy set: zero-copy; a kernel on the engine's stream may rewrite the
        weights between two launches.  Valid until the next set_policy or close."""
        return _view(self._lib, self._lib.gymrs_policy_weights_ptr, self._h)

    def policy_actions(self, actions_dev: int) -> None:
        """Write the policy's uint8 action for every lane's current observation to ``actions_dev`` (one launch)."""
        _check(self._lib, self._lib.gymrs_policy_actions(self._h, C.c_void_p(actions_dev)))

    def rollout_policy(self, n_steps: int) -> None:
        """``n_steps`` closed-loop steps of every lane in one kernel launch: the effect of ``policy_actions(buf); step(buf)``
        n_steps times, bit for bit."""
        _check(self._lib, self._lib.gymrs_rollout_policy(self._h, int(n_steps)))

    def rollout_policy_record(self, n_steps: int, *, obs: int, actions: int, reward: int, done: int, truncated: int = 0,
                              lane_stride: Optional[int] = None) -> None:
        """``rollout_policy`` that also keeps the trajectory; buffers as for ``rollout_record`` (``actions`` = the policy's)."""
        stride = int(lane_stride) if lane_stride is not None else (self.n_envs + 15) // 16 * 16
        traj = Trajectory(C.c_void_p(obs), C.c_void_p(actions), C.c_void_p(reward), C.c_void_p(done),
                          C.c_void_p(truncated or None), stride)
        _check(self._lib, self._lib.gymrs_rollout_policy_record(self._h, int(n_steps), C.byref(traj)))

    # -- per-policy fitness: counters accumulated inside the closed-loop rollout kernel ------------------
    def rollout_policy_fitness(self, n_steps: int) -> None:
        """``rollout_policy`` that also adds every step's reward / done / truncated to the record of the lane's policy
        (``policy_fitness``).  Leaves the engine bit for bit as ``rollout_policy`` does."""
        _check(self._lib, self._lib.gymrs_rollout_policy_fitness(self._h, int(n_steps)))

    # -- the closed-loop calls behind one descriptor, and under per-lane physics ---------------------------
    def rollout_closed_loop(self, n_steps: int, *, lane_params: bool = False, fitness: bool = False, record=None,
                            flags: Optional[int] = None, explore: bool = False, sample: bool = False) -> None:
        """``gymrs_rollout_closed_loop``: ``rollout_policy`` (with ``record``: ``rollout_policy_record``; with ``fitness``:
        ``rollout_policy_fitness``) behind one descriptor.  ``lane_params`` (``GYMRS_CLOSED_LOOP_LANE_PARAMS``) lets it run while a
        parameter table is active: every lane steps with the row ``step`` would use for it, n_steps steps in one launch; without a
        table it changes nothing, so a training loop may always set it.  ``record``: a ``Trajectory`` or a mapping with the keyword
        arguments of ``rollout_policy_record``.  ``explore`` (``GYMRS_CLOSED_LOOP_EXPLORE``) plays the epsilon-greedy action of
        ``set_exploration`` in place of the argmax, ``sample`` (``GYMRS_CLOSED_LOOP_SAMPLE``) an action drawn from the softmax of the
        logits under ``set_sampling``; not both.  ``flags`` passes a raw flags word instead of the booleans."""
        desc = _closed_loop_desc(self.n_envs, n_steps, lane_params, fitness, record, flags, explore, sample)
        _check(self._lib, self._lib.gymrs_rollout_closed_loop(self._h, C.byref(desc)))

    def rollout_transitions(self, n_steps: int, *, record, final_obs: int, start_obs: Optional[int] = None, lane_params: bool = False,
                            explore: bool = False, flags: Optional[int] = None, sample: bool = False) -> None:
        """``gymrs_rollout_transitions``: ``rollout_closed_loop(n_steps, record=record, ...)`` that also writes, per step, the
        observation every ended lane showed before its re-arm into ``final_obs`` ([n_steps][D][lane_stride] f32, device address;
        only the elements of ended lane-steps are written) and, if given, the observations the launch starts from into
        ``start_obs`` ([D][lane_stride]).  The successor of step k is ``where(done[k] | truncated[k], final_obs[k], obs[k])``.
        Engines with ``AUTO_RESET`` only.  ``record``: a ``Trajectory`` or a mapping as in ``rollout_closed_loop`` (required)."""
        if record is None:
            raise ValueError("rollout_transitions needs a record")
        cl = _closed_loop_desc(self.n_envs, n_steps, lane_params, False, record, flags, explore, sample)
        desc = TransitionsDesc(int(n_steps), cl.flags, cl.record.contents, C.c_void_p(final_obs or None), C.c_void_p(start_obs or None), 0)
        _check(self._lib, self._lib.gymrs_rollout_transitions(self._h, C.byref(desc)))

    # -- advantages over a transitions record: a critic evaluated inside the kernel, the GAE scan in one launch ------
    def set_critic(self, weights, hidden: int = 0, lanes_per_critic: int = 1) -> None:
        """Install a critic set: ``weights`` is an array of shape (n_critics, critic_size(kind, hidden)) (or one flat critic),
        f32; lane i uses critic ((global_env_offset + i) // lanes_per_critic) % n_critics.  ``None`` removes the critic.  Touches
        no lane state, tick or statistics, and survives ``set_policy``."""
        _set_weights(self._lib, self._lib.gymrs_set_critic, self._h, self.kind, weights, hidden, lanes_per_critic, critic_size, "critics")

    def critic(self):
        """(weights of shape (n_critics, critic_size), hidden, lanes_per_critic) as set (synchronising)."""
        return _get_weights(self._lib, self._lib.gymrs_get_critic, self._h, self.kind, critic_size)

    def critic_weights_ptr(self) -> Tuple[int, int]:
        """(device address, number of floats) of the critic set: zero-copy; a kernel on the engine's stream may rewrite the
        weights between two launches.  Valid until the next set_critic or close."""
        return _view(self._lib, self._lib.gymrs_critic_weights_ptr, self._h)

    def advantages(self, n_steps: int, *, record, start_obs: int, advantages: int, final_obs: Optional[int] = None,
                   returns: Optional[int] = None, values: Optional[int] = None, gamma: float, lam: float, critic: bool = False,
                   flags: Optional[int] = None) -> None:
        """``gymrs_advantages``: GAE(lambda) advantages ([n_steps][lane_stride] f32, device address), optionally returns and
        values, from the rows ``rollout_transitions`` wrote, in one launch on the engine's stream (no sync needed in between).
        ``critic`` (``GYMRS_ADVANTAGES_CRITIC``) evaluates the critic set of ``set_critic`` inside the kernel; without it V = 0 and
        ``gamma = lam = 1`` gives the reward-to-go.  ``final_obs=None`` is for records of engines without auto-reset.  ``record``: a
        ``Trajectory`` or a mapping as in ``rollout_closed_loop`` (its ``actions`` is not read).  Reads and writes no lane array."""
        traj = _record("advantages", self.n_envs, n_steps, record, unread=("actions",))
        f = (ADVANTAGES_CRITIC if critic else 0) if flags is None else int(flags)
        desc = AdvantagesDesc(int(n_steps), f, float(gamma), float(lam), traj, C.c_void_p(final_obs or None), C.c_void_p(start_obs or None),
                              C.c_void_p(advantages or None), C.c_void_p(returns or None), C.c_void_p(values or None), 0)
        _check(self._lib, self._lib.gymrs_advantages(self._h, C.byref(desc)))

    # -- gradients over a transitions record: exact fixed-point sums per set, one launch per head -----------------
    def policy_gradient(self, n_steps: int, *, record, start_obs: int, coef: int, grad: int, excluded: int, prob: Optional[int] = None,
                        critic: bool = False, temperature: Optional[float] = None, scale: Optional[float] = None,
                        flags: Optional[int] = None) -> None:
        """``gymrs_policy_gradient``: ADDS sum over (k, i) of coef[k][i] * grad log pi(a[k][i] | x[k][i]) per policy, as int64 fixed
        point (the gradient is ``grad`` * 2**-24), to ``grad`` (device int64 [n_policies][policy_size]) and the number of (lane,
        parameter) pairs left out to ``excluded`` (device uint64 [n_policies]), in one launch on the engine's stream (no sync needed
        after ``advantages``).  ``critic`` (``GYMRS_GRADIENT_CRITIC``): sum coef * grad V(x) of the critic set instead, tables
        [n_critics][critic_size]; ``temperature`` / ``scale`` are for the policy head only (exactly one of them), ``prob`` (device
        f32 [n_steps][lane_stride]) receives p[a].  ``record``: a ``Trajectory`` or a mapping as in ``rollout_closed_loop`` (only
        ``obs`` and, for the policy head, ``actions`` are read).  The caller zeroes the tables.  Reads and writes no lane array."""
        traj = _record("policy_gradient", self.n_envs, n_steps, record, unread=("actions", "reward", "done"))
        f = (GRADIENT_CRITIC if critic else 0) if flags is None else int(flags)
        s = 0.0
        if not (f & GRADIENT_CRITIC):
            s = _sampling(0, temperature, scale).scale
        desc = GradientDesc(int(n_steps), f, float(s), 0, traj, C.c_void_p(start_obs or None), C.c_void_p(coef or None), C.c_void_p(prob or None),
                            C.c_void_p(grad or None), C.c_void_p(excluded or None), 0)
        _check(self._lib, self._lib.gymrs_policy_gradient(self._h, C.byref(desc)))

    # -- the clipped surrogate over a transitions record: one launch per PPO epoch --------------------------------
    def ppo_gradient(self, n_steps: int, *, record, start_obs: int, advantages: int, old_prob: int, grad: int, excluded: int,
                     counts: Optional[int] = None, prob: Optional[int] = None, clip: Optional[float] = 0.2, clip_low: Optional[float] = None,
                     clip_high: Optional[float] = None, temperature: Optional[float] = None, scale: Optional[float] = None,
                     flags: int = 0) -> None:
        """``gymrs_ppo_gradient``: ``policy_gradient`` with the policy head whose coefficient is computed in the kernel from the
        ``advantages`` row and the ``old_prob`` row (the ``prob`` row of the policy the record was drawn from): ratio = p[a] /
        old_prob, cut where the advantage pushes it out of [clip_low, clip_high], else advantage * ratio.  ADDS the gradient of PPO's
        clipped objective (to ascend) per policy to ``grad`` and ``excluded`` as ``policy_gradient`` does, and, with ``counts`` (device
        uint64 [n_policies][2]), the lane-steps seen and the lane-steps cut.  ``clip`` (epsilon) becomes ``np.float32(1 - clip)`` and
        ``np.float32(1 + clip)``; ``clip_low`` / ``clip_high`` give the bounds themselves.  ``prob`` receives the new p[a] and may
        not be ``old_prob``.  Exactly one of ``temperature`` / ``scale``.  Reads and writes no lane array."""
        traj = _record("ppo_gradient", self.n_envs, n_steps, record, unread=("actions", "reward", "done"))
        low, high = _clip_bounds(clip, clip_low, clip_high)
        s = _sampling(0, temperature, scale).scale
        desc = PpoDesc(int(n_steps), int(flags), float(s), low, high, 0, traj, C.c_void_p(start_obs or None), C.c_void_p(advantages or None),
                       C.c_void_p(old_prob or None), C.c_void_p(prob or None), C.c_void_p(grad or None), C.c_void_p(excluded or None),
                       C.c_void_p(counts or None), 0)
        _check(self._lib, self._lib.gymrs_ppo_gradient(self._h, C.byref(desc)))

    # -- V-trace targets and policy-gradient advantages over a transitions record: both networks and the scan in one launch ---------
    def vtrace(self, n_steps: int, *, record, start_obs: int, old_prob: int, vs: int, pg_advantages: int, final_obs: Optional[int] = None,
               values: Optional[int] = None, prob: Optional[int] = None, counts: Optional[int] = None, gamma: float, lam: float = 1.0,
               rho_bar: float = 1.0, c_bar: float = 1.0, pg_rho_bar: float = 1.0, temperature: Optional[float] = None,
               scale: Optional[float] = None, flags: int = 0) -> None:
        """``gymrs_vtrace``: the off-policy corrected counterpart of ``advantages``.  From the record, the ``old_prob`` row (the ``prob``
        row of the policy the record was drawn from), the CURRENT policy set and the critic set it writes ``vs`` (the ``returns`` row of
        ``value_gradient``) and ``pg_advantages`` (the ``coef`` / ``advantages`` row of ``policy_gradient`` / ``ppo_gradient``), and
        optionally ``values`` (V under the current critic), ``prob`` (the current p[a]; not ``old_prob``) and, ADDED to, ``counts``
        (device uint64 [n_policies][3]: lane-steps seen, with ratio > rho_bar, with ratio > c_bar).  One launch on the engine's stream:
        no sync is needed behind ``apply_gradient``.  A bar of ``inf`` does not clip.  Exactly one of ``temperature`` / ``scale``.
        Reads and writes no lane array."""
        traj = _record("vtrace", self.n_envs, n_steps, record)
        s = _sampling(0, temperature, scale).scale
        desc = VtraceDesc(int(n_steps), int(flags), float(gamma), float(lam), float(s), float(rho_bar), float(c_bar), float(pg_rho_bar), traj,
                          C.c_void_p(final_obs or None), C.c_void_p(start_obs or None), C.c_void_p(old_prob or None), C.c_void_p(vs or None),
                          C.c_void_p(pg_advantages or None), C.c_void_p(values or None), C.c_void_p(prob or None), C.c_void_p(counts or None), 0)
        _check(self._lib, self._lib.gymrs_vtrace(self._h, C.byref(desc)))

    # -- the entropy bonus and the KL estimate over a transitions record: one launch beside ppo_gradient ----------------
    def entropy_gradient(self, n_steps: int, *, record, start_obs: int, grad: int, excluded: int, sums: int, coef: float,
                         old_prob: Optional[int] = None, counts: Optional[int] = None, temperature: Optional[float] = None,
                         scale: Optional[float] = None, flags: int = 0) -> None:
        """``gymrs_entropy_gradient``: ADDS the gradient of ``coef`` * (the entropy of the policy at every lane-step, in nats) per
        policy to ``grad`` and ``excluded`` in the layout of ``ppo_gradient`` (one ``apply_gradient(ascend=True)`` consumes the sum of
        both), the fixed point (* 2**-24) of the entropy sum and, with ``old_prob`` (the row ``ppo_gradient`` reads), of the k3
        estimate of KL(recorded || current) to ``sums`` (device int64 [n_policies][2]) and, with ``counts`` (device uint64
        [n_policies][2]), the lane-steps in each sum.  ``record``: only ``obs`` is read, and ``actions`` with ``old_prob``.  Exactly
        one of ``temperature`` / ``scale``.  Reads and writes no lane array."""
        traj = _record("entropy_gradient", self.n_envs, n_steps, record, unread=("actions", "reward", "done"))
        s = _sampling(0, temperature, scale).scale
        desc = EntropyDesc(int(n_steps), int(flags), float(s), float(coef), traj, C.c_void_p(start_obs or None), C.c_void_p(old_prob or None),
                           C.c_void_p(grad or None), C.c_void_p(excluded or None), C.c_void_p(sums or None), C.c_void_p(counts or None), 0)
        _check(self._lib, self._lib.gymrs_entropy_gradient(self._h, C.byref(desc)))

    # -- the value loss over a transitions record: the critic head with its coefficient computed in the kernel -----------
    def value_gradient(self, n_steps: int, *, record, start_obs: int, returns: int, grad: int, excluded: int, old_values: Optional[int] = None,
                       clip: Optional[float] = None, values: Optional[int] = None, sums: Optional[int] = None, counts: Optional[int] = None,
                       flags: Optional[int] = None) -> None:
        """``gymrs_value_gradient``: ``policy_gradient(critic=True)`` whose coefficient is computed in the kernel: V(x) - returns, or
        with ``clip`` (then ``old_values`` is required: GYMRS_VALUE_CLIP) the gradient of 0.5 * max((V - R)^2, (V_clip - R)^2).  ADDS
        the gradient of the loss (to descend) per critic to ``grad`` and ``excluded``; ``values`` receives V under the current
        critic; ``sums`` (device int64 [n_sets][2]) the fixed points of the squared errors, ``counts`` (device uint64 [n_sets][2]) the
        lane-steps seen and cut.  ``record``: only ``obs`` is read.  Reads and writes no lane array.  With a hidden critic and no
        ``values`` the engine keeps a scratch row; the call that allocates or grows it synchronises the engine's stream."""
        traj = _record("value_gradient", self.n_envs, n_steps, record, unread=("actions", "reward", "done"))
        f = (VALUE_CLIP if clip is not None else 0) if flags is None else int(flags)
        desc = ValueDesc(int(n_steps), f, float(clip or 0.0), 0, traj, C.c_void_p(start_obs or None), C.c_void_p(returns or None),
                         C.c_void_p(old_values or None), C.c_void_p(values or None), C.c_void_p(grad or None), C.c_void_p(excluded or None),
                         C.c_void_p(sums or None), C.c_void_p(counts or None), 0)
        _check(self._lib, self._lib.gymrs_value_gradient(self._h, C.byref(desc)))

    # -- per-set standardisation of an advantages row, exact and order-independent -----------------------------------
    def normalize_advantages(self, n_steps: int, *, adv: int, out: int, stats: int, lane_stride: int, lanes_per_policy: int = 1, n_sets: int = 1,
                             eps: float = 1e-6, flags: int = 0) -> None:
        """``gymrs_normalize_advantages``: ``out[k][i] = (adv[k][i] - mean) / (sd + eps)`` with mean and sd (n - 1) per set from integer
        sums, the set of lane i being ``((global_env_offset + i) // lanes_per_policy) % n_sets``.  ``stats``: device memory of
        ``n_sets`` records of ``ADVANTAGE_STATS_DTYPE`` (40 bytes each), written.  ``out`` may be ``adv``.  Works for every env kind.
        The statistics are over this engine's lanes: engines that cut one batch each standardise their own part."""
        desc = NormalizeDesc(int(n_steps), int(flags), float(eps), int(n_sets), int(lanes_per_policy), int(lane_stride), C.c_void_p(adv or None),
                             C.c_void_p(out or None), C.c_void_p(stats or None), 0)
        _check(self._lib, self._lib.gymrs_normalize_advantages(self._h, C.byref(desc)))

    # -- Q-learning over a transitions record: a target set, TD errors and the Q-gradient in one call -------------------
    def q_target_sync(self) -> None:
        """``gymrs_q_target_sync``: copy the current policy set into the engine-owned target set (device to device, in stream order).
        A ``set_policy`` of the same shape keeps the target; any other, or the policy's removal, discards it."""
        _check(self._lib, self._lib.gymrs_q_target_sync(self._h))

    def q_target_ptr(self) -> Tuple[int, int]:
        """(device address, number of floats) of the target set: zero-copy, for a Polyak average on the engine's stream.  Valid until
        the target is discarded or the engine closed."""
        return _view(self._lib, self._lib.gymrs_q_target_ptr, self._h)

    def q_gradient(self, n_steps: int, *, record, start_obs: int, final_obs: int, td: int, grad: int, excluded: int, counts: Optional[int] = None,
                   gamma: float, kappa: float = float("inf"), double: bool = False, flags: Optional[int] = None) -> None:
        """``gymrs_q_gradient``: the policy's logits are Q-values.  Writes the TD error delta = Q(x, a) - (r + gamma * Q_target(x', b*))
        of every lane-step to ``td`` (device f32 [n_steps][lane_stride]) and ADDS the gradient of sum huber_kappa(delta) -- the loss to
        descend -- per policy to ``grad`` / ``excluded`` as ``policy_gradient`` does, and, with ``counts`` (device uint64
        [n_policies][2]), the lane-steps seen and those with |delta| > kappa.  The successor x' is ``final_obs`` where the step ended an
        episode; a done step bootstraps from 0, a truncated one from its final observation.  ``double`` (``GYMRS_Q_DOUBLE``) chooses b*
        with the online set.  Needs ``q_target_sync`` first.  Two kernels on the engine's stream; reads and writes no lane array."""
        traj = _record("q_gradient", self.n_envs, n_steps, record)
        f = (Q_DOUBLE if double else 0) if flags is None else int(flags)
        desc = QDesc(int(n_steps), f, float(gamma), float(kappa), traj, C.c_void_p(start_obs or None), C.c_void_p(final_obs or None),
                     C.c_void_p(td or None), C.c_void_p(grad or None), C.c_void_p(excluded or None), C.c_void_p(counts or None), 0)
        _check(self._lib, self._lib.gymrs_q_gradient(self._h, C.byref(desc)))

    # -- prioritized replay: a store in caller-owned device memory, filled, drawn from and re-prioritised on the engine's stream -----
    def replay_push(self, store: Replay, n_steps: int, *, record, start_obs: int, final_obs: int, priority: int = REPLAY_MAX_PRIORITY,
                    head: Optional[int] = None, flags: int = 0) -> None:
        """``gymrs_replay_push``: flatten a transitions record (``rollout_transitions``) into the ring at ``store.head`` (or ``head``),
        entry (head + k * n_envs + i) % capacity for step k and lane i, every one with ``priority``.  A truncated step is stored with
        done = 0 and its final observation as successor.  Afterwards ``store.head`` and ``store.count`` are advanced."""
        traj = _record("replay_push", self.n_envs, n_steps, record)
        at = store.head if head is None else int(head)
        desc = ReplayPushDesc(int(n_steps), int(flags), traj, C.c_void_p(start_obs or None), C.c_void_p(final_obs or None), store, at,
                              int(priority), 0, 0)
        _check(self._lib, self._lib.gymrs_replay_push(self._h, C.byref(desc)))
        pushed = int(n_steps) * self.n_envs
        store.head = (at + pushed) % store.capacity
        store.count = min(store.capacity, store.count + pushed)

    def replay_sample(self, store: Replay, n_samples: int, *, seed: int, draw: int, batch, start_obs: int, idx: int, total: int,
                      prio: Optional[int] = None, count: Optional[int] = None, flags: int = 0) -> None:
        """``gymrs_replay_sample``: draw ``n_samples`` entries of [0, ``store.count``) in proportion to their priorities (stratified; a
        pure function of the priorities, ``seed`` and ``draw``) and gather them into lane j of ``batch`` (``obs`` = the successor,
        ``actions``, ``reward``, ``done``) and ``start_obs``: what ``q_gradient`` reads with n_steps = 1, final_obs = batch obs.
        ``idx`` (uint32 [n_samples]), ``total`` (one uint64) and optionally ``prio`` (uint32 [n_samples]) are device addresses."""
        traj = _record("replay_sample", int(n_samples), 1, batch)
        desc = ReplaySampleDesc(store, store.count if count is None else int(count), int(n_samples), int(flags), int(seed) & (2**64 - 1),
                                int(draw) & (2**64 - 1), traj, C.c_void_p(start_obs or None), C.c_void_p(idx or None), C.c_void_p(prio or None),
                                C.c_void_p(total or None), 0)
        _check(self._lib, self._lib.gymrs_replay_sample(self._h, C.byref(desc)))

    def replay_update(self, store: Replay, n_samples: int, *, idx: int, td: int, alpha: float, eps: float, cap: float, flags: int = 0) -> None:
        """``gymrs_replay_update``: priority[idx[j]] = ``replay_priority(td[j])`` for j < n_samples, from the ``idx`` row of
        ``replay_sample`` and the ``td`` row of ``q_gradient``; an index >= capacity is skipped."""
        desc = ReplayUpdateDesc(store, C.c_void_p(idx or None), C.c_void_p(td or None), int(n_samples), int(flags), float(alpha), float(eps),
                                float(cap), 0.0, 0)
        _check(self._lib, self._lib.gymrs_replay_update(self._h, C.byref(desc)))

    # -- the optimizer: SGD or Adam per set, from a gradient table into the engine's own weights, in one launch --------------
    def apply_gradient(self, *, grad: int, excluded: int, lr: float, grad_scale: float, critic: bool = False, adam: bool = False,
                       beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8, max_norm: float = float("inf"), tau: float = 0.0,
                       ascend: bool = False, zero_grad: bool = False, skipped: Optional[int] = None, head: Optional[int] = None,
                       kind: Optional[int] = None, flags: Optional[int] = None) -> None:
        """``gymrs_apply_gradient``: w -= step (``ascend``: +=) for every set of the policy head (``critic``: the critic head), step =
        lr * g (``adam``: Adam's, with engine-owned moments) and g = ``grad`` * ``grad_scale`` after an optional clip of each set's
        norm to ``max_norm``.  ``grad`` (device int64 [n_sets][S]) and ``excluded`` (device uint64 [n_sets]) are the tables the
        gradient calls added to; a set with ``excluded`` != 0 is skipped and counted in ``skipped`` (one device uint64, added to).
        ``zero_grad`` zeroes both tables after reading them, so the next gradient launch needs no memset.  ``tau`` > 0 also moves the
        Q target towards the new weights (policy head, after ``q_target_sync``).  One launch on the engine's stream, no
        synchronisation; defined to the bit (include/gymrs_amd.h, "Optimizer")."""
        desc = _optimizer_desc((OPT_HEAD_CRITIC if critic else OPT_HEAD_POLICY) if head is None else head,
                               (OPT_ADAM if adam else OPT_SGD) if kind is None else kind, lr, grad_scale, beta1, beta2, eps, max_norm, tau,
                               ascend, zero_grad, flags, grad, excluded, skipped)
        _check(self._lib, self._lib.gymrs_apply_gradient(self._h, C.byref(desc)))

    def optimizer_reset(self, critic: bool = False) -> None:
        """``gymrs_optimizer_reset``: the head's Adam state back to fresh (m = v = 0, pw = 1) in stream order."""
        _check(self._lib, self._lib.gymrs_optimizer_reset(self._h, OPT_HEAD_CRITIC if critic else OPT_HEAD_POLICY))

    def optimizer_state(self, critic: bool = False):
        """(m [n_sets][S], v [n_sets][S], pw [n_sets][2]) of the head's Adam state, f32 (synchronising).  Raises before the first Adam
        call on the head."""
        w, _, _ = self.critic() if critic else self.get_policy()
        m, v, pw = np.empty_like(w), np.empty_like(w), np.empty((w.shape[0], 2), np.float32)
        fp = C.POINTER(C.c_float)
        _check(self._lib, self._lib.gymrs_get_optimizer_state(self._h, OPT_HEAD_CRITIC if critic else OPT_HEAD_POLICY, m.ctypes.data_as(fp),
                                                              v.ctypes.data_as(fp), pw.ctypes.data_as(fp)))
        return m, v, pw

    # -- evolution strategies: the centre, the population and the update stay on the device --------------------------------
    def es_init(self, centre, *, n_policies: int, sigma: float, seed: int = 0, hidden: int = 0, lanes_per_policy: int = 1,
                reserved: int = 0) -> None:
        """``gymrs_es_init``: install a population of ``n_policies`` (even) policies around ``centre`` (``policy_size`` floats) as
        the engine's policy set -- written by a kernel from the noise keyed by ``seed`` -- with a fresh Adam state and generation 0.
        Every policy call then works on that set; a generation is ``evaluate_policy`` followed by ``es_step``."""
        c = np.ascontiguousarray(centre, dtype=np.float32).reshape(-1)
        if 0 <= int(hidden) <= 64 and self.kind != PENDULUM and c.size != policy_size(self.kind, hidden):  # (the library words the other refusals)
            raise ValueError(f"es_init needs a centre of {policy_size(self.kind, hidden)} floats")
        desc = EsDesc(int(hidden), int(n_policies), int(lanes_per_policy), int(seed) & (2**64 - 1), float(sigma), int(reserved))
        _check(self._lib, self._lib.gymrs_es_init(self._h, C.byref(desc), c.ctypes.data_as(C.POINTER(C.c_float))))

    def es_step(self, *, lr: float, grad_scale: float, adam: bool = False, beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8,
                max_norm: float = float("inf"), sigma_next: float = 0.0, ascend: bool = True, utilities: Optional[int] = None,
                skipped: Optional[int] = None, kind: Optional[int] = None, flags: Optional[int] = None, reserved: int = 0) -> None:
        """``gymrs_es_step``: utilities from the latest ``evaluate_policy`` (or ``utilities``, the device address of P f32), the
        gradient of the centre, the optimizer's update (``grad_scale`` is typically 2**-24 / (P * sigma)) and the population of
        the next generation, in stream order with no synchronisation.  A step whose gradient excluded a term leaves the centre
        alone and adds 1 to ``skipped`` (one device uint64).  ``sigma_next`` > 0 becomes the sigma of the new population."""
        desc = EsStepDesc((OPT_ADAM if adam else OPT_SGD) if kind is None else int(kind), (OPT_ASCEND if ascend else 0) if flags is None else int(flags),
                          float(lr), float(grad_scale), float(beta1), float(beta2), float(eps), float(max_norm), float(sigma_next), int(reserved),
                          C.c_void_p(utilities or None), C.c_void_p(skipped or None))
        _check(self._lib, self._lib.gymrs_es_step(self._h, C.byref(desc)))

    def es_state(self, centre: bool = True):
        """dict(hidden, n_policies, lanes_per_policy, seed, sigma, generation) of the ES state and, with ``centre``, the centre as
        f32 (synchronising)."""
        desc, gen = EsDesc(), C.c_uint64()
        _check(self._lib, self._lib.gymrs_get_es(self._h, C.byref(desc), C.byref(gen), None, 0))
        out = dict(hidden=int(desc.hidden), n_policies=int(desc.n_policies), lanes_per_policy=int(desc.lanes_per_policy), seed=int(desc.seed),
                   sigma=float(desc.sigma), generation=int(gen.value))
        if centre:
            c = np.empty(policy_size(self.kind, desc.hidden), np.float32)
            _check(self._lib, self._lib.gymrs_get_es(self._h, C.byref(desc), None, c.ctypes.data_as(C.POINTER(C.c_float)), c.size))
            out["centre"] = c
        return out

    def es_optimizer_state(self):
        """(m [S], v [S], pw [2]) of the centre's Adam state, f32 (synchronising): fresh after ``es_init``."""
        size = policy_size(self.kind, self.es_state(centre=False)["hidden"])
        m, v, pw = np.empty(size, np.float32), np.empty(size, np.float32), np.empty(2, np.float32)
        fp = C.POINTER(C.c_float)
        _check(self._lib, self._lib.gymrs_get_es_optimizer_state(self._h, m.ctypes.data_as(fp), v.ctypes.data_as(fp), pw.ctypes.data_as(fp)))
        return m, v, pw

    def es_centre_ptr(self) -> Tuple[int, int]:
        """(device address, number of floats) of the current centre: zero-copy, at an address that stays the same while the state
        lives; every ``es_step`` rewrites it in stream order."""
        return _view(self._lib, self._lib.gymrs_es_centre_ptr, self._h)

    def es_utilities_ptr(self) -> Tuple[int, int]:
        """(device address, n_policies) of the f32 utilities the last ``es_step`` used: zero-copy."""
        return _view(self._lib, self._lib.gymrs_es_utilities_ptr, self._h, C.c_uint32)

    def es_ranks(self, utilities_dev: int, rank2_dev: int = 0, *, flags: int = 0, reserved: int = 0) -> None:
        """``gymrs_es_ranks``: the centred, tie-averaged rank utilities of every policy from the latest ``evaluate_policy``, written
        to ``utilities_dev`` (device address of P f32) and, unless 0, twice the average rank to ``rank2_dev`` (P uint32,
        ``ES_RANK_INVALID`` where a policy played no episode); in stream order with no synchronisation.  Pass ``utilities_dev`` on as
        ``es_step(utilities=...)``; any policy set will do, ``es_init`` is not needed."""
        desc = EsRanksDesc(C.c_void_p(utilities_dev or None), C.c_void_p(rank2_dev or None), int(flags), int(reserved))
        _check(self._lib, self._lib.gymrs_es_ranks(self._h, C.byref(desc)))

    # -- epsilon-greedy exploration inside the closed-loop calls ----------------------------------------------
    def set_exploration(self, seed: Optional[int] = 0, *, epsilon: Optional[float] = None, threshold: Optional[int] = None) -> None:
        """Install the exploration settings (``gymrs_set_exploration``): a step explores with probability ``threshold`` / 65536
        (``epsilon`` is rounded to that grid), drawing from a Philox stream keyed (``seed``, global lane id, engine tick).
        ``set_exploration(None)`` removes them.  Touches no lane state, tick, statistics or fitness table; launches play them only
        with ``rollout_closed_loop(..., explore=True)`` and ``explore_actions``."""
        if seed is None:
            _check(self._lib, self._lib.gymrs_set_exploration(self._h, None))
            return
        x = _exploration(seed, epsilon, threshold)
        _check(self._lib, self._lib.gymrs_set_exploration(self._h, C.byref(x)))

    def exploration(self) -> Tuple[int, int]:
        """(seed, threshold) as set; raises when the engine has no exploration settings."""
        x = Exploration()
        _check(self._lib, self._lib.gymrs_get_exploration(self._h, C.byref(x)))
        return int(x.seed), int(x.threshold)

    def explore_actions(self, actions_dev: int) -> None:
        """``policy_actions`` mixed with the exploration draw at the engine's current tick (one launch): ``explore_actions(buf);
        step(buf)``, K times, is ``rollout_closed_loop(K, explore=True)``."""
        _check(self._lib, self._lib.gymrs_explore_actions(self._h, C.c_void_p(actions_dev)))

    # -- softmax sampling inside the closed-loop calls -----------------------------------------------------------
    def set_sampling(self, seed: Optional[int] = 0, *, temperature: Optional[float] = None, scale: Optional[float] = None) -> None:
        """Install the sampling settings (``gymrs_set_sampling``): a ~ softmax(logits / ``temperature``), drawn from a Philox stream
        keyed (``seed``, global lane id, engine tick).  Give ``temperature`` or the kernel's own ``scale`` = log2(e) / temperature
        (0: the uniform policy).  ``set_sampling(None)`` removes them.  Touches no lane state, tick, statistics or fitness table;
        launches play them only with ``rollout_closed_loop(..., sample=True)``, ``rollout_transitions(..., sample=True)`` and
        ``sample_actions``."""
        if seed is None:
            _check(self._lib, self._lib.gymrs_set_sampling(self._h, None))
            return
        x = _sampling(seed, temperature, scale)
        _check(self._lib, self._lib.gymrs_set_sampling(self._h, C.byref(x)))

    def sampling(self) -> Tuple[int, float]:
        """(seed, scale) as set; raises when the engine has no sampling settings."""
        x = Sampling()
        _check(self._lib, self._lib.gymrs_get_sampling(self._h, C.byref(x)))
        return int(x.seed), float(x.scale)

    def sample_actions(self, actions_dev: int, prob: Optional[int] = None) -> None:
        """The sampled action of every lane at the engine's current tick (one launch); ``prob`` (device address of n_envs f32, or
        None) gets the probability of the action taken.  ``sample_actions(buf); step(buf)``, K times, is
        ``rollout_closed_loop(K, sample=True)``."""
        _check(self._lib, self._lib.gymrs_sample_actions(self._h, C.c_void_p(actions_dev), C.c_void_p(prob or None)))

    def policy_fitness(self, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        """The records of policies [first, first + count) as an int64 array of shape (count, 4): columns reward_sum, episodes,
        done, truncated (synchronising).  ``count`` defaults to the rest of the set."""
        return _policy_records(self._lib, self._lib.gymrs_get_policy_fitness, self._h, self._h, first, count, 4)

    def policy_fitness_ptr(self) -> Tuple[int, int]:
        """(device address, n_policies) of the records (``PolicyFitness``, 32 bytes each): zero-copy, under the stream rules of
        the other views.  Valid until the next set_policy or close."""
        return _view(self._lib, self._lib.gymrs_policy_fitness_ptr, self._h, C.c_uint32)

    def policy_fitness_clear(self) -> None:
        """Zero the records (in stream order)."""
        _check(self._lib, self._lib.gymrs_policy_fitness_clear(self._h))

    # -- episodic policy evaluation: E whole episodes per lane in one launch ---------------------------------
    def evaluate_policy(self, episodes_per_lane: int, max_episode_steps: int = 0, seed: int = 0, common_starts: bool = False,
                        lengths: int = 0, flags: Optional[int] = None, lane_params: bool = False) -> None:
        """Play ``episodes_per_lane`` whole episodes of every lane under its policy (``gymrs_evaluate_policy``): episode ``e`` of a
        lane starts where ``reset(seed + e)`` would put it and ends at its first done or after ``max_episode_steps`` steps (0 = the
        params' limit).  ``common_starts`` gives every policy the same start states.  ``lengths``: device address of a uint32
        ``[episodes_per_lane][n_envs]`` array for length | done << 31 of every episode, or 0.  ``lane_params``
        (``GYMRS_EVAL_LANE_PARAMS``): every lane plays with the row of the parameter table ``step`` would use for it (without a
        table it changes nothing); without it an engine with a table refuses the call.  ``flags`` overrides ``common_starts`` and
        ``lane_params`` with raw ``GYMRS_EVAL_*`` bits.  The engine's lanes are neither read nor written; the results
        (``policy_eval``) are those of the latest call."""
        desc = _eval_desc(episodes_per_lane, max_episode_steps, seed, common_starts, lengths, flags, lane_params)
        _check(self._lib, self._lib.gymrs_evaluate_policy(self._h, C.byref(desc)))

    def policy_eval(self, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        """The episodic records of policies [first, first + count) as an int64 array of shape (count, 8): columns return_sum,
        return_sq_sum, episodes, done, truncated, steps, return_min, return_max (synchronising; return_sq_sum is the uint64's
        bits).  ``count`` defaults to the rest of the set."""
        return _policy_records(self._lib, self._lib.gymrs_get_policy_eval, self._h, self._h, first, count, 8)

    def policy_eval_ptr(self) -> Tuple[int, int]:
        """(device address, n_policies) of the episodic records (``PolicyEval``, 64 bytes each): zero-copy, under the stream
        rules of the other views.  Valid until the next set_policy or close."""
        return _view(self._lib, self._lib.gymrs_policy_eval_ptr, self._h, C.c_uint32)

    def tick(self) -> Tuple[int, int]:
        t, s = C.c_uint64(), C.c_uint64()
        _check(self._lib, self._lib.gymrs_get_tick(self._h, C.byref(t), C.byref(s)))
        return t.value, s.value


class _ShardView(BatchedEngine):
    """Block r of a ShardedEngine: the engine's views (obs / reward / done pointers, stream, env_json).  Borrowed -- the
    sharder owns it, ``close`` is a no-op, and it must not be stepped directly while the sharder is in use."""

    def __init__(self, lib, handle, kind, n_envs, offset, flags, device):
        self._lib = lib
        self._h = C.c_void_p(handle)
        self.kind, self.n_envs, self.global_env_offset, self.flags, self.device = kind, n_envs, offset, flags, device
        self.state_dim, self.obs_dim, self.action_dtype = _STATE_DIM[kind], _OBS_DIM[kind], _ACTION_DTYPE[kind]
        self.params = None

    def close(self) -> None:
        self._h = C.c_void_p()


class ShardedEngine:
    """One batch of ``n_total`` lanes over several GPUs in ONE process (``gymrs_sharded_*``, include/gymrs_amd.h): contiguous
    blocks, one engine and one native host thread per block, global lane ids -- every result is bit-identical to one
    ``BatchedEngine`` of ``n_total`` lanes.  ``devices[r]`` is block r's device (a device may repeat)."""

    def __init__(self, kind: int, n_total: int, devices: Sequence[int], *, global_env_offset: int = 0, params=None, flags: int = 0):
        self._lib = load_library()
        self._h = C.c_void_p()
        self.kind, self.n_total, self.flags = int(kind), int(n_total), int(flags)
        self.state_dim, self.obs_dim, self.action_dtype = _STATE_DIM[self.kind], _OBS_DIM[self.kind], _ACTION_DTYPE[self.kind]
        self.params = params if params is not None else default_params(self.kind)
        devs = (C.c_int * len(devices))(*[int(d) for d in devices])
        _check(self._lib, self._lib.gymrs_sharded_create(self.kind, self.n_total, int(global_env_offset), len(devices), devs,
                                                         C.byref(self.params), self.flags, C.byref(self._h)))
        self.shards = []
        for r in range(len(devices)):
            eng, first, count, dev = C.c_void_p(), C.c_uint64(), C.c_uint64(), C.c_int()
            _check(self._lib, self._lib.gymrs_sharded_shard(self._h, r, C.byref(eng), C.byref(first), C.byref(count), C.byref(dev)))
            view = _ShardView(self._lib, eng.value, self.kind, count.value, int(global_env_offset) + first.value, self.flags, dev.value)
            view.first_lane = first.value
            self.shards.append(view)

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h:
            for s in self.shards:
                s.close()
            self._lib.gymrs_sharded_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _ptrs(self, addresses):
        if len(addresses) != len(self.shards):
            raise ValueError("one device address per shard expected")
        return (C.c_void_p * len(addresses))(*[C.c_void_p(int(a)) for a in addresses])

    def reset(self, seed: Optional[int] = None, options: Optional[Sequence[float]] = None) -> int:
        bounds = None
        if options is not None:
            arr = np.ascontiguousarray(options, dtype=np.float32)
            if arr.size != 2 * self.state_dim:
                raise ValueError(f"options needs {2 * self.state_dim} floats (lows then highs)")
            bounds = arr.ctypes.data_as(C.POINTER(C.c_float))
        used = C.c_uint64()
        _check(self._lib, self._lib.gymrs_sharded_reset(self._h, 0 if seed is None else 1, 0 if seed is None else int(seed), bounds, C.byref(used)))
        return used.value

    def step(self, actions_dev: Sequence[int]) -> None:
        """``actions_dev[r]``: device address (on block r's device) of block r's actions.  Asynchronous."""
        _check(self._lib, self._lib.gymrs_sharded_step(self._h, self._ptrs(actions_dev)))

    def step_many(self, actions_dev: Sequence[int], stride_bytes: int, n_buffers: int, n_steps: int, use_graph: bool = False) -> None:
        _check(self._lib, self._lib.gymrs_sharded_step_many(self._h, self._ptrs(actions_dev), int(stride_bytes), int(n_buffers), int(n_steps),
                                                            1 if use_graph else 0))

    def fill_actions(self, actions_dev: Sequence[int], seed: int, t: int) -> None:
        _check(self._lib, self._lib.gymrs_sharded_fill_actions(self._h, self._ptrs(actions_dev), int(seed), int(t)))

    def rollout(self, n_steps: int, action_seed: int, action_t0: int = 0) -> None:
        """``BatchedEngine.rollout`` on every block: ``n_steps`` random-policy steps fused into one launch per block."""
        _check(self._lib, self._lib.gymrs_sharded_rollout(self._h, int(n_steps), int(action_seed), int(action_t0)))

    # -- closed-loop rollouts and per-policy fitness on every block (the policy set is keyed by global lane ids) --
    def set_policy(self, weights, hidden: int = 0, lanes_per_policy: int = 1) -> None:
        """``BatchedEngine.set_policy`` on every block: the same set everywhere.  ``None`` removes the policy."""
        _set_weights(self._lib, self._lib.gymrs_sharded_set_policy, self._h, self.kind, weights, hidden, lanes_per_policy, policy_size, "policies")

    def rollout_policy(self, n_steps: int) -> None:
        """``BatchedEngine.rollout_policy`` on every block."""
        _check(self._lib, self._lib.gymrs_sharded_rollout_policy(self._h, int(n_steps)))

    def rollout_policy_fitness(self, n_steps: int) -> None:
        """``BatchedEngine.rollout_policy_fitness`` on every block."""
        _check(self._lib, self._lib.gymrs_sharded_rollout_policy_fitness(self._h, int(n_steps)))

    def rollout_closed_loop(self, n_steps: int, *, lane_params: bool = False, fitness: bool = False, record=None,
                            flags: Optional[int] = None, explore: bool = False, sample: bool = False) -> None:
        """``BatchedEngine.rollout_closed_loop`` on every block (``record`` must stay None: the blocks live on several devices)."""
        desc = _closed_loop_desc(self.n_total, n_steps, lane_params, fitness, record, flags, explore, sample)
        _check(self._lib, self._lib.gymrs_sharded_rollout_closed_loop(self._h, C.byref(desc)))

    def set_exploration(self, seed: Optional[int] = 0, *, epsilon: Optional[float] = None, threshold: Optional[int] = None) -> None:
        """``BatchedEngine.set_exploration`` on every block: the same settings everywhere (the draw is keyed by global lane ids)."""
        if seed is None:
            _check(self._lib, self._lib.gymrs_sharded_set_exploration(self._h, None))
            return
        x = _exploration(seed, epsilon, threshold)
        _check(self._lib, self._lib.gymrs_sharded_set_exploration(self._h, C.byref(x)))

    def exploration(self) -> Tuple[int, int]:
        """(seed, threshold) as set (every block holds the same)."""
        return self.shards[0].exploration()

    def explore_actions(self, actions_dev) -> None:
        """``BatchedEngine.explore_actions`` on every block: ``actions_dev[r]`` is the device address of block r's buffer."""
        for s, a in zip(self.shards, actions_dev):
            s.explore_actions(a)

    def set_sampling(self, seed: Optional[int] = 0, *, temperature: Optional[float] = None, scale: Optional[float] = None) -> None:
        """``BatchedEngine.set_sampling`` on every block: the same settings everywhere (the draw is keyed by global lane ids)."""
        if seed is None:
            _check(self._lib, self._lib.gymrs_sharded_set_sampling(self._h, None))
            return
        x = _sampling(seed, temperature, scale)
        _check(self._lib, self._lib.gymrs_sharded_set_sampling(self._h, C.byref(x)))

    def sampling(self) -> Tuple[int, float]:
        """(seed, scale) as set (every block holds the same)."""
        return self.shards[0].sampling()

    def sample_actions(self, actions_dev, prob=None) -> None:
        """``BatchedEngine.sample_actions`` on every block: ``actions_dev[r]`` (and ``prob[r]``) are the device addresses of block
        r's buffers."""
        for r, (s, a) in enumerate(zip(self.shards, actions_dev)):
            s.sample_actions(a, None if prob is None else prob[r])

    def policy_fitness(self, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        """The records of the WHOLE batch, (count, 4) int64 as ``BatchedEngine.policy_fitness``: the blocks' records summed
        (exact; synchronising)."""
        # (every block holds the same set: block 0's description is the batch's)
        return _policy_records(self._lib, self._lib.gymrs_sharded_get_policy_fitness, self._h, self.shards[0]._h, first, count, 4)

    def policy_fitness_ptr(self):
        """[(device address, n_policies)] per block: each block's own records (``shards[r].policy_fitness_ptr()``); their sum
        is the batch's."""
        return [s.policy_fitness_ptr() for s in self.shards]

    def policy_fitness_clear(self) -> None:
        _check(self._lib, self._lib.gymrs_sharded_policy_fitness_clear(self._h))

    def evaluate_policy(self, episodes_per_lane: int, max_episode_steps: int = 0, seed: int = 0, common_starts: bool = False,
                        lengths: int = 0, flags: Optional[int] = None, lane_params: bool = False) -> None:
        """``BatchedEngine.evaluate_policy`` on every block (``lengths`` must stay 0: ask ``shards[r]`` for per-episode lengths).
        ``lane_params`` plays the table of ``set_param_table`` / ``set_param_index``."""
        desc = _eval_desc(episodes_per_lane, max_episode_steps, seed, common_starts, lengths, flags, lane_params)
        _check(self._lib, self._lib.gymrs_sharded_evaluate_policy(self._h, C.byref(desc)))

    def policy_eval(self, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        """The episodic records of the WHOLE batch, (count, 8) int64 as ``BatchedEngine.policy_eval``: the blocks' records merged
        (sums added, min of mins, max of maxes; synchronising)."""
        return _policy_records(self._lib, self._lib.gymrs_sharded_get_policy_eval, self._h, self.shards[0]._h, first, count, 8)

    def policy_eval_ptr(self):
        """[(device address, n_policies)] per block: each block's own records (``shards[r].policy_eval_ptr()``)."""
        return [s.policy_eval_ptr() for s in self.shards]

    def set_params(self, params) -> None:
        """Assign the pub physics fields of every lane of the batch (``gymrs_set_params`` on every block)."""
        if not isinstance(params, _PARAMS[self.kind]):
            raise TypeError(f"expected {_PARAMS[self.kind].__name__}")
        _check(self._lib, self._lib.gymrs_sharded_set_params(self._h, C.byref(params)))
        self.params = type(params).from_buffer_copy(params)

    # -- per-lane physics on the batch: the same rows on every block, the index in batch lane numbering --
    def set_param_table(self, rows) -> None:
        """``BatchedEngine.set_param_table`` on every block: the same rows everywhere (``None`` or ``[]`` switches the table off)."""
        rows = list(rows or [])
        cls = _PARAMS[self.kind]
        if any(not isinstance(r, cls) for r in rows):
            raise TypeError(f"expected {cls.__name__} rows")
        arr = (cls * len(rows))(*rows) if rows else None
        _check(self._lib, self._lib.gymrs_sharded_set_param_table(self._h, arr, len(rows)))
        p = cls()
        _check(self._lib, self._lib.gymrs_get_params(self.shards[0]._h, C.byref(p)))
        self.params = p

    def param_table(self) -> list:
        """The rows of the active table in f64 exactly as set ([] without a table), read from block 0."""
        k = C.c_uint32()
        _check(self._lib, self._lib.gymrs_sharded_get_param_table(self._h, None, 0, C.byref(k)))
        if k.value == 0:
            return []
        arr = (_PARAMS[self.kind] * k.value)()
        _check(self._lib, self._lib.gymrs_sharded_get_param_table(self._h, arr, k.value, C.byref(k)))
        return list(arr)

    def set_param_index(self, index, first: int = 0) -> None:
        """The rows of lanes [first, first + len(index)) of the BATCH, cut across the blocks."""
        idx = np.ascontiguousarray(index, dtype=np.uint16)
        _check(self._lib, self._lib.gymrs_sharded_set_param_index(self._h, int(first), idx.size, idx.ctypes.data_as(C.c_void_p)))

    def get_param_index(self, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        count = self.n_total - first if count is None else count
        out = np.empty(count, dtype=np.uint16)
        _check(self._lib, self._lib.gymrs_sharded_get_param_index(self._h, int(first), int(count), out.ctypes.data_as(C.c_void_p)))
        return out

    def sync(self) -> None:
        _check(self._lib, self._lib.gymrs_sharded_sync(self._h))

    def stats(self) -> np.ndarray:
        """{sum_return, sum_length, n_episodes, n_steps} of the WHOLE batch (RCCL all-reduce on distinct devices, host sum otherwise)."""
        out = (C.c_double * 4)()
        _check(self._lib, self._lib.gymrs_sharded_stats(self._h, out))
        return np.array(out[:], dtype=np.float64)

    def stats_clear(self) -> None:
        _check(self._lib, self._lib.gymrs_sharded_stats_clear(self._h))

    @property
    def reduce_path(self) -> str:
        return self._lib.gymrs_sharded_reduce_path(self._h).decode()

    def get_state(self, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        count = self.n_total - first if count is None else count
        out = np.empty((self.state_dim, count), dtype=np.float32)
        _check(self._lib, self._lib.gymrs_sharded_get_state(self._h, first, count, out.ctypes.data_as(C.c_void_p)))
        return out

    def get_final_obs(self, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        """FINAL_OBS: the final observations of lanes [first, first + count) of the whole batch, gathered from the blocks (each block's
        own views: ``shards[r].final_obs_ptrs()`` / ``get_final_obs``), shape (obs_dim, count)."""
        count = self.n_total - first if count is None else count
        out = np.empty((self.obs_dim, count), dtype=np.float32)
        for s in self.shards:
            lo, hi = max(first, s.first_lane), min(first + count, s.first_lane + s.n_envs)
            if lo < hi:
                out[:, lo - first:hi - first] = s.get_final_obs(lo - s.first_lane, hi - lo)
        return out

    def get_step_result(self, first: int = 0, count: Optional[int] = None):
        count = self.n_total - first if count is None else count
        reward, done, trunc = np.empty(count, np.float32), np.empty(count, np.uint8), np.empty(count, np.uint8)
        _check(self._lib, self._lib.gymrs_sharded_get_step_result(self._h, first, count, reward.ctypes.data_as(C.c_void_p),
                                                                  done.ctypes.data_as(C.c_void_p), trunc.ctypes.data_as(C.c_void_p)))
        return reward, done, trunc
