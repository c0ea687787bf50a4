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
