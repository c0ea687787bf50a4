"""A closed-loop rollout computed on the CPU alone: the f32 twin (oracle.bindings.TwinEngine) stepped with the actions of
tests/cpp/policy_ref.c (plain C, libm's fmaf, gcc -O2 -ffp-contract=off).  Neither shares code with the library's policy or rollout
kernels, and this module never imports the library: what it returns is the yardstick of tests/test_gpu_policy_matrix.py, and
tests/test_closed_loop_ref.py shows without a GPU that the yardstick's cases are worth comparing with (episodes end, actions vary,
policies disagree, inside the lanes of every copy of the kernel).

A plain module like spawn_server.py, imported by test files; no fixtures, no pytest hooks."""
import ctypes as C
import tempfile
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import spawn_server

from oracle.bindings import Twin, TwinEngine

A, S, T, F = 1, 2, 4, 8  # GYMRS_AUTO_RESET, TRACK_STATS, TIME_LIMIT, FINAL_OBS
FLAG_SETS = [0, A, A | S, T, A | T, A | S | T, A | F, A | S | F, A | T | F, A | S | T | F]  # every set the rollout kernels are built for
DIMS = {0: (4, 2), 1: (2, 3)}  # kind -> (observation size, number of actions)
COPIES = ("uniform-full", "gathered-full", "uniform-ragged", "gathered-ragged")  # wave_classes' values index this

_lib = None
_dir = None
_twin = None


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def size_of(kind, hidden):
    d, a = DIMS[kind]
    return a * (d + 1) if hidden == 0 else hidden * (d + 1) + a * (hidden + 1)


def make_weights(kind, hidden, n_policies, seed):
    """seeded normals, f32: scale 1 (affine), 1 / sqrt(fan_in) (hidden)"""
    d, a = DIMS[kind]
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n_policies):
        if hidden == 0:
            parts = [rng.standard_normal(a * d), rng.standard_normal(a)]
        else:
            parts = [rng.standard_normal(hidden * d) / np.sqrt(d), rng.standard_normal(hidden) / np.sqrt(d),
                     rng.standard_normal(a * hidden) / np.sqrt(hidden), rng.standard_normal(a) / np.sqrt(hidden)]
        out.append(np.concatenate(parts).astype(np.float32))
    w = np.stack(out)
    assert w.shape == (n_policies, size_of(kind, hidden))
    return w


def _policy_lib():
    global _lib, _dir
    if _lib is None:
        _dir = tempfile.TemporaryDirectory(prefix="policy_ref")  # removed when the interpreter exits
        out = Path(_dir.name) / "libpolicy_ref.so"
        src = Path(__file__).resolve().parent / "cpp" / "policy_ref.c"
        spawn_server.run(["gcc", "-O2", "-ffp-contract=off", "-shared", "-fPIC", str(src), "-o", str(out), "-lm"], check=True)
        _lib = C.CDLL(str(out))
        head = [C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p]
        _lib.policy_ref.restype = None
        _lib.policy_ref.argtypes = head + [C.c_void_p]
        _lib.policy_ref_logits.restype = None
        _lib.policy_ref_logits.argtypes = head + [C.c_void_p, C.c_void_p]
    return _lib


def _args(kind, hidden, weights, obs):
    d, a = DIMS[kind]
    w = np.ascontiguousarray(weights, np.float32)
    obs = np.ascontiguousarray(obs, np.float32)
    assert obs.ndim == 2 and obs.shape[0] == d and w.size % size_of(kind, hidden) == 0
    return d, a, w, obs


def policy_ref(kind, hidden, weights, lanes_per_policy, gid0, obs):
    """The actions (uint8, one per column of obs) of the policy set `weights`; column i is lane gid0 + i of the batch."""
    d, a, w, obs = _args(kind, hidden, weights, obs)
    n = obs.shape[1]
    act = np.empty(n, np.uint8)
    _policy_lib().policy_ref(d, a, hidden, w.size // size_of(kind, hidden), lanes_per_policy, gid0, n, w.ctypes.data, obs.ctypes.data,
                             act.ctypes.data)
    return act


def policy_logits(kind, hidden, weights, lanes_per_policy, gid0, obs):
    """(y, z): the logits policy_ref chose from, shape (A, n), and the hidden layer's pre-activations, shape (hidden, n)."""
    d, a, w, obs = _args(kind, hidden, weights, obs)
    n = obs.shape[1]
    y = np.empty((a, n), np.float32)
    z = np.empty((hidden, n), np.float32)
    _policy_lib().policy_ref_logits(d, a, hidden, w.size // size_of(kind, hidden), lanes_per_policy, gid0, n, w.ctypes.data, obs.ctypes.data,
                                    y.ctypes.data, z.ctypes.data if hidden else None)
    return y, z


def wave_classes(n, vec, gid0, n_policies, lanes_per_policy):
    """Which copy of rollout_block steps each of the n lanes: an int8 array of indices into COPIES.

    This MIRRORS the kernels' selection rule and must follow it if it changes: `policy_select` in gym-rs_amd/csrc/gymrs_policy.h
    (a wave of 64 work-items x vec lanes is uniform if there is one policy, or if the block of lanes_per_policy lanes that holds
    the wave's first lane has at least 64 * vec lanes left from there) and the `full` test of rollout_policy_kernel in
    gymrs_rollout_policy.hip (a wave is full if all its 64 * vec lanes are below n).  gymrs_policy_actions follows the same rule
    at vec = 4 (given a 4-byte aligned action buffer)."""
    per_wave = 64 * vec
    out = np.empty(n, np.int8)
    for first in range(0, n, per_wave):  # python ints: global ids and lanes_per_policy go beyond 2^32
        left = lanes_per_policy - (gid0 + first) % lanes_per_policy
        uniform = n_policies == 1 or left >= per_wave
        full = first + per_wave <= n
        out[first:first + per_wave] = (0 if uniform else 1) + (0 if full else 2)
    return out


def lanes_per_copy(n, vec, gid0, n_policies, lanes_per_policy):
    """{copy name: number of lanes}, copies without lanes left out"""
    count = np.bincount(wave_classes(n, vec, gid0, n_policies, lanes_per_policy), minlength=4)
    return {COPIES[c]: int(k) for c, k in enumerate(count) if k}


def final_obs_after(tw0, state, act):
    """The observation the flags = 0 twin tw0 shows after stepping `state` with `act`: what a lane whose step ends an episode keeps
    as its final observation (the auto-reset twin has re-armed that lane by then)"""
    tw0.set_state(state)
    tw0.step(act)
    return tw0.get_obs()


def reference(kind, n, gid0, params, flags, weights, hidden, lanes_per_policy, reset_seed, schedule, prepare=None, tick0=1, bounds=None):
    """What an engine of n lanes at global offset gid0 holds after each launch of `schedule` (steps per launch) of closed-loop
    stepping from reset(reset_seed).  `weights`: one policy set, or a list of one set per launch (a learner rewriting them between
    launches).  `prepare(state, first)` (optional) returns the start state to use in place of the reset state `state`, whose column
    i is lane first + i of the batch; the caller applies the same function to the engine.  tick0 (default 1: the tick a reset leaves)
    is the engine tick the first step starts from: tick0 - 1 is the shift of tests/time_shift.py.  bounds (default None: the env's own box)
    is the `options` of the reset, lows then highs: every re-arm draws from it too.

    Returns one SimpleNamespace per launch:
      state, obs, reward, done, truncated, stats, tick   as the engine's getters return them (twin with flags & ~F; tick counts the
                                                         reset and every step)
      final       the final-observation rows as tests/test_gpu_final_obs.py::checked_step tracks them: zero after reset; a
                  lane whose step ended an episode (done | truncated) takes the observation a flags = 0 twin shows after the same
                  step from the same state
      rec_obs [steps][D][n], rec_actions, rec_reward, rec_done, rec_truncated [steps][n]    the rows a recording launch keeps
      episodes [n]            episodes ended so far (steps with done | truncated set)
      actions_seen [A][n]     whether the lane ever took action a
      disagree [n]            whether two policies of the set, asked alone about the lane's observation, ever chose differently
    and, on the first only, start_state."""
    global _twin
    if _twin is None:
        _twin = Twin()
    d, n_act = DIMS[kind]
    sets = list(weights) if isinstance(weights, (list, tuple)) else [weights] * len(schedule)
    assert len(sets) == len(schedule)
    tw = TwinEngine(_twin, kind, n, params, flags=flags & ~F, gid0=gid0)
    tw0 = TwinEngine(_twin, kind, n, params, flags=0)
    tw.reset(reset_seed, bounds)
    if prepare is not None:
        tw.set_state(prepare(tw.get_state(), 0))
    if tick0 != 1:
        tw.shift_time(tick0 - 1)
    start = tw.get_state()
    final = np.zeros((d, n), np.float32)
    episodes = np.zeros(n, np.int64)
    seen = np.zeros((n_act, n), bool)
    disagree = np.zeros(n, bool)
    tick = tick0
    out = []
    for steps, w in zip(schedule, sets):
        w = np.ascontiguousarray(w, np.float32).reshape(-1, size_of(kind, hidden))
        rec = SimpleNamespace(obs=[], actions=[], reward=[], done=[], truncated=[])
        for _ in range(steps):
            obs = tw.get_obs()
            act = policy_ref(kind, hidden, w, lanes_per_policy, gid0, obs)
            seen[act, np.arange(n)] = True
            alone = [policy_ref(kind, hidden, w[i:i + 1], 1, 0, obs) for i in range(len(w))]
            for x in alone[1:]:
                disagree |= x != alone[0]
            last = final_obs_after(tw0, tw.get_state(), act)
            tw.step(act)
            r, dn, tr = tw.get_result()
            ended = (dn | tr) != 0
            if flags & A:  # (the engine keeps final observations only with auto-reset)
                final[:, ended] = last[:, ended]
            episodes += ended
            tick += 1
            for row, x in zip((rec.obs, rec.actions, rec.reward, rec.done, rec.truncated), (tw.get_obs(), act, r, dn, tr)):
                row.append(x)
        r, dn, tr = tw.get_result()
        out.append(SimpleNamespace(state=tw.get_state(), obs=tw.get_obs(), reward=r, done=dn, truncated=tr, stats=tw.stats(), tick=tick,
                                   final=final.copy(), rec_obs=np.stack(rec.obs), rec_actions=np.stack(rec.actions),
                                   rec_reward=np.stack(rec.reward), rec_done=np.stack(rec.done), rec_truncated=np.stack(rec.truncated),
                                   episodes=episodes.copy(), actions_seen=seen.copy(), disagree=disagree.copy()))
    out[0].start_state = start
    return out


# ---- the cases of tests/test_gpu_policy_matrix.py (checked without a GPU by tests/test_closed_loop_ref.py) -------------------
N_POLICIES = 3
SCHEDULE = (1, 7, 40, 3)
MAX_EPISODE_STEPS = 17
RESET_SEED = 3
HIDDEN = (0, 7, 8)  # affine; one full trip of the uniform copy's four-unit loop plus a remainder of three; two full trips
# (n, vec, global offset, lanes_per_policy): two shapes per vec, which between them put lanes into all four copies
SHAPES = [(4200, 4, (1 << 40) + 12345, 1000),  # uniform-full 3072, gathered-full 1024, uniform-ragged 104
          (5000, 4, 12345, 1024),              # uniform-full 3840, gathered-full 1024, gathered-ragged 136
          (4200, 8, (1 << 40) + 12345, 1000),  # uniform-full 2048, gathered-full 2048, uniform-ragged 104
          (2900, 8, 12345, 1000)]              # uniform-full 1536, gathered-full 1024, gathered-ragged 340
# Seed of make_weights per (kind, hidden, index into SHAPES): the first seed, searched with this module alone, for which under
# every flag set and inside the lanes of every copy an episode ends (sets with A or T), two different actions occur, two policies
# disagree and (sets with F) a final observation is kept.  Many a random policy takes one action only inside a ragged wave of
# ~100 lanes.  tests/test_closed_loop_ref.py asserts that these seeds do meet the conditions.
SEEDS = {(0, 0, 0): 3, (0, 0, 1): 3, (0, 0, 2): 3, (0, 0, 3): 1, (0, 7, 0): 17, (0, 7, 1): 17, (0, 7, 2): 17, (0, 7, 3): 1,
         (0, 8, 0): 2, (0, 8, 1): 2, (0, 8, 2): 2, (0, 8, 3): 1, (1, 0, 0): 3, (1, 0, 1): 3, (1, 0, 2): 3, (1, 0, 3): 1,
         (1, 7, 0): 1, (1, 7, 1): 1, (1, 7, 2): 1, (1, 7, 3): 2, (1, 8, 0): 2, (1, 8, 1): 2, (1, 8, 2): 2, (1, 8, 3): 1}


RECORD_HIDDEN = (0, 8)


def cases(record):
    """(kind, index into SHAPES, flag set, hidden) of every case of the matrix: the fused kernel's, or the recording kernel's (which
    exists at 4 lanes per work-item only)"""
    return [(kind, shape, flags, hidden) for kind in (0, 1) for shape, s in enumerate(SHAPES) if not record or s[1] == 4
            for flags in FLAG_SETS for hidden in (RECORD_HIDDEN if record else HIDDEN)]


def coverage():
    """{(kind, vec, flag set, record): lanes stepped per copy (in COPIES order), summed over the matrix's cases}: one entry per
    instantiation of rollout_policy_kernel.  No cell may be zero."""
    out = {}
    for record in (False, True):
        for kind, shape, flags, hidden in cases(record):
            n, vec, gid0, lpp = SHAPES[shape]
            row = out.setdefault((kind, vec, flags, record), np.zeros(4, np.int64))
            row += np.bincount(wave_classes(n, vec, gid0, N_POLICIES, lpp), minlength=4)
    return out


def mountain_car_prepare(state, first):
    """MountainCar without a time limit ends almost no episode in 51 steps: every 7th lane of the batch starts next to the goal,
    moving towards it."""
    state = state.copy()
    k = (-first) % 7
    state[0, k::7] = 0.45
    state[1, k::7] = 0.04
    return state


def case(kind, shape, flags, hidden, params, bounds=None):
    """The arguments of `reference` for one case of the matrix; `params` = the engine's default parameters of `kind` (edited here)."""
    n, vec, gid0, lpp = SHAPES[shape]
    params.max_episode_steps = MAX_EPISODE_STEPS
    w = make_weights(kind, hidden, N_POLICIES, SEEDS[kind, hidden, shape])
    prepare = mountain_car_prepare if kind == 1 else None
    return SimpleNamespace(kind=kind, n=n, vec=vec, gid0=gid0, params=params, flags=flags, weights=w, hidden=hidden, lanes_per_policy=lpp,
                           reset_seed=RESET_SEED, schedule=SCHEDULE, prepare=prepare, bounds=bounds,
                           classes=wave_classes(n, vec, gid0, N_POLICIES, lpp))


def run_case(c, tick0=1):
    return reference(c.kind, c.n, c.gid0, c.params, c.flags, c.weights, c.hidden, c.lanes_per_policy, c.reset_seed, c.schedule, c.prepare, tick0,
                     getattr(c, "bounds", None))


def worth_comparing(c, ref):
    """The conditions of SEEDS for one case and its reference; returns a list of what is missing (empty: all met)."""
    last = ref[-1]
    missing = []
    for copy in np.unique(c.classes):
        m = c.classes == copy
        name = COPIES[copy]
        if c.flags & (A | T) and not last.episodes[m].any():
            missing.append(f"{name}: no episode ended")
        if (last.actions_seen[:, m].any(axis=1)).sum() < 2:
            missing.append(f"{name}: one action only")
        if not last.disagree[m].any():
            missing.append(f"{name}: the policies never disagree")
        if c.flags & F and not last.final[:, m].any():
            missing.append(f"{name}: no final observation")
    return missing
