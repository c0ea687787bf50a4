"""The cases that take the closed-loop and evaluation kernels off the fast physics path, computed on the CPU alone.

Every kernel that steps lanes has a wave-uniform branch-free physics branch and a per-lane general one; a wave takes the general
one if it is ragged or if any of its lanes is outside Env::kRangeMax (gym-rs_amd/csrc/gymrs_tile.h; lane_params_ref.beyond_range
restates it).  The matrices of closed_loop_ref and policy_eval_ref start from reset() under default thresholds and never leave
the range.  The cases here do: parameter rows whose episodes end only far outside the range (a 40 times harder push, a pole
that may fall to 2 rad, a MountainCar track of +-1e9 with a strong engine) and, for the rollouts, the start states of
lane_params_ref.slow_prepare on every 7th lane of the batch (angles up to 1e30, NaN, inf).

The references are closed_loop_ref.reference, policy_eval_ref.reference and policy_eval_table_ref.reference, unchanged: the f32 twin
and tests/cpp/policy_ref.c already run the twin's general path.  What this module adds is the cases, and the figures that show, from
the reference alone, that they go there (rollout_findings, eval_findings, table_findings).  It never imports the library: what it
returns is the yardstick of tests/test_gpu_policy_slowpaths.py, and tests/test_closed_loop_slow_ref.py asserts the conditions
without a GPU.

A plain module like closed_loop_ref.py, imported by test files; no fixtures, no pytest hooks."""
from types import SimpleNamespace

import closed_loop_ref as ref
import lane_params_ref as lp
import numpy as np
import policy_eval_ref as ev
import policy_eval_table_ref as tb
from closed_loop_ref import A, COPIES, F, S, T

N_POLICIES = 3


# ---- parameter rows (lane_params_ref rows: the twin reads them as they are, lane_params_ref.rows_for gives the engine's type) -----
def hard_push_row(max_steps, integrator=0):
    """CartPole: 40 times the default force; an episode ends only at |theta| > 50 rad or |x| > 1e6 (policy_eval_table_ref's row 1)"""
    row = tb.hard_push_rows(max_steps)[1]
    row.kinematics_integrator = integrator
    return row


def wide_row(kind, max_steps, goal=None, integrator=0):
    """CartPole: the pole may fall to 2 rad, the cart run to 1e6.  MountainCar: a track of +-1e9, 40 for the speed limit, an engine
    of 3 against a gravity of 2.5 (a thousand times the default: it is what makes the episode lengths of one policy vary), the goal
    at `goal`, far outside |3 * position| <= 200."""
    row = lp.default_row(kind, max_steps, integrator)
    if kind == 0:
        row.theta_threshold_radians = 2.0
        row.x_threshold = 1.0e6
    else:
        row.min_position, row.max_position, row.max_speed, row.force, row.gravity = -1.0e9, 1.0e9, 40.0, 3.0, 2.5
        row.goal_position = goal
    return row


def slow_start(kind):
    """lane_params_ref.slow_prepare(kind) as a prepare(state, first) of closed_loop_ref.reference: column i of `state` is lane
    first + i of the batch, and the special values sit where they would sit had the whole batch been prepared at once"""
    prepare = lp.slow_prepare(kind)

    def start(state, first):
        whole = np.zeros((state.shape[0], first + state.shape[1]), np.float32)
        whole[:, first:] = state
        return np.ascontiguousarray(prepare(whole)[:, first:])
    return start


# ---- closed-loop rollouts ------------------------------------------------------------------------------------------------------------
ROLLOUT_GOAL = 300.0
HIDDEN = 7  # the fused and the fitness kernel
RECORD_HIDDEN = ref.RECORD_HIDDEN  # (0, 8): the recording kernel, at the two shapes with 4 lanes per work-item
RECORD_SHAPES = [i for i, s in enumerate(ref.SHAPES) if s[1] == 4]
INTEGRATOR_1 = [(0, 1, A | S | T | F, HIDDEN, 1), (0, 3, A | S | T | F, HIDDEN, 1)]  # CartPole, once per vector width

def rollout_row(kind, integrator=0):
    return hard_push_row(ref.MAX_EPISODE_STEPS, integrator) if kind == 0 else wide_row(1, ref.MAX_EPISODE_STEPS, ROLLOUT_GOAL)


def rollout_cases(record):
    """(kind, index into SHAPES, flag set, hidden, integrator) of every case: the fused and fitness kernels', or the recording kernel's"""
    if record:
        return [(kind, shape, flags, hidden, 0) for kind in (0, 1) for shape in RECORD_SHAPES for flags in ref.FLAG_SETS for hidden in RECORD_HIDDEN]
    return [(kind, shape, flags, HIDDEN, 0) for kind in (0, 1) for shape in range(len(ref.SHAPES)) for flags in ref.FLAG_SETS] + INTEGRATOR_1


def flag_sets_of(kind, shape, hidden, integrator):
    """The flag sets under which the cases of one SEEDS entry play"""
    return sorted({c[2] for record in (False, True) for c in rollout_cases(record) if (c[0], c[1], c[3], c[4]) == (kind, shape, hidden, integrator)})


# Seed of closed_loop_ref.make_weights per (kind, hidden, index into closed_loop_ref.SHAPES, integrator): the first seed, searched with
# this module alone (first_rollout_seed, from 1), with which rollout_missing is empty under every flag set the case plays.  It is 1 for
# every case; tests/test_closed_loop_slow_ref.py asserts that seed 1 does meet the conditions.
SEEDS = {(c[0], c[3], c[1], c[4]): 1 for record in (False, True) for c in rollout_cases(record)}


def rollout_case(kind, shape, flags, hidden, integrator=0, seed=None):
    """The arguments of closed_loop_ref.reference for one case (closed_loop_ref.run_case runs it)"""
    n, vec, gid0, lpp = ref.SHAPES[shape]
    seed = SEEDS[kind, hidden, shape, integrator] if seed is None else seed
    return SimpleNamespace(kind=kind, n=n, vec=vec, gid0=gid0, params=rollout_row(kind, integrator), flags=flags,
                           weights=ref.make_weights(kind, hidden, N_POLICIES, seed), hidden=hidden, lanes_per_policy=lpp,
                           reset_seed=ref.RESET_SEED, schedule=ref.SCHEDULE, prepare=slow_start(kind),
                           classes=ref.wave_classes(n, vec, gid0, N_POLICIES, lpp))


def rollout_findings(c, launches):
    """What the reference alone says about the general branch in one case.  Per copy of the kernel that has lanes (COPIES names):
      beyond        lane-steps that start from a state outside the fast range
      mixed         (the two full copies) wave-steps of a full wave with lanes outside AND lanes inside the range
      ended         lane-steps that start outside the range and end an episode (done | truncated)
      actions       how many different actions were taken from states outside the range
      disagree      lane-steps outside the range on which two policies of the set, asked alone, choose differently
    and for the whole case
      nan_obs       lane-steps on which the policy reads a NaN observation
      final_kept    (F) lanes whose last ended episode ended on a step that started outside the range and whose final row is not zero"""
    w = np.ascontiguousarray(c.weights, np.float32).reshape(-1, ref.size_of(c.kind, c.hidden))
    after = np.concatenate([x.rec_obs for x in launches])  # [steps][D][n]; the observation is the state, re-armed lanes included
    start = np.concatenate([launches[0].start_state[None], after[:-1]])
    actions = np.concatenate([x.rec_actions for x in launches])
    ended = (np.concatenate([x.rec_done for x in launches]) | np.concatenate([x.rec_truncated for x in launches])) != 0
    beyond = lp.beyond_range(c.kind, start.transpose(1, 0, 2))  # [steps][n]
    disagree = np.zeros_like(beyond)
    for t, obs in enumerate(start):
        alone = [ref.policy_ref(c.kind, c.hidden, w[i:i + 1], 1, 0, obs) for i in range(len(w))]
        for x in alone[1:]:
            disagree[t] |= x != alone[0]
    per_wave = 64 * c.vec
    out = SimpleNamespace(copies={}, nan_obs=int(np.isnan(start).any(axis=1).sum()), final_kept=0)
    for copy in np.unique(c.classes):
        m = c.classes == copy
        b = beyond[:, m]
        f = SimpleNamespace(lanes=int(m.sum()), beyond=int(b.sum()), ended=int((b & ended[:, m]).sum()),
                            actions=len(np.unique(actions[:, m][b])), disagree=int((b & disagree[:, m]).sum()), mixed=None)
        if copy < 2:  # a full copy: its waves are whole
            waves = [beyond[:, first:first + per_wave] for first in range(0, c.n - per_wave + 1, per_wave) if m[first]]
            f.mixed = int(sum((x.any(axis=1) & ~x.all(axis=1)).sum() for x in waves))
        out.copies[COPIES[copy]] = f
    if c.flags & F:
        last = np.where(ended.any(axis=0), len(ended) - 1 - np.argmax(ended[::-1], axis=0), -1)  # the lane's last step that ended an episode
        lanes = np.flatnonzero(last >= 0)
        kept = (launches[-1].final[:, lanes] != 0).any(axis=0)  # (a NaN is not zero)
        out.final_kept = int((beyond[last[lanes], lanes] & kept).sum())
    return out


def rollout_missing(c, launches, found=None):
    """The conditions of SEEDS for one case and its reference; returns a list of what is missing (empty: all met)."""
    found = rollout_findings(c, launches) if found is None else found
    missing = []
    for name, f in found.copies.items():
        if f.beyond < 64:
            missing.append(f"{name}: {f.beyond} lane-steps beyond the range")
        if f.mixed is not None and f.mixed < 1:
            missing.append(f"{name}: no full wave mixes lanes beyond and inside the range")
        if f.ended < 1:
            missing.append(f"{name}: no episode ends from beyond the range")
        if f.actions < 2:
            missing.append(f"{name}: one action only beyond the range")
        if f.disagree < 1:
            missing.append(f"{name}: the policies never disagree beyond the range")
    if found.nan_obs < 1:
        missing.append("the policy never reads a NaN observation")
    if c.flags & F and found.final_kept < 1:
        missing.append("no final observation is kept from beyond the range")
    return missing


def first_rollout_seed(kind, hidden, shape, integrator=0, seeds=range(1, 64)):
    """How SEEDS were chosen"""
    for seed in seeds:
        ok = True
        for flags in flag_sets_of(kind, shape, hidden, integrator):
            c = rollout_case(kind, shape, flags, hidden, integrator, seed)
            if rollout_missing(c, ref.run_case(c)):
                ok = False
                break
        if ok:
            return seed
    return None


# ---- episodic evaluation -------------------------------------------------------------------------------------------------------------
EPISODES, EVAL_SEED = 2, ev.SEED
MAX_STEPS = {0: 120, 1: 40}
EVAL_GOAL = 120.0
# (n, global offset, lanes_per_policy): at 500 lanes per policy nearly every wave of 256 lanes is gathered; policy_eval_ref's first
# shape has uniform-full waves
EVAL_SHAPES = [(1300, 12345, 500), (ev.SHAPES[0][0], ev.SHAPES[0][2], ev.SHAPES[0][3])]
EVAL_HIDDEN = (0, 7)
# Seed of closed_loop_ref.make_weights per (kind, index into EVAL_SHAPES, hidden, integrator), common starts off and on alike: the first
# seed (first_eval_seed) with which eval_missing is empty.  CartPole's seed 1 with 7 hidden units ends no episode at the limit.
EVAL_SEEDS = {(0, 0, 0, 0): 1, (0, 0, 7, 0): 2, (0, 0, 7, 1): 2, (0, 1, 7, 0): 2, (1, 0, 0, 0): 1, (1, 0, 7, 0): 1, (1, 1, 7, 0): 1}


def eval_cases():
    """(kind, index into EVAL_SHAPES, hidden, common starts, integrator)"""
    return ([(kind, 0, hidden, common, 0) for kind in (0, 1) for hidden in EVAL_HIDDEN for common in (False, True)] + [(0, 0, 7, False, 1)] +
            [(kind, 1, 7, False, 0) for kind in (0, 1)])


def eval_row(kind, integrator=0):
    return wide_row(kind, MAX_STEPS[kind], EVAL_GOAL, integrator)


def eval_case(kind, shape, hidden, common, integrator=0, seed=None):
    n, gid0, lpp = EVAL_SHAPES[shape]
    seed = EVAL_SEEDS[kind, shape, hidden, integrator] if seed is None else seed
    return SimpleNamespace(kind=kind, n=n, gid0=gid0, row=eval_row(kind, integrator), default=lp.default_row(kind, MAX_STEPS[kind], integrator),
                           weights=ref.make_weights(kind, hidden, N_POLICIES, seed), hidden=hidden, lanes_per_policy=lpp, common=common,
                           episodes=EPISODES, max_steps=MAX_STEPS[kind], n_policies=N_POLICIES,
                           classes=ref.wave_classes(n, 4, gid0, N_POLICIES, lpp))


def run_eval(c, row=None):
    return ev.reference(c.kind, c.n, c.gid0, c.row if row is None else row, c.weights, c.hidden, c.lanes_per_policy, c.n_policies, EVAL_SEED,
                        c.episodes, c.max_steps, c.common)


def beyond_by_trip(c, r, row=None):
    """(beyond, parked), both bool [trips][n], of the evaluation kernel's loop: on trip t lane i takes a step that starts outside the
    fast range / is through with all its episodes.  A lane plays its episodes back to back, so step k of its episode e is trip
    (lengths of its earlier episodes) + k; r = the reference's result (its .starts, .length)."""
    from oracle.bindings import TwinEngine
    row = c.row if row is None else row
    w = np.ascontiguousarray(c.weights, np.float32).reshape(-1, ref.size_of(c.kind, c.hidden))
    tw = TwinEngine(lp.twin(), c.kind, c.n, row, flags=0, gid0=c.gid0)
    total = r.length.sum(axis=0)
    beyond = np.zeros((int(total.max()), c.n), bool)
    before = np.zeros(c.n, np.int64)
    lanes = np.arange(c.n)
    for e, st in enumerate(r.starts):
        tw.reset(0)
        tw.set_state(st)
        for k in range(int(r.length[e].max())):
            playing = k < r.length[e]
            out = lp.beyond_range(c.kind, tw.get_state()) & playing
            beyond[(before + k)[out], lanes[out]] = True
            tw.step(ref.policy_ref(c.kind, c.hidden, w, c.lanes_per_policy, c.gid0, tw.get_obs()))
        before += r.length[e]
    parked = np.arange(len(beyond))[:, None] >= total[None, :]
    return beyond, parked


def eval_findings(c, r, row=None):
    """beyond: lane-steps that start outside the fast range while the lane is playing (what policy_eval_table_ref.states_leave_the_fast_range
    counts: tests/test_closed_loop_slow_ref.py holds the two walks against each other); per copy: `beyond` lane-steps and `parked`, the largest number of trips
    on which one wave (256 lanes) holds a lane that is through with its episodes and a lane outside the range; lengths, done, truncated:
    distinct episode lengths, episodes ended by done, episodes that ran into the limit"""
    beyond, parked = beyond_by_trip(c, r, row)
    out = SimpleNamespace(beyond=int(beyond.sum()), lengths=len(np.unique(r.length)), done=int(r.done.sum()), truncated=int((r.length == c.max_steps).sum()), copies={})
    for copy in np.unique(c.classes):
        shared = [int((beyond[:, f:f + 256].any(axis=1) & parked[:, f:f + 256].any(axis=1)).sum()) for f in range(0, c.n, 256) if c.classes[f] == copy]
        out.copies[COPIES[copy]] = SimpleNamespace(lanes=int((c.classes == copy).sum()), beyond=int(beyond[:, c.classes == copy].sum()), parked=max(shared))
    return out


def eval_missing(c, r, r_default, found=None):
    found = eval_findings(c, r) if found is None else found
    missing = []
    if found.beyond <= c.n:
        missing.append(f"{found.beyond} lane-steps beyond the range")
    if found.lengths < 6:
        missing.append(f"{found.lengths} distinct episode lengths")
    if not found.done or not found.truncated:
        missing.append(f"{found.done} episodes end by done, {found.truncated} run into the limit")
    if not (r.records != r_default.records).any():
        missing.append("the default parameters give the same records")
    return missing


def first_eval_seed(kind, shape, hidden, integrator=0, seeds=range(1, 64)):
    for seed in seeds:
        ok = True
        for common in sorted({x[3] for x in eval_cases() if (x[0], x[1], x[2], x[4]) == (kind, shape, hidden, integrator)}):
            c = eval_case(kind, shape, hidden, common, integrator, seed)
            ok = ok and not eval_missing(c, run_eval(c), run_eval(c, c.default))
        if ok:
            return seed
    return None


# ---- evaluation under a table, MountainCar: the counterpart of policy_eval_table_ref.hard_push_rows ---------------------------------------
TABLE_INDEX_SEED = 41
TABLE_SEEDS = {0: 1, 7: 1}  # per hidden width, common starts off and on alike (first_table_seed)


def wide_rows():
    """Row 0 is the default; rows 1 and 2 are the wide track with the goal at 120 and at 250"""
    return [lp.default_row(1, MAX_STEPS[1]), wide_row(1, MAX_STEPS[1], EVAL_GOAL), wide_row(1, MAX_STEPS[1], 250.0)]


def table_cases():
    """(hidden, common starts)"""
    return [(0, False), (7, False), (7, True)]


def table_case(hidden, common, seed=None):
    n, gid0, lpp = EVAL_SHAPES[0]
    rows = wide_rows()
    seed = TABLE_SEEDS[hidden] if seed is None else seed
    return SimpleNamespace(kind=1, n=n, gid0=gid0, rows=rows, index=lp.make_index(n, len(rows), TABLE_INDEX_SEED),
                           weights=ref.make_weights(1, hidden, N_POLICIES, seed), hidden=hidden, lanes_per_policy=lpp, common=common,
                           episodes=EPISODES, max_steps=MAX_STEPS[1], n_policies=N_POLICIES, classes=ref.wave_classes(n, 4, gid0, N_POLICIES, lpp))


def run_table(c, index=None):
    return tb.reference(c.kind, c.n, c.gid0, c.rows, c.index if index is None else index, c.weights, c.hidden, c.lanes_per_policy, c.n_policies,
                        EVAL_SEED, c.episodes, c.max_steps, c.common)


def table_findings(c, r):
    """Per row: (lanes on the row, lane-steps of those lanes that start outside the range)"""
    out = []
    for k, row in enumerate(c.rows):
        m = c.index == k
        out.append((int(m.sum()), tb.states_leave_the_fast_range(c.kind, c.n, c.gid0, row, c.weights, c.hidden, c.lanes_per_policy, r.starts,
                                                                 c.max_steps, lanes=m)))
    return out


def table_missing(c, r, r0, found=None):
    """r0 = run_table(c, every lane on row 0)"""
    found = table_findings(c, r) if found is None else found
    missing = []
    if found[0][1] != 0:
        missing.append(f"the default row's lanes leave the range ({found[0][1]} lane-steps)")
    for k, (lanes, beyond) in enumerate(found[1:], 1):
        if beyond <= lanes:
            missing.append(f"row {k}: {beyond} lane-steps beyond the range on {lanes} lanes")
    if len(np.unique(r.length)) < 6:
        missing.append("fewer than 6 distinct episode lengths")
    if not r.done.any() or not (r.length == c.max_steps).any():
        missing.append("done and truncated episodes do not both occur")
    if not (r.records != r0.records).any():
        missing.append("with every lane on the default row the records are the same")
    if not any(len(np.unique(c.index[f:f + 256])) == len(c.rows) for f in range(0, c.n, 256)):
        missing.append("no wave holds all three rows")
    return missing


def first_table_seed(hidden, seeds=range(1, 64)):
    for seed in seeds:
        ok = True
        for common in sorted({x[1] for x in table_cases() if x[0] == hidden}):
            c = table_case(hidden, common, seed)
            ok = ok and not table_missing(c, run_table(c), run_table(c, np.zeros(c.n, np.int64)))
        if ok:
            return seed
    return None


# ---- parked lanes: a lane through with its episodes next to lanes that go on playing outside the range --------------------------------
PARKED_N, PARKED_GID0 = 700, 12345  # two full waves and a ragged one; one lane per policy: every wave gathers


def parked_case(kind):
    """Two affine policies alternate lane by lane (lanes_per_policy = 1).  MountainCar on the wide track, goal at 120: policy 0 always
    pushes right and is at the goal within a dozen steps, policy 1 always pushes left and runs down the track to the limit.
    CartPole with 10 times the default force, |x| <= 1 and |theta| <= 4: policy 0 always pushes right and drives the cart off the
    track in 6 or 7 steps; policy 1 pushes against 5 x + x_dot, which keeps the cart near the middle while the pole falls and swings
    through the bottom: its episodes last 82 to 120 steps, three in ten run into the limit of 120 and the others end at 4 rad, so how
    long they last is decided outside |theta| <= pi / 4.  (Against x_dot alone the cart drifts off the track after some 30 steps.)"""
    d, a = ref.DIMS[kind]
    w = np.zeros((2, ref.size_of(kind, 0)), np.float32)  # [A][D] weights, then [A] biases
    if kind == 0:
        row = lp.default_row(0, MAX_STEPS[0])
        row.force_mag *= 10.0
        row.x_threshold = 1.0
        row.theta_threshold_radians = 4.0
        w[0, a * d + 1] = 1.0
        w[1, 0 * d:0 * d + 2], w[1, 1 * d:1 * d + 2] = (5.0, 1.0), (-5.0, -1.0)
    else:
        row = eval_row(1)
        w[0, a * d + 2] = 1.0
        w[1, a * d + 0] = 1.0
    return SimpleNamespace(kind=kind, n=PARKED_N, gid0=PARKED_GID0, row=row, default=lp.default_row(kind, MAX_STEPS[kind]), weights=w, hidden=0,
                           lanes_per_policy=1, common=False, episodes=EPISODES, max_steps=MAX_STEPS[kind], n_policies=2,
                           classes=ref.wave_classes(PARKED_N, 4, PARKED_GID0, 2, 1))


# ---- the sharded cases -------------------------------------------------------------------------------------------------------------------
SHARDED_SHAPE, SHARDED_FLAGS, SHARDED_SEED = 1, A | S | T | F, 1


def sharded_rollout_case(kind):
    """One rollout case per env for the sharded handle: CartPole on the wide row (the matrix plays the hard-push row), MountainCar as in
    the matrix; closed_loop_ref's second shape, every flag, 7 hidden units"""
    c = rollout_case(kind, SHARDED_SHAPE, SHARDED_FLAGS, HIDDEN, seed=SHARDED_SEED)
    if kind == 0:
        c.params = wide_row(0, ref.MAX_EPISODE_STEPS)
    return c
