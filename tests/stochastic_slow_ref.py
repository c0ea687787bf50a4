"""The cases that take the exploring, sampling and transitions kernels off the fast physics path, computed on the CPU alone.

Every kernel that steps lanes has a wave-uniform branch-free physics branch and a per-lane general one; a wave takes the general one
if it is ragged or if any of its lanes is outside Env::kRangeMax (gym-rs_amd/csrc/gymrs_tile.h; lane_params_ref.beyond_range restates
it).  The matrices of explore_ref, sample_ref and transitions_ref start from reset() under default thresholds and never leave the
range.  The cases here are theirs with two attributes replaced: `rows` -- parameter rows whose episodes end only far outside the range
(closed_loop_slow_ref.rollout_row; under a table the default row, that row and closed_loop_slow_ref.wide_row take turns) -- and
`prepare` = lane_params_ref.slow_prepare(kind): angles up to 1e30, NaN and +-inf on every 7th lane.

The references are explore_ref.Run, sample_ref.Run, transitions_ref.Run and sample_ref.TransitionsRun, unchanged: they read the case's
rows and prepare as they are, and the f32 twin, tests/cpp/policy_ref.c and tests/cpp/sample_ref.c already run the general arithmetic.
What this module adds is the cases and the figures that show, from the reference alone, that they go there (findings, missing,
nan_shares).  It never imports the library: what it returns is the yardstick of tests/test_gpu_stochastic_slowpaths.py, and
tests/test_stochastic_slow_ref.py asserts the conditions without a GPU.

A plain module like closed_loop_slow_ref.py, imported by test files; no fixtures, no pytest hooks."""
from types import SimpleNamespace

import closed_loop_ref as cl
import closed_loop_slow_ref as sl
import explore_ref as ex
import lane_params_ref as lp
import numpy as np
import sample_ref as sm
import transitions_ref as tr
from closed_loop_ref import A, COPIES, DIMS, F, S, T, bits  # noqa: F401  (re-exported to the test files)

FULL = A | S | T | F
MAX_EPISODE_STEPS = cl.MAX_EPISODE_STEPS
assert ex.MAX_EPISODE_STEPS == MAX_EPISODE_STEPS  # closed_loop_slow_ref.rollout_row is built with closed_loop_ref's limit
TABLE_GOAL = 120.0  # MountainCar's second wide row; the first has closed_loop_slow_ref.ROLLOUT_GOAL = 300
SOURCES = ("greedy", "explore", "sample")  # where the action of a step comes from
ENGINES = (("fused", 4), ("fitness", 4), ("record", 4), ("fused", 8), ("fitness", 8))  # the engines of one explore / sample case
NAN_CAP = 0.1  # the largest share of NaN elements a compared float array of a reference may hold


# ---- the two attributes ----------------------------------------------------------------------------------------------------------------
def slow_rows(kind, k, table, integrator=0):
    """Without a table the one hard row; with one, k rows that cycle through the default row, the hard row and the wide row (CartPole:
    theta up to 2 rad; MountainCar: the goal at 120 instead of 300).  max_episode_steps and kinematics_integrator are shared."""
    make = (lambda: lp.default_row(kind, MAX_EPISODE_STEPS, integrator), lambda: sl.rollout_row(kind, integrator),
            lambda: sl.wide_row(kind, MAX_EPISODE_STEPS, TABLE_GOAL, integrator))
    if not table:
        return [make[1]()]
    return [make[r % 3]() for r in range(k)]


def slowed(c, source, integrator=0):
    c.rows = slow_rows(c.kind, len(c.rows), c.table, integrator)
    c.prepare = lp.slow_prepare(c.kind)
    c.source, c.integrator = source, integrator
    return c


# ---- exploring and sampling: explore_ref's matrix and axes, and CartPole's second integrator ---------------------------------------------
# (kind, flag set, table, case number of explore_ref.axes, integrator).  The two extra cases play CartPole with
# kinematics_integrator = 1 under every flag, once without and once with a table; a case runs all of ENGINES, so each kernel family
# meets the integrator at each vector width.  Case numbers 13 and 22: offset 6, whole waves uniform, H = 8 in one launch and H = 0 in three.
INTEGRATOR_1 = [(0, FULL, False, 13, 1), (0, FULL, True, 22, 1)]
# Seed of closed_loop_ref.make_weights per (source, kind, flag set, table, case number, integrator): explore_ref.WEIGHTS_SEED unless an
# entry here replaces it -- the first seed from 1 upwards (first_seed, searched with this module alone) with which `missing` is empty.
# What the replaced seed misses is, in all but one entry, the ragged wave of twenty lanes at 4 lanes per work-item: fewer than 64
# lane-steps beyond the range there, or none explored or sampled away.  tests/test_stochastic_slow_ref.py asserts that every entry
# replaces a seed that does miss a condition and that the search gives the entry back.
SEEDS = {("explore", 1, A | T, True, 29, 0): 1, ("explore", 1, A | F, False, 32, 0): 1, ("sample", 0, 0, False, 0, 0): 1, ("sample", 0, A, False, 2, 0): 1,
         ("sample", 0, FULL, False, 18, 0): 1, ("sample", 0, FULL, True, 19, 0): 4, ("sample", 1, 0, False, 20, 0): 1, ("sample", 1, A | T, False, 28, 0): 1,
         ("sample", 1, A | F, False, 32, 0): 1, ("sample", 1, A | T | F, False, 36, 0): 1, ("sample", 1, A | T | F, True, 37, 0): 1,
         ("sample", 1, FULL, False, 38, 0): 1}


def matrix():
    return [(kind, flags, table, i, 0) for kind, flags, table, i in ex.matrix()] + INTEGRATOR_1


def case(source, kind, flags, table, i, integrator=0, seed=None):
    """explore_ref.matrix_case / sample_ref.matrix_case of the same arguments, slowed"""
    assert source in SOURCES[1:]
    c = (ex if source == "explore" else sm).matrix_case(kind, flags, table, i)
    seed = SEEDS.get((source, kind, flags, table, i, integrator), ex.WEIGHTS_SEED) if seed is None else seed
    c.weights = cl.make_weights(kind, c.hidden, c.n_policies, seed)
    c.weights_seed = seed
    return slowed(c, source, integrator)


def plain_case(source, kind, flags, table, gid0, policy_set, hidden, schedule, integrator=0):
    """A case beside the matrix (the per-step and the sharded comparisons)"""
    c = (ex if source == "explore" else sm).case(kind, flags, table, gid0, policy_set, hidden, schedule)
    return slowed(c, source, integrator)


def run_case(c):
    return (ex if c.source == "explore" else sm).run_case(c)


# ---- the per-step kernels and the sharded handle ------------------------------------------------------------------------------------------
def per_step_cases():
    """(source, kind, table, global offset, policy set, hidden, lanes per work-item): one per env x table x source; offset, policy set,
    hidden layer and vector width take turns"""
    out = []
    for s, source in enumerate(SOURCES[1:]):
        for kind in (0, 1):
            for t, table in enumerate((False, True)):
                j = s + kind + t
                out.append((source, kind, table, ex.OFFSETS[j % 3], ex.POLICY_SETS[(j + 1) % 3], ex.HIDDEN[(kind + t) % 2], (4, 8)[(s + t) % 2]))
    return out


def per_step_case(source, kind, table, gid0, policy_set, hidden):
    return plain_case(source, kind, FULL, table, gid0, policy_set, hidden, ex.SPLITS[1])


def sharded_case(source, kind):
    """The sharded tests' case of test_gpu_explore.py / test_gpu_sample.py (offset 6: the first block takes the per-lane block path), slowed"""
    return plain_case(source, kind, FULL, True, 6, (3, 512), 8, ex.SPLITS[1])


# ---- transitions ------------------------------------------------------------------------------------------------------------------------------
# Seed of make_weights per (kind, table, flag set): transitions_ref.seed_of unless an entry here replaces it (first_seed).
# MountainCar under a table with A | S | T (sampling, 4200 lanes): seed 3 leaves 43 lane-steps beyond the range in the ragged wave.
TRANSITIONS_SEEDS = {(1, True, A | S | T): 1}


def transitions_matrix():
    """[(kind, table, flag set, shape, hidden, source)]: every kernel family (env x table) under each of the eight flag sets once.  The
    source is flag set number + kind + table modulo 3, so each source meets every family; inside a family the flag sets of one source
    are three (or two) apart, and the shape changes every third flag set: every source meets both shapes -- all four kernel copies --
    in every family.  The hidden layer alternates."""
    out = []
    for kind in (0, 1):
        for table in (False, True):
            for f, flags in enumerate(tr.FLAG_SETS):
                out.append((kind, table, flags, (f // 3 + kind) % 2, tr.HIDDEN[(f + table) % 2], SOURCES[(f + kind + table) % 3]))
    return out


def transitions_case(kind, table, flags, shape, hidden, source, seed=None):
    c = tr.case(kind, shape, flags, hidden, table, source == "explore")
    seed = TRANSITIONS_SEEDS.get((kind, table, flags), tr.seed_of(kind, hidden, shape, table, source == "explore")) if seed is None else seed
    c.weights = cl.make_weights(kind, hidden, cl.N_POLICIES, seed)
    c.weights_seed = seed
    if source == "sample":
        c.seed, c.scale = sm.SEED, sm.SCALE
    return slowed(c, source)


def run_transitions(c):
    run = sm.TransitionsRun(c) if c.source == "sample" else tr.Run(c)
    out = [run.launch(steps) for steps in c.schedule]
    out[0].start_state = run.start_state
    return out


# ---- what the reference says about the general branch --------------------------------------------------------------------------------------------
def walk(c, launches):
    """start [steps][D][n] (the state every step starts from: the observation is the state, re-armed lanes included), beyond, actions,
    greedy, ended [steps][n].  greedy is closed_loop_ref.policy_ref on the start observations, whatever the source of the action."""
    after = np.concatenate([x.rec_obs for x in launches])
    start = np.concatenate([launches[0].start_state[None], after[:-1]])
    actions = np.concatenate([x.rec_actions for x in launches])
    ended = (np.concatenate([x.rec_done for x in launches]) | np.concatenate([x.rec_truncated for x in launches])) != 0
    greedy = np.stack([cl.policy_ref(c.kind, c.hidden, c.weights, c.lanes_per_policy, c.gid0, obs) for obs in start])
    return SimpleNamespace(start=start, beyond=lp.beyond_range(c.kind, start.transpose(1, 0, 2)), actions=actions, greedy=greedy, ended=ended)


def vecs_of(c):
    """The lanes per work-item a case's kernels exist at: the transitions kernels (transitions_ref.case sets `vec`) at 4 only"""
    return (4,) if hasattr(c, "vec") else (4, 8)


def findings(c, launches, vecs=None):
    """Per lanes per work-item in `vecs` (default vecs_of(c)) and per copy of the kernel that has lanes there (COPIES names), .copies[vec][name]:
      lanes         how many lanes the copy steps
      beyond        lane-steps that start from a state outside the fast range
      mixed         (the two full copies) wave-steps of a full wave with lanes outside AND lanes inside the range
      ended         lane-steps that start outside the range and end an episode (done | truncated)
      away          lane-steps outside the range on which the action taken is not the greedy one (explored or sampled away)
      actions       how many different actions were taken from states outside the range
      rows          the table rows that own lanes with a step outside the range
    and, transitions (launches that have final_obs) only,
      final_nan     of the `ended` lane-steps, those whose final observation holds a NaN
    For the whole case: nan_obs, the lane-steps on which the policy reads a NaN observation."""
    w = walk(c, launches)
    final_nan = None
    if hasattr(launches[0], "final_obs"):
        final_nan = np.isnan(np.concatenate([x.final_obs for x in launches])).any(axis=1)
    out = SimpleNamespace(copies={}, nan_obs=int(np.isnan(w.start).any(axis=1).sum()))
    index = np.asarray(c.index, np.int64)
    for vec in vecs_of(c) if vecs is None else vecs:
        classes, per_wave = c.classes[vec], 64 * vec
        out.copies[vec] = {}
        for copy in np.unique(classes):
            m = classes == copy
            b = w.beyond[:, m]
            f = SimpleNamespace(lanes=int(m.sum()), beyond=int(b.sum()), ended=int((b & w.ended[:, m]).sum()),
                                away=int((b & (w.actions[:, m] != w.greedy[:, m])).sum()), actions=len(np.unique(w.actions[:, m][b])),
                                rows=sorted(set(index[m][b.any(axis=0)].tolist())), mixed=None, final_nan=None)
            if copy < 2:  # a full copy: its waves are whole
                waves = [w.beyond[:, first:first + per_wave] for first in range(0, c.n - per_wave + 1, per_wave) if m[first]]
                f.mixed = int(sum((x.any(axis=1) & ~x.all(axis=1)).sum() for x in waves))
            if final_nan is not None:
                f.final_nan = int((b & w.ended[:, m] & final_nan[:, m]).sum())
            out.copies[vec][COPIES[copy]] = f
    return out


def missing(c, found):
    """The conditions of a case; returns a list of what is missing (empty: all met).  A greedy launch cannot take an action other
    than the greedy one, so `away` is asked of the exploring and sampling cases only."""
    out = []
    for vec, copies in found.copies.items():
        for name, f in copies.items():
            at = f"{vec} lanes per work-item, {name}"
            if f.beyond < 64:
                out.append(f"{at}: {f.beyond} lane-steps beyond the range")
            if f.mixed is not None and f.mixed < 1:
                out.append(f"{at}: no full wave mixes lanes beyond and inside the range")
            if f.ended < 1:
                out.append(f"{at}: no episode ends from beyond the range")
            if f.actions < 2:
                out.append(f"{at}: one action only beyond the range")
            if c.source != "greedy" and f.away < 1:
                out.append(f"{at}: no action beyond the range differs from the greedy one")
    if found.nan_obs < 1:
        out.append("the policy never reads a NaN observation")
    return out


def transitions_missing(c, found):
    """`missing`, and what the FinalObsRows sink is there for.  (`ended` >= 1 in every copy, asked by `missing`, is a final observation
    kept from a step that started beyond the range: the reference keeps one on every ended lane-step.)"""
    out = missing(c, found)
    copies = found.copies[4]
    owned = set().union(*(f.rows for f in copies.values()))
    if owned != set(range(len(c.rows))):
        out.append(f"rows {sorted(set(range(len(c.rows))) - owned)} own no lane beyond the range")
    if c.kind == 0 and sum(f.final_nan for f in copies.values()) < 1:
        out.append("no kept final observation is NaN")
    return out


def nan_shares(c, launches):
    """{array name: the largest share of NaN elements in one launch's compared float array}.  final_obs (transitions) is compared
    whole: the elements of ended lane-steps with the reference under the NaN rule, every other one exactly with the sentinel the buffer
    was filled with, so the reference's NaNs are those of the ended lane-steps and the share is taken over the whole array.  (Among
    the ended lane-steps alone the share is larger -- findings' final_nan / ended -- up to one in five in a launch of one step from
    the planted states, where little else ends.)"""
    out = {}
    names = ["state", "obs", "reward", "rec_obs", "rec_reward"] + (["final"] if c.flags & F else []) + (["prob"] if hasattr(launches[0], "prob") else [])
    for x in launches:
        for name in names:
            a = getattr(x, name)
            out[name] = max(out.get(name, 0.0), float(np.isnan(a).mean()))
        if hasattr(x, "final_obs"):
            kept = np.isnan(x.final_obs) & x.ended[:, None, :]
            out["final_obs"] = max(out.get("final_obs", 0.0), float(kept.mean()))
        if hasattr(x, "start_obs"):
            out["start_obs"] = max(out.get("start_obs", 0.0), float(np.isnan(x.start_obs).mean()))
    return out


def first_seed(make, run, check, seeds=range(1, 64)):
    """How SEEDS and TRANSITIONS_SEEDS entries are chosen: make(seed) -> case, run(case) -> launches, check(case, found) -> missing"""
    for seed in seeds:
        c = make(seed)
        if not check(c, findings(c, run(c), vecs_of(c))):
            return seed
    return None
