"""The CPU reference of gymrs_rollout_transitions: the per-step loop of tests/explore_ref.py (itself lane_params_ref.TableReference
driven by the policy of closed_loop_ref and the numpy Philox draw), one step at a time, keeping after every step the value that
loop computes with closed_loop_ref.final_obs_after and then overwrites: the observation every ended lane showed before its
re-arm.  Nothing of those modules is changed; this one never loads the library.

A plain module, imported by test files; no fixtures, no pytest hooks."""
from types import SimpleNamespace

import closed_loop_ref as cl
import closed_loop_table_ref as clt
import explore_ref as ex
import lane_params_ref as lp
import numpy as np
import policy_fitness_ref as pf
from closed_loop_ref import A, COPIES, DIMS, F, S, T, bits  # noqa: F401  (re-exported to the test files)

FLAG_SETS = [f for f in cl.FLAG_SETS if f & A]  # the eight the transition kernels are built for
SHAPES = cl.SHAPES[:2]  # 4200 and 5000 lanes at 4 lanes per work-item: between them all four kernel copies
SCHEDULE = clt.SCHEDULE  # (1, 7, 40, 4): the totals are no multiple of the 17-step limit (closed_loop_table_ref says why)
HIDDEN = cl.RECORD_HIDDEN
K = lp.K  # rows of the table
THRESHOLD = ex.THRESHOLD
SEED = ex.SEED
SENTINEL = 0x7FC0BEEF  # the NaN bit pattern the buffers are pre-filled with
# Seed of make_weights per (kind, hidden, shape, table, explore): closed_loop_table_ref.seed_of unless an entry here replaces it --
# the next seed, searched with this module alone, for which worth_comparing holds (tests/test_transitions_ref.py asserts it).
SEEDS = {(0, 8, 0, False, False): 11, (0, 8, 1, False, False): 11, (0, 8, 0, False, True): 3, (0, 8, 0, True, True): 3, (0, 8, 0, True, False): 3,
         (0, 8, 1, True, False): 3, (0, 0, 0, True, False): 17, (1, 8, 0, True, False): 4, (1, 8, 0, True, True): 4}


def seed_of(kind, hidden, shape, table, explore):
    return SEEDS.get((kind, hidden, shape, table, explore), clt.seed_of(kind, hidden, shape))


def case(kind, shape, flags, hidden, table, explore, bounds=None):
    n, vec, gid0, lpp = SHAPES[shape]
    assert vec == 4 and flags & A
    k = K if table else 1
    rows = lp.make_rows(kind, k, lp.ROWS_SEED + kind, cl.MAX_EPISODE_STEPS) if table else [lp.default_row(kind, cl.MAX_EPISODE_STEPS)]
    index = lp.make_index(n, k, lp.INDEX_SEED + kind) if table else np.zeros(n, np.uint16)
    w = cl.make_weights(kind, hidden, cl.N_POLICIES, seed_of(kind, hidden, shape, table, explore))
    prepare = (lambda state: cl.mountain_car_prepare(state, 0)) if kind == 1 else None
    classes = cl.wave_classes(n, 4, gid0, cl.N_POLICIES, lpp)
    return SimpleNamespace(kind=kind, n=n, vec=4, gid0=gid0, flags=flags, table=table, explore=explore, rows=rows, index=index, weights=w,
                           hidden=hidden, n_policies=cl.N_POLICIES, lanes_per_policy=lpp, reset_seed=cl.RESET_SEED, schedule=SCHEDULE,
                           prepare=prepare, bounds=bounds, seed=SEED, threshold=THRESHOLD, policies=pf.policies_of(n, gid0, lpp, cl.N_POLICIES),
                           classes={4: classes, 8: classes})


def matrix():
    """[(kind, table, flag set, shape, hidden, explore)]: every kernel family (env x table) under every flag set once; shape, hidden
    layer and exploration take turns inside a family, so each value of each meets every family"""
    out = []
    for kind in (0, 1):
        for table in (False, True):
            for f, flags in enumerate(FLAG_SETS):
                out.append((kind, table, flags, (f + kind) % 2, HIDDEN[(f // 2 + table) % 2], bool((f // 4 + kind + table) % 2)))
    return out


class Run:
    """explore_ref.Run stepped one step at a time.  launch(steps) returns what explore_ref.Run.launch returns for the whole launch,
    and with it final_obs [steps][D][n] (valid where ended), ended [steps][n] (bool) and start_obs [D][n]."""

    def __init__(self, c, tick0=1):
        self.c = c
        self.run = ex.Run(c, tick0=tick0)
        self.start_state = self.run.start_state

    def launch(self, steps, explore=None):
        explore = ((self.c.seed, self.c.threshold) if self.c.explore else None) if explore is None else explore
        start = self.run.ref.obs.copy()
        parts, finals = [], []
        for _ in range(steps):
            parts.append(self.run.launch(1, explore))
            finals.append(parts[-1].final)  # TableReference has just written the ended lanes of THIS step
        last = parts[-1]
        for f in ("rec_obs", "rec_actions", "rec_reward", "rec_done", "rec_truncated"):
            setattr(last, f, np.concatenate([getattr(p, f) for p in parts]))
        last.ended = (last.rec_done | last.rec_truncated) != 0
        last.final_obs = np.stack(finals)
        last.start_obs = start
        return last


def run_case(c, tick0=1):
    run = Run(c, tick0)
    out = [run.launch(steps) for steps in c.schedule]
    out[0].start_state = run.start_state
    return out


def worth_comparing(c, out):
    """What is missing for the case to show anything (empty: nothing): inside the lanes of every kernel copy present an episode
    ends by done, one by truncation (sets with T), one lane ends two episodes inside ONE launch (the engine's own array keeps one),
    and on every ended lane-step the final observation differs bitwise from the recorded (re-armed) one.  MountainCar without the
    time limit is spared the two-episodes condition: a re-armed lane starts from a reset draw in the valley and no policy brings it
    to the goal in under 80 steps, so inside a launch of at most 40 steps it can end once, from its prepared start, and no more."""
    missing = []
    classes = c.classes[4]
    for copy in np.unique(classes):
        m = classes == copy
        name = COPIES[copy]
        if not any(x.rec_done[:, m].any() for x in out):
            missing.append(f"{name}: no episode ended by done")
        if c.flags & T and not any(x.rec_truncated[:, m].any() for x in out):
            missing.append(f"{name}: no episode ended by truncation")
        if (c.kind == 0 or c.flags & T) and not any((x.ended[:, m].sum(axis=0) >= 2).any() for x in out):
            missing.append(f"{name}: no lane ends two episodes inside one launch")
    for k, x in enumerate(out):
        if ((bits(x.final_obs) == bits(x.rec_obs)).all(axis=1) & x.ended).any():
            missing.append(f"launch {k}: a final observation equals the re-armed one")
    return missing
