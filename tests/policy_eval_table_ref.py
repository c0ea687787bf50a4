"""gymrs_evaluate_policy with GYMRS_EVAL_LANE_PARAMS on an engine with a parameter table (include/gymrs_amd.h, "episodic policy
evaluation" and "per-lane physics"), computed on the CPU alone from policy_eval_ref and lane_params_ref.

Lanes are independent and the start states do not depend on the physics fields, so lane i of a table engine plays the episodes lane
i plays on a uniform engine whose params are rows[index[i]]: for every row r that some lane uses, policy_eval_ref.play runs all the
lanes with row r's params, and lane i's episodes are taken from the run of index[i].  A lane whose index is not in the table plays
nothing: it is left out of the records, and its entries of the `lengths` buffer are never written.

This module never imports the library: what it returns is the yardstick of tests/test_gpu_policy_eval_table.py, and
tests/test_policy_eval_table_ref.py shows without a GPU that its cases are worth comparing with.

A plain module, imported by test files; no fixtures, no pytest hooks."""
from types import SimpleNamespace

import closed_loop_ref as ref
import lane_params_ref as lp
import numpy as np
import policy_eval_ref as ev
import policy_fitness_ref as fit

EPISODES, MAX_STEPS, N_POLICIES, SEED, HIDDEN, SHAPES = ev.EPISODES, ev.MAX_STEPS, ev.N_POLICIES, ev.SEED, ev.HIDDEN, ev.SHAPES
K = 5


def reference(kind, n, gid0, rows, index, weights, hidden, lanes_per_policy, n_policies, seed, episodes, max_steps, common=False):
    """What the call leaves: .records (n_policies, 8) int64; .length / .done [E][n] and .lengths uint32 [E][n] (meaningless where
    .valid [n] is False: the lanes whose index is not in the table); .pol [n]"""
    index = np.asarray(index, np.int64)
    assert index.shape == (n,) and index.min() >= 0
    valid = index < len(rows)
    starts = ev.start_states(kind, n, gid0, rows[0], seed, episodes, lanes_per_policy, common)  # (independent of the row)
    length = np.zeros((episodes, n), np.int64)
    done = np.zeros((episodes, n), bool)
    for r in np.unique(index[valid]):
        ln, dn = ev.play(kind, n, gid0, rows[r], weights, hidden, lanes_per_policy, starts, max_steps)
        m = index == r
        length[:, m] = ln[:, m]
        done[:, m] = dn[:, m]
    pol = fit.policies_of(n, gid0, lanes_per_policy, n_policies)
    pol_played = np.where(valid, pol, -1)  # (no record counts a lane that plays nothing)
    return SimpleNamespace(records=ev.records(kind, length, done, pol_played, n_policies, max_steps), lengths=ev.packed(length, done),
                           length=length, done=done, pol=pol, valid=valid, starts=starts)


# ---- the cases of tests/test_gpu_policy_eval_table.py (checked without a GPU by tests/test_policy_eval_table_ref.py) --------------
# Seeds of closed_loop_ref.make_weights per (kind, hidden, index into SHAPES) and of lane_params_ref.make_rows / make_index per kind,
# common starts off and on alike: searched with this module alone (search_seeds) for cases that meet worth_comparing.
WEIGHT_SEEDS = dict(ev.WEIGHT_SEEDS)
ROWS_SEED = {0: 31, 1: 32}
INDEX_SEED = {0: 32, 1: 33}


def cases():
    return ev.cases()


def case(kind, shape, hidden, common, weight_seed=None, rows_seed=None, index_seed=None, integrator=0):
    """One case: rows are lane_params_ref rows (CartPoleRow / MountainCarRow; lane_params_ref.rows_for gives the engine's type)"""
    n, vec, gid0, lpp = SHAPES[shape]
    rows = lp.make_rows(kind, K, ROWS_SEED[kind] if rows_seed is None else rows_seed, MAX_STEPS, integrator)
    assert kind == 0 or lp.low_goal_rows(kind, rows)  # MountainCar's default goal ends no episode in MAX_STEPS steps
    index = lp.make_index(n, K, INDEX_SEED[kind] if index_seed is None else index_seed)
    seed = WEIGHT_SEEDS[kind, hidden, shape] if weight_seed is None else weight_seed
    return SimpleNamespace(kind=kind, n=n, gid0=gid0, rows=rows, index=index, weights=ref.make_weights(kind, hidden, N_POLICIES, seed),
                           hidden=hidden, lanes_per_policy=lpp, common=common, classes=ref.wave_classes(n, 4, gid0, N_POLICIES, lpp))


def run_case(c, index=None):
    return reference(c.kind, c.n, c.gid0, c.rows, c.index if index is None else index, c.weights, c.hidden, c.lanes_per_policy, N_POLICIES, SEED,
                     EPISODES, MAX_STEPS, c.common)


def worth_comparing(c, r, r0):
    """What a case must show to be worth a GPU comparison; r = run_case(c), r0 = run_case(c, index = every lane on row 0).
    Returns a list of what is missing (empty: all met)."""
    missing = list(ev.worth_comparing(c, r))
    for copy in np.unique(c.classes):
        m = c.classes == copy
        if not (r.length[:, m] != r0.length[:, m]).any():
            missing.append(f"{ref.COPIES[copy]}: with every lane on row 0 all lengths are the same")
    for p in range(N_POLICIES):
        if (r.pol == p).any() and not (r.records[p] != r0.records[p]).any():
            missing.append(f"policy {p}: with every lane on row 0 its record is the same")
    if not any(len(np.unique(c.index[f:f + 256])) >= 2 for f in range(0, c.n, 256)):
        missing.append("no wave mixes two rows")
    return missing


def search_seeds(kind, hidden, shape, weight_seeds=range(1, 64), rows_seed=None, index_seed=None):
    """The first weight seed with which the case, common starts off and on, meets worth_comparing (how WEIGHT_SEEDS were chosen)"""
    for ws in weight_seeds:
        ok = True
        for common in (False, True):
            c = case(kind, shape, hidden, common, ws, rows_seed, index_seed)
            ok = ok and not worth_comparing(c, run_case(c), run_case(c, np.zeros(c.n, np.int64)))
        if ok:
            return ws
    return None


# ---- the cases beside the matrix ---------------------------------------------------------------------------------------------------
def hard_push_rows(max_steps=MAX_STEPS):
    """CartPole rows for the general path: row 1 pushes with 40 times the default force and, like row 2, ends an episode only far
    beyond the fast path's range of |theta| <= pi / 4, so its lanes go on playing out there; row 0 is the default."""
    rows = [lp.default_row(0, max_steps) for _ in range(3)]
    rows[1].force_mag *= 40.0
    rows[1].theta_threshold_radians = 50.0
    rows[1].x_threshold = 1.0e6
    rows[2].theta_threshold_radians = 2.0
    return rows


def states_leave_the_fast_range(kind, n, gid0, row, weights, hidden, lanes_per_policy, starts, max_steps, lanes=None):
    """How many lane-steps of play(...) with `row` start from a state outside the fast path's range while the lane is still playing
    (`lanes`: a boolean mask of the lanes to count, default all)"""
    from oracle.bindings import TwinEngine
    w = np.ascontiguousarray(weights, np.float32).reshape(-1, ref.size_of(kind, hidden))
    tw = TwinEngine(lp.twin(), kind, n, row, flags=0, gid0=gid0)
    count = 0
    for st in starts:
        tw.reset(0)
        tw.set_state(st)
        playing = np.ones(n, bool) if lanes is None else np.array(lanes, bool)
        for k in range(1, max_steps + 1):
            count += int((lp.beyond_range(kind, tw.get_state()) & playing).sum())
            tw.step(ref.policy_ref(kind, hidden, w, lanes_per_policy, gid0, tw.get_obs()))
            playing &= ~(np.asarray(tw.get_result()[1]) != 0)
            if not playing.any():
                break
    return count
