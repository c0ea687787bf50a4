"""The cases of tests/closed_loop_slow_ref.py, checked without a GPU: from the CPU reference alone, every one of them sends the
closed-loop and evaluation kernels through the general, per-lane physics branch in a way a wrong branch could not survive.  These are
conditions, not measurements: a case that misses one is replaced.

Rollouts (fused, recording and fitness kernels), inside the lanes of every kernel copy that has lanes, under every flag set, over the 51
steps: at least 64 lane-steps start outside the fast range; a full wave mixes lanes outside and inside; an episode ends on a step that
started outside; two different actions are taken out there and two policies of the set disagree there; the policy reads a NaN
observation; with F a final observation is kept from a step that started outside.  Evaluation: more lane-steps outside the range than
lanes, at least 6 distinct episode lengths, episodes that end by done and episodes that run into the limit, records that differ from
those under default parameters.  Under a table: more such lane-steps than lanes on each wide row, none on the default row.  Parked
lanes: a lane through with its episodes shares a wave with a lane outside the range for at least 10 trips of the kernel's loop."""
from functools import lru_cache

import closed_loop_ref as ref
import closed_loop_slow_ref as sl
import lane_params_ref as lp
import numpy as np
import policy_eval_table_ref as tb
import pytest
from closed_loop_ref import A, F, S, T

ROLLOUT_KEYS = sorted(sl.SEEDS)  # (kind, hidden, index into SHAPES, integrator)


# ---- the start states and the rows -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1])
def test_slow_start_follows_the_batch_not_the_engine(kind):
    d = ref.DIMS[kind][0]
    base = np.random.default_rng(5).uniform(-0.05, 0.05, (d, 300)).astype(np.float32)
    whole = sl.slow_start(kind)(base, 0)
    assert np.array_equal(ref.bits(whole), ref.bits(lp.slow_prepare(kind)(base)))  # at offset 0 it is slow_prepare itself
    for first in (0, 1, 3, 4, 6, 7, 33, 104, 105):
        part = sl.slow_start(kind)(base[:, first:], first)
        assert part.flags["C_CONTIGUOUS"] and np.array_equal(ref.bits(part), ref.bits(whole[:, first:])), first
    changed = (ref.bits(whole) != ref.bits(base)).any(axis=0)
    assert np.array_equal(np.flatnonzero(changed), np.arange(3, 300, 7))  # every 7th lane of the batch, from lane 3
    special = lp.CARTPOLE_SLOW if kind == 0 else lp.MOUNTAIN_CAR_SLOW
    assert changed.sum() > len(special)  # every special value is used
    # (two whole cycles of the 15 special values fit into 300 lanes; 6 of MountainCar's and 10 of CartPole's lie outside the range)
    assert lp.beyond_range(kind, whole).sum() >= 12 and np.isnan(whole).any() and np.isinf(whole).any()


def test_the_rows_are_the_ones_the_cases_are_named_after():
    hard, wide, dflt = sl.hard_push_row(17), sl.wide_row(0, 17), lp.default_row(0, 17)
    assert hard.force_mag == 40.0 * dflt.force_mag and hard.theta_threshold_radians == 50.0 and hard.x_threshold == 1.0e6
    assert wide.force_mag == dflt.force_mag and wide.theta_threshold_radians == 2.0 and wide.x_threshold == 1.0e6
    assert sl.hard_push_row(17, 1).kinematics_integrator == 1 and sl.wide_row(0, 17, integrator=1).kinematics_integrator == 1
    assert hard.kinematics_integrator == 0 and hard.max_episode_steps == wide.max_episode_steps == 17
    for field in ("gravity", "masscart", "masspole", "length", "tau"):
        assert getattr(hard, field) == getattr(wide, field) == getattr(dflt, field)
    car = sl.wide_row(1, 17, 300.0)
    assert (car.min_position, car.max_position, car.max_speed, car.force, car.gravity, car.goal_position) == (-1e9, 1e9, 40.0, 3.0, 2.5, 300.0)
    assert car.goal_velocity == lp.default_row(1, 17).goal_velocity
    assert sl.rollout_row(1).goal_position == 300.0 and sl.eval_row(1).goal_position == 120.0
    assert [r.goal_position for r in sl.wide_rows()] == [lp.default_row(1, 40).goal_position, 120.0, 250.0]
    # the thresholds lie outside the fast range: an episode of these rows ends only out there
    assert 2.0 > np.float32(0.7853982) and 3.0 * 120.0 > 200.0


def test_the_case_tables():
    fused, record = sl.rollout_cases(False), sl.rollout_cases(True)
    assert len(fused) == 2 * 4 * 10 + 2 and len(record) == 2 * 2 * 10 * 2 and len(set(fused)) == len(fused) and len(set(record)) == len(record)
    assert {c[3] for c in fused} == {7} and {c[3] for c in record} == {0, 8} and {ref.SHAPES[c[1]][1] for c in record} == {4}
    assert sorted(ref.SHAPES[c[1]][1] for c in fused if c[4] == 1) == [4, 8] and all(c[0] == 0 for c in fused if c[4] == 1)
    for kind in (0, 1):  # every flag set at every shape
        assert {(c[1], c[2]) for c in fused if c[0] == kind and c[4] == 0} == {(s, f) for s in range(4) for f in ref.FLAG_SETS}
    assert set(sl.SEEDS) == {(c[0], c[3], c[1], c[4]) for c in fused + record}
    cases = sl.eval_cases()
    assert len(cases) == 11 and len(set(cases)) == 11
    assert {(c[0], c[2], c[3]) for c in cases if c[1] == 0 and c[4] == 0} == {(k, h, cm) for k in (0, 1) for h in (0, 7) for cm in (False, True)}
    assert [c for c in cases if c[4] == 1] == [(0, 0, 7, False, 1)] and sorted(c[0] for c in cases if c[1] == 1) == [0, 1]
    assert set(sl.EVAL_SEEDS) == {(c[0], c[1], c[2], c[4]) for c in cases}
    assert sl.EVAL_SHAPES[0] == (1300, 12345, 500) and sl.EVAL_SHAPES[1] == (4200, (1 << 40) + 12345, 1000)
    assert (sl.EPISODES, sl.MAX_STEPS, sl.EVAL_SEED, sl.N_POLICIES) == (2, {0: 120, 1: 40}, 11, 3)
    assert max(s[0] for s in ref.SHAPES) <= 5000


def test_the_matrices_these_cases_complement_never_leave_the_range():
    """closed_loop_ref's own cases: no lane-step starts outside the fast range, so only their ragged waves run the general branch"""
    for kind in (0, 1):
        c = ref.case(kind, 1, A | S | T | F, 7, lp.default_row(kind, 0))
        found = sl.rollout_findings(c, ref.run_case(c))
        assert [f.beyond for f in found.copies.values()] == [0, 0, 0] and found.nan_obs == 0


# ---- rollouts ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,hidden,shape,integrator", ROLLOUT_KEYS)
def test_every_rollout_case_meets_the_conditions(kind, hidden, shape, integrator):
    flag_sets = sl.flag_sets_of(kind, shape, hidden, integrator)
    assert flag_sets == (sorted(ref.FLAG_SETS) if integrator == 0 else [A | S | T | F])
    for flags in flag_sets:
        c = sl.rollout_case(kind, shape, flags, hidden, integrator)
        out = ref.run_case(c)
        found = sl.rollout_findings(c, out)
        assert sl.rollout_missing(c, out, found) == [], (flags, sl.rollout_missing(c, out, found))
        assert len(found.copies) == 3 and sum(f.lanes for f in found.copies.values()) == c.n
        assert out[-1].tick == 1 + sum(ref.SCHEDULE) and c.params.max_episode_steps == ref.MAX_EPISODE_STEPS
        if kind == 0:
            assert c.params.kinematics_integrator == integrator
        if not flags & A:
            assert not out[-1].final.any()


def test_the_second_integrator_is_told_apart():
    for case in sl.INTEGRATOR_1:
        c1, c0 = sl.rollout_case(*case), sl.rollout_case(*case[:4])
        # after the third launch, 48 steps: after all 51 = 3 x 17 most lanes have just been re-armed at the time limit, to the same draws
        a, b = ref.run_case(c1)[2], ref.run_case(c0)[2]
        assert (ref.bits(a.state) != ref.bits(b.state)).any(axis=0).mean() > 0.9


def test_rollout_seeds_are_the_first_that_qualify():
    """Every entry is 1, the first seed tried: no earlier seed can be shown to fail here (test_eval_seeds_are_the_first_that_qualify has
    one).  The search gives the entry back."""
    assert set(sl.SEEDS.values()) == {1}
    assert sl.first_rollout_seed(1, 8, 0) == sl.SEEDS[1, 8, 0, 0]


@pytest.mark.parametrize("kind", [0, 1])
def test_the_sharded_rollout_case_meets_the_conditions(kind):
    c = sl.sharded_rollout_case(kind)
    out = ref.run_case(c)
    assert sl.rollout_missing(c, out) == []
    if kind == 0:  # the wide row, not the matrix's
        assert c.params.theta_threshold_radians == 2.0 and c.params.force_mag == lp.default_row(0, 17).force_mag


# ---- evaluation ----------------------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def evaluated(kind, shape, hidden, common, integrator):
    c = sl.eval_case(kind, shape, hidden, common, integrator)
    r = sl.run_eval(c)
    return c, r, sl.run_eval(c, c.default), sl.eval_findings(c, r)


@pytest.mark.parametrize("kind,shape,hidden,common,integrator", sl.eval_cases())
def test_every_evaluation_case_meets_the_conditions(kind, shape, hidden, common, integrator):
    c, r, r_default, found = evaluated(kind, shape, hidden, common, integrator)
    assert sl.eval_missing(c, r, r_default, found) == []
    assert r.records[:, 2].sum() == sl.EPISODES * c.n and c.row.max_episode_steps == c.max_steps
    assert all(f.beyond > 0 for f in found.copies.values()), {k: vars(f) for k, f in found.copies.items()}  # in every copy that has lanes
    if shape == 1:  # uniform-full waves exist, and in them too lanes park while others play on outside the range
        assert found.copies["uniform-full"].lanes >= 1024 and found.copies["uniform-full"].parked >= 10
    if integrator == 1:
        _, euler, _, _ = evaluated(kind, shape, hidden, common, 0)
        assert c.row.kinematics_integrator == 1 and (r.lengths != euler.lengths).any() and (r.records != euler.records).any()


def test_the_figures_the_cases_were_proposed_with():
    """(lane-steps outside the range, distinct lengths) at n = 1300, common starts off: the cases are the ones that were tried"""
    got = {(k, h): (evaluated(k, 0, h, False, 0)[3].beyond, evaluated(k, 0, h, False, 0)[3].lengths) for k in (0, 1) for h in (0, 7)}
    assert got == {(0, 0): (23958, 56), (0, 7): (31301, 53), (1, 0): (4309, 32), (1, 7): (60222, 30)}
    for (k, h), (beyond, _) in got.items():  # the per-trip walk of closed_loop_slow_ref counts what policy_eval_table_ref's helper counts
        c, r, _, _ = evaluated(k, 0, h, False, 0)
        assert tb.states_leave_the_fast_range(k, c.n, c.gid0, c.row, c.weights, h, c.lanes_per_policy, r.starts, c.max_steps) == beyond


def test_eval_seeds_are_the_first_that_qualify():
    """CartPole, 7 hidden units: seed 1 misses a condition (no episode runs into the limit), seed 2 is the entry"""
    assert sl.EVAL_SEEDS[0, 0, 7, 0] == 2
    c = sl.eval_case(0, 0, 7, False, 0, seed=1)
    assert sl.eval_missing(c, sl.run_eval(c), sl.run_eval(c, c.default)) != []
    assert sl.first_eval_seed(0, 0, 7) == 2


def test_mountain_cars_default_gravity_gives_one_length_per_policy():
    """Why the wide row has a gravity of 2.5: with the default 0.0025 every lane of a policy plays the same length"""
    c = sl.eval_case(1, 0, 7, False)
    row = sl.eval_row(1)
    row.gravity = lp.default_row(1, 40).gravity
    r = sl.run_eval(c, row)
    assert all(len(np.unique(r.length[:, r.pol == p])) == 1 for p in range(sl.N_POLICIES))


# ---- evaluation under a table ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hidden,common", sl.table_cases())
def test_every_table_case_meets_the_conditions(hidden, common):
    c = sl.table_case(hidden, common)
    r, r0 = sl.run_table(c), sl.run_table(c, np.zeros(c.n, np.int64))
    found = sl.table_findings(c, r)
    assert sl.table_missing(c, r, r0, found) == [], found
    assert sum(lanes for lanes, _ in found) == c.n and min(lanes for lanes, _ in found) > 300 and r.valid.all()
    assert (r0.length == c.max_steps).all() and not r0.done.any()  # the default row ends no episode in 40 steps: its lanes run into the limit
    for k in (1, 2):  # the two goals are told apart
        other = np.where(c.index == k, 3 - k, c.index)
        assert (sl.run_table(c, other).lengths[:, c.index == k] != r.lengths[:, c.index == k]).any()


# ---- parked lanes ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1])
def test_parked_lanes_share_their_waves_with_lanes_beyond_the_range(kind):
    c = sl.parked_case(kind)
    r = sl.run_eval(c)
    found = sl.eval_findings(c, r)
    assert set(found.copies) == {"gathered-full", "gathered-ragged"} and found.copies["gathered-full"].lanes == 512
    for name, f in found.copies.items():
        assert f.parked >= 10 and f.beyond > f.lanes, (name, vars(f))
    assert np.array_equal(r.pol, (c.gid0 + np.arange(c.n)) % 2)  # the two policies alternate lane by lane
    quick, slow = r.length[:, r.pol == 0], r.length[:, r.pol == 1]
    assert quick.max() <= 12 and r.done[:, r.pol == 0].all()  # policy 0 is through with both episodes within 24 trips ...
    assert slow.min() >= 40 and (slow == c.max_steps).any()  # ... while policy 1 plays at least 80, in the same work-items
    assert len(np.unique(quick)) >= 2 and (kind == 1 or len(np.unique(slow)) >= 6)
    assert (r.records != sl.run_eval(c, c.default).records).any()
    beyond, parked = sl.beyond_by_trip(c, r)
    assert not (beyond & parked).any() and not beyond[:, r.pol == 0][quick.sum(axis=0).max():].any()
