"""The cases of tests/stochastic_slow_ref.py, checked without a GPU: from the CPU reference alone, every one of them sends the exploring,
sampling and transitions kernels through the general, per-lane physics branch in a way a wrong branch could not survive.  These are
conditions, not measurements: a case that misses one gets another weights seed.

Per case, inside the lanes of every kernel copy that has lanes, at each vector width the case's kernels exist at: at least 64 lane-steps
start outside the fast range; a full wave mixes lanes outside and inside; an episode ends on a step that started outside; two different
actions are taken out there and (exploring, sampling) one of them is not the greedy one.  Per case: the policy reads a NaN observation;
no compared float array of the reference holds more than one NaN element in ten (the GPU comparison treats any NaN as equal to any
NaN: that leniency must not carry it).  Transitions: every copy keeps a final observation from a step that started outside, every
table row owns a lane outside, and CartPole keeps a NaN final observation.  Over each matrix: every kernel family at every vector
width under every action source meets all four copies with lanes outside the range.

`pytest -s` prints the table of the figures per kernel family, vector width and copy."""
from functools import lru_cache

import closed_loop_slow_ref as sl
import explore_ref as ex
import lane_params_ref as lp
import numpy as np
import pytest
import sample_ref as sm
import stochastic_slow_ref as ref
import transitions_ref as tr
from stochastic_slow_ref import A, COPIES, F, FULL, T

CASES = [(source,) + m for source in ref.SOURCES[1:] for m in ref.matrix()]


@lru_cache(maxsize=None)
def found_for(source, kind, flags, table, i, integrator):
    """(case, findings, missing, NaN shares, ticks) of a case of the exploring / sampling matrix; the launches themselves are dropped"""
    c = ref.case(source, kind, flags, table, i, integrator)
    out = ref.run_case(c)
    found = ref.findings(c, out)
    return c, found, ref.missing(c, found), ref.nan_shares(c, out), out[-1].tick


@lru_cache(maxsize=None)
def transitions_found_for(kind, table, flags, shape, hidden, source):
    c = ref.transitions_case(kind, table, flags, shape, hidden, source)
    out = ref.run_transitions(c)
    found = ref.findings(c, out)
    return c, found, ref.transitions_missing(c, found), ref.nan_shares(c, out), out[-1].tick


# ---- the rows, the start states, the case tables ---------------------------------------------------------------------------------------------
def test_the_rows_are_the_ones_the_cases_are_named_after():
    for kind in (0, 1):
        assert bytes(ref.slow_rows(kind, 1, False)[0]) == bytes(sl.rollout_row(kind))
        for k in (3, 5):
            rows = ref.slow_rows(kind, k, True)
            want = [lp.default_row(kind, 17), sl.rollout_row(kind), sl.wide_row(kind, 17, 120.0)]
            assert [bytes(r) for r in rows] == [bytes(want[r % 3]) for r in range(k)] and len({id(r) for r in rows}) == k
            assert {r.max_episode_steps for r in rows} == {17}
    assert [r.goal_position for r in ref.slow_rows(1, 3, True)[1:]] == [300.0, 120.0]  # two goals, both outside |3 * position| <= 200
    assert all(r.kinematics_integrator == 1 for r in ref.slow_rows(0, 3, True, 1) + ref.slow_rows(0, 1, False, 1))
    assert ex.TABLE_ROWS == 3 and tr.K == 5


def test_the_case_tables():
    m = ref.matrix()
    assert [x[:4] for x in m[:40]] == ex.matrix() and m[40:] == ref.INTEGRATOR_1 and len(set(m)) == 42
    assert {(x[0], x[1], x[2]) for x in m if x[4] == 0} == {(k, f, t) for k in (0, 1) for f in ex.FLAG_SETS for t in (False, True)}
    assert [(x[0], x[1], x[2]) for x in ref.INTEGRATOR_1] == [(0, FULL, False), (0, FULL, True)]
    for source in ref.SOURCES[1:]:
        c = ref.case(source, 0, FULL, True, 22, 1)
        base = (ex if source == "explore" else sm).matrix_case(0, FULL, True, 22)
        assert (c.n, c.gid0, c.hidden, c.schedule, c.lanes_per_policy, c.seed) == (base.n, base.gid0, base.hidden, base.schedule, base.lanes_per_policy, base.seed)
        assert np.array_equal(c.index, base.index) and np.array_equal(c.weights, base.weights)  # the index and (seed unmoved) the weights stay the case's own
        assert all(r.kinematics_integrator == 1 for r in c.rows) and c.n == 1300
    t = ref.transitions_matrix()
    assert {(k, tb, f) for k, tb, f, *_ in t} == {(k, tb, f) for k in (0, 1) for tb in (False, True) for f in tr.FLAG_SETS} and len(t) == 32
    for kind in (0, 1):
        for table in (False, True):
            mine = [x for x in t if x[0] == kind and x[1] == table]
            assert {x[4] for x in mine} == set(tr.HIDDEN)
            for source in ref.SOURCES:  # each source meets every family at both shapes: all four copies
                assert {x[3] for x in mine if x[5] == source} == {0, 1}, (kind, table, source)
    steps = ref.per_step_cases()
    assert {(s, k, tb) for s, k, tb, *_ in steps} == {(s, k, tb) for s in ref.SOURCES[1:] for k in (0, 1) for tb in (False, True)} and len(steps) == 8
    assert {x[3] for x in steps} == set(ex.OFFSETS) and {x[4] for x in steps} == set(ex.POLICY_SETS) and {x[5] for x in steps} == {0, 8} and {x[6] for x in steps} == {4, 8}


def test_the_matrices_these_cases_complement_never_leave_the_range():
    """explore_ref's, sample_ref's and transitions_ref's own cases: no lane-step starts outside the fast range and no observation is NaN"""
    for kind in (0, 1):
        for source, c in (("explore", ex.matrix_case(kind, FULL, True, 4)), ("sample", sm.matrix_case(kind, FULL, False, 22))):
            c.source = source
            found = ref.findings(c, ref.run_case(c))
            assert all(f.beyond == 0 for copies in found.copies.values() for f in copies.values()) and found.nan_obs == 0
        c = tr.case(kind, 1, A | T, 8, True, True)
        found = ref.findings(c, tr.run_case(c))
        assert all(f.beyond == 0 for f in found.copies[4].values()) and found.nan_obs == 0 and list(found.copies) == [4]


# ---- exploring and sampling ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("source,kind,flags,table,i,integrator", CASES)
def test_every_case_meets_the_conditions(source, kind, flags, table, i, integrator):
    c, found, missing, shares, tick = found_for(source, kind, flags, table, i, integrator)
    assert missing == [], missing
    assert tick == 1 + ex.STEPS and sorted(found.copies) == [4, 8]
    for vec, copies in found.copies.items():
        assert sum(f.lanes for f in copies.values()) == c.n
    assert max(shares.values()) <= ref.NAN_CAP, shares
    assert set(shares) >= {"state", "obs", "reward", "rec_obs", "rec_reward"} and ("final" in shares) == bool(flags & F)
    if table:  # lanes of every row are outside the range, in every copy of a few hundred lanes (the ragged wave at 4 has twenty)
        for vec, copies in found.copies.items():
            assert all(f.rows == [0, 1, 2] for f in copies.values() if f.lanes >= 256), (vec, {k: f.rows for k, f in copies.items()})


def test_every_family_meets_all_four_copies_beyond_the_range_and_the_table_of_figures():
    """Kernel family = source x (plain, fitness, recording) x env x table, at the vector widths of ENGINES.  Prints the totals."""
    totals = {}
    worst = 0.0
    for source, kind, flags, table, i, integrator in CASES:
        c, found, _, shares, _ = found_for(source, kind, flags, table, i, integrator)
        worst = max(worst, max(shares.values()))
        for mode, vec in ref.ENGINES:
            for name, f in found.copies[vec].items():
                row = totals.setdefault((source, mode, kind, table, vec), {}).setdefault(name, np.zeros(4, np.int64))
                row += (f.beyond, f.mixed or 0, f.ended, f.away)
    assert len(totals) == 2 * 5 * 2 * 2
    print("\nsource mode env table vec copy: lane-steps beyond, mixed full wave-steps, episodes ended out there, non-greedy actions out there")
    for key, copies in sorted(totals.items(), key=str):
        assert set(copies) == set(COPIES), (key, sorted(copies))
        for name in COPIES:
            assert copies[name][0] > 0 and copies[name][2] > 0 and copies[name][3] > 0, (key, name, copies[name])
            print(*key, name, *copies[name].tolist())
    print(f"largest NaN share of a compared array: {worst:.4f} (cap {ref.NAN_CAP})")
    assert 0 < worst <= ref.NAN_CAP


def test_seeds_are_the_first_that_qualify():
    """Every entry of SEEDS replaces a seed that misses a condition, and the search gives the entry back"""
    for (source, kind, flags, table, i, integrator), seed in ref.SEEDS.items():
        make = lambda s: ref.case(source, kind, flags, table, i, integrator, seed=s)  # noqa: E731
        c = make(ex.WEIGHTS_SEED)
        assert ref.missing(c, ref.findings(c, ref.run_case(c))) != []
        assert ref.first_seed(make, ref.run_case, ref.missing) == seed
    for (kind, table, flags), seed in ref.TRANSITIONS_SEEDS.items():
        _, _, _, shape, hidden, source = next(x for x in ref.transitions_matrix() if x[:3] == (kind, table, flags))
        make = lambda s: ref.transitions_case(kind, table, flags, shape, hidden, source, seed=s)  # noqa: E731
        c = make(tr.seed_of(kind, hidden, shape, table, source == "explore"))
        assert ref.transitions_missing(c, ref.findings(c, ref.run_transitions(c))) != []
        assert ref.first_seed(make, ref.run_transitions, ref.transitions_missing) == seed


# ---- the per-step kernels and the sharded handle ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("source,kind,table,gid0,policy_set,hidden,vec", ref.per_step_cases())
def test_the_per_step_cases_read_non_finite_observations_beyond_the_range(source, kind, table, gid0, policy_set, hidden, vec):
    c = ref.per_step_case(source, kind, table, gid0, policy_set, hidden)
    out = ref.run_case(c)
    found = ref.findings(c, out, (vec,))
    assert ref.missing(c, found) == [] and max(ref.nan_shares(c, out).values()) <= ref.NAN_CAP
    w = ref.walk(c, out)
    assert (~np.isfinite(w.start)).any(axis=1)[w.beyond].sum() >= 8  # NaN and inf observations reach explore_actions / sample_actions
    if source == "sample":
        prob = np.concatenate([x.prob for x in out])
        assert np.isfinite(prob).all() and (prob > 0).all() and (prob <= 1).all()  # the prob row is compared bit for bit: it holds no NaN
        if hidden == 0:  # an affine policy turns a NaN observation into NaN logits: all weights 0, the greedy action with probability 1
            nan = np.isnan(w.start).any(axis=1)
            assert nan.any() and (prob[nan] == 1).all() and (w.actions[nan] == w.greedy[nan]).all()


@pytest.mark.parametrize("source", ref.SOURCES[1:])
@pytest.mark.parametrize("kind", [0, 1])
def test_the_sharded_cases_meet_the_conditions(kind, source):
    c = ref.sharded_case(source, kind)
    out = ref.run_case(c)
    assert ref.missing(c, ref.findings(c, out, (4,))) == [] and max(ref.nan_shares(c, out).values()) <= ref.NAN_CAP
    assert c.gid0 == 6 and c.table and c.flags == FULL


# ---- transitions ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,table,flags,shape,hidden,source", ref.transitions_matrix())
def test_every_transitions_case_meets_the_conditions(kind, table, flags, shape, hidden, source):
    c, found, missing, shares, tick = transitions_found_for(kind, table, flags, shape, hidden, source)
    assert missing == [], missing
    assert tick == 1 + sum(tr.SCHEDULE) and list(found.copies) == [4] and len(found.copies[4]) == 3
    assert sum(f.lanes for f in found.copies[4].values()) == c.n and c.n == tr.SHAPES[shape][0]
    assert max(shares.values()) <= ref.NAN_CAP, shares
    assert set(shares) >= {"state", "obs", "reward", "rec_obs", "rec_reward", "final_obs", "start_obs"}
    for name, f in found.copies[4].items():  # a final observation kept from a step that started beyond the range, in every copy
        assert f.ended >= 1 and f.final_nan is not None, name
    if kind == 0:  # the comparison of the sink does meet NaNs
        assert shares["final_obs"] > 0 and sum(f.final_nan for f in found.copies[4].values()) >= 1
    assert c.explore == (source == "explore") and (source != "sample" or (c.seed, c.scale) == (sm.SEED, sm.SCALE))
    if not flags & T:
        assert len(c.rows) == (5 if table else 1)


def test_every_transitions_family_meets_all_four_copies_under_every_source():
    totals = {}
    worst = 0.0
    for kind, table, flags, shape, hidden, source in ref.transitions_matrix():
        _, found, _, shares, _ = transitions_found_for(kind, table, flags, shape, hidden, source)
        worst = max(worst, max(shares.values()))
        for name, f in found.copies[4].items():
            row = totals.setdefault((source, "transitions", kind, table, 4), {}).setdefault(name, np.zeros(5, np.int64))
            row += (f.beyond, f.mixed or 0, f.ended, f.away, f.final_nan)
    assert len(totals) == 3 * 2 * 2
    print("\nsource mode env table vec copy: lane-steps beyond, mixed full wave-steps, episodes ended out there (= final observations kept), "
          "non-greedy actions out there, NaN final observations")
    for key, copies in sorted(totals.items(), key=str):
        assert set(copies) == set(COPIES), (key, sorted(copies))
        for name in COPIES:
            assert copies[name][0] > 0 and copies[name][2] > 0 and (key[0] == "greedy") == (copies[name][3] == 0), (key, name, copies[name])
            print(*key, name, *copies[name].tolist())
    print(f"largest NaN share of a compared array: {worst:.4f} (cap {ref.NAN_CAP})")
    assert 0 < worst <= ref.NAN_CAP
