"""The CPU reference of gymrs_evaluate_policy under a parameter table (tests/policy_eval_table_ref.py) on the case table of
tests/test_gpu_policy_eval_table.py, checked without a GPU.  Every case is worth comparing: beyond what test_policy_eval_ref.py asks
of the uniform cases, in the lanes of every kernel copy some lane's length differs from what it would be with every lane on row 0,
every policy's record differs likewise, and some wave mixes two rows -- so the GPU comparison cannot pass with the rows ignored.  And
the yardstick itself: a one-row table is policy_eval_ref.reference, a lane whose index is not in the table counts nowhere."""
from functools import lru_cache

import lane_params_ref as lp
import numpy as np
import policy_eval_ref as ev
import policy_eval_table_ref as tb
import pytest
from closed_loop_ref import make_weights


@lru_cache(maxsize=None)
def run(kind, shape, hidden, common):
    c = tb.case(kind, shape, hidden, common)
    return c, tb.run_case(c), tb.run_case(c, np.zeros(c.n, np.int64))


@pytest.mark.parametrize("kind,shape,hidden,common", tb.cases())
def test_every_case_is_worth_comparing(kind, shape, hidden, common):
    c, r, r0 = run(kind, shape, hidden, common)
    assert tb.worth_comparing(c, r, r0) == []
    assert len(c.rows) == tb.K == 5 and set(np.unique(c.index)) == set(range(tb.K)) and r.valid.all()
    assert all(row.max_episode_steps == tb.MAX_STEPS for row in c.rows)


def test_the_cases_are_policy_eval_refs_shapes():
    assert tb.cases() == ev.cases() and len(tb.cases()) == 2 * 2 * len(ev.HIDDEN) * 2
    assert [(s[0], s[2], s[3]) for s in tb.SHAPES] == [(4200, (1 << 40) + 12345, 1000), (5000, 12345, 1024)]
    assert (tb.EPISODES, tb.MAX_STEPS, tb.N_POLICIES) == (3, 17, 3)
    rows = tb.case(1, 0, 0, False).rows
    assert lp.low_goal_rows(1, rows) == [1, 3]


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("common", [False, True])
def test_a_one_row_table_is_the_uniform_reference(kind, common):
    n, _, gid0, lpp = tb.SHAPES[0]
    row = lp.default_row(kind, tb.MAX_STEPS)
    if kind == 1:
        ev.mountain_car_params(row)
    w = make_weights(kind, 7, tb.N_POLICIES, ev.WEIGHT_SEEDS[kind, 7, 0])
    want = ev.reference(kind, n, gid0, row, w, 7, lpp, tb.N_POLICIES, tb.SEED, tb.EPISODES, tb.MAX_STEPS, common)
    got = tb.reference(kind, n, gid0, [row], np.zeros(n, np.int64), w, 7, lpp, tb.N_POLICIES, tb.SEED, tb.EPISODES, tb.MAX_STEPS, common)
    assert np.array_equal(got.records, want.records) and np.array_equal(got.lengths, want.lengths)
    assert np.array_equal(got.length, want.length) and np.array_equal(got.done, want.done) and np.array_equal(got.pol, want.pol)
    assert all(np.array_equal(a, b) for a, b in zip(got.starts, want.starts))


def test_lanes_come_from_the_run_of_their_own_row():
    c, r, _ = run(0, 1, 7, False)
    for row in range(tb.K):
        only = tb.run_case(c, np.full(c.n, row, np.int64))
        m = c.index == row
        assert m.any() and np.array_equal(r.lengths[:, m], only.lengths[:, m])
    merged = ev.merge([ev.records(0, r.length[:, c.index == row], r.done[:, c.index == row], r.pol[c.index == row], tb.N_POLICIES, tb.MAX_STEPS)
                       for row in range(tb.K)])
    assert np.array_equal(merged, r.records)


def test_a_lane_with_an_index_beyond_the_table_counts_nowhere():
    c, r, _ = run(1, 0, 8, False)
    index = c.index.astype(np.int64).copy()
    out = np.array([0, 5, 999, 1000, 1001, 2047, 4199])  # both sides of the policy boundary at lane 1000 - (gid0 % 1000), the last lane
    index[out] = [tb.K, tb.K + 1, 65535, tb.K, 40000, tb.K, 65535]
    got = tb.run_case(c, index)
    keep = np.ones(c.n, bool)
    keep[out] = False
    assert np.array_equal(got.valid, keep) and np.array_equal(got.lengths[:, keep], r.lengths[:, keep])
    assert got.records[:, 2].sum() == tb.EPISODES * (c.n - len(out)) and (got.records != r.records).any()
    assert np.array_equal(got.records, ev.records(1, r.length[:, keep], r.done[:, keep], r.pol[keep], tb.N_POLICIES, tb.MAX_STEPS))


def test_the_hard_push_rows_leave_the_fast_range():
    """The GPU test of the general path under a table relies on it: lanes of row 1 go on playing beyond |theta| = pi / 4"""
    n, _, gid0, lpp = tb.SHAPES[0]
    rows = tb.hard_push_rows()
    w = make_weights(0, 7, tb.N_POLICIES, 18)
    starts = ev.start_states(0, n, gid0, rows[0], tb.SEED, tb.EPISODES, lpp, False)
    beyond = [tb.states_leave_the_fast_range(0, n, gid0, row, w, 7, lpp, starts, tb.MAX_STEPS) for row in rows]
    assert beyond[0] == 0 and beyond[1] > n and beyond[2] > 0, beyond
