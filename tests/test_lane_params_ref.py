"""The CPU reference of per-lane parameter tables (tests/lane_params_ref.py) and the cases of tests/test_gpu_lane_params_paths.py,
checked without a GPU: the reference is a plain twin where it must be, and its cases can tell a wrong kernel from a right one
(every row ends episodes both ways, and at every compared point a lane stepped with another row would show)."""
import lane_params_ref as ref
import numpy as np
import pytest
from lane_params_ref import A, F, S, T, bits

from oracle.bindings import TwinEngine


def test_rows_have_the_layout_and_defaults_of_the_library(gymrs):
    for kind in (0, 1):
        p = gymrs.engine.default_params(kind)
        p.max_episode_steps = 23
        assert bytes(ref.default_row(kind, 23)) == bytes(p)
        assert [f for f, _ in ref.ROW[kind]._fields_] == [f for f, _ in type(p)._fields_]
        back = ref.rows_for(type(p), ref.make_rows(kind, 3, 1, 23))
        assert all(isinstance(r, type(p)) for r in back) and bytes(back[2]) == bytes(ref.make_rows(kind, 3, 1, 23)[2])


def test_make_rows_varies_every_physics_field():
    for kind, integrator in ((0, 0), (0, 1), (1, 0)):
        rows = ref.make_rows(kind, ref.K, 5, 17, integrator)
        assert len(rows) == ref.K and all(r.max_episode_steps == 17 for r in rows)
        physics = [f for f, t in ref.ROW[kind]._fields_ if f not in ("kinematics_integrator", "max_episode_steps", "_pad")]
        assert len(physics) == (8 if kind == 0 else 7)
        for f in physics:
            assert len({getattr(r, f) for r in rows}) >= 2, f
        if kind == 0:
            assert all(r.kinematics_integrator == integrator for r in rows)
            d = ref.default_row(0, 17)
            for f in physics:
                assert all(0.5 <= getattr(r, f) / getattr(d, f) <= 1.5 for r in rows)
        else:
            assert ref.low_goal_rows(1, rows) == [1, 3]
            assert {r.goal_velocity for r in rows} == {0.0, -1.0} and {r.min_position for r in rows} == {-1.2, -0.9}
            assert {r.max_position for r in rows} == {0.6, 0.3}
    a, b = ref.make_rows(0, 4, 9, 17), ref.make_rows(0, 4, 9, 17)
    assert [bytes(r) for r in a] == [bytes(r) for r in b]  # seeded


def same_as_twin(r, tw, at):
    assert np.array_equal(bits(r.state), bits(tw.get_state())), at
    assert np.array_equal(bits(r.obs), bits(tw.get_obs())), at
    rw, dn, tr = tw.get_result()
    assert np.array_equal(bits(r.reward), bits(rw)) and np.array_equal(r.done, dn) and np.array_equal(r.truncated, tr), at
    assert np.array_equal(r.stats, tw.stats()), (at, r.stats, tw.stats())


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("flags", ref.FLAG_SETS)
def test_one_row_is_a_plain_twin(twin, kind, flags):
    """K = 1, and every lane on row r of K: bit-identical to a TwinEngine with that row, the rebuilt statistics included"""
    n, gid0, steps = 700, 12345, 40
    rows = ref.make_rows(kind, 3, 2, 9)
    for table, r in (([rows[1]], 0), (rows, 0), (rows, 2)):
        got = ref.TableReference(kind, n, gid0, table, np.full(n, r), flags, 4, action_seed=8)
        tw = TwinEngine(twin, kind, n, table[r], flags=flags & ~F, gid0=gid0)
        tw.reset(4)
        same_as_twin(got, tw, "reset")
        for t in range(steps):
            got.step()
            tw.step(tw.fill_actions(8, t))
            same_as_twin(got, tw, t)
        assert got.tick == steps + 1 and len(got.records) == steps
        if flags & A:
            if kind == 0 or flags & T:  # (MountainCar without the limit ends episodes on its low-goal row only)
                assert got.final.any() and (got.stats[2] > 0 or not flags & S)
        else:
            assert not got.final.any() and not got.stats[:3].any()


def test_mixed_rows_are_the_lanes_of_uniform_twins(twin):
    """Two rows, random index: every lane equals the same lane of the plain twin of its row, and the statistics are the sums over
    the lanes each twin contributes (counted here from the twins' own flags)"""
    kind, n, gid0, flags = 0, 900, 64, A | S | T | F
    rows = ref.make_rows(kind, 2, 3, 9)
    index = ref.make_index(n, 2, 1)
    got = ref.TableReference(kind, n, gid0, rows, index, flags, 4, action_seed=8)
    tws = [TwinEngine(twin, kind, n, row, flags=flags & ~F, gid0=gid0) for row in rows]
    for tw in tws:
        tw.reset(4)
    episodes = 0
    for t in range(30):
        got.step()
        for r, tw in enumerate(tws):
            tw.step(tw.fill_actions(8, t))
            m = index == r
            assert np.array_equal(bits(got.state[:, m]), bits(tw.get_state()[:, m]))
            _, dn, tr = tw.get_result()
            assert np.array_equal(got.done[m], dn[m]) and np.array_equal(got.truncated[m], tr[m])
            episodes += int(((dn | tr) != 0)[m].sum())
    assert got.stats[2] == episodes and got.stats[3] == 30 * n and got.stats[0] == got.stats[1] > 0


def test_set_index_continues_every_lane_from_its_own_state(twin):
    kind, n, gid0, flags = 0, 500, 12345, A | S
    rows = ref.make_rows(kind, 2, 3, 9)
    got = ref.TableReference(kind, n, gid0, rows, np.zeros(n, int), flags, 4, action_seed=8)
    got.step(5)
    tw = TwinEngine(twin, kind, n, rows[1], flags=flags, gid0=gid0)
    tw.reset(4)
    for t in range(5):  # (the tick must follow: the re-arm draws are keyed by it)
        tw.step(tw.fill_actions(8, t))
    tw.set_state(got.state)
    got.set_index(np.ones(n, int))
    for t in range(5, 12):
        got.step()
        tw.step(tw.fill_actions(8, t))
        assert np.array_equal(bits(got.state), bits(tw.get_state())) and np.array_equal(got.done, tw.get_result()[1])


def cases_with_auto_reset():
    """(kind, flags, gid0, integrator) of every multi-row case of the GPU file that has A set"""
    out = [(kind, flags, gid0, 0) for kind in (0, 1) for flags in ref.FLAG_SETS if flags & A for gid0 in ref.OFFSETS]
    return out + [(0, flags, ref.OFFSETS[0], 1) for flags in ref.INTEGRATOR_1_FLAGS]


@pytest.mark.parametrize("kind,flags,gid0,integrator", cases_with_auto_reset())
def test_every_row_ends_episodes_both_ways(kind, flags, gid0, integrator):
    """Every row has lanes that terminate and, with T, lanes that are truncated.  MountainCar: a random policy reaches only the
    lowered goal, so only those rows must terminate, and there are at least two."""
    r = ref.matrix_reference(ref.matrix_case(kind, flags, gid0, integrator))
    for _, steps in ref.STAGES:
        r.step(steps)
    must_terminate = range(ref.K) if kind == 0 else ref.low_goal_rows(1, r.rows)
    assert len(must_terminate) >= 2
    assert all(r.ended_by[0][row] > 0 for row in must_terminate), r.ended_by
    if flags & T:
        assert (r.ended_by[1] > 0).all(), r.ended_by
    else:
        assert not r.ended_by[1].any()
    if flags & F:
        for row in range(ref.K) if (flags & T or kind == 0) else must_terminate:
            assert r.final[:, r.index == row].any(), row
    if flags & S:
        assert r.stats[2] == sum(int(((x.done | x.truncated) != 0).sum()) for x in r.records) > 0


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("flags", ref.FLAG_SETS)
def test_a_wrong_row_shows_at_every_compared_point(kind, flags):
    """After every stage of the path matrix, of the lanes not on that row anyway, at least TOLD_APART differ bitwise from the state
    they would have under row 0, and under row (index + 1) % K.  (With n = 3001, K = 5, 40 steps and max_episode_steps 9 or 17 the
    fraction is 0.99 or more; a step count that is a multiple of max_episode_steps drops it to 0.3 - 0.7, which STAGES avoids.)"""
    for gid0 in ref.OFFSETS:
        for integrator in (0, 1) if kind == 0 and flags in ref.INTEGRATOR_1_FLAGS else (0,):
            r = ref.matrix_reference(ref.matrix_case(kind, flags, gid0, integrator))
            total = 0
            for name, steps in ref.STAGES:
                r.step(steps)
                total += steps
                assert total % ref.MAX_EPISODE_STEPS != 0
                for other in (np.zeros(r.n, int), (r.index + 1) % ref.K):
                    assert r.told_apart(other) >= ref.TOLD_APART, (gid0, name, total, r.told_apart(other))


def test_the_recording_case_is_worth_comparing_too():
    for kind in (0, 1):
        for flags in ref.FLAG_SETS:
            r = ref.matrix_reference(ref.matrix_case(kind, flags, ref.OFFSETS[0], stages=ref.RECORD_STAGES))
            for _, steps in ref.RECORD_STAGES:
                r.step(steps)
                assert r.t % ref.MAX_EPISODE_STEPS != 0
                for other in (np.zeros(r.n, int), (r.index + 1) % ref.K):
                    assert r.told_apart(other) >= ref.TOLD_APART
            if flags & A:
                ends = range(ref.K) if kind == 0 else ref.low_goal_rows(1, r.rows)
                assert all(r.ended_by[0][row] > 0 for row in ends) and (not flags & T or (r.ended_by[1] > 0).all())


def test_the_elision_case_ends_episodes_both_ways_in_every_row():
    c = ref.elision_case()
    r = ref.matrix_reference(c).step(ref.ELISION_STEPS)
    assert c.rows[0].max_episode_steps == ref.ELISION_LIMIT and (r.ended_by > 0).all(), r.ended_by
    assert ref.ELISION_STEPS % ref.ELISION_LIMIT != 0 and r.told_apart((r.index + 1) % ref.K) >= ref.TOLD_APART


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("flags", ref.REWRITE_FLAGS)
def test_a_stale_index_would_show_after_the_rewrite(kind, flags):
    c = ref.matrix_case(kind, flags, ref.OFFSETS[0], stages=())
    new = ref.rewritten_index(kind)
    assert (new != c.index).mean() > 0.7
    r = ref.matrix_reference(c).step(ref.REWRITE_STEPS[0])
    r.set_index(new)
    r.step(ref.REWRITE_STEPS[1])
    assert r.told_apart(c.index) >= ref.TOLD_APART  # of the lanes whose row changed: stepped with the old row they would differ
    ends = range(ref.K) if kind == 0 else ref.low_goal_rows(1, r.rows)
    assert all(r.ended_by[0][row] > 0 for row in ends)


@pytest.mark.parametrize("kind", [0, 1])
def test_the_policy_case_takes_several_actions_and_ends_episodes(kind):
    c, r, w = ref.policy_reference(kind)
    assert w.shape[0] == ref.POLICY.n_policies == 2 and c.n > 2 * ref.POLICY.lanes_per_policy
    r.step(ref.POLICY.steps)
    taken = set(np.concatenate([x.actions for x in r.records]).tolist())
    assert len(taken) >= 2 and r.stats[2] > 0 and (r.ended_by.sum(axis=0) > 0).all()  # (episodes end in every row, one way or the other)
    assert r.told_apart((r.index + 1) % ref.K) >= ref.TOLD_APART and ref.POLICY.steps % ref.MAX_EPISODE_STEPS != 0


def test_integrator_1_differs_from_euler_at_once():
    flags = ref.INTEGRATOR_1_FLAGS[0]
    euler = ref.matrix_reference(ref.matrix_case(0, flags, ref.OFFSETS[0])).step(3)
    other = ref.matrix_reference(ref.matrix_case(0, flags, ref.OFFSETS[0], integrator=1)).step(3)
    assert (bits(euler.state) != bits(other.state)).any(axis=0).mean() >= ref.TOLD_APART


def test_the_index_spreads_the_rows_over_every_wave_and_work_item_slot():
    """Every row occurs in the full waves and in the ragged one at both widths, and in each of the 8 lanes of a work-item"""
    for kind in (0, 1):
        index = ref.make_index(ref.N, ref.K, ref.INDEX_SEED + kind)
        for vec in (4, 8):
            full = ref.N // (64 * vec) * (64 * vec)
            assert 0 < full < ref.N
            assert set(index[:full]) == set(index[full:]) == set(range(ref.K))
        for slot in range(8):
            assert set(index[slot::8]) == set(range(ref.K))
    assert ref.N % 256 == 185 and ref.N - 512 * (ref.N // 512) == 441 and all(g % 4 for g in ref.OFFSETS[:1]) and ref.OFFSETS[1] % 4 == 0


@pytest.mark.parametrize("kind", [0, 1])
def test_slow_path_start_states_reach_several_rows(kind):
    """The prepared lanes beyond the fast path's range belong to at least three different rows, sit in full and ragged waves, and
    with flags 0 / T (nobody re-arms them) some are still beyond the range steps later"""
    c = ref.matrix_case(kind, 0, ref.OFFSETS[0])
    r = ref.matrix_reference(c, ref.slow_prepare(kind))
    out = ref.beyond_range(kind, r.state)
    assert out.sum() >= 100  # (of the N // 7 prepared lanes: some special values are inside the range, a NaN velocity for one)
    assert len(set(r.index[out])) >= 3
    full = ref.N // 512 * 512
    assert out[:full].any() and out[full:].any()
    assert not np.isfinite(r.state).all()
    r.step(3)
    assert kind == 1 or ref.beyond_range(kind, r.state).any()  # (MountainCar's clip brings every position back at once)
    a = ref.matrix_reference(ref.matrix_case(kind, A | S, ref.OFFSETS[0]), ref.slow_prepare(kind))
    a.step(3)
    if kind == 0:  # every run-away CartPole lane terminated on its first step and was re-armed
        assert not ref.beyond_range(0, a.state).any() and np.isfinite(a.state).all()
