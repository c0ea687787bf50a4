"""The cases of tests/test_gpu_elided_stores.py and their CPU reference (tests/elided_stores_ref.py), checked without a GPU: every
script leaves the array dirty where it says it does and clean after the repair, the model of the reward protocol predicts the
reference, and with a clearing point switched off the model predicts a stale lane in every case that relies on that point --
which is the proof that the case would notice the missing invalidation on the device."""
import elided_stores_ref as ref
import numpy as np
import pytest
from elided_stores_ref import A, S, T

CASES = ref.reward_cases()
# the physics does not matter to what the model says: the teeth tests run on one engine per env kind
MODEL_CASES = [c for c in CASES if c.engine in ("mc-AST", "cp-A")]


def ids(cases):
    return [ref.case_id(c) for c in cases]


def test_the_dirty_lanes_sit_where_a_shape_change_reads_a_word_the_other_layout_left_set():
    assert [ref.slot(lane, 4) for lane in ref.DIRTY] == [1, 4, 5] and [ref.slot(lane, 8) for lane in ref.DIRTY] == [0, 2, 2]
    assert ref.N // 256 == 5 and 0 < ref.N % 256 and ref.N // 512 == 2 and 0 < ref.N % 512  # full waves and a ragged one at both shapes
    assert ref.slot(ref.DIRTY[2], 4) == ref.N // 256 and ref.slot(ref.DIRTY[2], 8) == ref.N // 512  # lane 1299 is in the ragged wave
    # the word a dirty lane's wave reads after the change is one that only CLEAN lanes' waves wrote under the other layout
    for old, new in ((4, 8), (8, 4)):
        dirty_old = {ref.slot(lane, old) for lane in ref.DIRTY}
        assert any(ref.slot(lane, new) not in dirty_old for lane in ref.DIRTY), (old, new)


@pytest.mark.parametrize("engine", ref.ENGINES)
@pytest.mark.parametrize("table", [False, True])
def test_the_twin_table_equals_the_table_reference_of_the_lane_parameter_tests(engine, table):
    """40 steps with invalid actions on the DIRTY lanes in every seventh: state, results and statistics of TwinTable against
    lane_params_ref.TableReference (which tests/test_lane_params_ref.py holds against a plain twin)"""
    import lane_params_ref as lp

    kind, flags, _ = ref.ENGINES[engine]
    rows, index = ref.rows_of(engine, table), ref.index_of(engine, table)
    assert len(rows) == (ref.K if table else 1) and (len(set(index.tolist())) == ref.K) == table
    acts = []
    for t in range(40):
        a = lp.fill_actions(kind, ref.N, 0, ref.ACTION_SEED, t)
        if t % 7 == 3:
            a[list(ref.DIRTY)] = ref.BAD_ACTION
        acts.append(a)
    want = lp.TableReference(kind, ref.N, 0, rows, index, flags, ref.RESET_SEED, actions=lambda t, obs: acts[t])
    got = ref.TwinTable(kind, flags, rows, index)
    for t in range(40):
        want.step()
        got.step(acts[t])
        assert np.array_equal(got.state.view(np.uint32), want.state.view(np.uint32)) and np.array_equal(got.reward, want.reward), t
        assert np.array_equal(got.done, want.done) and np.array_equal(got.truncated, want.truncated), t
        assert np.array_equal(got.stats, want.stats) and got.tick == want.tick, (t, got.stats, want.stats)
    assert want.stats[2] > 0 or not (flags & S and kind == 0)  # CartPole's episodes end: the rebuilt statistics were exercised


def test_the_table_reaches_every_source_event_and_repair_at_both_shapes_on_every_engine():
    seen = {(c.engine, c.shape): set() for c in CASES}
    for c in CASES:
        seen[c.engine, c.shape] |= {("source", c.source), ("event", c.event), ("repair", c.repair)}
    want = ({("source", s) for s in ref.UNIFORM_SOURCES + ref.TABLE_SOURCES} | {("event", e) for e in ref.EVENTS} |
            {("repair", r) for r in ref.REPAIRS})
    assert set(seen) == {(e, s) for e in ref.ENGINES for s in ref.SHAPES}
    assert all(v == want for v in seen.values())
    for shape in ref.SHAPES:
        one = [c for c in CASES if c.engine == "mc-A" and c.shape == shape]
        assert {(c.event, c.repair) for c in one if c.source == "step"} == {(e, r) for e in ref.EVENTS for r in ref.REPAIRS}
        assert {(c.source, c.repair) for c in one if c.source in ref.FUSED} == {(s, r) for s in ref.FUSED for r in ("step",) + ref.REPAIRS[2:]}
    assert len(set(CASES)) == len(CASES)
    assert {ref.ENGINES[e][:2] for e in ref.ENGINES} == {(1, A), (1, A | S | T), (0, A), (0, A | S), (0, A | S | T)}


@pytest.mark.parametrize("c", CASES, ids=ids(CASES))
def test_the_reference_is_dirty_after_the_dirtying_call_and_clean_after_the_repair(c):
    calls, dirty_at, repair_at = ref.calls_of(c)
    exp = ref.expected(c)
    const = np.float32(ref.CONST[ref.ENGINES[c.engine][0]])
    dirty = np.zeros(ref.N, bool)
    dirty[list(ref.DIRTY)] = True
    assert (exp[dirty_at - 1].reward == const).all()  # the valid steps before it paid every lane
    after = exp[dirty_at].reward
    if c.source.endswith("-mid"):  # a later launch of the same step_many call has repaired the array already
        assert (after == const).all()
    else:
        assert (after[dirty] == 0).all() and (after[~dirty] == const).all()
    # a rejected lane: state unchanged, reward 0, no flag
    if not c.source.startswith("many-"):
        before = exp[dirty_at - 1]
        assert np.array_equal(exp[dirty_at].state[:, dirty].view(np.uint32), before.state[:, dirty].view(np.uint32))
        assert not exp[dirty_at].done[dirty].any() and not exp[dirty_at].truncated[dirty].any()
    # nothing between the dirtying call and the repair writes a reward, except a fused launch (record8 stores every reward)
    for k in range(dirty_at + 1, repair_at):
        if not exp[k].launches:
            assert np.array_equal(exp[k].reward, after), calls[k]
    for k in range(repair_at, len(calls)):
        assert (exp[k].reward == const).all(), calls[k]
    assert calls[dirty_at + 1] == ("consume",) and len(exp[repair_at].launches) >= 1
    # the dirtying call is what it says: launches that do not pay the DIRTY lanes, and no other call has one
    for k, e in enumerate(exp):
        unpaid = [lanes for _, _, paid in e.launches for lanes in [np.flatnonzero(~paid).tolist()] if lanes]
        assert unpaid == ([list(ref.DIRTY)] * len(unpaid) if k == dirty_at else []), (k, calls[k])
    assert any(not paid.all() for _, _, paid in exp[dirty_at].launches)
    if ref.ENGINES[c.engine][1] & S and c.event != "stats-clear":
        assert exp[-1].stats[3] == ref.N * sum(len(e.launches) for e in exp)


@pytest.mark.parametrize("c", MODEL_CASES, ids=ids(MODEL_CASES))
def test_the_protocol_model_predicts_the_reference(c):
    for k, (got, e) in enumerate(zip(ref.predicted_rewards(c), ref.expected(c))):
        assert np.array_equal(got, e.reward), (k, ref.calls_of(c)[0][k], np.flatnonzero(got != e.reward)[:8])


def stale_lanes(c, off):
    """lanes where the model with clearing points `off` left out disagrees with the reference, from the repairing step on"""
    repair_at = ref.calls_of(c)[2]
    got, exp = ref.predicted_rewards(c, off), ref.expected(c)
    return sorted({int(lane) for g, e in zip(got[repair_at:], exp[repair_at:]) for lane in np.flatnonzero(g != e.reward)})


TEETH = [c for c in MODEL_CASES if c.event in ref.CLEARED_BY or c.source in ref.FUSED]


@pytest.mark.parametrize("c", TEETH, ids=ids(TEETH))
def test_without_its_clearing_point_a_case_shows_a_stale_lane(c):
    """Every case that names an event with a clearing point (a change of launch shape, a snapshot load), and every fused launch
    under a table: the model without that point leaves 0.0 on a DIRTY lane after the repair; with it, nothing is stale.  (A
    recording launch runs at 4 lanes per work-item: on an engine tuned to 8 it changes the launch shape as well, and either of
    the two points saves the case -- both have to go before it shows.)"""
    assert stale_lanes(c, ()) == []
    points = set()
    if c.event in ref.CLEARED_BY:
        points.add(ref.CLEARED_BY[c.event])
    if c.source in ref.FUSED:
        points.add("fused")
        if c.source in ("record", "cl-record", "transitions") and c.shape == 8:
            points.add("shape")
            assert stale_lanes(c, ("shape",)) == [] and stale_lanes(c, ("fused",)) == []
    stale = stale_lanes(c, tuple(points))
    assert stale and set(stale) <= set(ref.DIRTY), (points, stale)
    others = [p for p in ref.RewardProtocol.POINTS if p not in points]
    assert stale_lanes(c, others) == []  # and no other point matters to this case


def test_cases_without_an_event_do_not_need_the_shape_or_load_points():
    """The no-event cases of the per-step sources must pass on a device whose shape-change clearing is missing: the run that
    shows the shape-change cases failing there tells the two apart."""
    for c in MODEL_CASES:
        if c.event == "none" and c.source in ref.UNIFORM_SOURCES + ("index-step",):
            assert stale_lanes(c, ("shape", "load", "fused")) == [], ref.case_id(c)
        if c.event == "tune-other":
            assert stale_lanes(c, ("shape",)) != [], ref.case_id(c)


def test_a_reset_without_its_clearing_point_leaves_zeros():
    m = ref.RewardProtocol(ref.N, off=("reset",))
    m.reset()
    for _ in range(2):
        m.step(4, np.ones(ref.N, bool))
    assert m.holds.all()
    m.reset()
    m.step(4, np.ones(ref.N, bool))
    assert not m.holds.any()
    ok = ref.RewardProtocol(ref.N)
    ok.reset()
    ok.step(4, np.ones(ref.N, bool))
    ok.reset()
    ok.step(4, np.ones(ref.N, bool))
    assert ok.holds.all()


# ---- Pendulum ---------------------------------------------------------------------------------------------------------------------
P_CASES = ref.pendulum_cases()


def run_pendulum(c):
    r = ref.PendulumReference(c)
    calls, event_at = ref.pendulum_calls(c)
    column, value_at_event = [], None
    for k, call in enumerate(calls):
        if k == event_at:
            value_at_event = column[-1]
        e = r.apply(call)
        column += e.truncated_steps
        assert not e.done.any()
    return column, value_at_event, calls, event_at


@pytest.mark.parametrize("c", P_CASES, ids=[ref.pendulum_id(c) for c in P_CASES])
def test_pendulum_truncated_column_is_one_on_exactly_the_truncating_steps(c):
    column, value_at_event, calls, event_at = run_pendulum(c)
    assert len(column) >= ref.P_STEPS
    want = ref.truncating_steps(c, len(column))
    assert [s + 1 for s, v in enumerate(column) if v] == want
    assert value_at_event == (1 if c.after else 0)  # what the array holds when the event comes
    taken_before = sum(1 for call in calls[:event_at] if call[0] == "step")
    if not c.after:
        if c.event == "set-limit":  # the step that would have truncated no longer does: the 0 must stay
            assert column[taken_before] == 0
        else:
            assert column[taken_before] == 1, "the step after the event truncates: 0 -> 1 across the event"
    elif c.flags & A:
        assert column[taken_before] == 0, "1 -> 0 across the event"
    elif c.event == "set-limit":
        assert column[taken_before] == 0, "the raised limit takes the flag back: 1 -> 0 without auto-reset"
    else:
        assert column[taken_before] == 1  # without auto-reset nothing re-arms the clock: the array holds 1 and keeps it


def test_pendulum_events_cross_both_transitions_and_rollouts_end_on_and_off_a_truncating_step():
    for flags in ref.P_FLAGS:
        for event in ref.P_EVENTS:
            crossed = set()
            for c in P_CASES:
                if c.flags == flags and c.event == event and c.shape == 4:
                    column, held, calls, event_at = run_pendulum(c)
                    taken = sum(1 for call in calls[:event_at] if call[0] == "step")
                    crossed.add((held, column[taken]))
            if flags & A and event != "set-limit":
                assert {(0, 1), (1, 0)} <= crossed, (flags, event, crossed)
            else:
                assert (0, 1) in crossed or event == "set-limit", (flags, event, crossed)
        ends = set()
        for c in P_CASES:
            if c.flags == flags and c.event.startswith("rollout-") and c.shape == 4:
                column, _, calls, event_at = run_pendulum(c)
                taken = sum(1 for call in calls[:event_at] if call[0] == "step")
                ends.add(column[taken + calls[event_at][1] - 1])
        assert ends == ({0, 1} if flags & A else {1}), (flags, ends)
    assert {c.shape for c in P_CASES} == {4, 8} and set(ref.P_FLAGS) == {T, A | T, A | S | T}


def test_the_restore_target_holds_the_opposite_value():
    """The engine a Pendulum snapshot is loaded into has stepped other_steps_before_restore(c) times from its own reset: its
    `truncated` array then holds the opposite of what the blob's holds."""
    for c in P_CASES:
        if c.event == "restore":
            tw = ref.PendulumReference(c)
            tw.apply(("reset",))
            held = [tw.apply(("step",)).truncated_steps[0] for _ in range(ref.other_steps_before_restore(c))][-1]
            assert held == (0 if c.after else 1)
