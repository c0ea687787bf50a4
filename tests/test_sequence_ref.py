"""tests/sequence_ref.py without a GPU: the model equals the single-feature references bit for bit where a sequence stays inside one
family, the committed list of sequences meets its coverage conditions, every sequence is worth comparing with, and every planted
fault of sequence_ref.FAULTS shows in at least one of them."""
import collections

import closed_loop_ref as cl
import closed_loop_table_ref as clt
import explore_ref as ex
import lane_params_ref as lp
import numpy as np
import policy_fitness_ref as pf
import pytest
import sample_ref as sr
import sequence_ref as sq
import transitions_ref as tr
from sequence_ref import A, F, S, T, bits

from oracle.bindings import TwinEngine

FULL = A | S | T | F


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(bits(got.astype(np.float32)) if got.dtype.kind == "f" else got, bits(want.astype(np.float32)) if want.dtype.kind == "f" else want), what


def model_of(c, flags, cap, hidden, lpp, weights, table, prepare=None):
    """a Model at a case of one of the single-feature references: its rows, index, weights and start state"""
    m = sq.Model(sq.Config(c.kind, c.n, c.gid0, flags, cap, hidden, lpp))
    m.policy.weights = weights
    if table:
        m.rows, m.index, m.table = list(c.rows), np.asarray(c.index, np.int64), True
    m.apply(("reset", c.reset_seed, None))
    if prepare is not None:
        m.ref.set_state(prepare(m.state))
    return m


def same_engine(m, x, what):
    for f in ("state", "obs", "reward", "done", "truncated", "final", "tick"):
        same(getattr(m, f), getattr(x, f), (what, f))
    assert np.array_equal(m.stats, x.stats), (what, m.stats, x.stats)


def same_rows(m, x, what):
    for f in ("obs", "actions", "reward", "done", "truncated"):
        same(m.record[f], getattr(x, "rec_" + f), (what, f))


# ---- the model is the single-feature references where a sequence stays in one family -------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("mode", ["fitness", "record", "plain"])
def test_greedy_launches_under_a_table_equal_closed_loop_table_ref(kind, mode):
    c = clt.case(kind, 0, FULL, 8)
    run = clt.Run(c)
    m = model_of(c, FULL, clt.MAX_EPISODE_STEPS, 8, c.lanes_per_policy, c.weights, True, c.prepare)
    for k, steps in enumerate(c.schedule):
        x = run.launch(steps)
        m.apply(("closed", "greedy", mode, steps, True))
        same_engine(m, x, (k, steps))
        if mode == "record":
            same_rows(m, x, k)
    if mode == "fitness":
        assert np.array_equal(m.fitness, x.fitness) and m.fitness.any()
    assert m.told_apart() > 0  # (K = 5 rows here: the neighbour of sequence_ref.K = 3 is another row for most lanes)


@pytest.mark.parametrize("kind,table", [(0, False), (1, True)])
def test_exploring_launches_equal_explore_ref(kind, table):
    c = ex.case(kind, FULL, table, gid0=6, policy_set=(3, 1), hidden=8, schedule=(1, 7, 32))
    run = ex.Run(c)
    m = model_of(c, FULL, ex.MAX_EPISODE_STEPS, 8, 1, c.weights, table, c.prepare)
    m.apply(("set_exploration", c.seed, c.threshold))
    for k, steps in enumerate(c.schedule):
        x = run.launch(steps, (c.seed, c.threshold))
        m.apply(("closed", "explore", "record" if k % 2 else "fitness", steps, table))
        same_engine(m, x, (k, steps))
        if k % 2:
            same_rows(m, x, k)
    per_step = ex.Run(c)  # the per-step pair: explore_actions, step
    m = model_of(c, FULL, ex.MAX_EPISODE_STEPS, 8, 1, c.weights, table, c.prepare)
    m.apply(("set_exploration", c.seed, c.threshold))
    for k in range(9):
        x = per_step.launch(1, (c.seed, c.threshold))
        m.apply(("step", "explore", 0, k))
        same_engine(m, x, k)


@pytest.mark.parametrize("kind,table", [(0, True), (1, False)])
def test_sampling_launches_and_transitions_equal_sample_ref(kind, table):
    c = sr.case(kind, FULL, table, gid0=(1 << 32) + 4, policy_set=(3, 512), hidden=0, schedule=(1, 7, 32))
    run, trun = sr.Run(c), sr.TransitionsRun(c)
    m = model_of(c, FULL, ex.MAX_EPISODE_STEPS, 0, 512, c.weights, table, c.prepare)
    mt = model_of(c, FULL, ex.MAX_EPISODE_STEPS, 0, 512, c.weights, table, c.prepare)
    for mm in (m, mt):
        mm.apply(("set_sampling", c.seed, c.scale))
    for k, steps in enumerate(c.schedule):
        x = run.launch(steps, (c.seed, c.scale))
        m.apply(("closed", "sample", "record", steps, table))
        same_engine(m, x, (k, steps))
        same_rows(m, x, k)
        y = trun.launch(steps)
        mt.apply(("transitions", "sample", steps, table))
        same_engine(mt, y, ("transitions", k))
        same_rows(mt, y, ("transitions", k))
        same(mt.record["start_obs"], y.start_obs, k)
        assert np.array_equal(mt.record["ended"], y.ended)
        mask = np.broadcast_to(y.ended[:, None, :], y.final_obs.shape)
        same(mt.record["final_obs"][mask], y.final_obs[mask], ("final_obs", k))
    assert y.ended.any()


@pytest.mark.parametrize("kind,table,explore", [(0, True, True), (1, False, False)])
def test_transitions_equal_transitions_ref(kind, table, explore):
    c = tr.case(kind, 0, A | S | T, 8, table, explore)
    run = tr.Run(c)
    m = model_of(c, A | S | T, cl.MAX_EPISODE_STEPS, 8, c.lanes_per_policy, c.weights, table, c.prepare)
    m.apply(("set_exploration", c.seed, c.threshold))
    for k, steps in enumerate(c.schedule[:3]):
        x = run.launch(steps)
        m.apply(("transitions", "explore" if explore else "greedy", steps, table))
        same_engine(m, x, k)
        same_rows(m, x, k)
        mask = np.broadcast_to(x.ended[:, None, :], x.final_obs.shape)
        same(m.record["final_obs"][mask], x.final_obs[mask], k)
        same(m.record["start_obs"], x.start_obs, k)


@pytest.mark.parametrize("kind", [0, 1])
def test_random_policy_paths_equal_the_table_reference(kind):
    """rollout, rollout_record, step and step_host play fill_actions(seed, t): TableReference's own default policy"""
    c = lp.matrix_case(kind, FULL, lp.OFFSETS[0], stages=())
    want = lp.TableReference(kind, c.n, c.gid0, c.rows, c.index, FULL, lp.RESET_SEED, action_seed=lp.ACTION_SEED)
    m = sq.Model(sq.Config(kind, c.n, c.gid0, FULL, lp.MAX_EPISODE_STEPS, 0, 1))
    m.rows, m.index, m.table = list(c.rows), np.asarray(c.index, np.int64), True
    m.apply(("reset", lp.RESET_SEED, None))
    for op, steps in ((("rollout", 7, lp.ACTION_SEED, 0), 7), (("step", "step", lp.ACTION_SEED, 7), 1), (("rollout_record", 12, lp.ACTION_SEED, 8), 12),
                      (("step", "step_host", lp.ACTION_SEED, 20), 1)):
        first = len(want.records)
        want.step(steps)
        m.apply(op)
        same_engine(m, want, op)
        assert (m.record is not None) == (op[0] == "rollout_record")
        if m.record is not None:
            for f in ("obs", "actions", "reward", "done", "truncated"):
                same(m.record[f], np.stack([getattr(x, f) for x in want.records[first:]]), (op, f))
    assert want.stats[2] > 0 and want.final.any()


@pytest.mark.parametrize("kind", [0, 1])
def test_uniform_greedy_launches_equal_closed_loop_ref_and_policy_fitness_ref(kind):
    """closed_loop_ref.reference is ONE twin with the twin's own statistics: the model's three equal rows and rebuilt statistics
    must give the same, and the records policy_fitness_ref.of_case folds from it"""
    for flags in (FULL, T, A | S):
        c = cl.case(kind, 0, flags, 7, lp.default_row(kind, 0))
        launches = cl.run_case(c)
        fitness = pf.of_case(c, launches)
        m = sq.Model(sq.Config(kind, c.n, c.gid0, flags, cl.MAX_EPISODE_STEPS, 7, c.lanes_per_policy))
        m.policy.weights = c.weights
        m.apply(("reset", c.reset_seed, None))
        if c.prepare is not None:
            m.ref.set_state(c.prepare(m.state, 0))
        for k, (steps, x) in enumerate(zip(c.schedule, launches)):
            m.apply(("policy", "fitness", steps))
            same_engine(m, x, (flags, k))
            assert np.array_equal(m.fitness, fitness[k]), (flags, k)


@pytest.mark.parametrize("kind,flags", [(0, A | S | T), (0, 0), (0, T), (1, A | S | T)])
def test_a_lane_that_changes_its_row_takes_its_episode_along(kind, flags):
    """All lanes from row 0 to row 1 between two steps == one twin whose params are assigned between the same two steps: the
    episode clocks (time limit) and CartPole's steps_beyond_terminated (no auto-reset: the reward) travel from twin to twin."""
    n, rows = 300, lp.make_rows(kind, 2, 31, 9)
    r = lp.TableReference(kind, n, 12345, rows, np.zeros(n, np.int64), flags, 3, action_seed=6)
    tw = TwinEngine(lp.twin(), kind, n, rows[0], flags=flags, gid0=12345)
    tw.reset(3)
    state = sq.new_state(kind, tw.get_state(), n)  # (lanes next to their end: episodes end under both rows, at different steps)
    tw.set_state(state)
    r.set_state(state)
    ended = False
    for t in range(30):
        if t == 11:
            r.set_index(np.ones(n, np.int64))
            tw.set_params(rows[1])
        tw.step(tw.fill_actions(6, t))
        r.step(1)
        same(r.state, tw.get_state(), t)
        for got, want, what in zip((r.reward, r.done, r.truncated), tw.get_result(), ("reward", "done", "truncated")):
            same(got, want, (t, what))
        ended |= t > 11 and bool(r.done.any() or r.truncated.any())
    if flags & A and flags & S:
        assert np.array_equal(r.stats, tw.stats())
    clocks = [x.get_clocks() for x in r.tws]
    assert ended
    assert not np.array_equal(clocks[0][0], clocks[1][0]) or not (flags & T) or not (flags & A)  # (the other twin went its own way)


# ---- the committed list -------------------------------------------------------------------------------------------------------------
OP_KINDS = (["step", "step_host", "policy+step", "explore+step", "sample+step", "many-hip", "many-graph", "rollout", "rollout_record",
             "rollout_policy", "rollout_policy_record", "rollout_policy_fitness"]
            + [f"closed-{s}-{m}{t}" for s in ("greedy", "explore", "sample") for m in ("plain", "fitness", "record") for t in ("", "-lp")]
            + [f"transitions-{s}{t}" for s in ("greedy", "explore", "sample") for t in ("", "-lp")] + list(sq.EVENTS) + list(sq.QUIET))


def test_the_committed_list_meets_its_coverage_conditions(capsys):
    seqs = sq.sequences()
    assert seqs == tuple(sq.generate(sq.GENERATOR_SEED))  # deterministic
    assert sq.MIN_SEQUENCES <= len(seqs) <= sq.MAX_SEQUENCES
    cov = sq.Coverage()
    refusals, tunings, eight, special = collections.Counter(), set(), set(), set()
    for c, ops in seqs:
        cov.add(c, ops)
        assert sq.MIN_OPS <= len(ops) <= sq.MAX_OPS and c.n <= 5000 and c.n in sq.LANES and c.flags in sq.FLAG_SETS and c.gid0 in sq.OFFSETS + (sq.BIG_OFFSET,)
        assert ops[0][0] == "reset" and all(sq.steps_of(op) <= sq.MAX_STEPS for op in ops)
        assert all(32 <= op[2] for op in ops if op[:2] == ("many", "graph"))
        assert 8 * sum(op[0] == "refused" for op in ops) <= len(ops)
        table, vec, hint, under, launched = False, 4, 0, 0, True
        for op in ops:
            if op[0] == "refused":
                assert sq.REFUSALS[op[1]][0](c, table), (c, op)
                refusals[op[1]] += 1
            if c.kind == 2:
                assert op[0] in ("reset", "step", "many", "rollout", "rollout_record", "set_state", "set_params", "tune", "stats_clear", "clone",
                                 "restore", "sync", "stats", "refused") and op[:2] not in (("step", "policy"), ("step", "explore"), ("step", "sample"))
                assert not (op[:2] == ("many", "graph") and c.flags & T)
            if op[0] in ("policy",) or (op[0] == "closed" and not op[4]) or (op[0] == "transitions" and not op[3]):
                assert not table, (c, op)
            if op[0] == "transitions":
                assert c.flags & A
            if op[0] == "set_index" or op[:2] == ("table", False):
                assert table
            # counted here by hand, not by Coverage: what runs at 8 lanes per work-item, and the conditions on single sequences
            if op[0] == "tune":
                assert launched, (c, "a tuning nothing was launched under", op)
                vec, hint, launched = op[1], op[2], False
            if sq.op_class(op):
                launched = True
                tunings.update({("vec", vec), ("hint", hint)})
            what = sq.at_eight(op)
            if vec == 8 and what and c.kind != 2 and c.n >= sq.WIDE:
                eight.update({(c.kind, what)} | ({(sq.WIDE, what)} if c.n == sq.WIDE else set()))
            if op[0] == "set_index" and c.kind == 0 and c.flags & A and c.flags & T and under >= c.cap:
                special.add("set_index")
            if table and (op[0] == "set_params" or op[:2] == ("table", False)):
                assert under > 0, (c, "a table went without a launch under it")
            if op[0] == "table":
                table, under = bool(op[1]), 0
            elif op[0] == "set_params":
                table = False
            under += sq.steps_of(op) if table else 0
        assert launched
        if c.kind == 0 and c.flags & (A | S | T) == A | S | T and c.cap == 45 and c.n >= 1024 and sum(sq.steps_of(op) for op in ops[:4]) >= 2 * c.cap:
            special.add("cap45")
    missing = cov.missing(OP_KINDS)
    with capsys.disabled():
        print(f"\n{len(seqs)} sequences, {sum(len(ops) for _, ops in seqs)} ops, {sum(sq.steps_of(op) for _, ops in seqs for op in ops)} steps")
        for kind in OP_KINDS:
            print(f"  {kind:28s} {cov.kinds.get(kind, 0):3d}")
        print("  lanes:", dict(cov.lanes), " refusals:", dict(refusals))
        print("  at 8 lanes per work-item (0 CartPole, 1 MountainCar on 257 lanes or more; 257: on 257 lanes):", sorted(eight))
        print("  pairs of stepping classes still open:", len(cov.pairs), " event followers still open:", len(cov.follows))
    assert not missing, missing
    assert set(refusals) == set(sq.REFUSALS), set(sq.REFUSALS) - set(refusals)  # every refusal of the fixed list is drawn
    assert tunings == {("vec", 4), ("vec", 8)} | {("hint", h) for h in range(4)}, tunings
    assert eight == {(k, w) for k in (0, 1, sq.WIDE) for w in sq.AT_EIGHT}, {(k, w) for k in (0, 1, sq.WIDE) for w in sq.AT_EIGHT} - eight
    assert special == {"set_index", "cap45"}, special


def test_every_sequence_is_worth_comparing_with():
    missing = {sq.sequence_id(k, c): m for k, (c, ops) in enumerate(sq.sequences()) for m in [sq.worth_comparing(c, ops)] if m}
    assert not missing, missing


@pytest.mark.parametrize("fault", sq.FAULTS)
def test_every_planted_fault_shows_in_a_committed_sequence(fault, capsys):
    found = []
    needs = {"clone-box": lambda c, ops: any(op[0] == "clone" for op in ops) and any(op[0] == "reset" and op[2] for op in ops),
             "fused-final": lambda c, ops: c.flags & F, "set-params-table": lambda c, ops: any(op[0] == "set_params" for op in ops),
             "stats-clear-open": lambda c, ops: ("stats_clear",) in ops, "record8-shift": lambda c, ops: any(op[:2] == ("tune", 8) for op in ops),
             "restore-truncated": lambda c, ops: ("restore",) in ops and c.flags & T}[fault]
    for k, (c, ops) in enumerate(sq.sequences()):
        if not needs(c, ops) or len(found) >= 3:  # (the model is run on the sequences the fault can show in; three of them are enough)
            continue
        d = sq.first_difference(c, ops, (fault,))
        if d is not None:
            found.append(f"{sq.sequence_id(k, c)} at op {d[0]} ({sq.fmt(d[1])}): {', '.join(d[2])}")
    with capsys.disabled():
        print(f"\n{fault}: {len(found)} sequences; first: {found[:1]}")
    assert found, fault


def test_the_intact_model_is_deterministic():
    c, ops = sq.sequences()[0]
    a, b = sq.snapshot(sq.run(c, ops)), sq.snapshot(sq.run(c, ops))
    assert a.keys() == b.keys() and all(np.array_equal(a[f].view(np.uint8), b[f].view(np.uint8)) for f in a)
