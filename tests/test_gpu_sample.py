"""Softmax action sampling inside the closed-loop fused rollouts (gymrs_set_sampling, GYMRS_CLOSED_LOOP_SAMPLE, gymrs_sample_actions)
against the CPU reference of tests/sample_ref.py: the rule restated in plain C (tests/cpp/sample_ref.c), a Philox4x32-10 in numpy,
the f32 twin.  The reference shares no code with the kernels and never loads the library; tests/test_sample_ref.py shows on the CPU
that its cases are worth comparing with.

The sampling kernels (gym-rs_amd/csrc/gymrs_sample.hip, gymrs_sample_fitness.hip, gymrs_table_sample_<env>.hip) are built per env,
flag set (10), lanes per work-item (4, 8; recording and transitions at 4), with and without the fitness hook, with and without a
parameter table, and each compiles four copies of rollout_block that a wave picks from at run time.  The matrix runs every one of
these instantiations at explore_ref's shapes: n = 1300 lanes, offsets 0, 6 (the per-lane block path) and 2^32 + 4, one policy /
whole waves uniform / gathered weights, H = 0 and 8, 40 steps in one launch and as 1 + 7 + 32.

Every comparison is bit for bit (uint32 views of floats, equal integers, statistics with ==) after every launch, no lane left out."""
import ctypes as C

import numpy as np
import pytest
import sample_ref as ref
import torch
from sample_ref import A, DIMS, F, S, T, bits
from test_gpu_closed_loop_table import DEV, Recorder, compare, same
from test_gpu_explore import action_buffer, rows_of
from test_gpu_transitions import Sink
from transitions_ref import SENTINEL

pytestmark = pytest.mark.gpu

FULL = A | S | T | F


def make_engine(gymrs, c, vec, sample=True, prepare=None, weights=None):
    """An engine for case c at `vec` lanes per work-item: its table and index (cases with one), reset, prepared, c's policy set and
    (unless sample is False) c's sampling settings"""
    rows = rows_of(gymrs, c)
    eng = gymrs.BatchedEngine(c.kind, c.n, global_env_offset=c.gid0, flags=c.flags, params=rows[0], lanes_per_thread=vec)
    if c.table:
        eng.set_param_table(rows)
        eng.set_param_index(c.index)
    eng.reset(seed=c.reset_seed, options=getattr(c, "bounds", None))
    prepare = prepare if prepare is not None else c.prepare
    if prepare is not None:
        eng.set_state(prepare(eng.get_state()))
    eng.set_policy(c.weights if weights is None else weights, hidden=c.hidden, lanes_per_policy=c.lanes_per_policy)
    if sample:
        eng.set_sampling(c.seed, scale=c.scale)
    return eng


def prob_buffer(n):
    buf = torch.full((n + 16,), -7.0, dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()  # torch filled it on its stream; the engine writes it on its own
    return buf


# ---- the matrix: every instantiation of the sampling closed-loop kernels --------------------------------------------------------------
@pytest.mark.parametrize("kind,flags,table,i", ref.matrix())
def test_sampling_launches_equal_the_cpu_reference(gymrs, kind, flags, table, i):
    """One reference, five engines: the plain and the fitness launch at 4 and at 8 lanes per work-item, the recording launch at 4.
    State, last results, final observations, statistics and tick after every launch; the record rows (`actions` = the action
    taken); the fitness records accumulated over the launches."""
    c = ref.matrix_case(kind, flags, table, i)
    want = ref.run_case(c)
    engines = {(mode, vec): make_engine(gymrs, c, vec) for mode, vec in (("fused", 4), ("fitness", 4), ("record", 4), ("fused", 8), ("fitness", 8))}
    rec = Recorder(kind, c.n, max(c.schedule))
    for key, eng in engines.items():
        same("start state", eng.get_state(), want[0].start_state, key, c.classes[key[1]], c.index)
    for k, steps in enumerate(c.schedule):
        for (mode, vec), eng in engines.items():
            eng.rollout_closed_loop(steps, lane_params=table, sample=True, fitness=mode == "fitness",
                                    record=rec.fresh() if mode == "record" else None)
        for (mode, vec), eng in engines.items():
            eng.sync()
            compare(eng, want[k], (mode, vec, k), c.classes[vec])
            if mode == "fitness":
                got = eng.policy_fitness()
                assert np.array_equal(got, want[k].fitness), ("fitness", vec, k, got.tolist(), want[k].fitness.tolist())
        rec.check(want[k], steps, flags, k, c.classes[4])
    assert not engines["fused", 4].policy_fitness().any()  # the plain call counts nothing
    assert engines["fused", 8].sampling() == (c.seed, c.scale)
    for eng in engines.values():
        eng.close()


# ---- the fused launch against the loop it replaces, and sample_actions alone: actions and probabilities -------------------------------
@pytest.mark.parametrize("gid0,policy_set,hidden,vec", [(0, (3, 512), 8, 4), (6, (3, 1), 0, 8), ((1 << 32) + 4, (1, 1), 8, 4), (6, (3, 512), 0, 4)])
@pytest.mark.parametrize("table", [False, True])
@pytest.mark.parametrize("kind", [0, 1])
def test_fused_equals_sample_actions_plus_step(gymrs, kind, table, gid0, policy_set, hidden, vec):
    """rollout_closed_loop(K, sample) == K x (sample_actions + step) on the device, both == the reference; every buffer
    sample_actions fills == the reference's action row of that step, and prob_dev == the reference's prob[action], bit for bit."""
    c = ref.case(kind, FULL, table, gid0, policy_set, hidden, ref.SPLITS[1])
    want = ref.run_case(c)
    rows = np.concatenate([w.rec_actions for w in want])
    probs = np.concatenate([w.prob for w in want])
    fused, loop = make_engine(gymrs, c, vec), make_engine(gymrs, c, vec)
    buf, pbuf = action_buffer(c.n), prob_buffer(c.n)
    for k, steps in enumerate(c.schedule):
        fused.rollout_closed_loop(steps, lane_params=table, sample=True)
    for t in range(ref.STEPS):
        loop.sample_actions(buf.data_ptr(), pbuf.data_ptr() if t % 2 == 0 else None)
        loop.sync()
        got = buf.cpu().numpy()
        same("sample_actions", got[:c.n], rows[t], t, c.classes[4], c.index)
        assert (got[c.n:] == 9).all()  # nothing beyond n_envs is written
        if t % 2 == 0:
            gp = pbuf.cpu().numpy()
            same("prob", gp[:c.n], probs[t], t, c.classes[4], c.index)
            assert (gp[c.n:] == -7.0).all()
        loop.step(buf.data_ptr())
    for name, eng in (("fused", fused), ("loop", loop)):
        eng.sync()
        compare(eng, want[-1], name, c.classes[vec])
    # buffers that are not aligned for the vector stores take the ragged path in every wave: same values
    odd, podd = action_buffer(c.n + 4), prob_buffer(c.n + 4)
    loop.sample_actions(odd.data_ptr() + 1, podd.data_ptr() + 4)
    fused.sample_actions(buf.data_ptr(), pbuf.data_ptr())
    loop.sync()
    fused.sync()
    assert np.array_equal(odd.cpu().numpy()[1:c.n + 1], buf.cpu().numpy()[:c.n]) and odd.cpu().numpy()[0] == 9 and odd.cpu().numpy()[c.n + 1] == 9
    assert np.array_equal(bits(podd.cpu().numpy()[1:c.n + 1]), bits(pbuf.cpu().numpy()[:c.n])) and podd.cpu().numpy()[0] == -7.0 and podd.cpu().numpy()[c.n + 1] == -7.0
    fused.close()
    loop.close()


# ---- transitions -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [f for f in ref.FLAG_SETS if f & A])
@pytest.mark.parametrize("table", [False, True])
@pytest.mark.parametrize("kind", [0, 1])
def test_sampling_transitions_equal_the_reference(gymrs, kind, table, flags):
    """gymrs_rollout_transitions(sample) against the per-step reference with the sampled actions: the record rows, final_obs written
    on the ended lane-steps only (the rest keeps the sentinel), start_obs; the light axes rotate with the flag set."""
    i = ref.FLAG_SETS.index(flags) + 10 * kind + 5 * table
    gid0, policy_set, hidden, schedule = ref.axes(i)
    c = ref.case(kind, flags, table, gid0, policy_set, hidden, schedule)
    run = ref.TransitionsRun(c)
    eng = make_engine(gymrs, c, 4)
    rec = Recorder(kind, c.n, max(c.schedule))
    sink = Sink(rec)
    ended = 0
    for k, steps in enumerate(c.schedule):
        want = run.launch(steps)
        eng.rollout_transitions(steps, record=rec.fresh(), lane_params=table, sample=True, **sink.fresh())
        eng.sync()
        compare(eng, want, ("transitions", k), c.classes[4])
        rec.check(want, steps, flags, ("transitions", k), c.classes[4])
        sink.check(want, steps, k, c.classes[4])
        ended += int(want.ended.sum())
    assert ended > 0
    eng.close()


# ---- corner policies ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["zero", "nan", "inf"])
@pytest.mark.parametrize("kind", [0, 1])
def test_corner_weights(gymrs, kind, which):
    """All-zero weights (every logit ties: the uniform draw); a NaN, or a +inf, output bias -- of action p % A in policy p, so the
    special logit is the first one in some lanes (a NaN or infinite maximum: all weights 0, the greedy action) and a later one in
    others (a NaN never wins and weighs nothing): plain at 8, recording at 4, per-step probabilities."""
    c = ref.case(kind, FULL, True, 6, (3, 1), 8, ref.SPLITS[1])
    n_actions = DIMS[kind][1]
    w = c.weights.copy()
    if which == "zero":
        w[:] = 0
    else:
        for p in range(c.n_policies):  # (the layout ends with b2[A]; the ReLU would turn a NaN of the hidden layer into 0)
            w[p, -n_actions + p % n_actions] = np.nan if which == "nan" else np.inf
    want = ref.run_case(c, weights=w)
    whole = ref.whole(want)
    prob = np.concatenate([x.prob for x in want])
    if which == "zero":
        assert set(whole.actions.ravel()) == set(range(n_actions)) and (prob == np.float32(1 / n_actions)).all()
    elif which == "inf":
        assert not whole.explored.any() and (prob == 1).all()  # the infinite logit is the maximum: greedy, with probability 1
    else:
        first = c.policies % n_actions == 0  # lanes whose NaN is logit 0: it is the maximum by the argmax rule
        assert (whole.actions[:, first] == 0).all() and (prob[:, first] == 1).all()
        assert (whole.actions[:, ~first] != (c.policies % n_actions)[~first]).all()  # elsewhere the NaN's action is never taken
        assert n_actions == 2 or whole.explored[:, ~first].any()  # (two actions: one is left)
    fused, recd, loop = (make_engine(gymrs, c, v, weights=w) for v in (8, 4, 4))
    rec = Recorder(kind, c.n, max(c.schedule))
    for k, steps in enumerate(c.schedule):
        fused.rollout_closed_loop(steps, lane_params=True, sample=True)
        recd.rollout_closed_loop(steps, lane_params=True, sample=True, record=rec.fresh())
        fused.sync()
        recd.sync()
        compare(fused, want[k], (which, 8, k), c.classes[8], nan_equal=True)
        compare(recd, want[k], (which, 4, k), c.classes[4], nan_equal=True)
        rec.check(want[k], steps, c.flags, (which, k), c.classes[4], nan_equal=True)
    buf, pbuf = action_buffer(c.n), prob_buffer(c.n)
    loop.sample_actions(buf.data_ptr(), pbuf.data_ptr())
    loop.sync()
    same("actions", buf.cpu().numpy()[:c.n], want[0].rec_actions[0], which, c.classes[4], c.index)
    same("prob", pbuf.cpu().numpy()[:c.n], want[0].prob[0], which, c.classes[4], c.index)
    for e in (fused, recd, loop):
        e.close()


@pytest.mark.parametrize("table", [False, True])
@pytest.mark.parametrize("kind", [0, 1])
def test_scale_0_is_uniform_and_scale_1e30_is_greedy(gymrs, kind, table):
    c0 = ref.case(kind, FULL, table, 6, (3, 512), 0, ref.SPLITS[1], scale=0.0)
    want = ref.run_case(c0)
    assert (np.concatenate([x.prob for x in want]) == np.float32(1 / DIMS[kind][1])).all()
    eng = make_engine(gymrs, c0, 8)
    for k, steps in enumerate(c0.schedule):
        eng.rollout_closed_loop(steps, lane_params=table, sample=True, fitness=True)
        compare(eng, want[k], ("scale 0", k), c0.classes[8])
        assert np.array_equal(eng.policy_fitness(), want[k].fitness)
    eng.close()
    # 1e30: the argmax wherever the logits have no exact tie -- the reference says there is none here -- so the greedy launch
    c1 = ref.case(kind, FULL, table, 6, (3, 512), 8, ref.SPLITS[1], scale=1e30)
    hard, greedy = ref.Run(c1), ref.Run(c1)
    sampled, plain = make_engine(gymrs, c1, 4), make_engine(gymrs, c1, 4, sample=False)
    rec = {name: Recorder(kind, c1.n, max(c1.schedule)) for name in ("sampled", "plain")}
    for k, steps in enumerate(c1.schedule):
        w, g = hard.launch(steps, (c1.seed, c1.scale)), greedy.launch(steps, None)
        assert np.array_equal(w.rec_actions, g.rec_actions) and (w.prob == 1).all()
        sampled.rollout_closed_loop(steps, lane_params=table, sample=True, record=rec["sampled"].fresh())
        plain.rollout_closed_loop(steps, lane_params=table, record=rec["plain"].fresh())
        for name, e in (("sampled", sampled), ("plain", plain)):
            e.sync()
            compare(e, w, (name, k), c1.classes[4])
            rec[name].check(w, steps, c1.flags, (name, k), c1.classes[4])
    sampled.close()
    plain.close()


# ---- opt-in ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("table", [False, True])
@pytest.mark.parametrize("vec", [4, 8])
@pytest.mark.parametrize("kind", [0, 1])
def test_settings_without_the_flag_are_the_greedy_launch(gymrs, kind, vec, table):
    """Settings present and the flag absent leave the greedy result (and rollout_policy's, without a table): plain, fitness,
    recording (at 4) and transitions (at 4); the settings survive set_policy and are in no clone or snapshot."""
    c = ref.case(kind, FULL, table, 6, (3, 512), 8, ref.SPLITS[1])
    run = ref.Run(c)
    unflagged = make_engine(gymrs, c, vec)
    plain = make_engine(gymrs, c, vec, sample=False)
    old = make_engine(gymrs, c, vec) if not table else None
    recs = {name: Recorder(kind, c.n, max(c.schedule)) for name in ("unflagged", "plain")}
    snap = len(unflagged.snapshot())
    for k, steps in enumerate(c.schedule):
        fitness, record = k == 1, k == 2 and vec == 4
        want = run.launch(steps, None, count=fitness)
        unflagged.rollout_closed_loop(steps, lane_params=table, fitness=fitness, record=recs["unflagged"].fresh() if record else None)
        plain.rollout_closed_loop(steps, lane_params=table, fitness=fitness, record=recs["plain"].fresh() if record else None)
        if old is not None:
            (old.rollout_policy_fitness if fitness else old.rollout_policy)(steps)
        for name, eng in (("unflagged", unflagged), ("plain", plain), ("rollout_policy", old)):
            if eng is not None:
                eng.sync()
                compare(eng, want, (name, k), c.classes[vec])
                assert np.array_equal(eng.policy_fitness(), want.fitness), (name, k)
        if record:
            for name in recs:
                recs[name].check(want, steps, c.flags, (name, k), c.classes[4])
    assert want.fitness.any() and unflagged.sampling() == (c.seed, c.scale) and len(unflagged.snapshot()) == snap
    unflagged.set_policy(c.weights, hidden=c.hidden, lanes_per_policy=c.lanes_per_policy)
    assert unflagged.sampling() == (c.seed, c.scale)  # set_policy keeps the settings
    clone = unflagged.clone()
    with pytest.raises(gymrs.GymrsError, match="gymrs_set_sampling"):
        clone.sampling()
    # the settings take effect in stream order: a launch enqueued before a change plays the old ones
    other = (c.seed + 1, float(np.float32(0.7)))
    unflagged.set_sampling(c.seed, temperature=ref.TEMPERATURE)
    assert unflagged.sampling() == (c.seed, c.scale)
    unflagged.rollout_closed_loop(5, lane_params=table, sample=True)
    unflagged.set_sampling(other[0], scale=other[1])
    unflagged.rollout_closed_loop(6, lane_params=table, sample=True)
    run.launch(5, (c.seed, c.scale))
    want = run.launch(6, other)
    unflagged.sync()
    compare(unflagged, want, "after the change", c.classes[vec])
    unflagged.set_sampling(None)
    with pytest.raises(gymrs.GymrsError, match="gymrs_set_sampling"):
        unflagged.sampling()
    for eng in (unflagged, plain, old, clone):
        if eng is not None:
            eng.close()


# ---- the refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals(gymrs):
    c = ref.case(0, A | S, True, 0, (3, 512), 0)
    eng = make_engine(gymrs, c, 4, sample=False)
    before = eng.get_state(), eng.tick()
    buf = action_buffer(c.n)
    rec = Recorder(0, c.n, 4)
    sink = Sink(rec)

    def untouched():
        assert np.array_equal(bits(eng.get_state()), bits(before[0])) and eng.tick() == before[1]

    with pytest.raises(gymrs.GymrsError, match="gymrs_set_sampling"):  # the flag without settings
        eng.rollout_closed_loop(3, lane_params=True, sample=True)
    with pytest.raises(gymrs.GymrsError, match="gymrs_set_sampling"):
        eng.rollout_closed_loop(3, lane_params=True, sample=True, fitness=True)
    with pytest.raises(gymrs.GymrsError, match="gymrs_set_sampling"):
        eng.rollout_transitions(3, record=rec.fresh(), lane_params=True, sample=True, **sink.fresh())
    with pytest.raises(gymrs.GymrsError, match="gymrs_set_sampling"):
        eng.sample_actions(buf.data_ptr())
    with pytest.raises(gymrs.GymrsError, match="gymrs_set_sampling"):
        eng.sampling()
    untouched()
    for scale in (float("nan"), float("inf"), -1.0, -1e-38):
        bad = gymrs.Sampling(1, scale, 0)
        assert eng._lib.gymrs_set_sampling(eng._h, C.byref(bad)) == 1 and b"scale" in eng._lib.gymrs_last_error()
    bad = gymrs.Sampling(1, 1.0, 1)
    assert eng._lib.gymrs_set_sampling(eng._h, C.byref(bad)) == 1 and b"reserved" in eng._lib.gymrs_last_error()
    with pytest.raises(gymrs.GymrsError, match="gymrs_set_sampling"):  # a refused call stored nothing
        eng.sampling()
    with pytest.raises(ValueError):
        eng.set_sampling(1, temperature=0.5, scale=3.0)
    with pytest.raises(ValueError):
        eng.set_sampling(1)
    assert eng._lib.gymrs_set_sampling(None, None) == 1 and eng._lib.gymrs_get_sampling(eng._h, None) == 1
    assert eng._lib.gymrs_sample_actions(eng._h, None, None) == 1 and eng._lib.gymrs_sample_actions(None, C.c_void_p(buf.data_ptr()), None) == 1
    eng.set_sampling(7, scale=0.0)  # the uniform policy is legal
    assert eng.sampling() == (7, 0.0)
    # with settings: both action sources at once, and the descriptor's other refusals
    eng.set_exploration(3, threshold=100)
    for call in (lambda: eng.rollout_closed_loop(3, lane_params=True, sample=True, explore=True),
                 lambda: eng.rollout_transitions(3, record=rec.fresh(), lane_params=True, sample=True, explore=True, **sink.fresh())):
        with pytest.raises(gymrs.GymrsError, match="GYMRS_CLOSED_LOOP_SAMPLE.*GYMRS_CLOSED_LOOP_EXPLORE"):
            call()
    with pytest.raises(gymrs.GymrsError, match="GYMRS_CLOSED_LOOP_LANE_PARAMS"):
        eng.rollout_closed_loop(3, sample=True)
    with pytest.raises(gymrs.GymrsError, match="recording fitness"):
        eng.rollout_closed_loop(3, lane_params=True, sample=True, fitness=True, record=rec.fresh())
    for more in (2, 8, 1 << 31):
        with pytest.raises(gymrs.GymrsError, match="unknown flag bits"):
            eng.rollout_closed_loop(3, flags=gymrs.CLOSED_LOOP_LANE_PARAMS | gymrs.CLOSED_LOOP_SAMPLE | more)
        with pytest.raises(gymrs.GymrsError, match="unknown flag bits"):
            eng.rollout_transitions(3, record=rec.fresh(), flags=gymrs.CLOSED_LOOP_LANE_PARAMS | gymrs.CLOSED_LOOP_SAMPLE | more, **sink.fresh())
    desc = gymrs.ClosedLoopDesc(3, gymrs.CLOSED_LOOP_LANE_PARAMS | gymrs.CLOSED_LOOP_SAMPLE, None, 1)
    assert eng._lib.gymrs_rollout_closed_loop(eng._h, C.byref(desc)) == 1 and b"reserved" in eng._lib.gymrs_last_error()
    with pytest.raises(gymrs.GymrsError, match="GYMRS_POLICY_FITNESS_MAX_STEPS"):
        eng.rollout_closed_loop((1 << 24) + 1, lane_params=True, sample=True, fitness=True)
    eng.rollout_closed_loop(0, lane_params=True, sample=True)  # a no-op
    untouched()
    final, start = sink.host()
    assert (final == SENTINEL).all() and (start == SENTINEL).all()  # no refused call wrote a buffer
    eng.set_policy(None)  # the settings need no policy; the calls that play them do
    assert eng.sampling() == (7, 0.0)
    with pytest.raises(gymrs.GymrsError, match="no policy"):
        eng.rollout_closed_loop(3, lane_params=True, sample=True)
    with pytest.raises(gymrs.GymrsError, match="no policy"):
        eng.sample_actions(buf.data_ptr())
    untouched()
    eng.close()
    pend = gymrs.BatchedEngine(gymrs.PENDULUM, 64)
    pend.reset(seed=1)
    with pytest.raises(gymrs.GymrsError, match="Pendulum"):
        pend.set_sampling(1, scale=1.0)
    with pytest.raises(gymrs.GymrsError, match="Pendulum"):
        pend.set_sampling(None)
    pend.close()


# ---- the native sharder --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blocks", [2, 3])
@pytest.mark.parametrize("kind", [0, 1])
def test_sharded_blocks_on_one_gpu_equal_one_engine(gymrs, kind, blocks):
    """k blocks on device 0 of a batch at offset 6 (the first block takes the per-lane block path): state, statistics and fitness
    equal ONE engine's and the reference's"""
    c = ref.case(kind, FULL, True, 6, (3, 512), 8, ref.SPLITS[1])
    want = ref.run_case(c)
    rows = rows_of(gymrs, c)
    one = make_engine(gymrs, c, 4)
    sh = gymrs.ShardedEngine(kind, c.n, [0] * blocks, global_env_offset=c.gid0, flags=c.flags, params=rows[0])
    sh.set_param_table(rows)
    sh.set_param_index(c.index)
    sh.reset(seed=c.reset_seed)
    if c.prepare is not None:
        start = c.prepare(sh.get_state())
        for s in sh.shards:
            s.set_state(start[:, s.first_lane:s.first_lane + s.n_envs])
    sh.set_policy(c.weights, hidden=c.hidden, lanes_per_policy=c.lanes_per_policy)
    with pytest.raises(gymrs.GymrsError, match="gymrs_set_sampling"):
        sh.rollout_closed_loop(3, lane_params=True, sample=True)
    sh.set_sampling(c.seed, scale=c.scale)
    assert sh.sampling() == (c.seed, c.scale) and all(s.sampling() == (c.seed, c.scale) for s in sh.shards)
    for k, steps in enumerate(c.schedule):
        sh.rollout_closed_loop(steps, lane_params=True, sample=True, fitness=True)
        one.rollout_closed_loop(steps, lane_params=True, sample=True, fitness=True)
        sh.sync()
        w = want[k]
        kw = dict(classes=c.classes[4], index=c.index)
        same("state", sh.get_state(), w.state, k, **kw)
        same("state, one engine", sh.get_state(), one.get_state(), k, **kw)
        reward, done, trunc = sh.get_step_result()
        same("reward", reward, w.reward, k, **kw)
        same("done", done, w.done, k, **kw)
        same("truncated", trunc, w.truncated, k, **kw)
        same("final_obs", sh.get_final_obs(), w.final, k, **kw)
        assert np.array_equal(sh.stats(), w.stats) and np.array_equal(sh.stats(), one.stats()), (k, sh.stats(), w.stats)
        assert all(s.tick()[0] == w.tick for s in sh.shards)
        assert np.array_equal(sh.policy_fitness(), w.fitness) and np.array_equal(one.policy_fitness(), w.fitness), k
    sh.set_sampling(None)
    with pytest.raises(gymrs.GymrsError, match="gymrs_set_sampling"):
        sh.rollout_closed_loop(3, lane_params=True, sample=True)
    sh.close()
    one.close()
