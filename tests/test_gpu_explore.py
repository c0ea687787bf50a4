"""Epsilon-greedy exploration inside the closed-loop fused rollout (gymrs_set_exploration, GYMRS_CLOSED_LOOP_EXPLORE,
gymrs_explore_actions) against the CPU reference of tests/explore_ref.py: a Philox4x32-10 in numpy, the f32 twin, the policy of
tests/cpp/policy_ref.c.  The reference shares no code with the kernels and never loads the library; tests/test_explore_ref.py shows
on the CPU that its cases are worth comparing with.

The exploring kernels (gym-rs_amd/csrc/gymrs_explore.hip, gymrs_explore_fitness.hip, gymrs_table_explore_<env>.hip) are built per env,
flag set (10), lanes per work-item (4, 8; recording at 4), with and without the fitness hook, with and without a parameter table,
and each compiles four copies of rollout_block that a wave picks from at run time.  The matrix runs every one of these
instantiations: n = 1300 lanes (five full waves and a ragged one at 4 lanes per work-item, two and a ragged one at 8), offsets 0, 6
(the per-lane block path) and 2^32 + 4, one policy / whole waves uniform / gathered weights, H = 0 and 8, 40 steps in one launch
and as 1 + 7 + 32, threshold 16384.

Every comparison is bit for bit (uint32 views of floats, equal integers, statistics with ==) after every launch, no lane left out."""
import ctypes as C

import explore_ref as ref
import lane_params_ref as lp
import numpy as np
import pytest
import torch
from explore_ref import A, COPIES, DIMS, F, S, T, bits
from test_gpu_closed_loop_table import DEV, Recorder, compare, same

pytestmark = pytest.mark.gpu

FULL = A | S | T | F


def rows_of(gymrs, c):
    return lp.rows_for(type(gymrs.engine.default_params(c.kind)), c.rows)


def make_engine(gymrs, c, vec, explore=True, prepare=None):
    """An engine for case c at `vec` lanes per work-item: its table and index (cases with one), reset, prepared, c's policy set and
    (unless explore is False) c's exploration settings"""
    rows = rows_of(gymrs, c)
    eng = gymrs.BatchedEngine(c.kind, c.n, global_env_offset=c.gid0, flags=c.flags, params=rows[0], lanes_per_thread=vec)
    if c.table:
        eng.set_param_table(rows)
        eng.set_param_index(c.index)
    eng.reset(seed=c.reset_seed, options=getattr(c, "bounds", None))
    prepare = prepare if prepare is not None else c.prepare
    if prepare is not None:
        eng.set_state(prepare(eng.get_state()))
    eng.set_policy(c.weights, hidden=c.hidden, lanes_per_policy=c.lanes_per_policy)
    if explore:
        eng.set_exploration(c.seed, threshold=c.threshold)
    return eng


def action_buffer(n):
    buf = torch.full((n + 16,), 9, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()  # torch filled it on its stream; the engine writes it on its own
    return buf


# ---- the matrix: every instantiation of the exploring kernels -----------------------------------------------------------------------
@pytest.mark.parametrize("kind,flags,table,i", ref.matrix())
def test_exploring_launches_equal_the_cpu_reference(gymrs, kind, flags, table, i):
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
            eng.rollout_closed_loop(steps, lane_params=table, explore=True, fitness=mode == "fitness",
                                    record=rec.fresh() if mode == "record" else None)
        for (mode, vec), eng in engines.items():
            eng.sync()
            compare(eng, want[k], (mode, vec, k), c.classes[vec])
            if mode == "fitness":
                got = eng.policy_fitness()
                assert np.array_equal(got, want[k].fitness), ("fitness", vec, k, got.tolist(), want[k].fitness.tolist())
        rec.check(want[k], steps, flags, k, c.classes[4])
    assert not engines["fused", 4].policy_fitness().any()  # the plain call counts nothing
    assert engines["fused", 8].exploration() == (c.seed, c.threshold)
    for eng in engines.values():
        eng.close()


# ---- the fused launch against the loop it replaces, and explore_actions alone -------------------------------------------------------
@pytest.mark.parametrize("gid0,policy_set,hidden,vec", [(0, (3, 512), 8, 4), (6, (3, 1), 0, 8), ((1 << 32) + 4, (1, 1), 8, 4), (6, (3, 512), 0, 4)])
@pytest.mark.parametrize("table", [False, True])
@pytest.mark.parametrize("kind", [0, 1])
def test_fused_equals_explore_actions_plus_step(gymrs, kind, table, gid0, policy_set, hidden, vec):
    """rollout_closed_loop(K, explore) == K x (explore_actions + step) on the device, both == the reference; every buffer
    explore_actions fills == the reference's action row of that step (it works under a table, like policy_actions)."""
    c = ref.case(kind, FULL, table, gid0, policy_set, hidden, ref.SPLITS[1])
    want = ref.run_case(c)
    rows = np.concatenate([w.rec_actions for w in want])
    fused, loop = make_engine(gymrs, c, vec), make_engine(gymrs, c, vec)
    buf = action_buffer(c.n)
    for k, steps in enumerate(c.schedule):
        fused.rollout_closed_loop(steps, lane_params=table, explore=True)
    for t in range(ref.STEPS):
        loop.explore_actions(buf.data_ptr())
        loop.sync()
        got = buf.cpu().numpy()
        same("explore_actions", got[:c.n], rows[t], t, c.classes[4], c.index)
        assert (got[c.n:] == 9).all()  # nothing beyond n_envs is written
        loop.step(buf.data_ptr())
    for name, eng in (("fused", fused), ("loop", loop)):
        eng.sync()
        compare(eng, want[-1], name, c.classes[vec])
    # an action buffer that is not 4-byte aligned takes the ragged path in every wave: same values
    odd = action_buffer(c.n + 4)
    loop.explore_actions(odd.data_ptr() + 1)
    fused.explore_actions(buf.data_ptr())
    loop.sync()
    fused.sync()
    assert np.array_equal(odd.cpu().numpy()[1:c.n + 1], buf.cpu().numpy()[:c.n]) and odd.cpu().numpy()[0] == 9 and odd.cpu().numpy()[c.n + 1] == 9
    fused.close()
    loop.close()


# ---- greedy equivalence ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("table", [False, True])
@pytest.mark.parametrize("vec", [4, 8])
@pytest.mark.parametrize("kind", [0, 1])
def test_threshold_0_and_the_flag_left_out_are_the_greedy_launch(gymrs, kind, vec, table):
    """Threshold 0 with the flag == rollout_closed_loop without it; settings present and the flag absent leave the greedy result
    (and rollout_policy's, without a table); all == the reference's greedy launch.  Plain, fitness and (at 4) recording."""
    c = ref.case(kind, FULL, table, 6, (3, 512), 8, ref.SPLITS[1])
    run = ref.Run(c)
    zero = make_engine(gymrs, c, vec, explore=False)
    zero.set_exploration(c.seed, threshold=0)
    unflagged = make_engine(gymrs, c, vec)  # threshold 16384 set, never asked for
    plain = make_engine(gymrs, c, vec, explore=False)
    old = make_engine(gymrs, c, vec) if not table else None
    recs = {name: Recorder(kind, c.n, max(c.schedule)) for name in ("zero", "unflagged")}
    for k, steps in enumerate(c.schedule):
        fitness, record = k == 1, k == 2 and vec == 4
        want = run.launch(steps, None, count=fitness)
        zero.rollout_closed_loop(steps, lane_params=table, explore=True, fitness=fitness, record=recs["zero"].fresh() if record else None)
        unflagged.rollout_closed_loop(steps, lane_params=table, fitness=fitness, record=recs["unflagged"].fresh() if record else None)
        plain.rollout_closed_loop(steps, lane_params=table, fitness=fitness)
        if old is not None:
            (old.rollout_policy_fitness if fitness else old.rollout_policy)(steps)
        for name, eng in (("zero", zero), ("unflagged", unflagged), ("plain", plain), ("rollout_policy", old)):
            if eng is not None:
                eng.sync()
                compare(eng, want, (name, k), c.classes[vec])
                assert np.array_equal(eng.policy_fitness(), want.fitness), (name, k)
        if record:
            for name in recs:
                recs[name].check(want, steps, c.flags, (name, k), c.classes[4])
    assert want.fitness.any() and zero.exploration() == (c.seed, 0) and unflagged.exploration() == (c.seed, c.threshold)
    for eng in (zero, unflagged, plain, old):
        if eng is not None:
            eng.close()


# ---- the settings: stream order, set_policy, clone, snapshot -------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1])
def test_settings_take_effect_in_stream_order_and_survive_set_policy(gymrs, kind):
    c = ref.case(kind, FULL, True, 6, (3, 1), 8)
    other = (c.seed + 1, 40000)
    run = ref.Run(c)
    eng = make_engine(gymrs, c, 4)
    before = eng.get_state(), eng.tick(), eng.stats(), len(eng.snapshot())
    eng.set_exploration(*other[:1], threshold=other[1])
    eng.set_exploration(c.seed, epsilon=0.25)  # 0.25 * 65536 = 16384
    assert eng.exploration() == (c.seed, 16384)
    assert np.array_equal(bits(eng.get_state()), bits(before[0])) and eng.tick() == before[1] and np.array_equal(eng.stats(), before[2])
    assert len(eng.snapshot()) == before[3]  # the snapshot does not carry the settings
    eng.rollout_closed_loop(9, lane_params=True, explore=True, fitness=True)  # enqueued before the change: the old settings
    eng.set_exploration(other[0], threshold=other[1])
    eng.rollout_closed_loop(11, lane_params=True, explore=True, fitness=True)
    run.launch(9, (c.seed, c.threshold))
    want = run.launch(11, other)
    eng.sync()
    compare(eng, want, "after the change", c.classes[4])
    assert np.array_equal(eng.policy_fitness(), want.fitness)
    unchanged = ref.Run(c)
    unchanged.launch(9, (c.seed, c.threshold))
    assert not np.array_equal(bits(unchanged.launch(11, (c.seed, c.threshold)).state), bits(want.state))  # the old settings would be noticed
    # set_policy keeps the settings (and discards the fitness table, as always)
    eng.set_policy(c.weights, hidden=c.hidden, lanes_per_policy=c.lanes_per_policy)
    assert eng.exploration() == other and not eng.policy_fitness().any()
    run.fitness[:] = 0
    eng.rollout_closed_loop(5, lane_params=True, explore=True, fitness=True)
    want = run.launch(5, other)
    compare(eng, want, "after set_policy", c.classes[4])
    assert np.array_equal(eng.policy_fitness(), want.fitness)
    # a clone and a restored engine hold the lanes and no settings
    clone = eng.clone()
    with pytest.raises(gymrs.GymrsError, match="gymrs_set_exploration"):
        clone.exploration()
    clone.set_policy(c.weights, hidden=c.hidden, lanes_per_policy=c.lanes_per_policy)
    with pytest.raises(gymrs.GymrsError, match="gymrs_set_exploration"):
        clone.rollout_closed_loop(3, lane_params=True, explore=True)
    fresh = make_engine(gymrs, c, 4, explore=False)
    fresh.restore(eng.snapshot())
    with pytest.raises(gymrs.GymrsError, match="gymrs_set_exploration"):
        fresh.exploration()
    for e in (clone, fresh):  # ... and go on like the original once they are given them
        e.set_exploration(other[0], threshold=other[1])
        e.rollout_closed_loop(4, lane_params=True, explore=True)
    want = run.launch(4, other)
    compare(clone, want, "clone", c.classes[4])
    compare(fresh, want, "restored", c.classes[4])
    eng.set_exploration(None)
    with pytest.raises(gymrs.GymrsError, match="gymrs_set_exploration"):
        eng.exploration()
    for e in (eng, clone, fresh):
        e.close()


# ---- the refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals(gymrs):
    c = ref.case(0, A | S, True, 0, (3, 512), 0)
    eng = make_engine(gymrs, c, 4, explore=False)
    before = eng.get_state(), eng.tick()
    buf = action_buffer(c.n)

    def untouched():
        assert np.array_equal(bits(eng.get_state()), bits(before[0])) and eng.tick() == before[1]

    with pytest.raises(gymrs.GymrsError, match="gymrs_set_exploration"):  # the flag without settings
        eng.rollout_closed_loop(3, lane_params=True, explore=True)
    with pytest.raises(gymrs.GymrsError, match="gymrs_set_exploration"):
        eng.rollout_closed_loop(3, lane_params=True, explore=True, fitness=True)
    with pytest.raises(gymrs.GymrsError, match="gymrs_set_exploration"):
        eng.explore_actions(buf.data_ptr())
    with pytest.raises(gymrs.GymrsError, match="gymrs_set_exploration"):
        eng.exploration()
    untouched()
    for bad in (gymrs.Exploration(1, 65537, 0), gymrs.Exploration(1, 1 << 31, 0), gymrs.Exploration(1, 16384, 1)):
        assert eng._lib.gymrs_set_exploration(eng._h, C.byref(bad)) == 1
        assert (b"threshold" if bad.reserved == 0 else b"reserved") in eng._lib.gymrs_last_error()
    with pytest.raises(gymrs.GymrsError, match="gymrs_set_exploration"):  # a refused call stored nothing
        eng.exploration()
    with pytest.raises(ValueError):
        eng.set_exploration(1, epsilon=0.5, threshold=3)
    with pytest.raises(ValueError):
        eng.set_exploration(1)
    with pytest.raises(ValueError):
        eng.set_exploration(1, epsilon=1.5)
    assert eng._lib.gymrs_set_exploration(None, None) == 1 and eng._lib.gymrs_get_exploration(eng._h, None) == 1
    assert eng._lib.gymrs_explore_actions(eng._h, None) == 1 and eng._lib.gymrs_explore_actions(None, C.c_void_p(buf.data_ptr())) == 1
    eng.set_exploration(7, threshold=65536)  # the largest threshold is legal
    assert eng.exploration() == (7, 65536)
    # with settings: the descriptor's other refusals stand
    with pytest.raises(gymrs.GymrsError, match="GYMRS_CLOSED_LOOP_LANE_PARAMS"):
        eng.rollout_closed_loop(3, explore=True)
    rec = Recorder(0, c.n, 4)
    with pytest.raises(gymrs.GymrsError, match="recording fitness"):
        eng.rollout_closed_loop(3, lane_params=True, explore=True, fitness=True, record=rec.fresh())
    for more in (2, 8, 1 << 31):
        with pytest.raises(gymrs.GymrsError, match="unknown flag bits"):
            eng.rollout_closed_loop(3, flags=gymrs.CLOSED_LOOP_LANE_PARAMS | gymrs.CLOSED_LOOP_EXPLORE | more)
    desc = gymrs.ClosedLoopDesc(3, gymrs.CLOSED_LOOP_LANE_PARAMS | gymrs.CLOSED_LOOP_EXPLORE, None, 1)
    assert eng._lib.gymrs_rollout_closed_loop(eng._h, C.byref(desc)) == 1 and b"reserved" in eng._lib.gymrs_last_error()
    with pytest.raises(gymrs.GymrsError, match="GYMRS_POLICY_FITNESS_MAX_STEPS"):
        eng.rollout_closed_loop((1 << 24) + 1, lane_params=True, explore=True, fitness=True)
    eng.rollout_closed_loop(0, lane_params=True, explore=True)  # a no-op
    untouched()
    eng.set_policy(None)  # the settings need no policy; the calls that play them do
    assert eng.exploration() == (7, 65536)
    eng.set_exploration(8, threshold=1)
    with pytest.raises(gymrs.GymrsError, match="no policy"):
        eng.rollout_closed_loop(3, lane_params=True, explore=True)
    with pytest.raises(gymrs.GymrsError, match="no policy"):
        eng.explore_actions(buf.data_ptr())
    untouched()
    eng.close()
    pend = gymrs.BatchedEngine(gymrs.PENDULUM, 64)
    pend.reset(seed=1)
    with pytest.raises(gymrs.GymrsError, match="Pendulum"):
        pend.set_exploration(1, threshold=5)
    with pytest.raises(gymrs.GymrsError, match="Pendulum"):
        pend.set_exploration(None)
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
    with pytest.raises(gymrs.GymrsError, match="gymrs_set_exploration"):
        sh.rollout_closed_loop(3, lane_params=True, explore=True)
    sh.set_exploration(c.seed, threshold=c.threshold)
    assert sh.exploration() == (c.seed, c.threshold) and all(s.exploration() == (c.seed, c.threshold) for s in sh.shards)
    for k, steps in enumerate(c.schedule):
        sh.rollout_closed_loop(steps, lane_params=True, explore=True, fitness=True)
        one.rollout_closed_loop(steps, lane_params=True, explore=True, fitness=True)
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
    sh.set_exploration(None)
    with pytest.raises(gymrs.GymrsError, match="gymrs_set_exploration"):
        sh.rollout_closed_loop(3, lane_params=True, explore=True)
    sh.close()
    one.close()
