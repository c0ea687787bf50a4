"""gymrs_rollout_closed_loop under a per-lane parameter table (GYMRS_CLOSED_LOOP_LANE_PARAMS) against the CPU reference of
tests/closed_loop_table_ref.py: one f32 twin per row, lane i read from twin index[i], stepped with the actions of
tests/cpp/policy_ref.c.  The reference shares no code with the kernels and never loads the library.

The TableT instantiations of rollout_policy_kernel and rollout_policy_fitness_kernel (gym-rs_amd/csrc/gymrs_table_policy_<env>.hip)
are built per flag set (10), lanes per work-item (4, 8; recording at 4) and each compiles four copies of rollout_block that a wave
picks from at run time (uniform or gathered weights x full or ragged wave).  The case table puts lanes of five different rows into
every copy of every instantiation; tests/test_closed_loop_table_ref.py shows on the CPU that at every point compared here an
episode has ended, actions vary, policies disagree and a lane stepped with its neighbour's row would differ.

Every comparison is bit for bit (uint32 views of floats, equal integers, statistics with ==) after every launch, no lane left out.
One exception, stated where it applies: the slow-path cases treat any NaN as equal to any NaN, as tests/test_gpu_slowpaths.py does
(sign and payload of a generated NaN are not specified)."""
import ctypes as C
import time

import closed_loop_ref as cl
import closed_loop_table_ref as ref
import lane_params_ref as lp
import numpy as np
import policy_fitness_ref as pf
import pytest
import torch
from closed_loop_table_ref import A, COPIES, DIMS, F, S, T

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
INVALID_ACTION = 5  # GYMRS_EACTION


def same(what, got, want, at, classes, index, nan_equal=False):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, at, got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype == np.float32:
        bad = got.view(np.uint32) != want.view(np.uint32)
        if nan_equal:
            bad &= ~(np.isnan(got) & np.isnan(want))
    else:
        bad = got != want
    if bad.any():
        lanes = np.flatnonzero(bad.reshape(-1, bad.shape[-1]).any(axis=0))
        per_copy = {COPIES[c]: int((classes[lanes] == c).sum()) for c in np.unique(classes[lanes])}
        per_row = np.bincount(np.minimum(np.asarray(index, np.int64)[lanes], ref.K), minlength=ref.K + 1).tolist()
        raise AssertionError((what, at, f"{len(lanes)} lanes differ", per_copy, {"per row": per_row}, lanes[:8].tolist()))


def compare(eng, want, at, classes, nan_equal=False, stats=True, lanes=None, first=0):
    """The engine's getters == the reference's record of a launch (`lanes`: a boolean mask of the lanes to look at, default all;
    `first`: the engine holds lanes [first, first + n_envs) of the reference's batch)"""
    sl = slice(first, first + eng.n_envs)
    pick = (lambda x: x[..., sl]) if lanes is None else (lambda x: x[..., sl][..., lanes])
    mine = (lambda x: x) if lanes is None else (lambda x: x[..., lanes])
    kw = dict(classes=pick(classes), index=pick(want.index), nan_equal=nan_equal)
    same("state", mine(eng.get_state()), pick(want.state), at, **kw)
    same("obs", mine(eng.get_obs()), pick(want.obs), at, **kw)
    reward, done, trunc = eng.get_step_result()
    same("reward", mine(reward), pick(want.reward), at, **kw)
    same("done", mine(done), pick(want.done), at, **kw)
    if want.flags & T:
        same("truncated", mine(trunc), pick(want.truncated), at, **kw)
    if want.flags & F:
        same("final_obs", mine(eng.get_final_obs()), pick(want.final), at, **kw)
    if stats:
        assert np.array_equal(eng.stats(), want.stats), ("stats", at, eng.stats(), want.stats)
    assert eng.tick()[0] == want.tick, ("tick", at, eng.tick(), want.tick)


def device(a):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    torch.cuda.synchronize()  # torch copied on its stream; the engine reads on its own
    return t


def rows_of(gymrs, c):
    return lp.rows_for(type(gymrs.engine.default_params(c.kind)), c.rows)


def make_engine(gymrs, c, prepare=None, table=True, policy=True):
    """An engine for case c: its table and index (unless table is False: row 0 for every lane), reset, prepared, c's policy set"""
    rows = rows_of(gymrs, c)
    eng = gymrs.BatchedEngine(c.kind, c.n, global_env_offset=c.gid0, flags=c.flags, params=rows[0], lanes_per_thread=c.vec)
    if table:
        eng.set_param_table(rows)
        eng.set_param_index(c.index)
    eng.reset(seed=c.reset_seed)
    prepare = prepare if prepare is not None else c.prepare
    if prepare is not None:
        eng.set_state(prepare(eng.get_state()))
    if policy:
        eng.set_policy(c.weights, hidden=c.hidden, lanes_per_policy=c.lanes_per_policy)
    return eng


class Recorder:
    """Trajectory buffers with padding columns and spare rows, pre-filled with NaN / 9 so that an unwritten cell shows"""

    def __init__(self, kind, n, rows):
        self.n, self.d = n, DIMS[kind][0]
        self.stride = (n + 15) // 16 * 16 + 16  # > n: rows have padding columns
        self.rows = rows

    def fresh(self):
        self.obs = torch.full((self.rows, self.d, self.stride), float("nan"), dtype=torch.float32, device=DEV)
        self.act = torch.full((self.rows, self.stride), 9, dtype=torch.uint8, device=DEV)
        self.rew = torch.full((self.rows, self.stride), float("nan"), dtype=torch.float32, device=DEV)
        self.done = torch.full((self.rows, self.stride), 9, dtype=torch.uint8, device=DEV)
        self.trunc = torch.full((self.rows, self.stride), 9, dtype=torch.uint8, device=DEV)
        torch.cuda.synchronize()  # torch filled these on its stream; the engine writes them on its own
        return dict(obs=self.obs.data_ptr(), actions=self.act.data_ptr(), reward=self.rew.data_ptr(), done=self.done.data_ptr(),
                    truncated=self.trunc.data_ptr(), lane_stride=self.stride)

    def check(self, want, steps, flags, at, classes, lanes=None, nan_equal=False):
        n = self.n
        obs_h, act_h, rew_h, done_h, trunc_h = (x.cpu().numpy() for x in (self.obs, self.act, self.rew, self.done, self.trunc))
        pick = (lambda x: x) if lanes is None else (lambda x: x[..., lanes])
        kw = dict(classes=pick(classes), index=pick(want.index), nan_equal=nan_equal)
        for t in range(steps):
            same("recorded obs", pick(obs_h[t, :, :n]), pick(want.rec_obs[t]), (at, t), **kw)
            same("recorded actions", pick(act_h[t, :n]), pick(want.rec_actions[t]), (at, t), **kw)
            same("recorded reward", pick(rew_h[t, :n]), pick(want.rec_reward[t]), (at, t), **kw)
            same("recorded done", pick(done_h[t, :n]), pick(want.rec_done[t]), (at, t), **kw)
            if flags & T:
                same("recorded truncated", pick(trunc_h[t, :n]), pick(want.rec_truncated[t]), (at, t), **kw)
        # padding columns and the rows beyond `steps` are never written (nor `truncated` without the time limit)
        assert np.isnan(obs_h[:, :, n:]).all() and np.isnan(rew_h[:, n:]).all()
        assert (act_h[:, n:] == 9).all() and (done_h[:, n:] == 9).all() and (trunc_h[:, n:] == 9).all()
        assert np.isnan(obs_h[steps:]).all() and np.isnan(rew_h[steps:]).all()
        assert (act_h[steps:] == 9).all() and (done_h[steps:] == 9).all() and (trunc_h[steps:] == 9).all()
        if not flags & T:
            assert (trunc_h == 9).all()
        return obs_h, act_h, rew_h, done_h, trunc_h


# ---- the matrix: the fused call, the fitness call and (at 4 lanes per work-item) the recording call -------------------------------
@pytest.mark.parametrize("kind,shape,flags,hidden", ref.cases())
def test_closed_loop_on_a_table_equals_the_cpu_reference_in_every_copy(gymrs, kind, shape, flags, hidden):
    """One reference, three engines: rollout_closed_loop(lane_params), the same with fitness (counters == the reference's records
    folded per policy, accumulated over the launches; the engine bit for bit as without them) and, where the recording kernel
    exists, with record (the rows of every step)."""
    c = ref.case(kind, shape, flags, hidden)
    want = ref.run_case(c)
    assert len(np.unique(c.classes)) == 3  # two full copies and the ragged wave's
    modes = ["fused", "fitness"] + (["record"] if ref.records_too(shape, hidden) else [])
    engines = {mode: make_engine(gymrs, c) for mode in modes}
    rec = Recorder(kind, c.n, max(c.schedule))
    for mode, eng in engines.items():
        same("start state", eng.get_state(), want[0].start_state, mode, c.classes, c.index)
    for k, steps in enumerate(c.schedule):
        engines["fused"].rollout_closed_loop(steps, lane_params=True)
        engines["fitness"].rollout_closed_loop(steps, lane_params=True, fitness=True)
        if "record" in engines:
            engines["record"].rollout_closed_loop(steps, lane_params=True, record=rec.fresh())
        for mode, eng in engines.items():
            eng.sync()
            compare(eng, want[k], (mode, k), c.classes)
        got = engines["fitness"].policy_fitness()
        assert np.array_equal(got, want[k].fitness), ("fitness", k, got.tolist(), want[k].fitness.tolist())
        if "record" in engines:
            rec.check(want[k], steps, flags, k, c.classes)
    if flags & F:
        for copy in np.unique(c.classes):
            assert want[-1].final[:, c.classes == copy].any(), COPIES[copy]  # an all-zero buffer cannot pass
    assert not engines["fused"].policy_fitness().any()  # the plain call counts nothing
    for eng in engines.values():
        eng.close()


# ---- CartPole's other integrator ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [1, 3])  # 4 and 8 lanes per work-item
@pytest.mark.parametrize("flags", lp.INTEGRATOR_1_FLAGS)
def test_kinematics_integrator_1(gymrs, flags, shape):
    """advance_fast_rows<.., 1> under the policy: fused, fitness and (at 4) recording"""
    c = ref.case(0, shape, flags, 8, integrator=1)
    assert all(row.kinematics_integrator == 1 for row in c.rows)
    want = ref.run_case(c)
    assert ref.worth_comparing(c, want) == []
    other = ref.run_case(ref.case(0, shape, flags, 8))
    assert not np.array_equal(ref.bits(want[-1].state), ref.bits(other[-1].state))  # integrator 0 would be noticed
    eng, fit = make_engine(gymrs, c), make_engine(gymrs, c)
    rec_eng = make_engine(gymrs, c) if c.vec == 4 else None
    rec = Recorder(0, c.n, max(c.schedule))
    for k, steps in enumerate(c.schedule):
        eng.rollout_closed_loop(steps, lane_params=True)
        fit.rollout_closed_loop(steps, lane_params=True, fitness=True)
        compare(eng, want[k], ("fused", k), c.classes)
        compare(fit, want[k], ("fitness", k), c.classes)
        assert np.array_equal(fit.policy_fitness(), want[k].fitness), k
        if rec_eng is not None:
            rec_eng.rollout_closed_loop(steps, lane_params=True, record=rec.fresh())
            rec_eng.sync()
            rec.check(want[k], steps, flags, k, c.classes)
            compare(rec_eng, want[k], ("record", k), c.classes)
    assert eng.get_params().kinematics_integrator == 1
    for e in (eng, fit, rec_eng):
        if e is not None:
            e.close()


# ---- the index rewritten between two launches ------------------------------------------------------------------------------------
class DeviceColumn:
    """A zero-copy torch view of an engine's device array"""

    def __init__(self, ptr, n, typestr):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (ptr, False), "version": 3}


@pytest.mark.parametrize("shape", [1, 3])
@pytest.mark.parametrize("flags", lp.REWRITE_FLAGS)
@pytest.mark.parametrize("kind", [0, 1])
def test_index_rewritten_between_two_launches(gymrs, kind, flags, shape):
    """A write through param_index_ptr on the engine's stream takes effect in the next launch: every lane goes on from its own state
    with its new row.  (Flag sets without the time limit; tests/test_gpu_sequences.py rewrites the index under the others.)"""
    c = ref.case(kind, shape, flags, 8)
    first, second = lp.REWRITE_STEPS
    new = lp.make_index(c.n, ref.K, lp.INDEX_SEED + 10 + kind)
    run = ref.Run(c)
    run.launch(first)
    run.set_index(new)
    want = run.launch(second)
    assert run.ref.told_apart(c.index) >= ref.TOLD_APART  # the old index would be noticed
    new_dev = device(new.view(np.int16))
    for fitness in (False, True):
        eng = make_engine(gymrs, c)
        view = torch.as_tensor(DeviceColumn(eng.param_index_ptr(), c.n, "<i2"), device=DEV)
        eng.rollout_closed_loop(first, lane_params=True, fitness=fitness)  # enqueued before the rewrite: the old index
        with torch.cuda.stream(torch.cuda.ExternalStream(eng.stream, device=DEV)):
            view.copy_(new_dev)
        eng.rollout_closed_loop(second, lane_params=True, fitness=fitness)
        eng.sync()
        compare(eng, want, ("after the rewrite", fitness), c.classes)
        assert np.array_equal(eng.get_param_index(), new)
        assert np.array_equal(eng.policy_fitness(), want.fitness if fitness else np.zeros_like(want.fitness))
        eng.close()


# ---- the slow path with per-lane constants ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [1, 3])
@pytest.mark.parametrize("flags", [0, T, A | S, A | S | T | F])
@pytest.mark.parametrize("kind", [0, 1])
def test_slow_path_lanes_step_with_their_own_rows(gymrs, kind, flags, shape):
    """Every 7th lane starts beyond the fast path's range (angles up to 1e30, NaN, inf: lane_params_ref.slow_prepare), in lanes of
    every row: their waves take Env::advance(lc[k], ..) for all their lanes, with the policy fed NaN and inf observations.  Any NaN
    equals any NaN here, everything else bit for bit."""
    c = ref.case(kind, shape, flags, 8)
    prepare = lp.slow_prepare(kind)
    run = ref.Run(c, prepare)
    assert len(set(c.index[lp.beyond_range(kind, run.start_state)])) >= 3
    eng, fit = make_engine(gymrs, c, prepare), make_engine(gymrs, c, prepare)
    same("start state", eng.get_state(), run.start_state, "reset", c.classes, c.index, nan_equal=True)
    for k, steps in enumerate(c.schedule):
        want = run.launch(steps)
        eng.rollout_closed_loop(steps, lane_params=True)
        fit.rollout_closed_loop(steps, lane_params=True, fitness=True)
        compare(eng, want, ("fused", k), c.classes, nan_equal=True)
        compare(fit, want, ("fitness", k), c.classes, nan_equal=True)
        assert np.array_equal(fit.policy_fitness(), want.fitness), (k, fit.policy_fitness().tolist(), want.fitness.tolist())
    eng.close()
    fit.close()


# ---- an index outside the table ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [0, 2])  # n = 4200 at 4 and 8 lanes per work-item
@pytest.mark.parametrize("kind", [0, 1])
def test_out_of_range_index_is_reported_not_stepped_and_not_counted(gymrs, kind, shape):
    """Two lanes with index K and 65535: the documented GYMRS_EACTION report naming the lowest lane; those lanes keep their state, pay
    0 and set no flag in every recorded row, add nothing to any fitness record; every other lane (their neighbours in the work-item
    and wave included) equals the reference."""
    flags, steps = A | S | T | F, 6
    c = ref.case(kind, shape, flags, 8)
    bad_lanes = [777, 2999]
    run = ref.Run(c)  # (lanes are independent: the reference's own row for the two lanes does not matter)
    want = run.launch(steps)
    ok = np.ones(c.n, bool)
    ok[bad_lanes] = False
    index = c.index.copy()
    index[bad_lanes] = [ref.K, 65535]
    fitness = pf.fold_rows(c.policies[ok], ref.N_POLICIES, want.rec_reward[:, ok], want.rec_done[:, ok], want.rec_truncated[:, ok])
    assert not np.array_equal(fitness, want.fitness)  # the two lanes, had they been stepped, would have counted
    for mode in ("fused", "fitness") + (("record",) if c.vec == 4 else ()):
        eng = make_engine(gymrs, c)
        eng.set_param_index(index)
        before = eng.get_state()
        rec = Recorder(kind, c.n, steps)
        eng.rollout_closed_loop(steps, lane_params=True, fitness=mode == "fitness", record=rec.fresh() if mode == "record" else None)
        with pytest.raises(gymrs.InvalidActionError) as ei:
            eng.sync()
        assert ei.value.status == INVALID_ACTION and f"lane {bad_lanes[0]} " in str(ei.value) and "parameter index" in str(ei.value)
        same("state of the rejected lanes", eng.get_state()[:, ~ok], before[:, ~ok], mode, c.classes[~ok], index[~ok])
        reward, done, trunc = eng.get_step_result()
        assert not reward[~ok].any() and not done[~ok].any() and not trunc[~ok].any(), mode
        compare(eng, want, (mode, "the other lanes"), c.classes, stats=False, lanes=ok)
        if mode == "fitness":
            assert np.array_equal(eng.policy_fitness(), fitness), (eng.policy_fitness().tolist(), fitness.tolist())
        if mode == "record":
            obs_h, act_h, rew_h, done_h, trunc_h = rec.check(want, steps, flags, mode, c.classes, lanes=ok)
            for t in range(steps):  # zero rows: the unchanged observation, no reward, no flag
                same("recorded obs of the rejected lanes", obs_h[t, :, :c.n][:, ~ok], before[:, ~ok], t, c.classes[~ok], index[~ok])
            assert not rew_h[:, :c.n][:, ~ok].any() and not done_h[:, :c.n][:, ~ok].any() and not trunc_h[:, :c.n][:, ~ok].any()
        eng.sync()  # the report was consumed
        eng.close()


# ---- without a table: the descriptor stands for the three older calls --------------------------------------------------------------
@pytest.mark.parametrize("lane_params", [False, True])
@pytest.mark.parametrize("shape", [1, 3])
@pytest.mark.parametrize("kind", [0, 1])
def test_without_a_table_the_call_is_the_old_calls_bit_for_bit(gymrs, kind, shape, lane_params):
    flags = A | S | T | F
    c = ref.case(kind, shape, flags, 8)

    def equal(a, b, at):
        for what, x, y in (("state", a.get_state(), b.get_state()), ("obs", a.get_obs(), b.get_obs()), ("final", a.get_final_obs(), b.get_final_obs())):
            same(what, x, y, at, c.classes, c.index)
        for what, x, y in zip(("reward", "done", "truncated"), a.get_step_result(), b.get_step_result()):
            same(what, x, y, at, c.classes, c.index)
        assert np.array_equal(a.stats(), b.stats()) and a.tick() == b.tick(), at
        assert np.array_equal(a.policy_fitness(), b.policy_fitness()), at

    new, old = make_engine(gymrs, c, table=False), make_engine(gymrs, c, table=False)
    for k, steps in enumerate(c.schedule):  # plain, then with fitness, alternating on the same pair
        new.rollout_closed_loop(steps, lane_params=lane_params, fitness=bool(k % 2))
        (old.rollout_policy_fitness if k % 2 else old.rollout_policy)(steps)
        equal(new, old, ("fused", k))
    assert new.policy_fitness().any() and new.stats()[2] > 0
    if c.vec == 4:
        steps = 9
        rec_new, rec_old = Recorder(kind, c.n, steps), Recorder(kind, c.n, steps)
        new.rollout_closed_loop(steps, lane_params=lane_params, record=rec_new.fresh())
        bufs = rec_old.fresh()
        old.rollout_policy_record(steps, **bufs)
        new.sync()
        old.sync()
        equal(new, old, "record")
        for what in ("obs", "act", "rew", "done", "trunc"):
            x, y = getattr(rec_new, what).cpu().numpy(), getattr(rec_old, what).cpu().numpy()
            assert np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y), what
        assert not np.isnan(rec_new.obs.cpu().numpy()[:, :, :c.n]).any()
    new.rollout_closed_loop(0, lane_params=lane_params)  # a no-op
    equal(new, old, "n_steps 0")
    new.close()
    old.close()


# ---- the refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals(gymrs):
    c = ref.case(0, 3, A | S, 0)
    eng = make_engine(gymrs, c)
    before = eng.get_state(), eng.tick()
    rec = Recorder(0, c.n, 4)
    with pytest.raises(gymrs.GymrsError, match="GYMRS_CLOSED_LOOP_LANE_PARAMS"):  # a table and a plain descriptor
        eng.rollout_closed_loop(3)
    with pytest.raises(gymrs.GymrsError, match="GYMRS_CLOSED_LOOP_LANE_PARAMS"):
        eng.rollout_closed_loop(3, fitness=True)
    with pytest.raises(gymrs.GymrsError, match="recording fitness"):
        eng.rollout_closed_loop(3, lane_params=True, fitness=True, record=rec.fresh())
    desc = gymrs.ClosedLoopDesc(3, gymrs.CLOSED_LOOP_LANE_PARAMS, None, 1)
    assert eng._lib.gymrs_rollout_closed_loop(eng._h, C.byref(desc)) == 1 and b"reserved" in eng._lib.gymrs_last_error()
    for bits in (2, 8, 1 << 31):
        with pytest.raises(gymrs.GymrsError, match="unknown flag bits"):
            eng.rollout_closed_loop(3, flags=gymrs.CLOSED_LOOP_LANE_PARAMS | bits)
    with pytest.raises(gymrs.GymrsError, match="GYMRS_POLICY_FITNESS_MAX_STEPS"):
        eng.rollout_closed_loop((1 << 24) + 1, lane_params=True, fitness=True)
    bufs = rec.fresh()
    for broken, word in ((dict(bufs, lane_stride=c.n - 4), "lane_stride"), (dict(bufs, reward=0), "required"), (dict(bufs, done=bufs["done"] + 4), "aligned")):
        with pytest.raises(gymrs.GymrsError, match=word):
            eng.rollout_closed_loop(3, lane_params=True, record=broken)
        with pytest.raises(gymrs.GymrsError, match=word):  # the checks come before the no-op
            eng.rollout_closed_loop(0, lane_params=True, record=broken)
    # the three older calls still refuse a table, word for word
    for call in (lambda: eng.rollout_policy(3), lambda: eng.rollout_policy_fitness(3), lambda: eng.rollout_policy_record(3, **bufs)):
        with pytest.raises(gymrs.GymrsError, match="a parameter table is active.*policy x table is not built yet: use gymrs_policy_actions \\+ gymrs_step"):
            call()
    eng.rollout_closed_loop(0, lane_params=True)  # a no-op
    assert np.array_equal(ref.bits(eng.get_state()), ref.bits(before[0])) and eng.tick() == before[1]
    eng.set_policy(None)
    with pytest.raises(gymrs.GymrsError, match="no policy"):
        eng.rollout_closed_loop(3, lane_params=True)
    eng.close()
    pend = gymrs.BatchedEngine(gymrs.PENDULUM, 64)
    pend.reset(seed=1)
    with pytest.raises(gymrs.GymrsError, match="Pendulum"):
        pend.rollout_closed_loop(3, lane_params=True)
    pend.close()


# ---- the native sharder ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blocks", [2, 3])
@pytest.mark.parametrize("kind", [0, 1])
def test_sharded_blocks_on_one_gpu_equal_one_engine(gymrs, kind, blocks):
    """k blocks on device 0 with the table and the batch's index: state and fitness equal ONE engine's and the reference's"""
    flags = A | S | T | F
    c = ref.case(kind, 1, flags, 8)
    want = ref.run_case(c)
    rows = rows_of(gymrs, c)
    one = make_engine(gymrs, c)
    sh = gymrs.ShardedEngine(kind, c.n, [0] * blocks, global_env_offset=c.gid0, flags=flags, params=rows[0])
    sh.set_param_table(rows)
    sh.set_param_index(c.index)
    sh.reset(seed=c.reset_seed)
    if c.prepare is not None:
        start = c.prepare(sh.get_state())
        for s in sh.shards:
            s.set_state(start[:, s.first_lane:s.first_lane + s.n_envs])
    sh.set_policy(c.weights, hidden=c.hidden, lanes_per_policy=c.lanes_per_policy)
    rec = Recorder(kind, c.n, 4)
    with pytest.raises(gymrs.GymrsError, match="record must be NULL"):
        sh.rollout_closed_loop(3, lane_params=True, record=rec.fresh())
    with pytest.raises(gymrs.GymrsError, match="GYMRS_CLOSED_LOOP_LANE_PARAMS"):
        sh.rollout_closed_loop(3)
    for k, steps in enumerate(c.schedule):
        fitness = k != 1  # (one launch without: the counters stay)
        sh.rollout_closed_loop(steps, lane_params=True, fitness=fitness)
        one.rollout_closed_loop(steps, lane_params=True, fitness=fitness)
        sh.sync()
        w = want[k]
        kw = dict(classes=c.classes, index=c.index)
        same("state", sh.get_state(), w.state, k, **kw)
        same("state, one engine", sh.get_state(), one.get_state(), k, **kw)
        reward, done, trunc = sh.get_step_result()
        same("reward", reward, w.reward, k, **kw)
        same("done", done, w.done, k, **kw)
        same("truncated", trunc, w.truncated, k, **kw)
        same("final_obs", sh.get_final_obs(), w.final, k, **kw)
        assert np.array_equal(sh.stats(), w.stats) and np.array_equal(sh.stats(), one.stats()), (k, sh.stats(), w.stats)
        assert all(s.tick()[0] == w.tick for s in sh.shards)
        assert np.array_equal(sh.policy_fitness(), one.policy_fitness()), k
    expect = want[-1].fitness - (want[1].fitness - want[0].fitness)
    assert np.array_equal(sh.policy_fitness(), expect), (sh.policy_fitness().tolist(), expect.tolist())
    sh.close()
    one.close()


# ---- one launch against the loop it replaces -----------------------------------------------------------------------------------------
@pytest.mark.perf
def test_one_launch_takes_less_time_than_the_per_step_loop_it_replaces(gymrs):
    """CartPole, 1024 affine policies x 1024 lanes (2^20), 5 rows, flags A | S | T, K = 100 steps.  (a) rollout_closed_loop(K,
    lane_params) against (b) K x (policy_actions + step) under the same table: (b) moves every array through the memory system
    and submits 2K launches, (a) does neither.  Best of 5 each, taking turns; time(a) < time(b), no margin."""
    kind, n, k_steps, flags = 0, 1 << 20, 100, A | S | T
    rows = lp.rows_for(type(gymrs.engine.default_params(kind)), lp.make_rows(kind, ref.K, lp.ROWS_SEED, 500))
    eng = gymrs.BatchedEngine(kind, n, flags=flags, params=rows[0])
    eng.set_param_table(rows)
    eng.set_param_index(lp.make_index(n, ref.K, lp.INDEX_SEED))
    eng.reset(seed=1)
    eng.set_policy(cl.make_weights(kind, 0, 1024, 7), hidden=0, lanes_per_policy=1024)
    buf = torch.zeros(n, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()

    def fused():
        eng.rollout_closed_loop(k_steps, lane_params=True)

    def loop():
        for _ in range(k_steps):
            eng.policy_actions(buf.data_ptr())
            eng.step(buf.data_ptr())

    def timed(fn):
        t0 = time.perf_counter()
        fn()
        eng.sync()
        return time.perf_counter() - t0

    timed(fused), timed(loop)  # warm-up: code objects, allocations
    a, b = [], []
    for _ in range(5):
        a.append(timed(fused))
        b.append(timed(loop))
    print(f"closed loop under a table, 2^20 lanes x {k_steps} steps: one launch {min(a) * 1e3:.3f} ms, per-step loop {min(b) * 1e3:.3f} ms, "
          f"ratio {min(a) / min(b):.3f}")
    assert min(a) < min(b), (a, b)
    eng.close()
