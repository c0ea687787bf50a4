"""The closed-loop and evaluation kernels on the general, per-lane physics branch, against the CPU references of
tests/closed_loop_ref.py, tests/policy_eval_ref.py and tests/policy_eval_table_ref.py on the cases of tests/closed_loop_slow_ref.py:
parameter rows whose episodes end only far outside the fast path's range (Env::kRangeMax, gym-rs_amd/csrc/gymrs_tile.h), start
states with angles up to 1e30, NaN and inf on every 7th lane.  tests/test_closed_loop_slow_ref.py shows on the CPU that full waves
of every kernel copy take the general branch with lanes inside and outside the range side by side, that episodes end, actions vary
and policies disagree out there, and that the in-kernel policy reads NaN observations.

rollout_policy_kernel, its recording variant and the fitness kernel: every flag set, both vector widths, all four copies;
evaluate_policy_kernel with and without a parameter table; lanes that are through with their episodes next to lanes that play on
outside the range; the sharded calls.

Every comparison is == on integers or on f32 bit patterns, no tolerance, no lane left out.  One rule from tests/test_gpu_slowpaths.py
applies to the float arrays: a NaN equals any NaN (sign and payload of a generated NaN are not specified, and the CPU's and the GPU's
differ)."""
from functools import lru_cache
from types import SimpleNamespace

import closed_loop_ref as ref
import closed_loop_slow_ref as sl
import lane_params_ref as lp
import numpy as np
import policy_eval_ref as ev
import policy_fitness_ref as fit
import pytest
import test_gpu_policy_matrix as matrix
import torch
from closed_loop_ref import A, COPIES, DIMS, F, S, T

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = 0x7fffffff  # a value no episode writes


# ---- helpers: those of tests/test_gpu_policy_matrix.py, with the NaN rule switched on ------------------------------------------------------------
def same(what, got, want, classes, at):
    matrix.same(what, got, want, classes, at, nan_equal=True)


def assert_launch(eng, want, flags, classes, at, first=0):
    matrix.assert_launch(eng, want, flags, classes, at, first, nan_equal=True)


assert_stats = matrix.assert_stats


def assert_fitness(got, want, at):
    assert got.dtype == np.int64 and want.dtype == np.int64 and got.shape == want.shape, (at, got.dtype, got.shape, want.shape)
    assert np.array_equal(got, want), (at, "policies that differ", np.flatnonzero((got != want).any(axis=1))[:8].tolist(), got[:4], want[:4])


def assert_records(got, want, at):
    assert got.dtype == np.int64 and want.dtype == np.int64 and got.shape == want.shape, (at, got.dtype, got.shape, want.shape)
    assert np.array_equal(got, want), (at, "fields that differ (policy, field)", np.argwhere(got != want)[:8].tolist(), got[:3], want[:3])


def assert_lengths(got, want, classes, at):
    assert got.shape == want.shape and got.dtype == want.dtype == np.uint32, (at, got.shape, want.shape)
    bad = np.flatnonzero((got != want).any(axis=0))
    assert not len(bad), (at, {COPIES[c]: int((classes[bad] == c).sum()) for c in np.unique(classes[bad])}, bad[:8].tolist(),
                          got[:, bad[:4]].tolist(), want[:, bad[:4]].tolist())


def engine_params(gymrs, kind, row):
    """A lane_params_ref row as the library's own params type"""
    return lp.rows_for(type(gymrs.engine.default_params(kind)), [row])[0]


def make_engine(gymrs, c, first=0, count=None):
    """matrix.make_engine for a case whose params are a lane_params_ref row"""
    return matrix.make_engine(gymrs, SimpleNamespace(**{**vars(c), "params": engine_params(gymrs, c.kind, c.params)}), first, count)


LAUNCH_FIELDS = ("state", "obs", "reward", "done", "truncated", "stats", "tick", "final")


def without_rows(c, launches):
    """What the fused and the fitness test compare with: the getters' view of every launch and the per-policy records; the recorded
    rows (most of a reference's memory) are summed into the records and dropped"""
    records = fit.cumulative(launches, c.n, c.gid0, c.lanes_per_policy, sl.N_POLICIES)
    slim = [SimpleNamespace(**{f: getattr(x, f) for f in LAUNCH_FIELDS}) for x in launches]
    slim[0].start_state = launches[0].start_state
    return c, slim, records


@lru_cache(maxsize=None)
def rollout_reference(kind, shape, flags, hidden, integrator):
    c = sl.rollout_case(kind, shape, flags, hidden, integrator)
    return without_rows(c, ref.run_case(c))


@lru_cache(maxsize=None)
def sharded_reference(kind):
    c = sl.sharded_rollout_case(kind)
    return without_rows(c, ref.run_case(c))


# ---- a. the fused kernel -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,shape,flags,hidden,integrator", sl.rollout_cases(record=False))
def test_rollout_policy_off_the_fast_path(gymrs, kind, shape, flags, hidden, integrator):
    c, want, _ = rollout_reference(kind, shape, flags, hidden, integrator)
    eng = make_engine(gymrs, c)
    same("start state", eng.get_state(), want[0].start_state, c.classes, 0)
    for k, steps in enumerate(c.schedule):
        eng.rollout_policy(steps)
        eng.sync()  # (raises if the error counter moved: no action of the policy is invalid)
        assert_launch(eng, want[k], flags, c.classes, k)
        assert_stats(eng, want[k], k)
    eng.close()


# ---- b. the recording kernel (4 lanes per work-item only) ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,shape,flags,hidden,integrator", sl.rollout_cases(record=True))
def test_rollout_policy_record_off_the_fast_path(gymrs, kind, shape, flags, hidden, integrator):
    c = sl.rollout_case(kind, shape, flags, hidden, integrator)
    want = ref.run_case(c)
    n, d = c.n, DIMS[kind][0]
    stride = (n + 15) // 16 * 16 + 16  # > n: rows have padding columns
    rows = max(c.schedule)
    eng = make_engine(gymrs, c)
    for k, steps in enumerate(c.schedule):
        obs = torch.full((rows, d, stride), 7.0, dtype=torch.float32, device=DEV)  # (not NaN: the rows to come hold NaNs of their own)
        act = torch.full((rows, stride), 9, dtype=torch.uint8, device=DEV)
        rew = torch.full((rows, stride), 7.0, dtype=torch.float32, device=DEV)
        done = torch.full((rows, stride), 9, dtype=torch.uint8, device=DEV)
        trunc = torch.full((rows, stride), 9, dtype=torch.uint8, device=DEV)
        torch.cuda.synchronize()  # torch filled these on its stream; the engine writes them on its own
        eng.rollout_policy_record(steps, obs=obs.data_ptr(), actions=act.data_ptr(), reward=rew.data_ptr(), done=done.data_ptr(),
                                  truncated=trunc.data_ptr(), lane_stride=stride)
        eng.sync()
        obs_h, act_h, rew_h, done_h, trunc_h = (x.cpu().numpy() for x in (obs, act, rew, done, trunc))
        w = want[k]
        for t in range(steps):
            same("recorded obs", obs_h[t, :, :n], w.rec_obs[t], c.classes, (k, t))
            same("recorded actions", act_h[t, :n], w.rec_actions[t], c.classes, (k, t))
            same("recorded reward", rew_h[t, :n], w.rec_reward[t], c.classes, (k, t))
            same("recorded done", done_h[t, :n], w.rec_done[t], c.classes, (k, t))
            if flags & T:
                same("recorded truncated", trunc_h[t, :n], w.rec_truncated[t], c.classes, (k, t))
        # padding columns and the rows beyond `steps` are never written
        assert (obs_h[:, :, n:] == 7.0).all() and (rew_h[:, n:] == 7.0).all()
        assert (act_h[:, n:] == 9).all() and (done_h[:, n:] == 9).all() and (trunc_h[:, n:] == 9).all()
        assert (obs_h[steps:] == 7.0).all() and (rew_h[steps:] == 7.0).all()
        assert (act_h[steps:] == 9).all() and (done_h[steps:] == 9).all() and (trunc_h[steps:] == 9).all()
        if not flags & T:
            assert (trunc_h == 9).all()
        assert_launch(eng, w, flags, c.classes, k)
        assert_stats(eng, w, k)
    eng.close()


# ---- c. the fitness kernel -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,shape,flags,hidden,integrator", sl.rollout_cases(record=False))
def test_rollout_policy_fitness_off_the_fast_path(gymrs, kind, shape, flags, hidden, integrator):
    c, want, records = rollout_reference(kind, shape, flags, hidden, integrator)
    eng = make_engine(gymrs, c)
    assert_fitness(eng.policy_fitness(), np.zeros((sl.N_POLICIES, 4), np.int64), "before the first launch")
    for k, steps in enumerate(c.schedule):
        eng.rollout_policy_fitness(steps)
        assert_fitness(eng.policy_fitness(), records[k], k)
        assert_launch(eng, want[k], flags, c.classes, k)  # the engine is left as rollout_policy leaves it
        assert_stats(eng, want[k], k)
    assert records[-1][:, 1].all()  # every policy ended episodes
    eng.close()


# ---- d. evaluation ---------------------------------------------------------------------------------------------------------------------------
def lengths_buffer(episodes, n):
    buf = torch.full((episodes, n), SENTINEL, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()  # torch filled it on its stream; the engine writes it on its own
    return buf


def evaluate(eng, c, lane_params=False):
    """(records, lengths) of one call"""
    buf = lengths_buffer(c.episodes, eng.n_envs)
    eng.evaluate_policy(c.episodes, c.max_steps, sl.EVAL_SEED, common_starts=c.common, lengths=buf.data_ptr(), lane_params=lane_params)
    rec = eng.policy_eval()
    eng.sync()
    return rec, buf.cpu().numpy().view(np.uint32)


def everything(eng):
    out = {"state": eng.get_state(), "obs": eng.get_obs(), "final_obs": eng.get_final_obs(), "tick": np.array(eng.tick(), np.uint64),
           "stats": eng.stats(), "fitness": eng.policy_fitness(), "snapshot": np.frombuffer(eng.snapshot(), np.uint8)}
    for name, x in zip(("reward", "done", "truncated"), eng.get_step_result()):
        out[name] = x
    return out


def assert_untouched(before, after, at):
    assert before.keys() == after.keys()
    for name in before:
        x, y = np.ascontiguousarray(before[name]), np.ascontiguousarray(after[name])
        assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes(), (at, name)


def evaluation_engine(gymrs, c, row):
    """An engine mid-episode under `row` (statistics, final observations and fitness counters that are not zero) with c's policy set"""
    eng = gymrs.BatchedEngine(c.kind, c.n, global_env_offset=c.gid0, flags=A | S | T | F, params=engine_params(gymrs, c.kind, row))
    eng.reset(seed=4)
    eng.set_policy(c.weights, hidden=c.hidden, lanes_per_policy=c.lanes_per_policy)
    eng.rollout_policy_fitness(c.max_steps + 3)
    return eng


def check_evaluation(gymrs, c, want):
    eng = evaluation_engine(gymrs, c, c.row)
    before = everything(eng)
    assert before["final_obs"].any() and before["fitness"].any() and before["stats"][2] > 0
    got, lengths = evaluate(eng, c)
    assert_lengths(lengths, want.lengths, c.classes, "lengths")
    assert_records(got, want.records, "records")
    assert_untouched(before, everything(eng), "after evaluate_policy")
    eng.close()


@lru_cache(maxsize=None)
def evaluation_reference(kind, shape, hidden, common, integrator):
    c = sl.eval_case(kind, shape, hidden, common, integrator)
    return c, sl.run_eval(c)


@pytest.mark.parametrize("kind,shape,hidden,common,integrator", sl.eval_cases())
def test_evaluate_policy_off_the_fast_path(gymrs, kind, shape, hidden, common, integrator):
    c, want = evaluation_reference(kind, shape, hidden, common, integrator)
    check_evaluation(gymrs, c, want)


@pytest.mark.parametrize("kind", [0, 1])
def test_parked_lanes_stay_parked_beside_lanes_beyond_the_range(gymrs, kind):
    """Two policies alternate lane by lane: one is through with both its episodes within two dozen trips of the kernel's loop, the other
    plays on far outside the range, in the same work-items (tests/test_closed_loop_slow_ref.py counts the trips they share)"""
    c = sl.parked_case(kind)
    check_evaluation(gymrs, c, sl.run_eval(c))


@pytest.mark.parametrize("hidden,common", sl.table_cases())
def test_evaluate_policy_under_a_table_off_the_fast_path(gymrs, hidden, common):
    """MountainCar, three rows: the default, and the wide track with the goal at 120 and at 250; rows share waves"""
    c = sl.table_case(hidden, common)
    want = sl.run_table(c)
    rows = lp.rows_for(type(gymrs.engine.default_params(c.kind)), c.rows)
    eng = evaluation_engine(gymrs, c, c.rows[0])  # (before the table: the fused policy rollouts refuse one)
    eng.set_param_table(rows)
    eng.set_param_index(c.index)
    eng.rollout(5, action_seed=3)  # mid-episode under the table
    before = everything(eng)
    before["index"] = eng.get_param_index()
    got, lengths = evaluate(eng, c, lane_params=True)
    assert_lengths(lengths, want.lengths, c.classes, "lengths")
    assert_records(got, want.records, "records")
    after = everything(eng)
    after["index"] = eng.get_param_index()
    assert_untouched(before, after, "after evaluate_policy")
    assert np.array_equal(after["index"], c.index)
    eng.close()


# ---- e. the sharded calls: two blocks on device 0 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1])
def test_sharded_rollout_policy_fitness_off_the_fast_path(gymrs, kind):
    """The wide parameters go in through gymrs_sharded_set_params and the prepared state through the blocks' set_state; state, results,
    final observations, statistics and fitness records are those of one engine, and of the CPU reference"""
    c, want, records = sharded_reference(kind)
    default, wide = gymrs.engine.default_params(kind), engine_params(gymrs, kind, c.params)
    sh = gymrs.ShardedEngine(kind, c.n, [0, 0], global_env_offset=c.gid0, params=default, flags=c.flags)
    one = gymrs.BatchedEngine(kind, c.n, global_env_offset=c.gid0, flags=c.flags, params=default)
    assert len(sh.shards) == 2 and 0 < sh.shards[1].first_lane < c.n
    sh.reset(seed=c.reset_seed)
    one.reset(seed=c.reset_seed)
    sh.set_params(wide)
    one.set_params(wide)
    for s in sh.shards:
        s.set_state(c.prepare(s.get_state(), s.first_lane))
    one.set_state(c.prepare(one.get_state(), 0))
    sh.set_policy(c.weights, hidden=c.hidden, lanes_per_policy=c.lanes_per_policy)
    one.set_policy(c.weights, hidden=c.hidden, lanes_per_policy=c.lanes_per_policy)
    none = np.zeros(c.n, np.int8)  # (a lane's copy depends on the cut)
    same("start state", sh.get_state(), want[0].start_state, none, 0)
    for k, steps in enumerate(c.schedule):
        sh.rollout_policy_fitness(steps)
        one.rollout_policy_fitness(steps)
        sh.sync()
        one.sync()
        for x, y in ((sh.get_state(), one.get_state()), (sh.get_final_obs(), one.get_final_obs())) + tuple(zip(sh.get_step_result(), one.get_step_result())):
            assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), k  # one engine: the same bytes, NaNs included
        assert np.array_equal(sh.stats(), one.stats()) and np.array_equal(sh.stats(), want[k].stats), (k, sh.stats(), one.stats(), want[k].stats)
        assert_fitness(sh.policy_fitness(), one.policy_fitness(), k)
        assert_fitness(sh.policy_fitness(), records[k], k)
        assert_fitness(sum(s.policy_fitness() for s in sh.shards), records[k], "the blocks' own records")
        assert_launch(one, want[k], c.flags, c.classes, k)
    sh.close()
    one.close()


@pytest.mark.parametrize("kind", [0, 1])
def test_sharded_evaluate_policy_off_the_fast_path(gymrs, kind):
    c, want = evaluation_reference(kind, 1, 7, False, 0)
    default, wide = gymrs.engine.default_params(kind), engine_params(gymrs, kind, c.row)
    sh = gymrs.ShardedEngine(kind, c.n, [0, 0], global_env_offset=c.gid0, params=default, flags=0)
    one = gymrs.BatchedEngine(kind, c.n, global_env_offset=c.gid0, flags=0, params=default)
    assert len(sh.shards) == 2
    sh.set_params(wide)
    one.set_params(wide)
    sh.set_policy(c.weights, hidden=c.hidden, lanes_per_policy=c.lanes_per_policy)
    one.set_policy(c.weights, hidden=c.hidden, lanes_per_policy=c.lanes_per_policy)
    sh.evaluate_policy(c.episodes, c.max_steps, sl.EVAL_SEED, common_starts=c.common)
    single, lengths = evaluate(one, c)
    assert_records(sh.policy_eval(), single, "sharded against one engine")
    assert_records(sh.policy_eval(), want.records, "sharded against the CPU reference")
    assert_records(ev.merge([s.policy_eval() for s in sh.shards]), want.records, "the blocks' own records")
    assert_lengths(lengths, want.lengths, c.classes, "one engine's lengths")
    parts = [evaluate(s, c)[1] for s in sh.shards]  # the blocks' own per-episode lengths
    assert_lengths(np.concatenate(parts, axis=1), want.lengths, c.classes, "the blocks' lengths")
    sh.close()
    one.close()
