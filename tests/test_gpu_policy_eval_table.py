"""gymrs_evaluate_policy with GYMRS_EVAL_LANE_PARAMS on the GPU: every lane plays its episodes with its own row of the parameter
table.  All eight fields of every policy's record and the whole per-episode `lengths` buffer against the CPU reference of
tests/policy_eval_table_ref.py, compared with == on integers: no tolerance anywhere.  The case table is policy_eval_table_ref's (2
envs x 2 shapes x 3 hidden widths x common starts off / on, K = 5 rows and a random index); tests/test_policy_eval_table_ref.py
shows without a GPU that none of them can pass with the rows ignored.  Then the flag without a table, a one-row table, the engine left
alone, the index rewritten in stream order, indices beyond the table, CartPole's second integrator, the general path, cut batches and
the sharded table calls, and the refusals that stay."""
from functools import lru_cache

import closed_loop_ref as ref
import lane_params_ref as lp
import numpy as np
import policy_eval_ref as ev
import policy_eval_table_ref as tb
import pytest
import torch
from closed_loop_ref import A, F, S, T, make_weights

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
E, M, P, K = tb.EPISODES, tb.MAX_STEPS, tb.N_POLICIES, tb.K
SENTINEL = 0x7fffffff  # a value no episode writes


class DeviceColumn:
    """A zero-copy torch view of an engine's device array"""

    def __init__(self, ptr, n, typestr):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (ptr, False), "version": 3}


def lengths_buffer(episodes, n):
    buf = torch.full((episodes, n), SENTINEL, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()  # torch filled it on its stream; the engine writes it on its own
    return buf


def read_lengths(eng, buf):
    eng.sync()
    return buf.cpu().numpy().view(np.uint32)


def assert_records(got, want, at):
    assert got.dtype == np.int64 and want.dtype == np.int64 and got.shape == want.shape, (at, got.dtype, got.shape, want.shape)
    assert np.array_equal(got, want), (at, "fields that differ (policy, field)", np.argwhere(got != want)[:8].tolist(), got[:3], want[:3])


def assert_lengths(got, want, classes, at, index=None):
    assert got.shape == want.shape and got.dtype == want.dtype == np.uint32, (at, got.shape, want.shape)
    bad = np.flatnonzero((got != want).any(axis=0))
    assert not len(bad), (at, {ref.COPIES[c]: int((classes[bad] == c).sum()) for c in np.unique(classes[bad])}, bad[:8].tolist(),
                          None if index is None else np.asarray(index)[bad[:8]].tolist(), got[:, bad[:4]].tolist(), want[:, bad[:4]].tolist())


def evaluate(eng, episodes=E, max_steps=M, seed=tb.SEED, common=False, lane_params=True):
    """(records, lengths) of one call"""
    buf = lengths_buffer(episodes, eng.n_envs)
    eng.evaluate_policy(episodes, max_steps, seed, common_starts=common, lengths=buf.data_ptr(), lane_params=lane_params)
    return eng.policy_eval(), read_lengths(eng, buf)


def params_type(gymrs, kind):
    return type(gymrs.engine.default_params(kind))


def table_engine(gymrs, kind, n, gid0, rows, index, weights, hidden, lpp, flags=0):
    """An engine with the table `rows` (lane_params_ref rows), the index and the policy set; never reset: the call reads no lane array"""
    rows = lp.rows_for(params_type(gymrs, kind), rows)
    eng = gymrs.BatchedEngine(kind, n, global_env_offset=gid0, flags=flags, params=rows[0])
    eng.set_param_table(rows)
    if index is not None:
        eng.set_param_index(np.asarray(index, np.uint16))
    eng.set_policy(weights, hidden=hidden, lanes_per_policy=lpp)
    return eng


def engine_of(gymrs, c, lo=0, hi=None):
    hi = c.n if hi is None else hi
    return table_engine(gymrs, c.kind, hi - lo, c.gid0 + lo, c.rows, c.index[lo:hi], c.weights, c.hidden, c.lanes_per_policy)


@lru_cache(maxsize=None)
def reference_of(kind, shape, hidden, common, integrator=0):
    c = tb.case(kind, shape, hidden, common, integrator=integrator)
    return c, tb.run_case(c)


def index_view(eng):
    """The engine's uint16 index as an int16 torch view (the same bits)"""
    return torch.as_tensor(DeviceColumn(eng.param_index_ptr(), eng.n_envs, "<i2"), device=DEV)


# ---- a. the matrix -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,shape,hidden,common", tb.cases())
def test_lane_params_equal_the_cpu_reference(gymrs, kind, shape, hidden, common):
    c, want = reference_of(kind, shape, hidden, common)
    eng = engine_of(gymrs, c)
    got, lengths = evaluate(eng, common=common)
    assert_lengths(lengths, want.lengths, c.classes, "lengths", c.index)
    assert_records(got, want.records, "records")
    assert np.array_equal(eng.get_param_index(), c.index)
    eng.close()


# ---- b. no table, a one-row table ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("common", [False, True])
def test_the_flag_without_a_table_and_a_one_row_table_change_nothing(gymrs, kind, common):
    n, _, gid0, lpp = tb.SHAPES[0]
    params = gymrs.engine.default_params(kind)
    if kind == 1:
        ev.mountain_car_params(params)
    w = make_weights(kind, 7, P, ev.WEIGHT_SEEDS[kind, 7, 0])
    eng = gymrs.BatchedEngine(kind, n, global_env_offset=gid0, flags=0, params=params)
    eng.set_policy(w, hidden=7, lanes_per_policy=lpp)
    plain = evaluate(eng, common=common, lane_params=False)
    assert plain[0][:, 2].sum() == E * n and plain[0][:, 3].any() and plain[0][:, 4].any()
    flagged = evaluate(eng, common=common)
    assert_records(flagged[0], plain[0], "the flag without a table")
    assert np.array_equal(flagged[1], plain[1])
    raw = lengths_buffer(E, n)
    eng.evaluate_policy(E, M, tb.SEED, lengths=raw.data_ptr(), flags=gymrs.EVAL_LANE_PARAMS | (gymrs.EVAL_COMMON_STARTS if common else 0))
    assert_records(eng.policy_eval(), plain[0], "raw flag bits")
    assert np.array_equal(read_lengths(eng, raw), plain[1])
    eng.set_param_table([params])  # one row, equal to the engine's params: the table kernel, every lane on row 0
    assert eng.param_table() and not eng.get_param_index().any()
    one_row = evaluate(eng, common=common)
    assert_records(one_row[0], plain[0], "a one-row table")
    assert np.array_equal(one_row[1], plain[1])
    eng.set_param_table(None)
    assert_records(evaluate(eng, common=common)[0], plain[0], "the table switched off again")
    eng.close()


# ---- c. the engine is left alone -------------------------------------------------------------------------------------------------------
def everything(eng):
    out = {"state": eng.get_state(), "obs": eng.get_obs(), "final_obs": eng.get_final_obs(), "tick": np.array(eng.tick(), np.uint64),
           "stats": eng.stats(), "fitness": eng.policy_fitness(), "index": eng.get_param_index(), "snapshot": np.frombuffer(eng.snapshot(), np.uint8)}
    for name, x in zip(("reward", "done", "truncated"), eng.get_step_result()):
        out[name] = x
    return out


@pytest.mark.parametrize("kind", [0, 1])
def test_the_engine_is_untouched(gymrs, kind):
    n, gid0, lpp, hidden, flags = 4200, 12345, 1000, 8, A | S | T | F
    rows = lp.make_rows(kind, K, tb.ROWS_SEED[kind], M)
    index = lp.make_index(n, K, tb.INDEX_SEED[kind])
    w = make_weights(kind, hidden, P, seed=2)
    eng = gymrs.BatchedEngine(kind, n, global_env_offset=gid0, flags=flags, params=lp.rows_for(params_type(gymrs, kind), rows)[0])
    eng.reset(seed=4)
    if kind == 1:
        eng.set_state(ref.mountain_car_prepare(eng.get_state(), 0))
    eng.set_policy(w, hidden=hidden, lanes_per_policy=lpp)
    eng.rollout_policy_fitness(23)  # (before the table: the fused policy rollouts refuse one) statistics, final observations, counters
    eng.set_param_table(lp.rows_for(params_type(gymrs, kind), rows))
    eng.set_param_index(index)
    eng.rollout(5, action_seed=3)  # mid-episode under the table
    before = everything(eng)
    assert before["final_obs"].any() and before["fitness"].any() and before["stats"][2] > 0 and np.array_equal(before["index"], index)
    got, _ = evaluate(eng, seed=7)
    assert got[:, 2].sum() == E * n
    after = everything(eng)
    assert before.keys() == after.keys()
    for name in before:
        x, y = np.ascontiguousarray(before[name]), np.ascontiguousarray(after[name])
        assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes(), name
    # the engine's flags and state do not matter to the result
    fresh = table_engine(gymrs, kind, n, gid0, rows, index, w, hidden, lpp)
    assert_records(evaluate(fresh, seed=7)[0], got, "a fresh flags = 0 engine against A|S|T|F mid-episode")
    eng.close()
    fresh.close()


# ---- d. the index: rewritten in stream order, beyond the table ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1])
def test_the_index_rewritten_in_stream_order(gymrs, kind):
    c, want = reference_of(kind, 0, 7, False)
    index2 = lp.make_index(c.n, K, tb.INDEX_SEED[kind] + 10)
    want2 = tb.run_case(c, index2)
    assert (want2.records != want.records).any() and (index2 != c.index).mean() > 0.5
    eng = engine_of(gymrs, c)
    view = index_view(eng)
    new = torch.from_numpy(index2.view(np.int16)).to(DEV)
    torch.cuda.synchronize()
    bufs = [lengths_buffer(E, c.n) for _ in range(2)]
    eng.evaluate_policy(E, M, tb.SEED, lengths=bufs[0].data_ptr(), lane_params=True)  # enqueued before the rewrite: the old index
    with torch.cuda.stream(torch.cuda.ExternalStream(eng.stream, device=DEV)):
        view.copy_(new)
    eng.evaluate_policy(E, M, tb.SEED, lengths=bufs[1].data_ptr(), lane_params=True)  # the next launch: the new one
    assert_records(eng.policy_eval(), want2.records, "the latest call, the new index")
    assert_lengths(read_lengths(eng, bufs[0]), want.lengths, c.classes, "first call", c.index)
    assert_lengths(read_lengths(eng, bufs[1]), want2.lengths, c.classes, "second call", index2)
    assert np.array_equal(eng.get_param_index(), index2)
    eng.close()


@pytest.mark.parametrize("kind", [0, 1])
def test_lanes_with_an_index_beyond_the_table_play_nothing(gymrs, kind):
    c, _ = reference_of(kind, 0, 8, False)
    index = c.index.astype(np.int64).copy()
    out = np.array([0, 5, 6, 7, 999, 1000, 1001, 2047, 2048, 4196, 4199])  # whole work-items and single lanes, both paths, the ragged end
    index[out] = [K, K + 1, 65535, K, 40000, K, 65535, K, K, 65535, K]
    want = tb.run_case(c, index)
    assert not want.valid[out].any() and want.valid.sum() == c.n - len(out)
    eng = engine_of(gymrs, c)
    view = index_view(eng)  # (gymrs_set_param_index copies what it is given: the view is how such an index gets there)
    with torch.cuda.stream(torch.cuda.ExternalStream(eng.stream, device=DEV)):
        view.copy_(torch.from_numpy(index.astype(np.uint16).view(np.int16)).to(DEV))
    got, lengths = evaluate(eng)
    assert (lengths[:, out] == SENTINEL).all(), lengths[:, out].tolist()
    assert_lengths(lengths[:, want.valid], want.lengths[:, want.valid], c.classes[want.valid], "the other lanes", index[want.valid])
    assert_records(got, want.records, "records over the other lanes")
    assert got[:, 2].sum() == E * (c.n - len(out))
    eng.sync()  # no error is raised, and the index stays
    assert np.array_equal(eng.get_param_index(), index.astype(np.uint16))
    eng.close()


# ---- e. the other code paths ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("common", [False, True])
def test_cartpole_semi_implicit_integrator(gymrs, common):
    c, want = reference_of(0, 1, 8, common, 1)
    _, euler = reference_of(0, 1, 8, common)
    assert all(r.kinematics_integrator == 1 for r in c.rows) and (want.lengths != euler.lengths).any() and (want.records != euler.records).any()
    eng = engine_of(gymrs, c)
    got, lengths = evaluate(eng, common=common)
    assert_lengths(lengths, want.lengths, c.classes, "integrator 1", c.index)
    assert_records(got, want.records, "integrator 1")
    eng.close()


@pytest.mark.parametrize("kind", [0, 1])
def test_non_finite_weights_under_a_table(gymrs, kind):
    """NaN and infinite weights are legal: the logits they give are NaN or infinite and the argmax rule still picks a discrete action.
    The states stay inside the fast path's range (an action of a Discrete env, whatever it was chosen from, moves no state out of
    it); tests/test_gpu_policy_slowpaths.py has the cases that leave it."""
    n, gid0, lpp = 1300, 12345, 500
    w = make_weights(kind, 7, P, seed=18)
    w[0, 3], w[1, 5], w[2, -1] = np.nan, np.inf, -np.inf
    rows = lp.make_rows(kind, K, tb.ROWS_SEED[kind], M)
    index = lp.make_index(n, K, tb.INDEX_SEED[kind])
    want = tb.reference(kind, n, gid0, rows, index, w, 7, lpp, P, 3, E, M)
    eng = table_engine(gymrs, kind, n, gid0, rows, index, w, 7, lpp)
    got, lengths = evaluate(eng, seed=3)
    assert_lengths(lengths, want.lengths, ref.wave_classes(n, 4, gid0, P, lpp), "non-finite weights", index)
    assert_records(got, want.records, "non-finite weights")
    eng.close()


def test_rows_that_drive_lanes_out_of_the_fast_range(gymrs):
    """CartPole: row 1 pushes 40 times as hard and ends an episode only far beyond |theta| = pi / 4, so its lanes go on playing on
    the general path (tests/test_policy_eval_table_ref.py counts them on the CPU); rows 0 and 2 share their waves."""
    n, _, gid0, lpp = tb.SHAPES[0]
    rows = tb.hard_push_rows()
    index = lp.make_index(n, len(rows), 41)
    w = make_weights(0, 7, P, 18)
    want = tb.reference(0, n, gid0, rows, index, w, 7, lpp, P, tb.SEED, E, M)
    assert (want.length[:, index == 1] == M).any() and (want.done[:, index == 0]).any()
    eng = table_engine(gymrs, 0, n, gid0, rows, index, w, 7, lpp)
    got, lengths = evaluate(eng)
    assert_lengths(lengths, want.lengths, ref.wave_classes(n, 4, gid0, P, lpp), "hard-push rows", index)
    assert_records(got, want.records, "hard-push rows")
    eng.close()


# ---- f. cutting the batch, the sharded table calls -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("common", [False, True])
def test_cut_batches_and_the_sharded_handle_equal_one_engine(gymrs, kind, common):
    c, want = reference_of(kind, 0, 7, common)
    cut = 2333  # not a multiple of a wave's 256 lanes, nor of 4
    parts = [engine_of(gymrs, c, lo, hi) for lo, hi in ((0, cut), (cut, c.n))]
    recs, lens = zip(*(evaluate(e, common=common) for e in parts))
    assert_lengths(np.concatenate(lens, axis=1), want.lengths, c.classes, "two engines", c.index)
    assert_records(ev.merge(recs), want.records, "two engines, merged")
    for e in parts:
        e.close()
    rows = lp.rows_for(params_type(gymrs, kind), c.rows)
    sh = gymrs.ShardedEngine(kind, c.n, [0, 0, 0], global_env_offset=c.gid0, params=rows[0], flags=0)
    assert len(sh.shards) == 3 and sh.param_table() == []
    sh.set_policy(c.weights, hidden=7, lanes_per_policy=c.lanes_per_policy)
    sh.set_param_table(rows)
    assert [bytes(r) for r in sh.param_table()] == [bytes(r) for r in rows] and not sh.get_param_index().any()
    sh.set_param_index(c.index)
    sh.evaluate_policy(E, M, tb.SEED, common_starts=common, lane_params=True)
    assert_records(sh.policy_eval(), want.records, "sharded, 3 blocks")
    assert_records(ev.merge([s.policy_eval() for s in sh.shards]), want.records, "the blocks' own records")
    with pytest.raises(gymrs.GymrsError) as err:
        sh.evaluate_policy(E, M, tb.SEED, common_starts=common)  # without the flag every block refuses
    assert err.value.status == 1 and "parameter table" in str(err.value) and "GYMRS_EVAL_LANE_PARAMS" in str(err.value)
    sh.close()


@pytest.mark.parametrize("kind", [0, 1])
def test_sharded_table_calls_reach_every_block(gymrs, kind):
    n, gid0, flags = 4200, 12345, A | S
    rows = lp.rows_for(params_type(gymrs, kind), lp.make_rows(kind, K, tb.ROWS_SEED[kind], M))
    index = lp.make_index(n, K, tb.INDEX_SEED[kind])
    sh = gymrs.ShardedEngine(kind, n, [0, 0, 0], global_env_offset=gid0, params=rows[0], flags=flags)
    one = gymrs.BatchedEngine(kind, n, global_env_offset=gid0, flags=flags, params=rows[0])
    bounds = [s.first_lane for s in sh.shards] + [n]
    assert bounds[1] % 1024 == 0 and 0 < bounds[1] < bounds[2] < n
    sh.set_param_table(rows)
    one.set_param_table(rows)
    # the index in batch numbering: ranges inside one block, across one boundary, across both, and the whole batch
    sh.set_param_index(index)
    assert np.array_equal(sh.get_param_index(), index)
    for first, count in ((3, 100), (bounds[1] - 7, 20), (bounds[1] - 1, bounds[2] - bounds[1] + 2), (bounds[2], n - bounds[2]), (n, 0), (17, 0)):
        assert np.array_equal(sh.get_param_index(first, count), index[first:first + count]), (first, count)
    patch_at, patch = bounds[1] - 5, ((np.arange(bounds[2] - bounds[1] + 11) * 3) % K).astype(np.uint16)
    sh.set_param_index(patch, first=patch_at)
    index[patch_at:patch_at + len(patch)] = patch
    assert np.array_equal(sh.get_param_index(), index)
    assert np.array_equal(np.concatenate([s.get_param_index() for s in sh.shards]), index)
    one.set_param_index(index)
    # three steps and a 7-step rollout with that table: the state of one engine with the same table, bit for bit
    sh.reset(seed=5)
    one.reset(seed=5)
    acts = [torch.zeros(s.n_envs, dtype=torch.uint8, device=DEV) for s in sh.shards]
    whole = torch.zeros(n, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    for t in range(3):
        sh.fill_actions([a.data_ptr() for a in acts], 9, t)
        sh.step([a.data_ptr() for a in acts])
        one.fill_actions(whole.data_ptr(), 9, t)
        one.step(whole.data_ptr())
    sh.sync()
    one.sync()
    assert sh.get_state().tobytes() == one.get_state().tobytes(), "3 steps"
    uniform = gymrs.BatchedEngine(kind, n, global_env_offset=gid0, flags=flags, params=rows[0])  # (... and the rows matter to it)
    uniform.reset(seed=5)
    for t in range(3):
        uniform.fill_actions(whole.data_ptr(), 9, t)
        uniform.step(whole.data_ptr())
    assert (uniform.get_state() != one.get_state()).any(axis=0).mean() > 0.5
    uniform.close()
    sh.rollout(7, action_seed=9, action_t0=3)
    one.rollout(7, action_seed=9, action_t0=3)
    sh.sync()
    assert sh.get_state().tobytes() == one.get_state().tobytes(), "7-step rollout"
    assert np.array_equal(sh.stats(), one.stats())
    sh.set_param_table(None)
    assert sh.param_table() == [] and all(s.param_table() == [] for s in sh.shards)
    sh.close()
    one.close()


# ---- g. refusals that stay ---------------------------------------------------------------------------------------------------------------------
def test_refusals(gymrs):
    rows = [gymrs.engine.default_params(0), gymrs.engine.default_params(0)]
    rows[1].gravity *= 1.25
    eng = gymrs.BatchedEngine(0, 1000, flags=A)
    eng.reset(seed=1)
    w = np.zeros((4, 10), np.float32)
    w[:, 8] = 1.0
    eng.set_policy(w, lanes_per_policy=100)
    eng.set_param_table(rows)

    def refused(e, *what, **kw):
        with pytest.raises(gymrs.GymrsError) as err:
            e.evaluate_policy(1, 5, **kw)
        assert err.value.status == 1 and all(x in str(err.value) for x in what) and "evaluate_policy" in str(err.value), (what, str(err.value))

    refused(eng, "parameter table", "gymrs_policy_actions + gymrs_step", "GYMRS_EVAL_LANE_PARAMS")  # without the flag, with a table
    refused(eng, "parameter table", "gymrs_policy_actions + gymrs_step", common_starts=True)
    refused(eng, "unknown flag bits", flags=4 | 2)
    refused(eng, "unknown flag bits", flags=4 | 0x80000000)
    eng.evaluate_policy(1, 5, lane_params=True)
    assert eng.policy_eval()[:, 2].tolist() == [300, 300, 200, 200]
    eng.close()
    sh = gymrs.ShardedEngine(0, 3000, [0, 0], flags=A)
    idx = np.zeros(8, np.uint16)
    for call in (lambda: sh.set_param_index(idx), lambda: sh.get_param_index(0, 8)):  # no table yet
        with pytest.raises(gymrs.GymrsError) as err:
            call()
        assert err.value.status == 1 and "no parameter table" in str(err.value)
    sh.set_param_table(rows)
    for call, name in ((lambda: sh.set_param_index(idx, first=2993), "gymrs_sharded_set_param_index"), (lambda: sh.get_param_index(3001, 0), "gymrs_sharded_get_param_index"),
                       (lambda: sh.get_param_index(2**64 - 4, 8), "gymrs_sharded_get_param_index")):
        with pytest.raises(gymrs.GymrsError) as err:
            call()
        assert err.value.status == 1 and name in str(err.value) and "out of bounds" in str(err.value), name
    sh.set_param_index(idx, first=2992)  # exactly to the end
    sh.close()
    pend = gymrs.ShardedEngine(2, 2000, [0, 0], flags=A | T)
    with pytest.raises(gymrs.GymrsError) as err:
        pend.set_param_table([gymrs.engine.default_params(2)])
    assert err.value.status == 1 and "Pendulum" in str(err.value)
    refused(pend, "Pendulum", lane_params=True)
    pend.close()
    one = gymrs.BatchedEngine(2, 500, flags=A | T)
    refused(one, "Pendulum", lane_params=True)
    one.close()
