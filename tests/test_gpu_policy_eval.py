"""gymrs_evaluate_policy on the GPU: all eight fields of every policy's record and the whole per-episode `lengths` buffer against the
CPU reference of tests/policy_eval_ref.py (f32 twin resets and steps, tests/cpp/policy_ref.c actions, Python-int sums), compared
with == on integers: no tolerance anywhere.  The case table is policy_eval_ref's (2 envs x 2 shapes x 3 hidden widths x common
starts off / on; between them the shapes put lanes into the uniform and the gathered path, in full and in ragged waves)."""
import time
from functools import lru_cache

import closed_loop_ref as ref
import numpy as np
import policy_eval_ref as ev
import pytest
import torch
from closed_loop_ref import A, F, S, T, make_weights

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
E, M, P = ev.EPISODES, ev.MAX_STEPS, ev.N_POLICIES


class DeviceColumn:
    """A zero-copy torch view of an engine's device array"""

    def __init__(self, ptr, n, typestr):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (ptr, False), "version": 3}


def lengths_buffer(episodes, n):
    buf = torch.full((episodes, n), 0x7fffffff, dtype=torch.int32, device=DEV)  # (a value no episode writes)
    torch.cuda.synchronize()  # torch filled it on its stream; the engine writes it on its own
    return buf


def read_lengths(eng, buf):
    eng.sync()
    return buf.cpu().numpy().view(np.uint32)


def assert_records(got, want, at):
    assert got.dtype == np.int64 and want.dtype == np.int64 and got.shape == want.shape, (at, got.dtype, got.shape, want.shape)
    assert np.array_equal(got, want), (at, "fields that differ (policy, field)", np.argwhere(got != want)[:8].tolist(), got[:3], want[:3])


def assert_lengths(got, want, classes, at):
    assert got.shape == want.shape and got.dtype == want.dtype == np.uint32, (at, got.shape, want.shape)
    bad = np.flatnonzero((got != want).any(axis=0))
    assert not len(bad), (at, {ref.COPIES[c]: int((classes[bad] == c).sum()) for c in np.unique(classes[bad])}, bad[:8].tolist(),
                          got[:, bad[:4]].tolist(), want[:, bad[:4]].tolist())


def evaluate(eng, episodes, max_steps, seed, common=False):
    """(records, lengths) of one call"""
    buf = lengths_buffer(episodes, eng.n_envs)
    eng.evaluate_policy(episodes, max_steps, seed, common_starts=common, lengths=buf.data_ptr())
    return eng.policy_eval(), read_lengths(eng, buf)


def engine_for(gymrs, kind, n, gid0, params, weights, hidden, lpp, flags=0, vec=4):
    eng = gymrs.BatchedEngine(kind, n, global_env_offset=gid0, flags=flags, params=params, lanes_per_thread=vec)
    eng.set_policy(weights, hidden=hidden, lanes_per_policy=lpp)  # (no reset: the call reads no lane array)
    return eng


@lru_cache(maxsize=None)
def reference_of(gymrs, kind, shape, hidden, common):
    c = ev.case(kind, shape, hidden, common, gymrs.engine.default_params(kind))
    return c, ev.run_case(c)


def small_reference(gymrs, kind, n, gid0, weights, hidden, lpp, n_pol, seed, episodes, max_steps, common=False, params=None):
    params = params or (ev.mountain_car_params(gymrs.engine.default_params(1)) if kind == 1 else gymrs.engine.default_params(0))
    return params, ev.reference(kind, n, gid0, params, weights, hidden, lpp, n_pol, seed, episodes, max_steps, common)


# ---- a. the matrix -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,shape,hidden,common", ev.cases())
def test_evaluate_policy_equals_the_cpu_reference(gymrs, kind, shape, hidden, common):
    c, want = reference_of(gymrs, kind, shape, hidden, common)
    eng = engine_for(gymrs, kind, c.n, c.gid0, c.params, c.weights, hidden, c.lanes_per_policy)
    assert_records(eng.policy_eval(), ev.identity(P), "before the first call: identities")
    got, lengths = evaluate(eng, E, M, ev.SEED, common)
    assert_lengths(lengths, want.lengths, c.classes, "lengths")
    assert_records(got, want.records, "records")
    eng.close()


# ---- b. edge shapes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("n,episodes,max_steps,lpp,n_pol", [(1, 3, 17, 1000, 3), (63, 3, 17, 20, 3), (300, 1, 1, 100, 3), (700, 3, 17, 1, 5)],
                         ids=["n1", "n63", "E1M1", "B1P5"])
def test_edge_shapes(gymrs, kind, n, episodes, max_steps, lpp, n_pol):
    gid0, hidden = 12345, 7
    w = make_weights(kind, hidden, n_pol, seed=4)
    for common in (False, True):
        params, want = small_reference(gymrs, kind, n, gid0, w, hidden, lpp, n_pol, 21, episodes, max_steps, common)
        eng = engine_for(gymrs, kind, n, gid0, params, w, hidden, lpp)
        got, lengths = evaluate(eng, episodes, max_steps, 21, common)
        assert_lengths(lengths, want.lengths, ref.wave_classes(n, 4, gid0, n_pol, lpp), (n, common))
        assert_records(got, want.records, (n, common))
        assert got[:, 2].sum() == episodes * n
        if n == 1:  # the policies without a lane keep the identity
            assert sum(row.tolist() == list(ev.IDENTITY) for row in got) == n_pol - 1
        eng.close()


def test_max_episode_steps_zero_takes_the_params_default(gymrs):
    """CartPole, E = 1, M = 0 -> 500: policies that push one way fall within a dozen steps, one that balances (push towards the
    pole's lean and its angular velocity) runs longer; the reference plays with M = 500."""
    n, lpp = 600, 200
    w = np.array([[0, 0, 0, 0, 0, 0, 0, 0, 1, 0], [0, 0, 0, 0, 0, 0, 0, 0, 0, 1], [0, 0, 0, 0, 0, 0, 2, 1, 0, 0]], np.float32)
    params, want = small_reference(gymrs, 0, n, 0, w, 0, lpp, 3, 5, 1, 500)
    assert want.length[:, :2 * lpp].max() < 20 and want.length[:, 2 * lpp:].max() > 20  # (checked on the CPU: nothing waits for 500 steps)
    eng = engine_for(gymrs, 0, n, 0, params, w, 0, lpp)
    got, lengths = evaluate(eng, 1, 0, 5)
    assert_lengths(lengths, want.lengths, np.zeros(n, np.int8), "M = 0")
    assert_records(got, want.records, "M = 0")
    p = gymrs.engine.default_params(0)
    p.max_episode_steps = 9  # ... and it is the engine's CURRENT params' limit
    eng.set_params(p)
    _, want9 = small_reference(gymrs, 0, n, 0, w, 0, lpp, 3, 5, 1, 9, params=p)
    got, lengths = evaluate(eng, 1, 0, 5)
    assert_lengths(lengths, want9.lengths, np.zeros(n, np.int8), "M = 0 after set_params")
    assert_records(got, want9.records, "M = 0 after set_params")
    assert got[:, 4].any()
    eng.close()


# ---- c. the engine is left alone -------------------------------------------------------------------------------------------------------
def everything(eng, flags):
    out = {"state": eng.get_state(), "obs": eng.get_obs(), "final_obs": eng.get_final_obs(), "tick": np.array(eng.tick(), np.uint64),
           "stats": eng.stats(), "fitness": eng.policy_fitness(), "snapshot": np.frombuffer(eng.snapshot(), np.uint8)}
    for name, x in zip(("reward", "done", "truncated"), eng.get_step_result()):
        out[name] = x
    return out


def assert_same_engine(a, b, at):
    assert a.keys() == b.keys()
    for name in a:
        x, y = np.ascontiguousarray(a[name]), np.ascontiguousarray(b[name])
        assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes(), (at, name)


@pytest.mark.parametrize("kind", [0, 1])
def test_the_engine_is_untouched(gymrs, kind):
    n, gid0, lpp, hidden, flags = 4200, 12345, 1000, 8, A | S | T | F
    p = gymrs.engine.default_params(kind)
    p.max_episode_steps = M
    w = make_weights(kind, hidden, P, seed=2)
    eng = gymrs.BatchedEngine(kind, n, global_env_offset=gid0, flags=flags, params=p)
    eng.reset(seed=4)
    if kind == 1:
        eng.set_state(ref.mountain_car_prepare(eng.get_state(), 0))
    eng.set_policy(w, hidden=hidden, lanes_per_policy=lpp)
    eng.rollout_policy_fitness(23)  # mid-episode, with statistics, final observations and fitness counters that are not zero
    other = eng.clone()  # never evaluates
    other.set_policy(w, hidden=hidden, lanes_per_policy=lpp)
    before = everything(eng, flags)
    assert before["final_obs"].any() and before["fitness"].any() and before["stats"][2] > 0
    got, _ = evaluate(eng, E, M, 7)
    assert got[:, 2].sum() == E * n
    assert_same_engine(everything(eng, flags), before, "after evaluate_policy")
    eng.rollout_policy(9)
    other.rollout_policy(9)
    for name in ("state", "obs", "final_obs", "reward", "done", "truncated", "tick", "stats"):
        x, y = everything(eng, flags)[name], everything(other, flags)[name]
        assert np.ascontiguousarray(x).tobytes() == np.ascontiguousarray(y).tobytes(), name
    # the engine's flags and tuning do not matter to the result
    plain = engine_for(gymrs, kind, n, gid0, p, w, hidden, lpp, flags=0, vec=8)
    assert_records(evaluate(plain, E, M, 7)[0], got, "flags 0, 8 lanes per work-item against A|S|T|F")
    for e in (eng, other, plain):
        e.close()


# ---- d. the definition against the public API -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1])
def test_an_episode_is_reset_then_policy_actions_and_step(gymrs, kind):
    c, want = reference_of(gymrs, kind, 0, 8, False)
    eng = engine_for(gymrs, kind, c.n, c.gid0, c.params, c.weights, 8, c.lanes_per_policy)
    _, lengths = evaluate(eng, E, M, ev.SEED)
    eng.close()
    act = torch.zeros(4, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    for lane, e in ((0, 0), (999, 1), (1500, 2), (4199, 0), (4100, 2)):
        one = gymrs.BatchedEngine(kind, 1, global_env_offset=c.gid0 + lane, flags=0, params=c.params)
        one.set_policy(c.weights, hidden=8, lanes_per_policy=c.lanes_per_policy)
        one.reset(seed=ev.SEED + e)
        steps, done = 0, False
        while steps < M and not done:
            one.policy_actions(act.data_ptr())
            one.step(act.data_ptr())
            steps += 1
            done = bool(one.get_step_result()[1][0])
        one.close()
        assert int(lengths[e, lane]) == steps | (0x80000000 if done else 0), (lane, e, steps, done, hex(int(lengths[e, lane])))


# ---- e. cutting the batch ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("common", [False, True])
def test_cut_batches_and_the_sharded_handle_equal_one_engine(gymrs, kind, common):
    c, want = reference_of(gymrs, kind, 1, 7, common)
    cut = 2333  # not a multiple of a wave's 256 lanes, nor of 4
    parts = [engine_for(gymrs, kind, hi - lo, c.gid0 + lo, c.params, c.weights, 7, c.lanes_per_policy) for lo, hi in ((0, cut), (cut, c.n))]
    recs, lens = zip(*(evaluate(e, E, M, ev.SEED, common) for e in parts))
    assert_lengths(np.concatenate(lens, axis=1), want.lengths, c.classes, "two engines")
    assert_records(ev.merge(recs), want.records, "two engines, merged")
    sh = gymrs.ShardedEngine(kind, c.n, [0, 0, 0], global_env_offset=c.gid0, params=c.params, flags=0)
    assert len(sh.shards) == 3
    sh.set_policy(c.weights, hidden=7, lanes_per_policy=c.lanes_per_policy)
    sh.evaluate_policy(E, M, ev.SEED, common_starts=common)
    assert_records(sh.policy_eval(), want.records, "sharded, 3 blocks")
    assert_records(sh.policy_eval(1, 2), want.records[1:3], "a window")
    assert_records(ev.merge([s.policy_eval() for s in sh.shards]), want.records, "the blocks' own records")
    assert sh.policy_eval(1, 0).shape == (0, 8) and [n for _, n in sh.policy_eval_ptr()] == [P] * 3
    buf = lengths_buffer(1, 8)
    with pytest.raises(gymrs.GymrsError) as err:
        sh.evaluate_policy(E, M, ev.SEED, lengths=buf.data_ptr())
    assert err.value.status == 1 and "lengths_dev must be NULL" in str(err.value)
    for e in parts:
        e.close()
    sh.close()


# ---- f. stream order and the table's lifetime ----------------------------------------------------------------------------------------------
def test_stream_order_second_call_overwrites_and_set_policy_discards(gymrs):
    kind, n, gid0, lpp, hidden = 0, 4200, 12345, 1000, 0
    w0, w1 = make_weights(kind, hidden, P, seed=21), make_weights(kind, hidden, P, seed=3)
    p0, want0 = small_reference(gymrs, kind, n, gid0, w0, hidden, lpp, P, 5, E, M)
    _, want1 = small_reference(gymrs, kind, n, gid0, w1, hidden, lpp, P, 5, E, M)
    assert (want0.records != want1.records).any()
    eng = engine_for(gymrs, kind, n, gid0, p0, w0, hidden, lpp)
    ptr, count = eng.policy_weights_ptr()
    view = torch.as_tensor(DeviceColumn(ptr, count, "<f4"), device=DEV)
    new = torch.from_numpy(w1.reshape(-1)).to(DEV)
    bufs = [lengths_buffer(E, n) for _ in range(2)]
    eng.evaluate_policy(E, M, 5, lengths=bufs[0].data_ptr())  # enqueued before the rewrite: the old weights
    with torch.cuda.stream(torch.cuda.ExternalStream(eng.stream, device=DEV)):
        view.copy_(new)
    eng.evaluate_policy(E, M, 5, lengths=bufs[1].data_ptr())  # the next launch: the new ones
    assert_records(eng.policy_eval(), want1.records, "the table holds the latest call's results, not the sum")
    classes = ref.wave_classes(n, 4, gid0, P, lpp)
    assert_lengths(read_lengths(eng, bufs[0]), want0.lengths, classes, "first call")
    assert_lengths(read_lengths(eng, bufs[1]), want1.lengths, classes, "second call")
    # the view: the same records, stable until the next set_policy
    tptr, tcount = eng.policy_eval_ptr()
    assert tcount == P and eng.policy_eval_ptr() == (tptr, P)
    table = torch.as_tensor(DeviceColumn(tptr, P * 8, "<i8"), device=DEV).cpu().numpy().reshape(P, 8)
    torch.cuda.synchronize()
    assert_records(table, want1.records, "device view")
    assert_records(eng.policy_eval(1, 2), want1.records[1:3], "a window")
    eng.reset(seed=1)
    eng.rollout_policy_fitness(5)
    assert_records(eng.policy_eval(), want1.records, "reset and fitness launches leave the table alone")
    eng.set_policy(w1, hidden=hidden, lanes_per_policy=lpp)  # the same set again: discarded all the same
    assert_records(eng.policy_eval(), ev.identity(P), "set_policy discards the table")
    w5 = make_weights(kind, hidden, 5, seed=4)
    eng.set_policy(w5, hidden=hidden, lanes_per_policy=lpp)
    assert eng.policy_eval().shape == (5, 8) and eng.policy_eval_ptr()[1] == 5
    _, want5 = small_reference(gymrs, kind, n, gid0, w5, hidden, lpp, 5, 5, E, M)
    eng.evaluate_policy(E, M, 5)  # lengths_dev NULL
    assert_records(eng.policy_eval(), want5.records, "a new set of another size")
    eng.close()


# ---- g. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals(gymrs):
    eng = gymrs.BatchedEngine(0, 1000, flags=A)
    eng.reset(seed=1)
    calls = {"evaluate_policy": lambda e: e.evaluate_policy(1, 5), "policy_eval": lambda e: e.policy_eval(0, 1),
             "policy_eval_ptr": lambda e: e.policy_eval_ptr()}
    for name, call in calls.items():
        with pytest.raises(gymrs.GymrsError) as err:
            call(eng)
        assert err.value.status == 1 and "no policy" in str(err.value), name
    w = np.zeros((4, 10), np.float32)
    w[:, 8] = 1.0  # always push left: every episode is over within a dozen steps, whatever the limit
    eng.set_policy(w, lanes_per_policy=100)
    before = eng.get_state()
    buf = lengths_buffer(2, 1000)

    def refused(what, **kw):
        args = dict(episodes_per_lane=1, max_episode_steps=5, seed=0)
        args.update(kw)
        with pytest.raises(gymrs.GymrsError) as err:
            eng.evaluate_policy(**args)
        assert err.value.status == 1 and what in str(err.value) and "gymrs_evaluate_policy" in str(err.value), (what, str(err.value))

    refused("episodes_per_lane", episodes_per_lane=0)
    refused("unknown flag bits", flags=2)
    refused("unknown flag bits", flags=0x80000001)
    refused("4-byte aligned", lengths=buf.data_ptr() + 2)
    refused("GYMRS_POLICY_EVAL_MAX_STEPS", episodes_per_lane=1 << 12, max_episode_steps=(1 << 12) + 1)
    refused("GYMRS_POLICY_EVAL_MAX_STEPS", episodes_per_lane=(1 << 24) // 500 + 1, max_episode_steps=0)  # M = 0 counts as the default 500
    refused("GYMRS_POLICY_EVAL_MAX_STEPS", episodes_per_lane=0xffffffff, max_episode_steps=0xffffffff)
    desc = gymrs.EvalDesc(1, 5, 0, 0, 1, None)
    lib = gymrs.load_library()
    assert lib.gymrs_evaluate_policy(eng._h, __import__("ctypes").byref(desc)) == 1 and "reserved" in lib.gymrs_last_error().decode()
    assert lib.gymrs_evaluate_policy(eng._h, None) == 1 and "NULL desc" in lib.gymrs_last_error().decode()
    for first, count in ((0, 5), (4, 1), (2**32 - 1, 2)):
        with pytest.raises(gymrs.GymrsError) as err:
            eng.policy_eval(first, count)
        assert err.value.status == 1 and "n_policies" in str(err.value)
    assert eng.policy_eval(4, 0).shape == (0, 8)
    assert_records(eng.policy_eval(), ev.identity(4), "a refused call changes nothing")
    rows = [gymrs.engine.default_params(0), gymrs.engine.default_params(0)]
    rows[1].gravity *= 1.25
    eng.set_param_table(rows)
    refused("parameter table")
    refused("gymrs_policy_actions + gymrs_step")
    eng.set_param_table(None)
    eng.evaluate_policy(1, (1 << 24))  # exactly at the bound
    assert eng.policy_eval()[:, 7].max() < 20
    eng.evaluate_policy(2, 5, lengths=buf.data_ptr())
    rec = eng.policy_eval()
    assert rec[:, 2].tolist() == [2 * 300, 2 * 300, 2 * 200, 2 * 200] and np.array_equal(eng.get_state(), before) and eng.tick()[0] == 1
    eng.close()
    pend = gymrs.BatchedEngine(2, 500, flags=A | T)
    pend.reset(seed=1)
    for name, call in calls.items():
        with pytest.raises(gymrs.GymrsError) as err:
            call(pend)
        assert err.value.status == 1 and "Pendulum" in str(err.value), name
    pend.close()


def test_non_finite_weights_are_legal(gymrs):
    kind, n, gid0, lpp = 0, 1300, 12345, 500
    w = make_weights(kind, 7, P, seed=18)
    w[0, 3], w[1, 5], w[2, -1] = np.nan, np.inf, -np.inf
    params, want = small_reference(gymrs, kind, n, gid0, w, 7, lpp, P, 3, E, M)
    eng = engine_for(gymrs, kind, n, gid0, params, w, 7, lpp)
    got, lengths = evaluate(eng, E, M, 3)
    assert_lengths(lengths, want.lengths, ref.wave_classes(n, 4, gid0, P, lpp), "non-finite weights")
    assert_records(got, want.records, "non-finite weights")
    eng.close()


# ---- speed -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.perf
def test_evaluating_whole_episodes_is_no_slower_than_the_fixed_length_launch(gymrs):
    """CartPole, 1024 affine policies x 1024 lanes, seeded normal weights, E = 4, M = 200, engine flags A | T with max_episode_steps = M.
    Best of 5 evaluate_policy against best of 5 rollout_policy_fitness(E * M) on the same engine and policy set, both timed here
    (host clock around a call and the synchronise that ends it).  t(evaluate) <= t(fitness); no margin."""
    n_pol, lanes, episodes, max_steps = 1024, 1024, 4, 200
    n = n_pol * lanes
    p = gymrs.engine.default_params(0)
    p.max_episode_steps = max_steps
    eng = gymrs.BatchedEngine(0, n, flags=A | T, params=p)
    eng.reset(seed=0)
    eng.set_policy(make_weights(0, 0, n_pol, seed=1), lanes_per_policy=lanes)

    def best(run):
        run()  # warm-up (the tables come into being)
        eng.sync()
        times = []
        for _ in range(5):
            t0 = time.perf_counter()
            run()
            eng.sync()
            times.append(time.perf_counter() - t0)
        return min(times)

    t_fit = best(lambda: eng.rollout_policy_fitness(episodes * max_steps))
    t_eval = best(lambda: eng.evaluate_policy(episodes, max_steps, 0))
    rec = eng.policy_eval()
    assert rec[:, 2].tolist() == [episodes * lanes] * n_pol
    print(f"\nevaluate_policy(E={episodes}, M={max_steps}): {t_eval * 1e3:.3f} ms for {int(rec[:, 5].sum())} lane-steps; "
          f"rollout_policy_fitness({episodes * max_steps}): {t_fit * 1e3:.3f} ms for {n * episodes * max_steps} lane-steps; ratio {t_eval / t_fit:.3f}")
    assert t_eval <= t_fit
    eng.close()
