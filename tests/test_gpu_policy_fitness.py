"""gymrs_rollout_policy_fitness on the GPU: the per-policy counters against the CPU reference of tests/policy_fitness_ref.py (the rows
of tests/closed_loop_ref.py summed per policy with Python ints), and the engine after the call against the same reference
gymrs_rollout_policy is held to: the call is gymrs_rollout_policy plus counters, nothing else.

Counters are compared with == on int64; state, observations, results, statistics, final observations and tick bit for bit.  No
tolerance anywhere.  The case table is closed_loop_ref's (every flag set, both vector widths, all four copies of the kernel)."""
import time
from types import SimpleNamespace

import closed_loop_ref as ref
import numpy as np
import policy_fitness_ref as fit
import pytest
import torch
from closed_loop_ref import A, COPIES, DIMS, F, S, T, make_weights

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


# ---- helpers (as tests/test_gpu_policy_matrix.py) ------------------------------------------------------------------------------
def where(got, want, classes):
    g, w = np.ascontiguousarray(got), np.ascontiguousarray(want)
    bad = (g.view(np.uint32) if g.dtype == np.float32 else g) != (w.view(np.uint32) if w.dtype == np.float32 else w)
    while bad.ndim > 1:
        bad = bad.any(axis=0)
    lanes = np.flatnonzero(bad)
    return {COPIES[c]: int((classes[lanes] == c).sum()) for c in np.unique(classes[lanes])}, lanes[:8].tolist()


def same(what, got, want, classes, at):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, at, got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype == np.float32:
        got, want = got.view(np.uint32), want.view(np.uint32)
    assert np.array_equal(got, want), (what, at) + where(got, want, classes)


def assert_launch(eng, want, flags, classes, at, first=0):
    sl = slice(first, first + eng.n_envs)
    classes = classes[sl]
    same("state", eng.get_state(), want.state[:, sl], classes, at)
    same("obs", eng.get_obs(), want.obs[:, sl], classes, at)
    r, d, tr = eng.get_step_result()
    same("reward", r, want.reward[sl], classes, at)
    same("done", d, want.done[sl], classes, at)
    if flags & T:
        same("truncated", tr, want.truncated[sl], classes, at)
    if flags & F:
        same("final_obs", eng.get_final_obs(), want.final[:, sl], classes, at)
    assert eng.tick()[0] == want.tick, (at, eng.tick(), want.tick)


def assert_stats(eng, want, at):
    gs = eng.stats()
    assert np.array_equal(gs[1:], want.stats[1:]) and gs[0] == want.stats[0], (at, gs, want.stats)


def assert_fitness(got, want, at):
    assert got.dtype == np.int64 and want.dtype == np.int64 and got.shape == want.shape, (at, got.dtype, got.shape, want.shape)
    assert np.array_equal(got, want), (at, "policies that differ", np.flatnonzero((got != want).any(axis=1))[:8].tolist(), got[:4], want[:4])


def make_engine(gymrs, c, first=0, count=None):
    count = c.n - first if count is None else count
    eng = gymrs.BatchedEngine(c.kind, count, global_env_offset=c.gid0 + first, flags=c.flags, params=c.params, lanes_per_thread=c.vec)
    eng.reset(seed=c.reset_seed)
    if c.prepare is not None:
        eng.set_state(c.prepare(eng.get_state(), first))
    eng.set_policy(c.weights, hidden=c.hidden, lanes_per_policy=c.lanes_per_policy)
    return eng


def small_engine(gymrs, kind, n, flags, weights, lpp, hidden=0, gid0=0, seed=5, vec=4, max_steps=ref.MAX_EPISODE_STEPS):
    p = gymrs.engine.default_params(kind)
    p.max_episode_steps = max_steps
    eng = gymrs.BatchedEngine(kind, n, global_env_offset=gid0, flags=flags, params=p, lanes_per_thread=vec)
    eng.reset(seed=seed)
    eng.set_policy(weights, hidden=hidden, lanes_per_policy=lpp)
    return eng


def recorded_lane_sums(eng, kind, steps, flags):
    """What `steps` steps of rollout_policy_record write to the reward / done / truncated rows, summed per LANE: (n, 4) int64 in
    record order (reward_sum, episodes, done, truncated)."""
    n, d = eng.n_envs, DIMS[kind][0]
    stride = (n + 15) // 16 * 16
    obs = torch.zeros((steps, d, stride), dtype=torch.float32, device=DEV)
    act = torch.zeros((steps, stride), dtype=torch.uint8, device=DEV)
    rew = torch.zeros((steps, stride), dtype=torch.float32, device=DEV)
    done = torch.zeros((steps, stride), dtype=torch.uint8, device=DEV)
    trunc = torch.zeros((steps, stride), dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()  # torch filled these on its stream; the engine writes them on its own
    eng.rollout_policy_record(steps, obs=obs.data_ptr(), actions=act.data_ptr(), reward=rew.data_ptr(), done=done.data_ptr(),
                              truncated=trunc.data_ptr() if flags & T else 0, lane_stride=stride)
    eng.sync()
    rew_h, done_h, trunc_h = (x.cpu().numpy()[:, :n] for x in (rew, done, trunc))
    r = rew_h.astype(np.int64)
    assert np.array_equal(r.astype(np.float32), rew_h)
    dn, tr = done_h.astype(np.int64), trunc_h.astype(np.int64)
    return np.stack([r.sum(axis=0), ((dn | tr) != 0).sum(axis=0), dn.sum(axis=0), tr.sum(axis=0)], axis=1).astype(np.int64)


def per_policy(lane_sums, gid0, lpp, n_policies):
    pol = fit.policies_of(len(lane_sums), gid0, lpp, n_policies)
    out = np.zeros((n_policies, 4), np.int64)
    np.add.at(out, pol, lane_sums)
    return out


# ---- a. the matrix: every copy of every kernel -----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,shape,flags,hidden", ref.cases(record=False))
def test_rollout_policy_fitness_equals_the_cpu_reference_in_every_copy(gymrs, kind, shape, flags, hidden):
    c = ref.case(kind, shape, flags, hidden, gymrs.engine.default_params(kind))
    want = ref.run_case(c)
    records = fit.of_case(c, want)
    eng = make_engine(gymrs, c)
    assert_fitness(eng.policy_fitness(), np.zeros((ref.N_POLICIES, 4), np.int64), "before the first launch")
    for k, steps in enumerate(c.schedule):
        eng.rollout_policy_fitness(steps)
        assert_fitness(eng.policy_fitness(), records[k], k)
        assert_launch(eng, want[k], flags, c.classes, k)  # the engine is left as rollout_policy leaves it
        assert_stats(eng, want[k], k)
    eng.close()


# ---- b. the definition, literally: the counters are per-policy sums of the rows rollout_policy_record writes -----------------------
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("flags", [0, A | S, A | S | T | F])
def test_counters_equal_sums_of_the_recorded_rows(gymrs, kind, flags):
    n, gid0, lpp, hidden = 4200, (1 << 40) + 12345, 1000, 8
    w = make_weights(kind, hidden, 3, seed=2)
    a = small_engine(gymrs, kind, n, flags, w, lpp, hidden, gid0)
    b = small_engine(gymrs, kind, n, flags, w, lpp, hidden, gid0)
    total = np.zeros((3, 4), np.int64)
    for steps in (7, 40):
        a.rollout_policy_fitness(steps)
        total += per_policy(recorded_lane_sums(b, kind, steps, flags), gid0, lpp, 3)
        assert_fitness(a.policy_fitness(), total, steps)
        assert np.array_equal(a.get_state().view(np.uint32), b.get_state().view(np.uint32))
    if kind == 0 or flags & T:  # (MountainCar from its reset state ends no episode in 47 steps without a time limit)
        assert total[:, 1].all()
    a.close()
    b.close()


# ---- c. the table's lifetime -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1])
def test_table_lifetime(gymrs, kind):
    n, flags, lpp = 3000, A | S | T, 700
    w = make_weights(kind, 0, 3, seed=3)
    eng = small_engine(gymrs, kind, n, flags, w, lpp)
    twin = small_engine(gymrs, kind, n, flags, w, lpp)  # the same steps with rollout_policy_record: says what each launch adds
    zero = np.zeros((3, 4), np.int64)
    bufs = [torch.zeros(n, dtype=torch.uint8, device=DEV) for _ in range(2)]  # one per engine: they run on streams of their own
    torch.cuda.synchronize()

    def both(steps):
        eng.rollout_policy_fitness(steps)
        return per_policy(recorded_lane_sums(twin, kind, steps, flags), 0, lpp, 3)

    first = both(20)
    assert first[:, 1].all()
    assert_fitness(eng.policy_fitness(), first, "first launch")
    eng.rollout_policy_fitness(0)  # K == 0 adds nothing
    assert_fitness(eng.policy_fitness(), first, "K == 0")
    # calls that must not touch the table (the twin takes the same steps, so the next comparison still holds)
    eng.rollout_policy(5)
    twin.rollout_policy(5)
    for e, buf in zip((eng, twin), bufs):
        e.policy_actions(buf.data_ptr())
        e.step(buf.data_ptr())
    eng.stats()
    assert_fitness(eng.policy_fitness(), first, "rollout_policy, policy_actions + step, stats")
    second = both(9)
    assert_fitness(eng.policy_fitness(), first + second, "second launch accumulates")
    assert_fitness(eng.policy_fitness(1, 2), (first + second)[1:3], "a window of records")
    eng.reset(seed=8)
    twin.reset(seed=8)
    assert_fitness(eng.policy_fitness(), first + second, "reset leaves the table alone")
    eng.policy_fitness_clear()
    assert_fitness(eng.policy_fitness(), zero, "clear")
    third = both(11)
    assert_fitness(eng.policy_fitness(), third, "after a clear, in stream order")
    both(4)  # a launch whose adds nobody has waited for: set_policy zeroes behind it, in stream order
    eng.set_policy(w, lanes_per_policy=lpp)  # the same set again: the table is discarded all the same
    assert_fitness(eng.policy_fitness(), zero, "set_policy discards the table")
    w5 = make_weights(kind, 0, 5, seed=4)
    eng.set_policy(w5, lanes_per_policy=lpp)
    twin.set_policy(w5, lanes_per_policy=lpp)
    assert eng.policy_fitness().shape == (5, 4) and eng.policy_fitness_ptr()[1] == 5
    eng.rollout_policy_fitness(6)
    assert_fitness(eng.policy_fitness(), per_policy(recorded_lane_sums(twin, kind, 6, flags), 0, lpp, 5), "a new set of another size")
    same("state", eng.get_state(), twin.get_state(), np.zeros(n, np.int8), "end")
    eng.close()
    twin.close()


# ---- d. population layouts -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("vec", [4, 8])
def test_one_lane_per_policy_with_more_policies_than_lanes(gymrs, kind, vec):
    n, n_pol, gid0, flags, steps = 1300, 2000, 12345, A | S | T, 30
    w = make_weights(kind, 0, n_pol, seed=5)
    eng = small_engine(gymrs, kind, n, flags, w, 1, gid0=gid0, vec=vec)
    twin = small_engine(gymrs, kind, n, flags, w, 1, gid0=gid0)
    if kind == 1:  # (MountainCar from its reset state: every lane is truncated at the same steps and nothing else happens)
        for e in (eng, twin):
            e.set_state(ref.mountain_car_prepare(e.get_state(), 0))
    eng.rollout_policy_fitness(steps)
    lanes = recorded_lane_sums(twin, kind, steps, flags)
    got = eng.policy_fitness()
    pol = fit.policies_of(n, gid0, 1, n_pol)
    assert len(set(pol)) == n  # every lane has a policy of its own
    assert_fitness(got[pol], lanes, "every used policy holds its lane's own sums")
    unused = np.setdiff1d(np.arange(n_pol), pol)
    assert len(unused) == n_pol - n and not got[unused].any()
    # episodes ended, and neighbouring lanes have different sums: a record credited to the lane next door would be noticed
    assert lanes[:, 1].any() and (lanes[1:] != lanes[:-1]).any()
    eng.close()
    twin.close()


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("vec", [4, 8])
@pytest.mark.parametrize("n_pol", [5, 1])
def test_wrapping_and_single_policy_layouts(gymrs, kind, vec, n_pol):
    """lanes_per_policy = 1 with 5 policies on 4200 lanes wraps (every work-item's lanes belong to different policies, every policy owns
    840 scattered lanes); one policy is the uniform path whatever lanes_per_policy says."""
    n, gid0, flags, hidden, schedule = 4200, 12345, A | S | T, 7, (3, 25)
    p = gymrs.engine.default_params(kind)
    p.max_episode_steps = ref.MAX_EPISODE_STEPS
    w = make_weights(kind, hidden, n_pol, seed=6)
    prepare = ref.mountain_car_prepare if kind == 1 else None
    want = ref.reference(kind, n, gid0, p, flags, w, hidden, 1, 5, schedule, prepare)
    records = fit.cumulative(want, n, gid0, 1, n_pol)
    assert records[-1][:, 1].all()
    eng = gymrs.BatchedEngine(kind, n, global_env_offset=gid0, flags=flags, params=p, lanes_per_thread=vec)
    eng.reset(seed=5)
    if prepare is not None:
        eng.set_state(prepare(eng.get_state(), 0))
    eng.set_policy(w, hidden=hidden, lanes_per_policy=1)
    classes = ref.wave_classes(n, vec, gid0, n_pol, 1)
    assert set(classes) == ({0, 2} if n_pol == 1 else {1, 3})
    for k, steps in enumerate(schedule):
        eng.rollout_policy_fitness(steps)
        assert_fitness(eng.policy_fitness(), records[k], k)
        assert_launch(eng, want[k], flags, classes, k)
        assert_stats(eng, want[k], k)
    eng.close()


# ---- e. the zero-copy view -------------------------------------------------------------------------------------------------------
class DeviceColumn:
    """A zero-copy torch view of an engine's device array"""

    def __init__(self, ptr, n, typestr):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (ptr, False), "version": 3}


def test_device_pointer_shows_the_records(gymrs):
    n, lpp, n_pol = 5000, 300, 7
    eng = small_engine(gymrs, 0, n, A | S | T, make_weights(0, 0, n_pol, seed=7), lpp)
    ptr, count = eng.policy_fitness_ptr()  # brings the table into being: zeros
    assert count == n_pol and ptr
    eng.rollout_policy_fitness(33)
    eng.sync()  # the engine's stream is done before torch's reads the memory
    view = torch.as_tensor(DeviceColumn(ptr, n_pol * 4, "<i8"), device=DEV)
    got = view.cpu().numpy().reshape(n_pol, 4)
    torch.cuda.synchronize()  # torch's stream is done before the engine touches the memory again
    host = eng.policy_fitness()
    assert_fitness(got, host, "view against getter")
    assert host[:, 1].all() and host[:, 0].all()
    assert eng.policy_fitness_ptr() == (ptr, n_pol)  # stable until the next set_policy
    eng.policy_fitness_clear()
    eng.sync()
    assert not view.cpu().numpy().any()
    torch.cuda.synchronize()
    eng.close()


# ---- f. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals(gymrs):
    eng = gymrs.BatchedEngine(0, 1000, flags=A)
    eng.reset(seed=1)
    calls = {"rollout_policy_fitness": lambda e: e.rollout_policy_fitness(3), "policy_fitness": lambda e: e.policy_fitness(0, 1),
             "policy_fitness_ptr": lambda e: e.policy_fitness_ptr(), "policy_fitness_clear": lambda e: e.policy_fitness_clear()}
    for name, call in calls.items():  # no policy set
        with pytest.raises(gymrs.GymrsError) as err:
            call(eng)
        assert err.value.status == 1 and "no policy" in str(err.value), name
    w = make_weights(0, 0, 4, seed=8)
    eng.set_policy(w, lanes_per_policy=100)
    for first, count in ((0, 5), (4, 1), (3, 2), (2**32 - 1, 2)):  # first + count > n_policies
        with pytest.raises(gymrs.GymrsError) as err:
            eng.policy_fitness(first, count)
        assert err.value.status == 1 and "n_policies" in str(err.value)
    assert eng.policy_fitness(4, 0).shape == (0, 4) and eng.policy_fitness(3, 1).shape == (1, 4)
    with pytest.raises(gymrs.GymrsError) as err:  # the in-register counters are 32 bits wide: the bound of the header
        eng.rollout_policy_fitness((1 << 24) + 1)
    assert err.value.status == 1 and "GYMRS_POLICY_FITNESS_MAX_STEPS" in str(err.value)
    assert eng.tick()[0] == 1 and not eng.policy_fitness().any()  # a refused call changes nothing
    rows = [gymrs.engine.default_params(0), gymrs.engine.default_params(0)]
    rows[1].gravity *= 1.25
    eng.set_param_table(rows)
    with pytest.raises(gymrs.GymrsError) as err:  # an active parameter table: as gymrs_rollout_policy says it
        eng.rollout_policy_fitness(3)
    assert err.value.status == 1 and "parameter table" in str(err.value) and "gymrs_policy_actions + gymrs_step" in str(err.value)
    eng.set_param_table(None)
    eng.rollout_policy_fitness(3)
    assert eng.policy_fitness()[:, 0].sum() == 3 * 1000  # CartPole with auto-reset pays 1 per lane-step
    eng.close()
    pend = gymrs.BatchedEngine(2, 500, flags=A | T)
    pend.reset(seed=1)
    for name, call in calls.items():
        with pytest.raises(gymrs.GymrsError) as err:
            call(pend)
        assert err.value.status == 1 and "Pendulum" in str(err.value), name
    pend.close()


# ---- g. cutting the batch ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("vec", [4, 8])
def test_three_engines_over_one_batch_add_up_to_one_engine(gymrs, kind, vec):
    n, gid0, lpp, hidden, flags = 9000, 12345, 1000, 8, A | S | T | F
    cuts = [0, 3001, 6202, n]
    assert all(lo % 256 for lo in cuts[1:-1])
    p = gymrs.engine.default_params(kind)
    p.max_episode_steps = ref.MAX_EPISODE_STEPS
    w = make_weights(kind, hidden, 3, seed=2)
    prepare = ref.mountain_car_prepare if kind == 1 else None
    c = SimpleNamespace(kind=kind, n=n, vec=vec, gid0=gid0, params=p, flags=flags, weights=w, hidden=hidden, lanes_per_policy=lpp,
                        reset_seed=4, prepare=prepare)
    one = make_engine(gymrs, c)
    parts = [make_engine(gymrs, c, lo, hi - lo) for lo, hi in zip(cuts, cuts[1:])]
    for steps in (7, 40):
        one.rollout_policy_fitness(steps)
        for e in parts:
            e.rollout_policy_fitness(steps)
        whole = one.policy_fitness()
        assert_fitness(sum(e.policy_fitness() for e in parts), whole, steps)
        same("state", np.concatenate([e.get_state() for e in parts], axis=1), one.get_state(), np.zeros(n, np.int8), steps)
    # after all 47 steps (the time limit is 17; no CartPole episode ends within the first 7): every policy ended episodes, some by truncation
    assert whole[:, 1].all() and whole[:, 3].any()
    for e in parts + [one]:
        e.close()


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("call", ["rollout_policy_fitness", "rollout_policy"])
def test_sharded_batch_equals_one_engine(gymrs, kind, call):
    """The native sharder with 3 blocks on the one GPU: state and fitness bit for bit those of one engine of the same lanes."""
    n, gid0, lpp, hidden, flags = 9000, 12345, 1000, 8, A | S | T | F
    p = gymrs.engine.default_params(kind)
    p.max_episode_steps = ref.MAX_EPISODE_STEPS
    w = make_weights(kind, hidden, 3, seed=2)
    sh = gymrs.ShardedEngine(kind, n, [0, 0, 0], global_env_offset=gid0, params=p, flags=flags)
    one = gymrs.BatchedEngine(kind, n, global_env_offset=gid0, flags=flags, params=p)
    assert len(sh.shards) == 3
    sh.reset(seed=9)
    one.reset(seed=9)
    sh.set_policy(w, hidden=hidden, lanes_per_policy=lpp)
    one.set_policy(w, hidden=hidden, lanes_per_policy=lpp)
    for steps in (7, 40):
        getattr(sh, call)(steps)
        getattr(one, call)(steps)
        sh.sync()
        one.sync()
        same("state", sh.get_state(), one.get_state(), np.zeros(n, np.int8), steps)
        for x, y in zip(sh.get_step_result(), one.get_step_result()):
            assert np.array_equal(x, y)
        same("final_obs", sh.get_final_obs(), one.get_final_obs(), np.zeros(n, np.int8), steps)
        got, want = sh.stats(), one.stats()
        assert np.array_equal(got, want), (got, want)
        whole = one.policy_fitness()
        assert_fitness(sh.policy_fitness(), whole, steps)
        assert_fitness(sh.policy_fitness(1, 2), whole[1:3], "a window")
        if call == "rollout_policy":
            assert not whole.any()  # rollout_policy adds nothing, sharded or not
        else:
            assert_fitness(sum(s.policy_fitness() for s in sh.shards), whole, "the blocks' own records")
    if call == "rollout_policy_fitness":  # after all 47 steps (time limit 17): every policy ended episodes, some by truncation
        assert whole[:, 1].all() and whole[:, 3].any()
    sh.policy_fitness_clear()
    assert not sh.policy_fitness().any()
    assert sh.policy_fitness(3).shape == (0, 4) and sh.policy_fitness(1, 0).shape == (0, 4)  # count == 0, as on one engine
    with pytest.raises(gymrs.GymrsError) as err:
        sh.policy_fitness(2, 2)
    assert err.value.status == 1
    sh.set_policy(None)
    with pytest.raises(gymrs.GymrsError) as err:
        sh.rollout_policy_fitness(1)
    assert err.value.status == 1 and "no policy" in str(err.value)
    sh.close()
    one.close()


# ---- speed -------------------------------------------------------------------------------------------------------------------------
def median_rate(run, lane_steps, reps=9, floor_s=0.1):
    """env-steps/s: median of `reps` repetitions of at least `floor_s` seconds each (host clock around work that ends in a synchronise)"""
    calls = 1
    while True:  # size one repetition
        t0 = time.perf_counter()
        run(calls)
        dt = time.perf_counter() - t0
        if dt >= floor_s:
            break
        calls = max(calls * 2, int(calls * floor_s / max(dt, 1e-6)) + 1)
    rates = []
    for _ in range(reps):
        t0 = time.perf_counter()
        run(calls)
        dt = time.perf_counter() - t0
        assert dt >= 0.8 * floor_s
        rates.append(calls * lane_steps / dt)
    return float(np.median(rates))


@pytest.mark.perf
def test_fitness_in_the_kernel_is_no_slower_than_record_and_sum(gymrs):
    """CartPole, 2^20 lanes, flags A, 1024 affine policies x 1024 lanes, seeded normal weights.  One rollout_policy_fitness(K = 256) per
    call against what it replaces: rollout_policy_record in chunks of 32 with a sync and the torch per-policy sum of the `done` rows
    after each chunk, for the same 256 steps.  rate(fitness) >= rate(record and sum); no margin."""
    n_pol, lanes, k, chunk = 1024, 1024, 256, 32
    n = n_pol * lanes
    w = make_weights(0, 0, n_pol, seed=1)
    fused = gymrs.BatchedEngine(0, n, flags=A)
    rec = gymrs.BatchedEngine(0, n, flags=A)
    for e in (fused, rec):
        e.reset(seed=0)
        e.set_policy(w, lanes_per_policy=lanes)
    stride = (n + 15) // 16 * 16
    obs = torch.empty((chunk, 4, stride), dtype=torch.float32, device=DEV)
    act = torch.empty((chunk, stride), dtype=torch.uint8, device=DEV)
    rew = torch.empty((chunk, stride), dtype=torch.float32, device=DEV)
    done = torch.empty((chunk, stride), dtype=torch.uint8, device=DEV)
    finished = torch.zeros(n_pol, dtype=torch.int64, device=DEV)
    torch.cuda.synchronize()

    def run_fused(calls):
        for _ in range(calls):
            fused.rollout_policy_fitness(k)
        fused.sync()

    def run_record(calls, wait_for_torch=False):
        """The loop of the example this call replaces, as it was written: the engine's next launch does not wait for torch's sum of the
        rows it is about to overwrite, so the loop is timed as it ran but its sums are only right with `wait_for_torch`."""
        for _ in range(calls):
            for _ in range(k // chunk):
                rec.rollout_policy_record(chunk, obs=obs.data_ptr(), actions=act.data_ptr(), reward=rew.data_ptr(), done=done.data_ptr(),
                                          lane_stride=stride)
                rec.sync()  # the rows were written on the engine's stream
                finished.add_(done[:chunk, :n].view(chunk, n_pol, lanes).sum(dim=(0, 2), dtype=torch.int64))
                if wait_for_torch:
                    torch.cuda.synchronize()  # torch has read the rows before the engine writes them again
        torch.cuda.synchronize()

    run_fused(1)
    run_record(1, wait_for_torch=True)
    # the two count the same thing: the same engines from the same reset took the same 256 steps
    assert np.array_equal(fused.policy_fitness()[:, 2], finished.cpu().numpy()) and finished.sum().item() > 0
    r_record = median_rate(run_record, n * k)
    r_fused = median_rate(run_fused, n * k)
    print(f"\nrollout_policy_fitness(K={k}): {r_fused:.4g} env-steps/s; rollout_policy_record in chunks of {chunk} + sync + torch sum: "
          f"{r_record:.4g} env-steps/s; ratio {r_fused / r_record:.3f}")
    assert r_fused >= r_record
    fused.close()
    rec.close()
