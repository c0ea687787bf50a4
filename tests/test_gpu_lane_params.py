"""Per-lane parameter tables on the GPU (gymrs_set_param_table): lane i steps with row index[i].

Lane i of a table engine must give, bit for bit, what lane i of an engine created with params = row[index[i]] gives (same size,
flags, seed and actions).  A one-row table holding the engine's own params must be invisible on every stepping path; large
tables are checked against the CPU f32 twin block by block and against the f64 oracle row by row."""
import ctypes as C
import json
import os
import struct

import numpy as np
import pytest
import torch

from oracle.bindings import Oracle, TwinEngine
from oracle import bindings as orc_bindings

pytestmark = pytest.mark.gpu

A, S, T, F = 1, 2, 4, 8
ALL_FLAGS = [0, A, A | S, T, A | T, A | S | T, A | F, A | S | F, A | T | F, A | S | T | F]
EINVAL = 1


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def params(gymrs, kind, max_steps=9):
    p = gymrs.engine.default_params(kind)
    p.max_episode_steps = max_steps
    return p


def perturbed(gymrs, kind, k, rng, max_steps=9):
    """k rows: the physics fields scaled by up to +-50 % (MountainCar: force, gravity, max_speed, goal)"""
    rows = []
    for _ in range(k):
        p = params(gymrs, kind, max_steps)
        names = (("gravity", "masscart", "masspole", "length", "force_mag", "tau", "theta_threshold_radians", "x_threshold") if kind == 0
                 else ("force", "gravity", "max_speed", "goal_position"))
        for f in names:
            setattr(p, f, getattr(p, f) * float(rng.uniform(0.5, 1.5)))
        rows.append(p)
    return rows


def same_outputs(a, b, flags):
    assert np.array_equal(bits(a.get_state()), bits(b.get_state()))
    for x, y in zip(a.get_step_result(), b.get_step_result()):
        assert np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8))
    if (flags & F) and (flags & A):
        assert np.array_equal(bits(a.get_final_obs()), bits(b.get_final_obs()))


class DeviceColumn:
    """A zero-copy torch view of an engine's device array"""

    def __init__(self, ptr, n, typestr):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (ptr, False), "version": 3}


def actions_ring(kind, n, nbuf, seed):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 2 if kind == 0 else 3, (nbuf, n)).astype(np.uint8)
    t = torch.from_numpy(a).to("cuda:0")
    torch.cuda.synchronize()
    return t


def run_paths(eng, kind, n, flags, ring):
    """step, step_host, step_many (eager and graph), rollout, rollout_record: the same calls on every engine"""
    eng.reset(seed=5)
    for t in range(3):
        eng.step(ring[t].data_ptr())
    eng.step_host(ring[3].cpu().numpy())
    eng.step_many(ring.data_ptr(), n, ring.shape[0], 8)
    eng.step_many(ring.data_ptr(), n, ring.shape[0], 8, use_graph=True)
    eng.step_many(ring.data_ptr(), n, ring.shape[0], 8, use_graph=True)
    eng.rollout(5, action_seed=3, action_t0=0)
    eng.sync()


@pytest.mark.parametrize("kind", [0, 1])
def test_one_row_table_is_invisible(gymrs, kind):
    for n in (10_000, 1 << 20):
        ring = actions_ring(kind, n, 4, 1)
        for vec in (4, 8):
            for flags in ALL_FLAGS:
                p = params(gymrs, kind)
                plain = gymrs.BatchedEngine(kind, n, flags=flags, params=p)
                tab = gymrs.BatchedEngine(kind, n, flags=flags, params=p)
                tab.set_param_table([p])
                for e in (plain, tab):
                    e.set_tuning(vec)
                    run_paths(e, kind, n, flags, ring)
                same_outputs(tab, plain, flags)
                assert np.array_equal(tab.stats(), plain.stats()), (n, vec, flags)
                assert json.loads(tab.env_json(0))["gymrs"]["last_launch"].startswith("HIP launch: gymrs::step_kernel<TableT<")
                plain.close()
                tab.close()
    # rollout_record (4 lanes per work-item)
    n, flags, steps = 10_000, A | S | T, 6
    bufs = {k: torch.zeros(v, dtype=d, device="cuda:0") for k, v, d in
            (("obs", steps * (4 if kind == 0 else 2) * 10_016, torch.float32), ("actions", steps * 10_016, torch.uint8),
             ("reward", steps * 10_016, torch.float32), ("done", steps * 10_016, torch.uint8), ("truncated", steps * 10_016, torch.uint8))}
    out = []
    for table in (False, True):
        e = gymrs.BatchedEngine(kind, n, flags=flags, params=params(gymrs, kind))
        if table:
            e.set_param_table([params(gymrs, kind)])
        e.reset(seed=9)
        for b in bufs.values():
            b.zero_()
        torch.cuda.synchronize()
        e.rollout_record(steps, 4, 0, lane_stride=10_016, **{k: b.data_ptr() for k, b in bufs.items()})
        e.sync()
        out.append([b.cpu().numpy().copy() for b in bufs.values()] + [e.get_state(), e.stats()])
        e.close()
    for x, y in zip(*out):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("kind", [0, 1])
def test_scattered_indices_match_uniform_engines(gymrs, kind):
    n, k, steps, flags = 1 << 20, 3, 180, A | S | T  # (the last step truncates the lanes that lived 60 steps)
    rng = np.random.default_rng(11 + kind)
    rows = perturbed(gymrs, kind, k, rng, max_steps=60)
    index = rng.integers(0, k, n).astype(np.uint16)
    tab = gymrs.BatchedEngine(kind, n, flags=flags, params=rows[0])
    tab.set_param_table(rows)
    tab.set_param_index(index)
    assert np.array_equal(tab.get_param_index(), index)
    uni = [gymrs.BatchedEngine(kind, n, flags=flags, params=r) for r in rows]
    engines = [tab] + uni
    acts = [torch.empty(n, dtype=torch.uint8, device="cuda:0") for _ in engines]  # one buffer per engine (stream)
    for e in engines:
        e.reset(seed=21)
    for t in range(steps):
        for e, act in zip(engines, acts):  # the action stream is keyed by global lane ids: the same actions for every engine
            e.fill_actions(act.data_ptr(), seed=2, t=t)
            e.step(act.data_ptr())
    st, res = tab.get_state(), tab.get_step_result()
    for r, u in enumerate(uni):
        m = index == r
        assert np.array_equal(bits(st)[:, m], bits(u.get_state())[:, m]), r
        for x, y in zip(res, u.get_step_result()):
            assert np.array_equal(x[m], y[m]), r
    assert res[2].any() and (kind == 1 or res[1].any())  # episodes did end, by the limit (and CartPole's by termination)
    for e in engines:
        e.close()


@pytest.mark.parametrize("k", [256, 257, 4096])
def test_large_tables_match_the_twin_block_by_block(gymrs, twin, k):
    kind, flags, block, steps = 0, A | S | T, 40, 25
    rng = np.random.default_rng(k)
    rows = perturbed(gymrs, kind, k, rng, max_steps=12)
    n = k * block
    eng = gymrs.BatchedEngine(kind, n, flags=flags, params=rows[0])
    eng.set_param_table(rows)
    eng.set_param_index(np.repeat(np.arange(k, dtype=np.uint16), block))
    tws = [TwinEngine(twin, kind, block, rows[r], flags=flags, gid0=r * block) for r in range(k)]
    eng.reset(seed=4)
    for tw in tws:
        tw.reset(4)
    act = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    for t in range(steps):
        eng.fill_actions(act.data_ptr(), seed=6, t=t)
        eng.step(act.data_ptr())
        for tw in tws:
            tw.step(tw.fill_actions(6, t))
    eng.sync()
    want_state = np.concatenate([tw.get_state() for tw in tws], axis=1)
    want_done = np.concatenate([tw.get_result()[1] for tw in tws])
    assert np.array_equal(bits(eng.get_state()), bits(want_state))
    assert np.array_equal(eng.get_step_result()[1], want_done)
    assert np.array_equal(eng.stats(), np.sum([tw.stats() for tw in tws], axis=0))
    eng.close()


def test_full_table_one_step_against_the_f64_oracle(gymrs):
    kind, k, per = 0, 65536, 4
    n = k * per
    rng = np.random.default_rng(65536)
    rows = perturbed(gymrs, kind, k, rng)
    eng = gymrs.BatchedEngine(kind, n, params=rows[0])
    eng.set_param_table(rows)
    index = np.tile(np.arange(k, dtype=np.uint16), per)
    eng.set_param_index(index)
    eng.reset(seed=8)
    st0 = eng.get_state().astype(np.float64)
    act = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    eng.fill_actions(act.data_ptr(), seed=1, t=0)
    eng.step(act.data_ptr())
    eng.sync()
    a = act.cpu().numpy()
    got, done = eng.get_state().astype(np.float64), eng.get_step_result()[1]
    orc = Oracle()
    P = orc_bindings.CartPoleParams
    lanes = np.arange(n).reshape(per, k).T  # row r: lanes r, r + k, ...
    for r in range(k):
        ln = lanes[r]
        p = P(**{f: getattr(rows[r], f) for f, _ in P._fields_})
        ref = np.ascontiguousarray(st0[:, ln])
        _, d, bad = orc.cartpole_step_batch(ref, np.zeros(per, np.uint8), a[ln], params=p)
        assert bad == 0 and np.array_equal(d, done[ln]), r
        err = np.abs(got[:, ln] - ref) / np.maximum(np.abs(ref), 1.0)
        assert err.max() <= 1e-6, (r, err.max())
    eng.close()


def test_changing_index_and_table_between_steps(gymrs):
    kind, n, flags = 0, 100_000, A | S
    rng = np.random.default_rng(3)
    rows = perturbed(gymrs, kind, 2, rng)
    eng = gymrs.BatchedEngine(kind, n, flags=flags, params=rows[0])
    ref = [gymrs.BatchedEngine(kind, n, flags=flags, params=r) for r in rows]
    eng.set_param_table(rows)
    acts = {}
    for e in [eng] + ref:
        e.reset(seed=1)

    def step_all(t, engines):
        for e in engines:  # one action buffer per engine: each fills and reads it on its own stream
            act = acts.setdefault(id(e), torch.empty(n, dtype=torch.uint8, device="cuda:0"))
            e.fill_actions(act.data_ptr(), seed=9, t=t)
            e.step(act.data_ptr())
    step_all(0, [eng] + ref)
    # a torch write on the engine's stream: every lane to row 1, effective for the next step
    view = torch.as_tensor(DeviceColumn(eng.param_index_ptr(), n, "<i2"), device="cuda:0")
    with torch.cuda.stream(torch.cuda.ExternalStream(eng.stream, device="cuda:0")):
        view.fill_(1)
    ref[1].set_state(ref[0].get_state())  # the reference for row 1 continues from the same state
    step_all(1, [eng, ref[1]])
    eng.sync()
    assert np.array_equal(eng.get_param_index(), np.ones(n, np.uint16))
    assert np.array_equal(bits(eng.get_state()), bits(ref[1].get_state()))
    # a table change leaves state, tick and statistics alone
    st, tick, stats = eng.get_state(), eng.tick(), eng.stats()
    eng.set_param_table(list(reversed(rows)))
    assert np.array_equal(bits(eng.get_state()), bits(st)) and eng.tick() == tick and np.array_equal(eng.stats(), stats)
    assert [bytes(r) for r in eng.param_table()] == [bytes(r) for r in reversed(rows)]
    assert bytes(eng.get_params()) == bytes(rows[1])  # row 0 of the table
    # back to the uniform kernels: set_params, and set_param_table(None)
    for off in ("set_params", "none"):
        a_ = gymrs.BatchedEngine(kind, n, flags=flags, params=rows[0])
        b_ = gymrs.BatchedEngine(kind, n, flags=flags, params=rows[0])
        a_.set_param_table(rows[::-1])
        if off == "set_params":
            a_.set_params(rows[0])
        else:
            a_.set_param_table([rows[0]] + rows[1:])
            a_.set_param_table(None)
        assert a_.param_table() == []
        with pytest.raises(gymrs.GymrsError):
            a_.param_index_ptr()
        for e in (a_, b_):
            e.reset(seed=2)
        step_all(0, [a_, b_])
        a_.sync()
        assert np.array_equal(bits(a_.get_state()), bits(b_.get_state()))
        assert "TableT" not in json.loads(a_.env_json(0))["gymrs"]["last_launch"]
        a_.close()
        b_.close()
    for e in [eng] + ref:
        e.close()


def test_out_of_range_index_is_reported_and_not_stepped(gymrs):
    kind, n = 0, 50_000
    p = params(gymrs, kind)
    eng = gymrs.BatchedEngine(kind, n, params=p)
    ref = gymrs.BatchedEngine(kind, n, params=p)
    eng.set_param_table([p, p])
    idx = np.zeros(n, np.uint16)
    idx[[777, 4321]] = [2, 65535]
    eng.set_param_index(idx)
    for e in (eng, ref):
        e.reset(seed=3)
    before = eng.get_state()
    act = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    eng.fill_actions(act.data_ptr(), seed=1, t=0)
    torch.cuda.synchronize()  # (filled on the engine's stream, read on both)
    eng.step(act.data_ptr())
    ref.step(act.data_ptr())
    with pytest.raises(gymrs.InvalidActionError) as ei:
        eng.sync()
    assert "lane 777" in str(ei.value) and "parameter index" in str(ei.value)
    ref.sync()
    st = eng.get_state()
    assert np.array_equal(bits(st)[:, [777, 4321]], bits(before)[:, [777, 4321]])
    ok = np.ones(n, bool)
    ok[[777, 4321]] = False
    assert np.array_equal(bits(st)[:, ok], bits(ref.get_state())[:, ok])
    with pytest.raises(gymrs.GymrsError):
        eng.lane_params(777)
    eng.sync()  # the report was consumed
    eng.close()
    ref.close()


def test_validation(gymrs):
    lib = gymrs.load_library()
    k = C.c_uint32()
    with gymrs.BatchedEngine(0, 64) as eng:
        p0, p1 = params(gymrs, 0), params(gymrs, 0)
        p1.kinematics_integrator = 1
        with pytest.raises(gymrs.GymrsError, match="row 1: kinematics_integrator"):
            eng.set_param_table([p0, p1])
        p1 = params(gymrs, 0, max_steps=10)
        with pytest.raises(gymrs.GymrsError, match="row 1: max_episode_steps"):
            eng.set_param_table([p0, p1])
        p2 = params(gymrs, 0)
        p2.kinematics_integrator = 5
        with pytest.raises(gymrs.GymrsError, match="row 2"):
            eng.set_param_table([p0, p0, p2])
        arr = (type(p0) * 1)(p0)
        assert lib.gymrs_set_param_table(eng._h, arr, 0) == EINVAL
        big = (type(p0) * 65537)(*([p0] * 65537))
        assert lib.gymrs_set_param_table(eng._h, big, 65537) == EINVAL
        assert "65536" in lib.gymrs_last_error().decode()
        assert lib.gymrs_get_param_table(eng._h, None, 0, C.byref(k)) == 0 and k.value == 0
        eng.set_param_table([p0] * 65536)  # the largest table
        assert lib.gymrs_get_param_table(eng._h, None, 0, C.byref(k)) == 0 and k.value == 65536
    with gymrs.BatchedEngine(2, 64) as pend:
        with pytest.raises(gymrs.GymrsError, match="Pendulum"):
            pend.set_param_table([params(gymrs, 2)])


class _Aql:
    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.before = os.environ.get("GYMRS_AQL")
        os.environ["GYMRS_AQL"] = self.value

    def __exit__(self, *exc):
        if self.before is None:
            os.environ.pop("GYMRS_AQL", None)
        else:
            os.environ["GYMRS_AQL"] = self.before


@pytest.mark.parametrize("kind", [0, 1])
def test_clone_snapshot_json_aql_and_shards(gymrs, kind):
    n, flags = 30_001, A | S | T
    rng = np.random.default_rng(40 + kind)
    rows = perturbed(gymrs, kind, 5, rng)
    index = rng.integers(0, 5, n).astype(np.uint16)
    eng = gymrs.BatchedEngine(kind, n, flags=flags, params=rows[0])
    eng.set_param_table(rows)
    eng.set_param_index(index)
    eng.reset(seed=12)
    act = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    def run(e, t0, k):
        for t in range(t0, t0 + k):
            e.fill_actions(act.data_ptr(), seed=7, t=t)
            e.step(act.data_ptr())
        e.sync()
    run(eng, 0, 10)
    blob = eng.snapshot()
    assert struct.unpack_from("<I", blob, 8)[0] == 5
    cl = eng.clone()
    assert np.array_equal(cl.get_param_index(), index)
    other = gymrs.BatchedEngine(kind, n, flags=flags, params=rows[0])
    other.restore(blob)
    for e in (eng, cl, other):
        run(e, 10, 50)
    for e in (cl, other):
        assert np.array_equal(bits(e.get_state()), bits(eng.get_state()))
        assert np.array_equal(e.stats(), eng.stats())
    with gymrs.BatchedEngine(kind, 1000, flags=flags) as plain:
        assert struct.unpack_from("<I", plain.snapshot(), 8)[0] == 4  # no table: v4 as before
    # the serde view prints the lane's own row
    for lane in (0, 17, n - 1):
        j = json.loads(eng.env_json(lane))
        assert j["gymrs"]["param_set"] == index[lane]
        p, _ = gymrs.engine.params_from_json(kind, eng.env_json(lane))
        want = eng.lane_params(lane)
        assert bytes(want) == bytes(rows[index[lane]])
        names = [f for f, _ in type(p)._fields_ if f != "max_episode_steps"]
        assert all(getattr(p, f) == getattr(want, f) for f in names)
    # GYMRS_AQL=1: HIP launches, the same bits
    ring = actions_ring(kind, n, 2, 5)
    a2 = eng.clone()
    with _Aql("1"):
        eng.step_many(ring.data_ptr(), n, 2, 16)
        eng.sync()
    with _Aql("0"):
        a2.step_many(ring.data_ptr(), n, 2, 16)
        a2.sync()
    g = json.loads(eng.env_json(0))["gymrs"]
    assert g["aql_launches"] == 0 and "parameter table" in g["aql"] and "TableT" in g["last_launch"]
    assert np.array_equal(bits(eng.get_state()), bits(a2.get_state()))
    for e in (eng, cl, other, a2):
        e.close()
    # native sharder: per-shard tables give the same bits as one engine
    for blocks in (2, 3):
        sh = gymrs.ShardedEngine(kind, n, [0] * blocks, flags=flags, params=rows[0])
        one = gymrs.BatchedEngine(kind, n, flags=flags, params=rows[0])
        one.set_param_table(rows)
        one.set_param_index(index)
        for s in sh.shards:
            s.set_param_table(rows)
            s.set_param_index(index[s.first_lane:s.first_lane + s.n_envs])
        sh.reset(seed=3)
        one.reset(seed=3)
        for t in range(12):
            a = torch.from_numpy(ring[t % 2].cpu().numpy()).to("cuda:0")
            torch.cuda.synchronize()
            sh.step([a.data_ptr() + s.first_lane for s in sh.shards])
            one.step(a.data_ptr())
        sh.sync()
        one.sync()
        assert np.array_equal(bits(sh.get_state()), bits(one.get_state()))
        assert np.array_equal(sh.stats(), one.stats())
        sh.close()
        one.close()
