"""GYMRS_FINAL_OBS on the GPU: the observation each lane's most recently finished episode ended in.

Expected values come from the CPU f32 twin with flags = 0 (no auto-reset), stepped from the engine's pre-step state with the
same actions: its observation after the step is what a re-armed lane would have shown.  Rows of lanes that finished must
equal it bit for bit; every other row must be what it was before the step.  Everything else an engine with the flag computes
(state, observations, reward, done, truncated, statistics) must be bit-identical to an engine with the same flags without it."""
import json
import os

import numpy as np
import pytest
import torch

from oracle.bindings import TwinEngine

pytestmark = pytest.mark.gpu

A, S, T, F = 1, 2, 4, 8
FLAG_SETS = [A | F, A | S | F, A | T | F, A | S | T | F]


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def host_actions(kind, n, rng):
    if kind == 2:
        return rng.uniform(-2.0, 2.0, n).astype(np.float32)
    return rng.integers(0, 2 if kind == 0 else 3, n).astype(np.uint8)


def to_device(a):
    t = torch.from_numpy(a).to("cuda:0")
    torch.cuda.synchronize()  # (torch's copy runs on torch's stream, the engine reads on its own)
    return t


def params(gymrs, kind, max_steps=7):
    p = gymrs.engine.default_params(kind)
    if max_steps is not None:
        p.max_episode_steps = max_steps
    return p


def assert_same_outputs(eng, ref):
    """Everything but the final observations: the flag changes nothing else."""
    assert np.array_equal(bits(eng.get_state()), bits(ref.get_state()))
    assert np.array_equal(bits(eng.get_obs()), bits(ref.get_obs()))
    for x, y in zip(eng.get_step_result(), ref.get_step_result()):
        assert np.array_equal(x, y)
    assert np.array_equal(eng.stats(), ref.stats())


def checked_step(eng, tw0, kind, a_host, prev_final, step=None):
    """One step of `eng` (by `step(device_actions)`, default eng.step) checked against the flags = 0 twin.  Returns the new final rows
    and the number of lanes that finished."""
    tw0.set_state(eng.get_state())
    tw0.step(a_host)
    want = tw0.get_obs()
    a_dev = to_device(a_host)
    (step or eng.step)(a_dev.data_ptr())
    eng.sync()
    _, done, trunc = eng.get_step_result()
    finished = (done | trunc) != 0
    expected = prev_final.copy()
    expected[:, finished] = want[:, finished]
    got = eng.get_final_obs()
    assert np.array_equal(bits(got), bits(expected)), f"{int(np.sum(np.any(bits(got) != bits(expected), axis=0)))} lanes differ"
    return got, int(finished.sum())


@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("flags", FLAG_SETS)
@pytest.mark.parametrize("n", [1000, 65613, 1 << 20])
@pytest.mark.parametrize("vec", [4, 8])
def test_final_obs_against_twin(gymrs, twin, kind, flags, n, vec):
    p = params(gymrs, kind)
    eng = gymrs.BatchedEngine(kind, n, flags=flags, params=p, lanes_per_thread=vec, global_env_offset=77)
    ref = gymrs.BatchedEngine(kind, n, flags=flags & ~F, params=p, lanes_per_thread=vec, global_env_offset=77)
    tw0 = TwinEngine(twin, kind, n, p, flags=0)
    eng.reset(seed=5)
    ref.reset(seed=5)
    final = eng.get_final_obs()
    assert final.shape == (eng.obs_dim, n) and not final.any()  # reset zeroes every row
    rng = np.random.default_rng(kind * 100 + flags + vec)
    n_finished = 0
    for t in range(16):
        a = host_actions(kind, n, rng)
        final, k = checked_step(eng, tw0, kind, a, final)
        ref.step_host(a)
        assert_same_outputs(eng, ref)
        n_finished += k
    if (flags & T) or kind == 0:  # MountainCar / Pendulum without a time limit rarely / never finish: their rows stay 0
        assert n_finished > 0
    eng.close()
    ref.close()


@pytest.mark.parametrize("kind", [0, 2])
def test_step_host_path(gymrs, twin, kind):
    n, flags = 3000, A | S | T | F
    p = params(gymrs, kind)
    eng = gymrs.BatchedEngine(kind, n, flags=flags, params=p)
    tw0 = TwinEngine(twin, kind, n, p, flags=0)
    eng.reset(seed=9)
    final = eng.get_final_obs()
    rng = np.random.default_rng(3)
    for _ in range(10):
        a = host_actions(kind, n, rng)
        tw0.set_state(eng.get_state())
        tw0.step(a)
        want = tw0.get_obs()
        eng.step_host(a)
        _, d, tr = eng.get_step_result()
        fin = (d | tr) != 0
        final[:, fin] = want[:, fin]
        assert np.array_equal(bits(eng.get_final_obs()), bits(final))


@pytest.mark.parametrize("flags", [A | S | F, A | S | T | F])
def test_small_engine_host_pool(gymrs, twin, flags):
    """<= 64 lanes live in mapped host memory: the same rows through that path."""
    n = 40
    p = params(gymrs, 0, 5)
    eng = gymrs.BatchedEngine(0, n, flags=flags, params=p)
    tw0 = TwinEngine(twin, 0, n, p, flags=0)
    eng.reset(seed=2)
    final = eng.get_final_obs()
    rng = np.random.default_rng(4)
    for _ in range(20):
        final, _ = checked_step(eng, tw0, 0, host_actions(0, n, rng), final)


@pytest.mark.parametrize("kind", [0, 1])
def test_invalid_actions_are_not_written(gymrs, twin, kind):
    n, flags = 4000, A | T | F
    p = params(gymrs, kind, 3)
    eng = gymrs.BatchedEngine(kind, n, flags=flags, params=p)
    ref = gymrs.BatchedEngine(kind, n, flags=flags & ~F, params=p)
    eng.reset(seed=1)
    ref.reset(seed=1)
    rng = np.random.default_rng(8)
    for _ in range(3):  # every lane's episode reaches the time limit of 3: every row is written once
        a = to_device(host_actions(kind, n, rng))
        eng.step(a.data_ptr())
        ref.step(a.data_ptr())
    before = eng.get_final_obs()
    assert np.all(np.any(before != 0, axis=0))
    bad = np.zeros(n, bool)
    bad[::7] = True
    for _ in range(3):  # the rejected lanes are never stepped: their time limit is reached, but they are not re-armed
        a_host = host_actions(kind, n, rng)
        a_host[bad] = 9
        a = to_device(a_host)
        eng.step(a.data_ptr())
        ref.step(a.data_ptr())
        with pytest.raises(gymrs.InvalidActionError):
            eng.sync()
        with pytest.raises(gymrs.InvalidActionError):
            ref.sync()
        after = eng.get_final_obs()
        assert np.array_equal(bits(after[:, bad]), bits(before[:, bad]))
        assert_same_outputs(eng, ref)
    assert not np.array_equal(bits(after[:, ~bad]), bits(before[:, ~bad]))


@pytest.mark.parametrize("flags", [A | F, A | S | T | F])
def test_cartpole_2p22_reward_elision(gymrs, twin, flags):
    n = 1 << 22  # the reward store is elided from this size on
    p = params(gymrs, 0)
    eng = gymrs.BatchedEngine(0, n, flags=flags, params=p)
    ref = gymrs.BatchedEngine(0, n, flags=flags & ~F, params=p)
    tw0 = TwinEngine(twin, 0, n, p, flags=0)
    assert json.loads(eng.env_json(0))["gymrs"]["reward_store_elided"] == 1
    eng.reset(seed=4)
    ref.reset(seed=4)
    final = eng.get_final_obs()
    rng = np.random.default_rng(11)
    for _ in range(9):
        a = host_actions(0, n, rng)
        final, _ = checked_step(eng, tw0, 0, a, final)
        ref.step_host(a)
        assert_same_outputs(eng, ref)


def test_cartpole_all_flags_limit_elision(gymrs, twin):
    """CartPole with all three flags elides the time limit while no lane can reach it: those launches are the reset-logged kernel (A|S|F)."""
    n, flags = 1 << 20, A | S | T | F
    p = params(gymrs, 0, None)  # 500 steps: every launch of this test runs without the limit
    eng = gymrs.BatchedEngine(0, n, flags=flags, params=p)
    ref = gymrs.BatchedEngine(0, n, flags=flags & ~F, params=p)
    tw0 = TwinEngine(twin, 0, n, p, flags=0)
    eng.reset(seed=6)
    ref.reset(seed=6)
    final = eng.get_final_obs()
    rng = np.random.default_rng(12)
    for _ in range(20):
        a = host_actions(0, n, rng)
        final, _ = checked_step(eng, tw0, 0, a, final)
        ref.step_host(a)
        assert_same_outputs(eng, ref)
    assert json.loads(eng.env_json(0))["gymrs"]["time_limit_elided_launches"] > 0


def ring_of(kind, n, nbuf, seed):
    rng = np.random.default_rng(seed)
    return to_device(np.stack([host_actions(kind, n, rng) for _ in range(nbuf)]))


class _Aql:
    """GYMRS_AQL for the calls inside the block (the library looks it up per gymrs_step_many call)."""

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


# (use_graph is refused for Pendulum with GYMRS_TIME_LIMIT, with or without the flag: that combination is not listed)
@pytest.mark.parametrize("kind,flags,mode", [(k, f, m) for k, f in [(0, A | S | F), (0, A | S | T | F), (1, A | T | F), (2, A | S | T | F), (2, A | F)]
                                             for m in ("eager", "graph", "aql") if not (m == "graph" and k == 2 and f & T)])
def test_step_many_equals_step_loop(gymrs, kind, flags, mode):
    n, nbuf, steps = 70001, 4, 40
    p = params(gymrs, kind)
    many = gymrs.BatchedEngine(kind, n, flags=flags, params=p)
    loop = gymrs.BatchedEngine(kind, n, flags=flags, params=p)
    many.reset(seed=21)
    loop.reset(seed=21)
    ring = ring_of(kind, n, nbuf, 31)
    stride = ring.stride(0) * ring.element_size()
    if mode == "aql":
        with _Aql("1"):
            many.step_many(ring.data_ptr(), stride, nbuf, steps)
    else:
        many.step_many(ring.data_ptr(), stride, nbuf, steps, use_graph=(mode == "graph"))
    for t in range(steps):
        loop.step(ring[t % nbuf].data_ptr())
    many.sync()
    loop.sync()
    assert np.array_equal(bits(many.get_final_obs()), bits(loop.get_final_obs()))
    if flags & T or kind == 0:  # (Pendulum without a time limit never finishes an episode: its rows stay 0)
        assert many.get_final_obs().any()
    assert_same_outputs(many, loop)


@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("flags", [A | S | T | F, A | T | F])
@pytest.mark.parametrize("record", [False, True])
def test_rollout_equals_fill_actions_plus_step(gymrs, kind, flags, record):
    n, steps = 5003, 23
    p = params(gymrs, kind)
    roll = gymrs.BatchedEngine(kind, n, flags=flags, params=p, global_env_offset=9)
    loop = gymrs.BatchedEngine(kind, n, flags=flags, params=p, global_env_offset=9)
    roll.reset(seed=8)
    loop.reset(seed=8)
    buf = torch.empty(n, dtype=torch.float32 if kind == 2 else torch.uint8, device="cuda:0")
    if record:
        stride = (n + 15) // 16 * 16
        obs = torch.empty((steps, roll.obs_dim, stride), dtype=torch.float32, device="cuda:0")
        act = torch.empty((steps, stride), dtype=buf.dtype, device="cuda:0")
        rew = torch.empty((steps, stride), dtype=torch.float32, device="cuda:0")
        dn = torch.empty((steps, stride), dtype=torch.uint8, device="cuda:0")
        tr = torch.empty((steps, stride), dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        roll.rollout_record(steps, 6, 100, obs=obs.data_ptr(), actions=act.data_ptr(), reward=rew.data_ptr(), done=dn.data_ptr(),
                            truncated=tr.data_ptr())
    else:
        roll.rollout(steps, action_seed=6, action_t0=100)
    for k in range(steps):
        loop.fill_actions(buf.data_ptr(), 6, 100 + k)
        loop.step(buf.data_ptr())
    roll.sync()
    loop.sync()
    assert np.array_equal(bits(roll.get_final_obs()), bits(loop.get_final_obs()))
    assert roll.get_final_obs().any()
    assert np.array_equal(bits(roll.get_state()), bits(loop.get_state()))
    assert roll.tick() == loop.tick()


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_clone_and_snapshot_carry_the_rows(gymrs, kind):
    n, flags = 9000, A | S | T | F
    p = params(gymrs, kind)
    eng = gymrs.BatchedEngine(kind, n, flags=flags, params=p)
    plain = gymrs.BatchedEngine(kind, n, flags=flags & ~F, params=p)
    eng.reset(seed=13)
    plain.reset(seed=13)
    rng = np.random.default_rng(14)
    for _ in range(10):
        a = to_device(host_actions(kind, n, rng))
        eng.step(a.data_ptr())
        plain.step(a.data_ptr())
    blob, blob_plain = eng.snapshot(), plain.snapshot()
    assert len(blob) - len(blob_plain) == eng.obs_dim * n * 4
    restored = gymrs.BatchedEngine(kind, n, flags=flags, params=p)
    restored.restore(blob)
    twin = eng.clone()
    for e in (restored, twin):
        assert np.array_equal(bits(e.get_final_obs()), bits(eng.get_final_obs()))
    with pytest.raises(gymrs.GymrsError):
        plain.restore(blob)  # flags differ
    for _ in range(9):
        a = to_device(host_actions(kind, n, rng))
        for e in (eng, restored, twin):
            e.step(a.data_ptr())
    for e in (restored, twin):
        assert np.array_equal(bits(e.get_final_obs()), bits(eng.get_final_obs()))
        assert_same_outputs(e, eng)


def test_snapshot_of_an_engine_without_the_flag_is_unchanged(gymrs):
    """Header + segments: the size formula of the blob without GYMRS_FINAL_OBS does not involve the flag at all."""
    for kind in (0, 1, 2):
        sizes = []
        for flags in (A | S | T, A | S | T | F):
            with gymrs.BatchedEngine(kind, 1234, flags=flags) as e:
                sizes.append(len(e.snapshot()))
        assert sizes[1] - sizes[0] == (3 if kind == 2 else (4 if kind == 0 else 2)) * 1234 * 4


def test_reset_zeroes_and_set_state_keeps(gymrs):
    n, flags = 2048, A | T | F
    p = params(gymrs, 0, 4)
    eng = gymrs.BatchedEngine(0, n, flags=flags, params=p)
    eng.reset(seed=1)
    buf = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    for t in range(6):
        eng.fill_actions(buf.data_ptr(), 2, t)
        eng.step(buf.data_ptr())
    rows = eng.get_final_obs()
    assert np.all(np.any(rows != 0, axis=0))
    eng.set_state(np.zeros((4, n), np.float32))
    assert np.array_equal(bits(eng.get_final_obs()), bits(rows))
    eng.reset(seed=2)
    assert not eng.get_final_obs().any()
    for t in range(6):
        eng.fill_actions(buf.data_ptr(), 2, t)
        eng.step(buf.data_ptr())
    eng.reset_pcg64(seed=3)
    assert not eng.get_final_obs().any()


def test_views_and_errors(gymrs):
    with gymrs.BatchedEngine(2, 100, flags=A | T) as plain:
        with pytest.raises(gymrs.GymrsError):
            plain.final_obs_ptrs()
        with pytest.raises(gymrs.GymrsError):
            plain.get_final_obs()
    with gymrs.BatchedEngine(2, 100, flags=A | T | F) as eng:
        ptrs = eng.final_obs_ptrs()
        assert len(ptrs) == 3 and all(p % 64 == 0 for p in ptrs)  # rows start aligned for a vector store
        assert eng.get_final_obs(10, 20).shape == (3, 20)
        with pytest.raises(gymrs.GymrsError):
            eng.get_final_obs(90, 20)


@pytest.mark.parametrize("kind", [0, 2])
def test_sharded_two_blocks_equal_one_engine(gymrs, kind):
    n, flags, steps = 70001, A | S | T | F, 15
    p = params(gymrs, kind)
    sh = gymrs.ShardedEngine(kind, n, [0, 0], flags=flags, params=p)
    one = gymrs.BatchedEngine(kind, n, flags=flags, params=p)
    sh.reset(seed=17)
    one.reset(seed=17)
    rng = np.random.default_rng(18)
    for _ in range(steps):
        a = to_device(host_actions(kind, n, rng))
        esz = a.element_size()
        sh.step([a.data_ptr() + s.first_lane * esz for s in sh.shards])
        one.step(a.data_ptr())
    sh.sync()
    one.sync()
    assert np.array_equal(bits(sh.get_final_obs()), bits(one.get_final_obs()))
    assert one.get_final_obs().any()
    for s in sh.shards:
        assert len(s.final_obs_ptrs()) == one.obs_dim
        assert np.array_equal(bits(s.get_final_obs()), bits(one.get_final_obs(s.first_lane, s.n_envs)))
    sh.close()
