"""gymrs_advantages against the CPU reference of tests/advantages_ref.py (which never loads the library; tests/test_advantages_ref.py
shows without a GPU that the reference is right and that its cases are worth comparing with).  Every comparison is bit for bit; a
NaN equals any NaN, as in tests/test_gpu_slowpaths.py (sign and payload of a generated NaN are not specified, and the CPU's and the
GPU's differ), so a NaN where the reference has a number -- a leaked sentinel -- still shows.

The kernels (gym-rs_amd/csrc/gymrs_advantages.hip) are built per env with the critic on and off, and each holds the copies uniform /
gathered critic weights x full / ragged wave that a wave picks from at run time.  Synthetic records -- built in numpy and copied to
the device, so the kernel is tested independently of the rollout kernels -- meet 1, 5, 257, 4200, 5000 and 300 lanes (all four
copies; lanes_per_critic = 1), K = 1, 2 and 17, H = 0, 7 and 8, with and without final_obs, truncated, returns and values, four
(gamma, lambda) pairs, observations with NaN, +-inf and 1e30, and final_obs pre-filled with a NaN sentinel outside ended steps.  The
end-to-end test runs gymrs_rollout_transitions with sampling immediately followed by gymrs_advantages, with no sync in between."""
import ctypes as C

import advantages_ref as ref
import closed_loop_ref as cl
import numpy as np
import pytest
import torch
from advantages_ref import DIMS, SENTINEL, bits
from test_gpu_closed_loop_table import DEV, DeviceColumn

pytestmark = pytest.mark.gpu
A, S, T = 1, 2, 4
EINVAL = 1


def stride_of(n):
    return (n + 15) // 16 * 16 + 16  # > n: rows have padding lanes


def padded(a, stride, fill):
    """the last axis widened to `stride` lanes, the padding lanes holding `fill` (a bit pattern for f32 arrays, a byte for u8)"""
    a = np.ascontiguousarray(a)
    out = np.full(a.shape[:-1] + (stride,), fill, np.uint32 if a.dtype == np.float32 else np.uint8)
    out[..., :a.shape[-1]] = a.view(out.dtype)
    return out


def upload(a):
    t = torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(DEV)
    torch.cuda.synchronize()  # torch copied on its stream; the engine reads on its own
    return t


class Buffers:
    """The record of a case on the device (padding lanes: the sentinel / 9) and sentinel-filled outputs"""

    def __init__(self, c, returns=True, values=True):
        self.c, self.stride = c, stride_of(c.n)
        s = self.stride
        host = dict(obs=padded(c.obs, s, SENTINEL), reward=padded(c.reward, s, SENTINEL), done=padded(c.done, s, 9), start_obs=padded(c.start_obs, s, SENTINEL))
        if c.truncated is not None:
            host["truncated"] = padded(c.truncated, s, 9)
        if c.final_obs is not None:
            host["final_obs"] = padded(c.final_obs, s, SENTINEL)
        self.host = host
        self.dev = {k: upload(v) for k, v in host.items()}
        self.out = {k: torch.full((max(c.steps, 1), s), SENTINEL, dtype=torch.int32, device=DEV)
                    for k, on in (("advantages", True), ("returns", returns), ("values", values)) if on}
        torch.cuda.synchronize()

    def ptr(self, name):
        t = self.dev.get(name, self.out.get(name))
        return t.data_ptr() if t is not None else None

    def args(self, **kw):
        c = self.c
        a = dict(record=dict(obs=self.ptr("obs"), actions=0, reward=self.ptr("reward"), done=self.ptr("done"), truncated=self.ptr("truncated") or 0,
                             lane_stride=self.stride),
                 start_obs=self.ptr("start_obs"), final_obs=self.ptr("final_obs"), advantages=self.ptr("advantages"), returns=self.ptr("returns"),
                 values=self.ptr("values"), gamma=c.gamma, lam=c.lam, critic=c.critic)
        a.update(kw)
        return a

    def results(self):
        return {k: v.cpu().numpy().view(np.uint32) for k, v in self.out.items()}

    def inputs_unchanged(self):
        for k, v in self.dev.items():
            assert np.array_equal(v.cpu().numpy().view(np.uint8), self.host[k].view(np.uint8)), ("an input buffer was written", k)

    def check(self, at):
        """outputs equal the reference at lanes < n, padding lanes keep the sentinel, every input keeps its bytes"""
        c = self.c
        want = dict(zip(("advantages", "returns", "values"), ref.reference(c)))
        for name, got in self.results().items():
            assert (got[:, c.n:] == SENTINEL).all(), ("padding lanes written", name, at)
            mine = got[:c.steps, :c.n]
            bad = np.argwhere((mine != bits(want[name])) & ~(np.isnan(mine.view(np.float32)) & np.isnan(want[name])))  # a NaN equals any NaN
            assert bad.size == 0, (name, at, len(bad), [(int(k), int(i), cl.COPIES[c.classes[i]], hex(got[k, i]), hex(bits(want[name])[k, i])) for k, i in bad[:4]])
        self.inputs_unchanged()


def engine_for(gymrs, c, flags=A | S | T):
    eng = gymrs.BatchedEngine(c.kind, c.n, global_env_offset=c.gid0, flags=flags)
    eng.reset(seed=3)
    eng.set_critic(c.weights, hidden=c.hidden, lanes_per_critic=c.lanes_per_critic)
    return eng


@pytest.mark.parametrize("kind,shape,steps,hidden,critic,final,trunc,returns,values,gl", ref.matrix())
def test_synthetic_records_equal_the_cpu_reference(gymrs, kind, shape, steps, hidden, critic, final, trunc, returns, values, gl):
    c = ref.synthetic(kind, shape, steps, hidden, critic, final, trunc, *gl)
    eng = engine_for(gymrs, c)
    buf = Buffers(c, returns, values)
    eng.advantages(steps, **buf.args())
    eng.sync()
    buf.check((kind, shape, steps, hidden))
    eng.close()


@pytest.mark.parametrize("kind,shape,hidden", [(0, 3, 64), (1, 4, 64), (0, 4, 16)])
def test_the_widest_critic(gymrs, kind, shape, hidden):
    """H = 64 (sixteen trips of the four-unit loop, 385 / 257 floats per critic) and the H = 16 of tools/bench_advantages.py"""
    c = ref.synthetic(kind, shape, 17, hidden)
    eng = engine_for(gymrs, c)
    buf = Buffers(c)
    eng.advantages(c.steps, **buf.args())
    eng.sync()
    buf.check((kind, shape, hidden))
    eng.close()


def policy_engine(gymrs, kind, n, gid0, lpp, hidden, flags):
    params = gymrs.engine.default_params(kind)
    params.max_episode_steps = cl.MAX_EPISODE_STEPS
    eng = gymrs.BatchedEngine(kind, n, global_env_offset=gid0, flags=flags, params=params)
    eng.reset(seed=cl.RESET_SEED)
    if kind == 1:
        eng.set_state(cl.mountain_car_prepare(eng.get_state(), 0))
    eng.set_policy(cl.make_weights(kind, hidden, cl.N_POLICIES, cl.SEEDS[kind, hidden, 0]), hidden=hidden, lanes_per_policy=lpp)
    eng.set_sampling(0x5A3B1E0FEEDC0DE5, temperature=8.0)
    return eng


@pytest.mark.parametrize("kind,shape,hidden", [(0, 3, 8), (1, 4, 7)])
def test_transitions_then_advantages_without_a_sync_in_between(gymrs, kind, shape, hidden):
    """a real engine (A | S | T, 17-step episodes): the outputs equal the reference applied to the record read back; the engine is left
    as the transitions launch alone leaves it"""
    n, gid0, lpc, n_critics = ref.SHAPES[shape]
    steps, d, s = 40, DIMS[kind][0], stride_of(n)
    eng, twin = (policy_engine(gymrs, kind, n, gid0, lpc, hidden, A | S | T) for _ in range(2))
    w = ref.make_critics(kind, hidden, n_critics, 9)
    eng.set_critic(w, hidden=hidden, lanes_per_critic=lpc)
    f32 = lambda *shape: torch.full(shape, SENTINEL, dtype=torch.int32, device=DEV)  # noqa: E731
    u8 = lambda *shape: torch.full(shape, 9, dtype=torch.uint8, device=DEV)  # noqa: E731
    obs, fin, start, rew, act, done, trunc = f32(steps, d, s), f32(steps, d, s), f32(d, s), f32(steps, s), u8(steps, s), u8(steps, s), u8(steps, s)
    adv, ret, val = f32(steps, s), f32(steps, s), f32(steps, s)
    torch.cuda.synchronize()
    record = dict(obs=obs.data_ptr(), actions=act.data_ptr(), reward=rew.data_ptr(), done=done.data_ptr(), truncated=trunc.data_ptr(), lane_stride=s)
    eng.rollout_transitions(steps, record=record, final_obs=fin.data_ptr(), start_obs=start.data_ptr(), sample=True)
    eng.advantages(steps, record=record, final_obs=fin.data_ptr(), start_obs=start.data_ptr(), advantages=adv.data_ptr(), returns=ret.data_ptr(),
                   values=val.data_ptr(), gamma=0.97, lam=0.9, critic=True)
    eng.sync()
    host = lambda t: t.cpu().numpy()[..., :n]  # noqa: E731
    c = ref.synthetic(kind, shape, steps, hidden, seed=1, specials=False)  # the shape's keys; the record replaces its arrays
    c.weights, c.gamma, c.lam = w, float(np.float32(0.97)), float(np.float32(0.9))
    c.obs, c.start_obs, c.reward = (host(t).view(np.float32) for t in (obs, start, rew))
    c.done, c.truncated = host(done), host(trunc)
    c.ended = (c.done | c.truncated) != 0
    c.final_obs = host(fin).view(np.float32)
    assert (bits(c.final_obs)[~np.broadcast_to(c.ended[:, None, :], c.final_obs.shape)] == SENTINEL).all()  # NaN outside ended steps: none may get through
    done_only, trunc_only = (c.done != 0) & (c.truncated == 0), (c.truncated != 0) & (c.done == 0)
    assert done_only.any() and trunc_only.any() and (c.ended.sum(axis=0) >= 2).any() and not c.ended.all(axis=0).any()
    want = ref.reference(c)
    for name, t, w_ in zip(("advantages", "returns", "values"), (adv, ret, val), want):
        got = t.cpu().numpy().view(np.uint32)
        assert np.array_equal(got[:, :n], bits(w_)), name  # (all finite, below: no NaN to allow for)
        assert (got[:, n:] == SENTINEL).all(), name
        assert np.isfinite(w_).all(), name
    # the engine: as after the transitions launch alone
    twin.rollout_transitions(steps, record=record, final_obs=fin.data_ptr(), start_obs=start.data_ptr(), sample=True)
    twin.sync()
    assert np.array_equal(bits(eng.get_state()), bits(twin.get_state())) and eng.tick() == twin.tick() and np.array_equal(eng.stats(), twin.stats())
    for a, b in zip(eng.get_step_result(), twin.get_step_result()):
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))
    eng.close()
    twin.close()


@pytest.mark.parametrize("kind", [0, 1])
def test_the_engine_and_the_inputs_are_untouched(gymrs, kind):
    c = ref.synthetic(kind, 2, 17, 8)
    eng = policy_engine(gymrs, kind, c.n, c.gid0, c.lanes_per_critic, 8, A | S | T)
    eng.set_critic(c.weights, hidden=c.hidden, lanes_per_critic=c.lanes_per_critic)
    eng.rollout_policy_fitness(20)
    eng.sync()
    before = eng.snapshot(), eng.tick(), eng.stats().copy(), eng.policy_fitness().copy(), eng.get_policy()[0].copy()
    buf = Buffers(c)
    eng.advantages(c.steps, **buf.args())
    eng.sync()
    buf.check("untouched")
    after = eng.snapshot(), eng.tick(), eng.stats(), eng.policy_fitness(), eng.get_policy()[0]
    assert before[0] == after[0] and before[1] == after[1]
    for a, b in zip(before[2:], after[2:]):
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))
    # n_steps = 0 writes nothing
    buf = Buffers(c)
    eng.advantages(0, **buf.args())
    eng.sync()
    assert all((got == SENTINEL).all() for got in buf.results().values())
    buf.inputs_unchanged()
    eng.close()


def test_critic_settings(gymrs):
    """a critic written in place through critic_weights_ptr on the engine's stream is seen by the next launch; set_policy does not
    disturb the critic; a critic without the flag gives the V = 0 bits"""
    c = ref.synthetic(0, 2, 17, 8)
    eng = engine_for(gymrs, c)
    got, hidden, block = eng.critic()
    assert np.array_equal(bits(got), bits(c.weights)) and (hidden, block) == (c.hidden, c.lanes_per_critic)
    w1 = ref.make_critics(0, 8, c.n_critics, 4242)
    ptr, count = eng.critic_weights_ptr()
    assert count == c.weights.size
    new = torch.from_numpy(w1.reshape(-1)).to(DEV)
    torch.cuda.synchronize()
    view = torch.as_tensor(DeviceColumn(ptr, count, "<f4"), device=DEV)
    first, second = Buffers(c), Buffers(c)
    eng.advantages(c.steps, **first.args())  # enqueued before the rewrite: the old critic
    with torch.cuda.stream(torch.cuda.ExternalStream(eng.stream, device=DEV)):
        view.copy_(new)
    eng.advantages(c.steps, **second.args())  # the next launch: the new one
    eng.sync()
    first.check("before the rewrite")
    c.weights = w1
    second.check("after the rewrite")
    assert not np.array_equal(first.results()["values"], second.results()["values"])
    # set_policy does not disturb the critic
    eng.set_policy(cl.make_weights(0, 0, 2, 1), hidden=0, lanes_per_policy=7)
    eng.set_policy(None)
    third = Buffers(c)
    eng.advantages(c.steps, **third.args())
    eng.sync()
    third.check("after set_policy")
    assert np.array_equal(bits(eng.critic()[0]), bits(w1))
    # a critic without the flag: V = 0
    c.critic = False
    c.classes = cl.wave_classes(c.n, 4, c.gid0, 1, c.lanes_per_critic)
    fourth = Buffers(c)
    eng.advantages(c.steps, **fourth.args())
    eng.sync()
    fourth.check("without the flag")
    assert not fourth.results()["values"][:, :c.n].any()
    # removal
    eng.set_critic(None)
    with pytest.raises(gymrs.GymrsError, match="gymrs_set_critic"):
        eng.critic()
    with pytest.raises(gymrs.GymrsError, match="gymrs_set_critic"):
        eng.critic_weights_ptr()
    fifth = Buffers(c)
    eng.advantages(c.steps, **fifth.args())  # still fine without the flag
    eng.sync()
    fifth.check("no critic set, no flag")
    eng.close()


def test_refusals(gymrs):
    c = ref.synthetic(0, 2, 2, 0)
    eng = engine_for(gymrs, c)
    buf = Buffers(c)
    before = eng.snapshot(), eng.tick()

    def refused(match, eng=eng, steps=2, **kw):
        args = buf.args(**kw)
        with pytest.raises(gymrs.GymrsError, match=match) as err:
            eng.advantages(steps, **args)
        assert err.value.status == EINVAL and "gymrs_advantages" in str(err.value)

    def record(**kw):
        r = dict(buf.args()["record"])
        r.update(kw)
        return r

    refused("unknown flag bits", flags=2)
    refused("unknown flag bits", flags=1 | 4)
    for bad in (float("nan"), -0.5, 1.5, float("inf")):
        refused("gamma", gamma=bad)
        refused("lambda", lam=bad)
    refused("record.obs", record=record(obs=0))
    refused("record.reward", record=record(reward=0))
    refused("record.done", record=record(done=0))
    refused("start_obs", start_obs=0)
    refused("advantages is NULL", advantages=0)
    for name in ("final_obs", "start_obs", "advantages", "returns", "values"):
        refused("16-byte aligned", **{name: buf.ptr(name) + 4})
    for name in ("obs", "reward", "done", "truncated"):
        refused("16-byte aligned", record=record(**{name: buf.ptr(name) + 8}))
    refused("lane_stride", record=record(lane_stride=c.n - 1 - (c.n - 1) % 16))
    refused("lane_stride", record=record(lane_stride=buf.stride + 8))
    desc = gymrs.AdvantagesDesc(2, 0, 1.0, 1.0, gymrs.engine.Trajectory(buf.ptr("obs"), None, buf.ptr("reward"), buf.ptr("done"), None, buf.stride), None,
                                buf.ptr("start_obs"), buf.ptr("advantages"), None, None, 1)
    lib = eng._lib
    assert lib.gymrs_advantages(eng._h, C.byref(desc)) == EINVAL and b"reserved" in lib.gymrs_last_error()
    assert lib.gymrs_advantages(None, C.byref(desc)) == EINVAL and lib.gymrs_advantages(eng._h, None) == EINVAL
    desc.reserved = 0
    assert lib.gymrs_advantages(eng._h, C.byref(desc)) == 0  # the minimal descriptor: no actions, truncated, final_obs, returns, values
    eng.sync()
    # the flag without a critic set
    eng.set_critic(None)
    refused("gymrs_set_critic", critic=True)
    assert eng.snapshot() == before[0] and eng.tick() == before[1]
    got = buf.results()
    assert (got["returns"] == SENTINEL).all() and (got["values"] == SENTINEL).all() and (got["advantages"][:, c.n:] == SENTINEL).all()
    # set_critic's refusals
    for match, kw in (("hidden must be <= 64", dict(hidden=65)), ("lanes_per_policy", dict(lanes_per_critic=0))):
        with pytest.raises((gymrs.GymrsError, ValueError), match=match):
            eng.set_critic(np.zeros(ref.critic_size(0, 0) if "lanes" in match else 65 * 6 + 1, np.float32), **kw)
    eng.close()
    pend = gymrs.BatchedEngine(gymrs.PENDULUM, 256, flags=A | T)
    pend.reset(seed=1)
    refused("Pendulum", eng=pend)
    with pytest.raises(gymrs.GymrsError, match="Pendulum"):
        pend.set_critic(np.zeros(5, np.float32))
    pend.close()
