"""gymrs_policy_gradient against the CPU reference of tests/gradient_ref.py (which never loads the library; tests/test_gradient_ref.py
shows without a GPU that the reference is right).  grad and excluded are compared integer for integer, prob bit for bit (a NaN equals
any NaN, as in tests/test_gpu_advantages.py: the CPU's and the GPU's generated NaN differ in sign and payload).

The kernels (gym-rs_amd/csrc/gymrs_gradient.hip) are built per env, head (policy / critic) and network (affine / hidden), and each
holds the copies uniform / gathered weights x full / ragged wave that a wave picks from at run time.  Synthetic records -- built in
numpy and copied to the device -- meet 1, 5, 257, 4200, 5000 and 300 lanes (all four copies; lanes_per_policy = 1), K = 1, 2 and 7,
H = 0, 1, 5 and 64 (a chunk of the hidden layer with a remainder; sixteen chunks), rows wider than n_envs with NaN in the padding
lanes, tables pre-filled with non-zero words, and the planted lanes of gradient_ref.synthetic."""
import ctypes as C

import closed_loop_ref as cl
import gradient_ref as ref
import numpy as np
import pytest
import torch
from gradient_ref import DIMS, SENTINEL, bits
from test_gpu_advantages import padded, policy_engine, stride_of, upload
from test_gpu_closed_loop_table import DEV

pytestmark = pytest.mark.gpu
A, S, T = 1, 2, 4
EINVAL = 1
GRAD_FILL, EXCLUDED_FILL = -(1 << 62) - 12345, (1 << 64) - 3  # the call ADDS, modulo 2^64


class Buffers:
    """The rows of a case on the device (padding lanes: a NaN / 9), tables pre-filled with non-zero words, prob with the sentinel"""

    def __init__(self, c, lanes=None, tables=None):
        self.c = c
        sl = lanes if lanes is not None else slice(0, c.n)
        self.n = sl.stop - sl.start
        self.stride = s = stride_of(self.n)
        host = dict(obs=padded(c.obs[..., sl], s, SENTINEL), start_obs=padded(c.start_obs[..., sl], s, SENTINEL), coef=padded(c.coef[..., sl], s, SENTINEL),
                    actions=padded(c.actions[..., sl], s, 9))
        self.host = host
        self.dev = {k: upload(v) for k, v in host.items()}
        size = ref.size_of(c.kind, c.hidden, c.critic)
        if tables is None:
            tables = (torch.full((c.n_sets, size), GRAD_FILL, dtype=torch.int64, device=DEV),
                      torch.full((c.n_sets,), EXCLUDED_FILL - (1 << 64), dtype=torch.int64, device=DEV))
        self.grad, self.excluded = tables
        self.prob = torch.full((max(c.steps, 1), s), SENTINEL, dtype=torch.int32, device=DEV)
        torch.cuda.synchronize()

    def args(self, with_prob=True, **kw):
        c = self.c
        a = dict(record=dict(obs=self.dev["obs"].data_ptr(), actions=self.dev["actions"].data_ptr(), lane_stride=self.stride),
                 start_obs=self.dev["start_obs"].data_ptr(), coef=self.dev["coef"].data_ptr(), grad=self.grad.data_ptr(), excluded=self.excluded.data_ptr(),
                 prob=self.prob.data_ptr() if with_prob and not c.critic else None, critic=c.critic)
        if not c.critic:
            a["scale"] = c.scale
        a.update(kw)
        return a

    def inputs_unchanged(self):
        for k, v in self.dev.items():
            assert np.array_equal(v.cpu().numpy().view(np.uint8), self.host[k].view(np.uint8)), ("an input buffer was written", k)

    def check(self, at, times=1, prob=True):
        c = self.c
        want_g, want_e, want_p = ref.reference(c, prob=not c.critic)
        got_g, got_e = self.grad.cpu().numpy().view(np.uint64), self.excluded.cpu().numpy().view(np.uint64)
        with np.errstate(over="ignore"):
            exp_g = np.uint64(GRAD_FILL % (1 << 64)) + np.uint64(times) * want_g.view(np.uint64)
            exp_e = np.uint64(EXCLUDED_FILL) + np.uint64(times) * want_e
        bad = np.argwhere(got_g != exp_g)
        assert bad.size == 0, ("grad", at, len(bad), [(int(m), int(s), int(got_g[m, s]) - int(exp_g[m, s])) for m, s in bad[:4]])
        assert np.array_equal(got_e, exp_e), ("excluded", at, got_e - np.uint64(EXCLUDED_FILL), want_e)
        got_p = self.prob.cpu().numpy().view(np.uint32)
        assert (got_p[:, c.n:] == SENTINEL).all(), ("padding lanes of prob written", at)
        if c.critic or not prob:
            assert (got_p == SENTINEL).all(), ("prob written", at)
        else:
            mine = got_p[:c.steps, :c.n]
            bad = np.argwhere((mine != bits(want_p)) & ~(np.isnan(mine.view(np.float32)) & np.isnan(want_p)))
            assert bad.size == 0, ("prob", at, len(bad), [(int(k), int(i), cl.COPIES[c.classes[i]], hex(mine[k, i]), hex(bits(want_p)[k, i])) for k, i in bad[:4]])
        self.inputs_unchanged()


def engine_for(gymrs, c, lanes=None, flags=A | S | T):
    sl = lanes if lanes is not None else slice(0, c.n)
    eng = gymrs.BatchedEngine(c.kind, sl.stop - sl.start, global_env_offset=c.gid0 + sl.start, flags=flags)
    eng.reset(seed=3)
    install(eng, c)
    return eng


def install(eng, c):
    if c.critic:
        eng.set_critic(c.weights, hidden=c.hidden, lanes_per_critic=c.lanes_per_set)
    else:
        eng.set_policy(c.weights, hidden=c.hidden, lanes_per_policy=c.lanes_per_set)


@pytest.mark.parametrize("kind,shape,hidden", ref.matrix())
def test_synthetic_records_equal_the_cpu_reference(gymrs, kind, shape, hidden):
    """both heads and K = 1, 2, 7 on one engine per (env, shape, H)"""
    n, gid0, _, _ = ref.SHAPES[shape]
    eng = gymrs.BatchedEngine(kind, n, global_env_offset=gid0, flags=A | S | T)
    eng.reset(seed=3)
    for critic in (False, True):
        for steps in ref.STEPS:
            c = ref.synthetic(kind, shape, steps, hidden, critic)
            install(eng, c)
            buf = Buffers(c)
            eng.policy_gradient(steps, **buf.args())
            eng.sync()
            buf.check((kind, shape, hidden, critic, steps))
    eng.close()


@pytest.mark.parametrize("kind,hidden", [(0, 5), (1, 0)])
def test_calling_twice_adds_twice_and_prob_is_optional(gymrs, kind, hidden):
    c = ref.synthetic(kind, 4, 7, hidden, False)
    eng = engine_for(gymrs, c)
    buf = Buffers(c)
    eng.policy_gradient(c.steps, **buf.args(with_prob=False))
    eng.policy_gradient(c.steps, **buf.args(with_prob=False))
    eng.sync()
    buf.check("twice", times=2, prob=False)
    eng.close()


@pytest.mark.parametrize("kind,shape,hidden", [(0, 3, 7), (1, 4, 0)])
def test_transitions_advantages_and_both_gradients_without_a_sync_in_between(gymrs, kind, shape, hidden):
    """a real engine (A | S | T, 17-step episodes) collects with sampling, turns the record into advantages and takes the policy's
    and the critic's gradient with coef = the advantages row, four launches back to back; the tables equal the reference applied to
    the record read back"""
    n, gid0, lps, n_sets = ref.SHAPES[shape]
    steps, d, s = 7, DIMS[kind][0], stride_of(n)
    eng = policy_engine(gymrs, kind, n, gid0, lps, hidden, A | S | T)
    policy = eng.get_policy()[0].copy()
    critics = ref.make_sets(kind, hidden, True, n_sets, 9)
    eng.set_critic(critics, hidden=hidden, lanes_per_critic=lps)
    f32 = lambda *shape: torch.full(shape, SENTINEL, dtype=torch.int32, device=DEV)  # noqa: E731
    u8 = lambda *shape: torch.full(shape, 9, dtype=torch.uint8, device=DEV)  # noqa: E731
    obs, fin, start, rew, act, done, trunc = f32(steps, d, s), f32(steps, d, s), f32(d, s), f32(steps, s), u8(steps, s), u8(steps, s), u8(steps, s)
    adv, prob = f32(steps, s), f32(steps, s)
    tables = {critic: (torch.zeros((n_sets, ref.size_of(kind, hidden, critic)), dtype=torch.int64, device=DEV), torch.zeros(n_sets, dtype=torch.int64, device=DEV))
              for critic in (False, True)}
    torch.cuda.synchronize()
    record = dict(obs=obs.data_ptr(), actions=act.data_ptr(), reward=rew.data_ptr(), done=done.data_ptr(), truncated=trunc.data_ptr(), lane_stride=s)
    eng.rollout_transitions(steps, record=record, final_obs=fin.data_ptr(), start_obs=start.data_ptr(), sample=True)
    eng.advantages(steps, record=record, final_obs=fin.data_ptr(), start_obs=start.data_ptr(), advantages=adv.data_ptr(), gamma=0.97, lam=0.9, critic=True)
    eng.policy_gradient(steps, record=record, start_obs=start.data_ptr(), coef=adv.data_ptr(), grad=tables[False][0].data_ptr(),
                        excluded=tables[False][1].data_ptr(), prob=prob.data_ptr(), temperature=8.0)
    eng.policy_gradient(steps, record=record, start_obs=start.data_ptr(), coef=adv.data_ptr(), grad=tables[True][0].data_ptr(),
                        excluded=tables[True][1].data_ptr(), critic=True)
    eng.sync()
    host = lambda t: t.cpu().numpy()[..., :n]  # noqa: E731
    for critic in (False, True):
        c = ref.synthetic(kind, shape, steps, hidden, critic, specials=False)  # the shape's keys; the record replaces its arrays
        c.weights = critics if critic else policy
        c.scale = float(np.float32(1.4426950408889634 / 8.0))
        c.obs, c.start_obs, c.coef = (host(t).view(np.float32) for t in (obs, start, adv))
        c.actions = host(act)
        assert np.isfinite(c.coef).all() and c.coef.any() and (c.actions < DIMS[kind][1]).all()
        want_g, want_e, want_p = ref.reference(c, prob=not critic)
        assert np.array_equal(tables[critic][0].cpu().numpy(), want_g), critic
        assert np.array_equal(tables[critic][1].cpu().numpy().view(np.uint64), want_e) and not want_e.any() and want_g.any(), critic
        if not critic:
            got = prob.cpu().numpy().view(np.uint32)
            assert np.array_equal(got[:, :n], bits(want_p)) and (got[:, n:] == SENTINEL).all()
    eng.close()


@pytest.mark.parametrize("kind,shape,hidden,critic", [(0, 3, 5, False), (1, 4, 0, False), (0, 4, 64, True)])
def test_two_engines_adding_into_the_same_tables_equal_one(gymrs, kind, shape, hidden, critic):
    c = ref.synthetic(kind, shape, 7, hidden, critic)
    cut = 1999  # the second block starts at an odd lane: its work-items straddle what the whole batch's do not
    first = Buffers(c, slice(0, cut))
    second = Buffers(c, slice(cut, c.n), tables=(first.grad, first.excluded))
    engines = [engine_for(gymrs, c, slice(0, cut)), engine_for(gymrs, c, slice(cut, c.n))]
    for eng, buf in zip(engines, (first, second)):
        eng.policy_gradient(c.steps, **buf.args(with_prob=False))
    for eng in engines:
        eng.sync()
    want_g, want_e, _ = ref.reference(c)
    with np.errstate(over="ignore"):
        assert np.array_equal(first.grad.cpu().numpy().view(np.uint64), np.uint64(GRAD_FILL % (1 << 64)) + want_g.view(np.uint64))
        assert np.array_equal(first.excluded.cpu().numpy().view(np.uint64), np.uint64(EXCLUDED_FILL) + want_e)
    for eng in engines:
        eng.close()


@pytest.mark.parametrize("kind,critic", [(0, False), (1, True)])
def test_the_engine_and_the_inputs_are_untouched(gymrs, kind, critic):
    c = ref.synthetic(kind, 2, 7, 5, critic)
    eng = policy_engine(gymrs, kind, c.n, c.gid0, c.lanes_per_set, 8, A | S | T)
    eng.set_critic(ref.make_sets(kind, 5, True, c.n_sets, 4), hidden=5, lanes_per_critic=c.lanes_per_set)
    if not critic:
        c.weights = ref.make_sets(kind, 8, False, c.n_sets, 5)
        c.hidden = 8
        eng.set_policy(c.weights, hidden=8, lanes_per_policy=c.lanes_per_set)
    else:
        c.weights = eng.critic()[0].copy()
    eng.rollout_policy_fitness(20)
    eng.sync()
    before = eng.snapshot(), eng.tick(), eng.stats().copy(), eng.policy_fitness().copy(), eng.get_policy()[0].copy(), eng.critic()[0].copy()
    buf = Buffers(c)
    eng.policy_gradient(c.steps, **buf.args())
    eng.sync()
    buf.check("untouched")
    after = eng.snapshot(), eng.tick(), eng.stats(), eng.policy_fitness(), eng.get_policy()[0], eng.critic()[0]
    assert before[0] == after[0] and before[1] == after[1]
    for a, b in zip(before[2:], after[2:]):
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))
    # n_steps = 0 adds and writes nothing
    buf = Buffers(c)
    eng.policy_gradient(0, **buf.args())
    eng.sync()
    assert (buf.grad.cpu().numpy() == GRAD_FILL).all() and (buf.excluded.cpu().numpy().view(np.uint64) == np.uint64(EXCLUDED_FILL)).all()
    assert (buf.prob.cpu().numpy().view(np.uint32) == SENTINEL).all()
    buf.inputs_unchanged()
    eng.close()


def test_refusals(gymrs):
    c = ref.synthetic(0, 2, 2, 0, False)
    eng = engine_for(gymrs, c)
    eng.set_critic(ref.make_sets(0, 0, True, 3, 1), hidden=0, lanes_per_critic=c.lanes_per_set)
    buf = Buffers(c)
    before = eng.snapshot(), eng.tick()

    def refused(match, eng=eng, steps=2, **kw):
        args = buf.args(**kw)
        if "temperature" in kw:
            args.pop("scale", None)
        with pytest.raises(gymrs.GymrsError, match=match) as err:
            eng.policy_gradient(steps, **args)
        assert err.value.status == EINVAL and "gymrs_policy_gradient" in str(err.value)

    def record(**kw):
        r = dict(buf.args()["record"])
        r.update(kw)
        return r

    refused("unknown flag bits", flags=2)
    refused("unknown flag bits", flags=1 | 4)
    for bad in (float("nan"), -0.5, float("inf")):
        refused("scale", scale=bad)
    refused("record.obs", record=record(obs=0))
    refused("record.actions", record=record(actions=0))
    refused("start_obs", start_obs=0)
    refused("coef is NULL", coef=0)
    refused("grad is NULL", grad=0)
    refused("excluded is NULL", excluded=0)
    refused("prob with GYMRS_GRADIENT_CRITIC", critic=True, scale=None)
    for name in ("start_obs", "coef"):
        refused("16-byte aligned", **{name: buf.dev[name].data_ptr() + 4})
    refused("16-byte aligned", prob=buf.prob.data_ptr() + 8)
    for name in ("obs", "actions"):
        refused("16-byte aligned", record=record(**{name: buf.dev[name].data_ptr() + 8}))
    refused("8-byte aligned", grad=buf.grad.data_ptr() + 4)
    refused("8-byte aligned", excluded=buf.excluded.data_ptr() + 4)
    refused("lane_stride", record=record(lane_stride=c.n - 1 - (c.n - 1) % 16))
    refused("lane_stride", record=record(lane_stride=buf.stride + 8))
    lib = eng._lib
    traj = gymrs.engine.Trajectory(buf.dev["obs"].data_ptr(), buf.dev["actions"].data_ptr(), None, None, None, buf.stride)
    desc = gymrs.GradientDesc(2, 0, c.scale, 0, traj, buf.dev["start_obs"].data_ptr(), buf.dev["coef"].data_ptr(), None, buf.grad.data_ptr(),
                              buf.excluded.data_ptr(), 1)
    assert lib.gymrs_policy_gradient(eng._h, C.byref(desc)) == EINVAL and b"reserved" in lib.gymrs_last_error()
    assert lib.gymrs_policy_gradient(None, C.byref(desc)) == EINVAL and lib.gymrs_policy_gradient(eng._h, None) == EINVAL
    # nothing was added so far
    eng.sync()
    assert (buf.grad.cpu().numpy() == GRAD_FILL).all() and (buf.prob.cpu().numpy().view(np.uint32) == SENTINEL).all()
    desc.reserved = 0
    assert lib.gymrs_policy_gradient(eng._h, C.byref(desc)) == 0  # the minimal descriptor: no reward, done, truncated, prob
    eng.sync()
    buf.check("minimal", prob=False)
    # the critic head reads no actions and no scale
    critic_table = torch.zeros((3, 5), dtype=torch.int64, device=DEV)
    torch.cuda.synchronize()
    desc = gymrs.GradientDesc(2, 1, float("nan"), 0, gymrs.engine.Trajectory(buf.dev["obs"].data_ptr(), None, None, None, None, buf.stride),
                              buf.dev["start_obs"].data_ptr(), buf.dev["coef"].data_ptr(), None, critic_table.data_ptr(),
                              buf.excluded.data_ptr(), 0)
    assert lib.gymrs_policy_gradient(eng._h, C.byref(desc)) == 0
    eng.sync()
    # no set
    eng.set_critic(None)
    refused("gymrs_set_critic", critic=True, prob=None, scale=None)
    eng.set_policy(None)
    refused("gymrs_set_policy")
    assert eng.snapshot() == before[0] and eng.tick() == before[1]
    eng.close()
    pend = gymrs.BatchedEngine(gymrs.PENDULUM, 256, flags=A | T)
    pend.reset(seed=1)
    refused("Pendulum", eng=pend)
    pend.close()
