"""gymrs_q_gradient against its definition as code (gymrs_q_lane summed over lanes: integer for integer, td bit for bit) and against
the f64 calculus of tests/q_ref.py.  The shapes of q_ref.SHAPES meet every code copy of the two kernels: one lane, a gathered ragged
wave at an offset, one full wave plus a ragged wave of one, 300 lanes with one lane per set (every wave gathers); H = 0, 1, 5, 64:
affine, one chunk with a remainder, two chunks with a remainder, the widest.  Rows are wider than n_envs with NaN in the padding
lanes, the tables are pre-filled with non-zero words, and final_obs holds a NaN sentinel wherever no step ended."""
import ctypes as C

import numpy as np
import pytest
import q_ref as ref
import torch
from test_gpu_advantages import padded, stride_of, upload
from test_gpu_closed_loop_table import DEV
from test_gpu_ppo import _Floats
from test_q_lane import check_against_calculus, lanes

pytestmark = pytest.mark.gpu
A, S, T = 1, 2, 4
EINVAL = 1
FILL = {"grad": -(1 << 62) - 12345, "excluded": (1 << 63) - 3, "counts": (1 << 62) + 77}  # the call ADDS, modulo 2^64
NAN = 0x7FC00123


class Buffers:
    """The rows of a case on the device (padding lanes: a NaN / 9), tables pre-filled with non-zero words, td with a sentinel"""

    def __init__(self, c, lanes=None, tables=None):
        sl = lanes if lanes is not None else slice(0, c.n)
        self.c, self.n = c, sl.stop - sl.start
        self.stride = s = stride_of(self.n)
        self.host = {k: padded(getattr(c, k)[..., sl], s, 9 if getattr(c, k).dtype == np.uint8 else NAN)
                     for k in ("obs", "start_obs", "final_obs", "reward", "done", "truncated", "actions")}
        self.dev = {k: upload(v) for k, v in self.host.items()}
        shapes = dict(grad=(c.n_sets, ref.size_of(c.kind, c.hidden)), excluded=(c.n_sets,), counts=(c.n_sets, 2))
        self.tables = tables or {k: torch.full(shape, FILL[k], dtype=torch.int64, device=DEV) for k, shape in shapes.items()}
        self.td = torch.full((max(c.steps, 1), s), NAN, dtype=torch.int32, device=DEV)
        torch.cuda.synchronize()

    def args(self, **kw):
        c, p = self.c, {k: v.data_ptr() for k, v in self.dev.items()}
        a = dict(record=dict(obs=p["obs"], actions=p["actions"], reward=p["reward"], done=p["done"], truncated=p["truncated"], lane_stride=self.stride),
                 start_obs=p["start_obs"], final_obs=p["final_obs"], td=self.td.data_ptr(), gamma=c.gamma, kappa=c.kappa, flags=c.flags,
                 **{k: v.data_ptr() for k, v in self.tables.items()})
        a.update(kw)
        return a

    def added(self):
        """what the calls added to (grad, excluded, counts), and td [K][n] after checking that nothing else was written"""
        for k, v in self.dev.items():
            assert np.array_equal(v.cpu().numpy().view(np.uint8), self.host[k].view(np.uint8)), ("an input buffer was written", k)
        td = self.td.cpu().numpy()
        assert (td[:, self.n:] == NAN).all(), "padding lanes of td written"
        with np.errstate(over="ignore"):
            return tuple(self.tables[k].cpu().numpy() - np.int64(FILL[k]) for k in ("grad", "excluded", "counts")) + (td[:self.c.steps, :self.n].view(np.float32),)


def engine_for(gymrs, c, lanes=None, target=True):
    sl = lanes if lanes is not None else slice(0, c.n)
    eng = gymrs.BatchedEngine(c.kind, sl.stop - sl.start, global_env_offset=c.gid0 + sl.start, flags=A | S | T)
    eng.reset(seed=3)
    if target:  # the target set is a copy of the policy set: install it first, then the online set of the same shape
        eng.set_policy(c.target, hidden=c.hidden, lanes_per_policy=c.lanes_per_set)
        eng.q_target_sync()
    eng.set_policy(c.weights, hidden=c.hidden, lanes_per_policy=c.lanes_per_set)
    return eng


def definition(gymrs, c):
    """(grad, excluded, counts) per set and td by gymrs_q_lane, summed over lanes in integers"""
    q, ex, td, n = lanes(gymrs, c)
    idx = ref.set_index(c)
    out = [np.zeros((c.n_sets,) + v.shape[1:], np.int64) for v in (q, ex, n)]
    with np.errstate(over="ignore"):
        for o, v in zip(out, (q, ex, n)):
            np.add.at(o, idx, v.view(np.int64))
    return out + [td]


def state_of(eng):
    return eng.snapshot(), eng.tick(), eng.stats().tobytes()


@pytest.mark.parametrize("flags", [0, ref.DOUBLE])
@pytest.mark.parametrize("hidden", [0, 1, 5, 64])
@pytest.mark.parametrize("shape", [0, 1, 2, 3])
@pytest.mark.parametrize("kind", [0, 1])
def test_record_equals_the_definition(gymrs, kind, shape, hidden, flags):
    for steps, (gamma, kappa) in zip((1, 2, 7), ((0.97, 1.0), (1.0, float("inf")), (0.9, 0.5))):
        c = ref.synthetic(kind, shape, steps, hidden, flags, gamma, kappa)
        eng, buf = engine_for(gymrs, c), Buffers(c)
        before = state_of(eng)
        eng.q_gradient(steps, **buf.args())
        eng.sync()
        grad, excluded, counts, td = buf.added()
        want = definition(gymrs, c)
        for name, got, exp in zip(("grad", "excluded", "counts"), (grad, excluded, counts), want):
            assert np.array_equal(got, exp), (name, steps, np.argwhere(got != exp)[:4])
        same = (td.view(np.uint32) == want[3].view(np.uint32)) | (np.isnan(td) & np.isnan(want[3]))
        assert same.all(), ("td", steps, np.argwhere(~same)[:4])
        check_against_calculus(c, grad, excluded.view(np.uint64), td, counts.view(np.uint64))
        assert state_of(eng) == before
        eng.close()


def test_target_set_life_cycle(gymrs):
    c = ref.synthetic(0, 1, 7, 5, ref.DOUBLE, 0.97, 1.0)
    eng, buf = engine_for(gymrs, c, target=False), Buffers(c)
    before = state_of(eng)
    with pytest.raises(gymrs.GymrsError, match="gymrs_q_target_sync"):
        eng.q_gradient(c.steps, **buf.args())
    with pytest.raises(gymrs.GymrsError, match="gymrs_q_target_sync"):
        eng.q_target_ptr()
    # sync, then rewrite the online weights in place: the two sets differ
    eng.set_policy(c.target, hidden=c.hidden, lanes_per_policy=c.lanes_per_set)
    eng.q_target_sync()
    eng.sync()  # (the copy reads the policy set on the engine's stream; torch writes it on its own)
    ptr, floats = eng.policy_weights_ptr()
    assert floats == c.weights.size and eng.q_target_ptr()[1] == floats and eng.q_target_ptr()[0] != ptr
    torch.as_tensor(_Floats(ptr, floats), device=DEV).copy_(torch.from_numpy(c.weights.reshape(-1)).to(DEV))
    torch.cuda.synchronize()
    eng.q_gradient(c.steps, **buf.args())
    eng.sync()
    want = definition(gymrs, c)
    assert all(np.array_equal(g, w) for g, w in zip(buf.added()[:3], want)) and want[0].any()
    # a set of the same shape keeps the target
    eng.set_policy(c.weights, hidden=c.hidden, lanes_per_policy=c.lanes_per_set)
    again = Buffers(c)
    eng.q_gradient(c.steps, **again.args())
    eng.sync()
    assert all(np.array_equal(g, w) for g, w in zip(again.added()[:3], want))
    # another hidden width discards it, and so does the removal of the policy
    eng.set_policy(np.zeros((c.n_sets, ref.size_of(0, 6)), np.float32), hidden=6, lanes_per_policy=c.lanes_per_set)
    with pytest.raises(gymrs.GymrsError, match="gymrs_q_target_sync"):
        eng.q_gradient(c.steps, **again.args())
    eng.q_target_sync()
    eng.set_policy(None)
    with pytest.raises(gymrs.GymrsError, match="gymrs_set_policy"):
        eng.q_target_sync()
    assert state_of(eng) == before
    eng.close()


@pytest.mark.parametrize("kind,hidden", [(0, 5), (1, 0)])
def test_chain_without_a_sync(gymrs, kind, hidden):
    """collection with exploration, then the call twice into one table: twice the single call's, which is the definition's on the record
    read back"""
    n, gid0, lps, n_sets = ref.SHAPES[3]
    steps, d, s = 7, ref.DIMS[kind][0], stride_of(n)
    c = ref.synthetic(kind, 3, steps, hidden, ref.DOUBLE, 0.97, 1.0)
    eng = engine_for(gymrs, c)
    eng.set_exploration(11, epsilon=0.25)
    f32 = lambda *shape: torch.full(shape, NAN, dtype=torch.int32, device=DEV)  # noqa: E731
    u8 = lambda *shape: torch.full(shape, 9, dtype=torch.uint8, device=DEV)  # noqa: E731
    obs, fin, start, rew, td = f32(steps, d, s), f32(steps, d, s), f32(d, s), f32(steps, s), f32(steps, s)
    act, done, trunc = u8(steps, s), u8(steps, s), u8(steps, s)
    once, twice = ({k: torch.zeros(shape, dtype=torch.int64, device=DEV) for k, shape in
                    dict(grad=(n_sets, ref.size_of(kind, hidden)), excluded=(n_sets,), counts=(n_sets, 2)).items()} for _ in range(2))
    torch.cuda.synchronize()
    record = dict(obs=obs.data_ptr(), actions=act.data_ptr(), reward=rew.data_ptr(), done=done.data_ptr(), truncated=trunc.data_ptr(), lane_stride=s)
    call = dict(record=record, start_obs=start.data_ptr(), final_obs=fin.data_ptr(), td=td.data_ptr(), gamma=c.gamma, kappa=c.kappa, double=True)
    eng.rollout_transitions(steps, record=record, final_obs=fin.data_ptr(), start_obs=start.data_ptr(), explore=True)
    eng.q_gradient(steps, **call, **{k: v.data_ptr() for k, v in once.items()})
    for _ in range(2):
        eng.q_gradient(steps, **call, **{k: v.data_ptr() for k, v in twice.items()})
    eng.sync()
    host = lambda t: t.cpu().numpy()[..., :n]  # noqa: E731
    c.obs, c.start_obs, c.final_obs, c.reward = (host(t).view(np.float32) for t in (obs, start, fin, rew))
    c.actions, c.done, c.truncated = host(act), host(done), host(trunc)
    want = definition(gymrs, c)
    for k, w in zip(("grad", "excluded", "counts"), want):
        assert np.array_equal(once[k].cpu().numpy(), w) and np.array_equal(twice[k].cpu().numpy(), 2 * w), k
    assert want[0].any() and want[2][:, 0].sum() == steps * n and np.array_equal(host(td).view(np.uint32), want[3].view(np.uint32))
    eng.close()


def test_two_engines_adding_into_one_table_equal_one(gymrs):
    c = ref.synthetic(1, 3, 7, 5, 0, 0.97, 1.0)
    cut = 131  # the second block starts at an odd lane
    first = Buffers(c, slice(0, cut))
    second = Buffers(c, slice(cut, c.n), tables=first.tables)
    engines = [engine_for(gymrs, c, slice(0, cut)), engine_for(gymrs, c, slice(cut, c.n))]
    for eng, buf in zip(engines, (first, second)):
        eng.q_gradient(c.steps, **buf.args())
    for eng in engines:
        eng.sync()
    assert all(np.array_equal(g, w) for g, w in zip(first.added()[:3], definition(gymrs, c)))
    for eng in engines:
        eng.close()


def test_refusals(gymrs):
    c = ref.synthetic(0, 1, 2, 0, 0, 0.97, 1.0)
    eng, buf = engine_for(gymrs, c), Buffers(c)
    before = state_of(eng)

    def refused(match, eng=eng, **kw):
        with pytest.raises(gymrs.GymrsError, match=match) as err:
            eng.q_gradient(2, **buf.args(**kw))
        assert err.value.status == EINVAL and "gymrs_q_gradient" in str(err.value)

    def record(**kw):
        r = dict(buf.args()["record"])
        r.update(kw)
        return r

    refused("flag", flags=2)
    for name, values in (("gamma", (float("nan"), -0.1, 1.5, float("inf"))), ("kappa", (float("nan"), 0.0, -1.0))):
        for bad in values:
            refused(name, **{name: bad})
    for name in ("obs", "actions", "reward", "done", "truncated", "start_obs", "final_obs"):
        row, ptr = name not in ("start_obs", "final_obs"), buf.dev[name].data_ptr()
        if name != "truncated":
            refused(name + " is NULL", **(dict(record=record(**{name: 0})) if row else {name: 0}))
        refused("16-byte aligned", **(dict(record=record(**{name: ptr + 8})) if row else {name: ptr + 8}))
        refused("alias", td=ptr)
    refused("td is NULL", td=0)
    refused("16-byte aligned", td=buf.td.data_ptr() + 4)
    for name in ("grad", "excluded", "counts"):
        if name != "counts":
            refused(name + " is NULL", **{name: 0})
        refused("8-byte aligned", **{name: buf.tables[name].data_ptr() + 4})
    for stride in (0, buf.stride + 8):
        refused("lane_stride", record=record(lane_stride=stride))
    lib = eng._lib
    d = gymrs.QDesc(2, 0, c.gamma, c.kappa, gymrs.engine.Trajectory(*(buf.dev[k].data_ptr() for k in ("obs", "actions", "reward", "done")), None, buf.stride),
                    buf.dev["start_obs"].data_ptr(), buf.dev["final_obs"].data_ptr(), buf.td.data_ptr(), buf.tables["grad"].data_ptr(),
                    buf.tables["excluded"].data_ptr(), None, 1)
    assert lib.gymrs_q_gradient(eng._h, C.byref(d)) == EINVAL and b"reserved" in lib.gymrs_last_error()
    assert lib.gymrs_q_gradient(None, C.byref(d)) == EINVAL and lib.gymrs_q_gradient(eng._h, None) == EINVAL
    d.reserved, d.n_steps = 0, 0
    assert lib.gymrs_q_gradient(eng._h, C.byref(d)) == 0  # no steps: a no-op after the checks
    eng.sync()
    got = buf.added()
    assert not any(t.any() for t in got[:3]) and (buf.td.cpu().numpy() == NAN).all() and state_of(eng) == before
    eng.set_policy(None)
    refused("gymrs_set_policy")
    eng.close()
    pend = gymrs.BatchedEngine(gymrs.PENDULUM, 256, flags=A | T)
    pend.reset(seed=1)
    refused("Pendulum", eng=pend)
    with pytest.raises(gymrs.GymrsError, match="Pendulum"):
        pend.q_target_sync()
    pend.close()
