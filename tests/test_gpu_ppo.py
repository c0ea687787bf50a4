"""gymrs_ppo_gradient against the CPU reference of tests/ppo_ref.py (which never loads the library; tests/test_ppo_ref.py shows without a
GPU that the reference is right).  grad, excluded and counts are compared integer for integer, prob bit for bit (a NaN equals any NaN,
as in tests/test_gpu_gradient.py).

The kernels (gym-rs_amd/csrc/gymrs_gradient_ppo.hip) are built per env and network (affine / hidden), and each holds the copies
uniform / gathered weights x full / ragged wave that a wave picks from at run time.  Synthetic cases -- built in numpy and copied to the
device -- meet 1, 5, 257, 4200, 5000 and 300 lanes (all four copies; lanes_per_policy = 1; ids beyond 2^32), K = 1, 2 and 7, H = 0, 1,
5 and 64, rows wider than n_envs with NaN in the padding lanes, tables pre-filled with non-zero words, the planted lanes of
ppo_ref.synthetic and bounds that sit on the ratio of a lane-step."""
import ctypes as C

import closed_loop_ref as cl
import numpy as np
import ppo_ref as ref
import pytest
import torch
from ppo_ref import DIMS, SENTINEL, bits
from test_gpu_advantages import padded, policy_engine, stride_of, upload
from test_gpu_closed_loop_table import DEV

pytestmark = pytest.mark.gpu
A, S, T = 1, 2, 4
EINVAL = 1
GRAD_FILL, EXCLUDED_FILL, COUNTS_FILL = -(1 << 62) - 12345, (1 << 64) - 3, (1 << 63) + 77  # the call ADDS, modulo 2^64


def filled(shape, value):
    return torch.full(shape, value - (1 << 64) if value >= 1 << 63 else value, dtype=torch.int64, device=DEV)


class Buffers:
    """The rows of a case on the device (padding lanes: a NaN / 9), tables pre-filled with non-zero words, prob with the sentinel"""

    def __init__(self, c, lanes=None, tables=None):
        self.c = c
        sl = lanes if lanes is not None else slice(0, c.n)
        self.n = sl.stop - sl.start
        self.stride = s = stride_of(self.n)
        host = dict(obs=padded(c.obs[..., sl], s, SENTINEL), start_obs=padded(c.start_obs[..., sl], s, SENTINEL),
                    advantages=padded(c.advantages[..., sl], s, SENTINEL), old_prob=padded(c.old_prob[..., sl], s, SENTINEL),
                    actions=padded(c.actions[..., sl], s, 9))
        self.host = host
        self.dev = {k: upload(v) for k, v in host.items()}
        if tables is None:
            tables = (filled((c.n_sets, ref.size_of(c.kind, c.hidden)), GRAD_FILL), filled((c.n_sets,), EXCLUDED_FILL), filled((c.n_sets, 2), COUNTS_FILL))
        self.grad, self.excluded, self.counts = tables
        self.prob = torch.full((max(c.steps, 1), s), SENTINEL, dtype=torch.int32, device=DEV)
        torch.cuda.synchronize()

    def args(self, with_prob=True, with_counts=True, **kw):
        c = self.c
        a = dict(record=dict(obs=self.dev["obs"].data_ptr(), actions=self.dev["actions"].data_ptr(), lane_stride=self.stride),
                 start_obs=self.dev["start_obs"].data_ptr(), advantages=self.dev["advantages"].data_ptr(), old_prob=self.dev["old_prob"].data_ptr(),
                 grad=self.grad.data_ptr(), excluded=self.excluded.data_ptr(), counts=self.counts.data_ptr() if with_counts else None,
                 prob=self.prob.data_ptr() if with_prob else None, clip_low=c.clip_low, clip_high=c.clip_high, scale=c.scale)
        a.update(kw)
        return a

    def inputs_unchanged(self):
        for k, v in self.dev.items():
            assert np.array_equal(v.cpu().numpy().view(np.uint8), self.host[k].view(np.uint8)), ("an input buffer was written", k)

    def tables(self):
        return tuple(t.cpu().numpy().view(np.uint64) for t in (self.grad, self.excluded, self.counts))

    def check(self, at, times=1, prob=True, counts=True, want=None):
        c = self.c
        want_g, want_e, want_n, want_p, _ = ref.reference(c) if want is None else want
        got_g, got_e, got_n = self.tables()
        with np.errstate(over="ignore"):
            exp_g = np.uint64(GRAD_FILL % (1 << 64)) + np.uint64(times) * want_g.view(np.uint64)
            exp_e = np.uint64(EXCLUDED_FILL) + np.uint64(times) * want_e
            exp_n = np.uint64(COUNTS_FILL) + np.uint64(times if counts else 0) * want_n
        bad = np.argwhere(got_g != exp_g)
        assert bad.size == 0, ("grad", at, len(bad), [(int(m), int(s), int(got_g[m, s]) - int(exp_g[m, s])) for m, s in bad[:4]])
        assert np.array_equal(got_e, exp_e), ("excluded", at, got_e - np.uint64(EXCLUDED_FILL), want_e)
        assert np.array_equal(got_n, exp_n), ("counts", at, got_n - np.uint64(COUNTS_FILL), want_n)
        got_p = self.prob.cpu().numpy().view(np.uint32)
        assert (got_p[:, c.n:] == SENTINEL).all(), ("padding lanes of prob written", at)
        if not prob:
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
    eng.set_policy(c.weights, hidden=c.hidden, lanes_per_policy=c.lanes_per_set)
    return eng


@pytest.mark.parametrize("kind,shape,hidden", ref.matrix())
def test_synthetic_cases_equal_the_cpu_reference(gymrs, kind, shape, hidden):
    """K = 1, 2, 7 on one engine per (env, shape, H)"""
    n, gid0, _, _ = ref.SHAPES[shape]
    eng = gymrs.BatchedEngine(kind, n, global_env_offset=gid0, flags=A | S | T)
    eng.reset(seed=3)
    for steps in ref.STEPS:
        c = ref.synthetic(kind, shape, steps, hidden)
        eng.set_policy(c.weights, hidden=c.hidden, lanes_per_policy=c.lanes_per_set)
        buf = Buffers(c)
        eng.ppo_gradient(steps, **buf.args())
        eng.sync()
        buf.check((kind, shape, hidden, steps))
    eng.close()


@pytest.mark.parametrize("kind,shape,hidden", [(0, 3, 0), (1, 4, 5), (0, 5, 64), (1, 2, 1), (0, 4, 5), (1, 3, 64)])
def test_the_fused_call_equals_the_composition_on_the_device(gymrs, kind, shape, hidden):
    """gymrs_policy_gradient writes prob (its table, fed a zero row, is discarded), the coefficient row is computed in numpy f32 by the rule,
    gymrs_policy_gradient runs again with it: grad and excluded are those of gymrs_ppo_gradient, and the counters are the rule's"""
    c = ref.synthetic(kind, shape, 7, hidden)
    eng = engine_for(gymrs, c)
    fused = Buffers(c)
    eng.ppo_gradient(c.steps, **fused.args())
    eng.sync()
    s = fused.stride
    zero = upload(np.zeros((c.steps, s), np.float32))
    scrap = (torch.zeros_like(fused.grad), torch.zeros_like(fused.excluded))
    prob = torch.full((c.steps, s), SENTINEL, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    common = dict(record=fused.args()["record"], start_obs=fused.dev["start_obs"].data_ptr(), scale=c.scale)
    eng.policy_gradient(c.steps, coef=zero.data_ptr(), grad=scrap[0].data_ptr(), excluded=scrap[1].data_ptr(), prob=prob.data_ptr(), **common)
    eng.sync()
    pa = prob.cpu().numpy().view(np.float32)[:, :c.n]
    assert np.array_equal(bits(pa), fused.prob.cpu().numpy().view(np.uint32)[:, :c.n])
    _, cut, coef, on = ref.rule(c, pa)
    composed = (filled(tuple(fused.grad.shape), GRAD_FILL), filled(tuple(fused.excluded.shape), EXCLUDED_FILL))
    row = upload(padded(coef, s, SENTINEL))
    eng.policy_gradient(c.steps, coef=row.data_ptr(), grad=composed[0].data_ptr(), excluded=composed[1].data_ptr(), **common)
    eng.sync()
    assert torch.equal(composed[0], fused.grad) and torch.equal(composed[1], fused.excluded)
    idx = ref.set_index(c)
    want = np.stack([np.bincount(idx, weights=m.sum(axis=0), minlength=c.n_sets) for m in (on, cut)], axis=1).astype(np.uint64)
    assert np.array_equal(fused.tables()[2] - np.uint64(COUNTS_FILL), want) and want[:, 1].any()
    eng.close()


@pytest.mark.parametrize("kind,hidden", [(0, 5), (1, 0)])
def test_calling_twice_adds_twice_and_counts_and_prob_are_optional(gymrs, kind, hidden):
    c = ref.synthetic(kind, 4, 7, hidden)
    eng = engine_for(gymrs, c)
    want = ref.reference(c)
    buf = Buffers(c)
    eng.ppo_gradient(c.steps, **buf.args(with_prob=False))
    eng.ppo_gradient(c.steps, **buf.args(with_prob=False))
    eng.sync()
    buf.check("twice", times=2, prob=False, want=want)
    buf = Buffers(c)
    eng.ppo_gradient(c.steps, **buf.args(with_counts=False))
    eng.sync()
    buf.check("no counts", counts=False, want=want)
    eng.close()


@pytest.mark.parametrize("kind,shape,hidden", [(0, 3, 7), (1, 4, 0)])
def test_the_chain_from_collection_to_the_clipped_gradient_without_a_sync_in_between(gymrs, kind, shape, hidden):
    """a real engine (A | S | T, 17-step episodes) collects with sampling, turns the record into advantages, records old_prob with
    gymrs_policy_gradient and takes the clipped gradient, four launches back to back.  The weights have not changed: every lane-step
    has ratio == 1 (old_prob > 0), nothing is cut and the table is gymrs_policy_gradient's with coef = the advantages.  Then the weights
    are perturbed in place through policy_weights_ptr and the call, made again, equals the CPU reference."""
    n, gid0, lps, n_sets = ref.SHAPES[shape]
    steps, d, s = 7, DIMS[kind][0], stride_of(n)
    eng = policy_engine(gymrs, kind, n, gid0, lps, hidden, A | S | T)
    policy = eng.get_policy()[0].copy()
    eng.set_critic(ref.gref.make_sets(kind, hidden, True, n_sets, 9), hidden=hidden, lanes_per_critic=lps)
    f32 = lambda *shape: torch.full(shape, SENTINEL, dtype=torch.int32, device=DEV)  # noqa: E731
    u8 = lambda *shape: torch.full(shape, 9, dtype=torch.uint8, device=DEV)  # noqa: E731
    obs, fin, start, rew, act, done, trunc = f32(steps, d, s), f32(steps, d, s), f32(d, s), f32(steps, s), u8(steps, s), u8(steps, s), u8(steps, s)
    adv, old, prob = f32(steps, s), f32(steps, s), f32(steps, s)
    size = ref.size_of(kind, hidden)
    plain, clipped, later = ((torch.zeros((n_sets, size), dtype=torch.int64, device=DEV), torch.zeros(n_sets, dtype=torch.int64, device=DEV),
                              torch.zeros((n_sets, 2), dtype=torch.int64, device=DEV)) for _ in range(3))
    torch.cuda.synchronize()
    record = dict(obs=obs.data_ptr(), actions=act.data_ptr(), reward=rew.data_ptr(), done=done.data_ptr(), truncated=trunc.data_ptr(), lane_stride=s)
    eng.rollout_transitions(steps, record=record, final_obs=fin.data_ptr(), start_obs=start.data_ptr(), sample=True)
    eng.advantages(steps, record=record, final_obs=fin.data_ptr(), start_obs=start.data_ptr(), advantages=adv.data_ptr(), gamma=0.97, lam=0.9, critic=True)
    eng.policy_gradient(steps, record=record, start_obs=start.data_ptr(), coef=adv.data_ptr(), grad=plain[0].data_ptr(), excluded=plain[1].data_ptr(),
                        prob=old.data_ptr(), temperature=8.0)
    eng.ppo_gradient(steps, record=record, start_obs=start.data_ptr(), advantages=adv.data_ptr(), old_prob=old.data_ptr(), grad=clipped[0].data_ptr(),
                     excluded=clipped[1].data_ptr(), counts=clipped[2].data_ptr(), prob=prob.data_ptr(), clip=0.2, temperature=8.0)
    eng.sync()
    host = lambda t: t.cpu().numpy()[..., :n]  # noqa: E731
    old_host = host(old).view(np.float32)
    assert (old_host > 0).all() and np.array_equal(host(prob), host(old))
    assert torch.equal(clipped[0], plain[0]) and torch.equal(clipped[1], plain[1]) and plain[0].any() and not plain[1].any()
    counts = clipped[2].cpu().numpy()
    assert not counts[:, 1].any() and counts[:, 0].sum() == steps * n
    # perturb the weights in place, on the device
    ptr, floats = eng.policy_weights_ptr()
    assert floats == n_sets * size
    rng = np.random.default_rng(5)
    moved = (policy + 4.0 * rng.standard_normal(policy.shape)).astype(np.float32)  # at temperature 8: ratios well beyond 0.8 .. 1.2
    table = torch.as_tensor(_Floats(ptr, floats), device=DEV)
    table.copy_(torch.from_numpy(moved.reshape(-1)).to(DEV))
    torch.cuda.synchronize()
    eng.ppo_gradient(steps, record=record, start_obs=start.data_ptr(), advantages=adv.data_ptr(), old_prob=old.data_ptr(), grad=later[0].data_ptr(),
                     excluded=later[1].data_ptr(), counts=later[2].data_ptr(), prob=prob.data_ptr(), clip=0.2, temperature=8.0)
    eng.sync()
    c = ref.synthetic(kind, shape, steps, hidden, specials=False, boundary=False)  # the shape's keys; the record replaces its arrays
    c.weights, c.scale = moved, float(np.float32(1.4426950408889634 / 8.0))
    c.clip_low, c.clip_high = float(np.float32(1 - 0.2)), float(np.float32(1 + 0.2))
    c.obs, c.start_obs, c.advantages = (host(t).view(np.float32) for t in (obs, start, adv))
    c.old_prob, c.actions = old_host, host(act)
    assert np.isfinite(c.advantages).all() and c.advantages.any() and (c.actions < DIMS[kind][1]).all()
    want_g, want_e, want_n, want_p, _ = ref.reference(c)
    assert np.array_equal(later[0].cpu().numpy(), want_g) and want_g.any()
    assert np.array_equal(later[1].cpu().numpy().view(np.uint64), want_e) and not want_e.any()
    assert np.array_equal(later[2].cpu().numpy().view(np.uint64), want_n) and want_n[:, 1].any() and (want_n[:, 1] < want_n[:, 0]).all()
    got = prob.cpu().numpy().view(np.uint32)
    assert np.array_equal(got[:, :n], bits(want_p)) and (got[:, n:] == SENTINEL).all()
    eng.close()


class _Floats:
    """n floats at a device address, for torch.as_tensor (zero-copy)"""

    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": "<f4", "data": (ptr, False), "version": 3}


@pytest.mark.parametrize("kind,shape,hidden", [(0, 3, 5), (1, 4, 0)])
def test_two_engines_adding_into_the_same_tables_equal_one(gymrs, kind, shape, hidden):
    c = ref.synthetic(kind, shape, 7, hidden)
    cut = 1999  # the second block starts at an odd lane: its work-items straddle what the whole batch's do not
    first = Buffers(c, slice(0, cut))
    second = Buffers(c, slice(cut, c.n), tables=(first.grad, first.excluded, first.counts))
    engines = [engine_for(gymrs, c, slice(0, cut)), engine_for(gymrs, c, slice(cut, c.n))]
    for eng, buf in zip(engines, (first, second)):
        eng.ppo_gradient(c.steps, **buf.args(with_prob=False))
    for eng in engines:
        eng.sync()
    want_g, want_e, want_n, _, _ = ref.reference(c)
    got_g, got_e, got_n = first.tables()
    with np.errstate(over="ignore"):
        assert np.array_equal(got_g, np.uint64(GRAD_FILL % (1 << 64)) + want_g.view(np.uint64))
        assert np.array_equal(got_e, np.uint64(EXCLUDED_FILL) + want_e)
        assert np.array_equal(got_n, np.uint64(COUNTS_FILL) + want_n)
    for eng in engines:
        eng.close()


@pytest.mark.parametrize("kind", [0, 1])
def test_the_engine_and_the_inputs_are_untouched(gymrs, kind):
    c = ref.synthetic(kind, 2, 7, 8)
    eng = policy_engine(gymrs, kind, c.n, c.gid0, c.lanes_per_set, 8, A | S | T)
    eng.set_critic(ref.gref.make_sets(kind, 5, True, c.n_sets, 4), hidden=5, lanes_per_critic=c.lanes_per_set)
    eng.set_policy(c.weights, hidden=8, lanes_per_policy=c.lanes_per_set)
    eng.rollout_policy_fitness(20)
    eng.sync()
    before = eng.snapshot(), eng.tick(), eng.stats().copy(), eng.policy_fitness().copy(), eng.get_policy()[0].copy(), eng.critic()[0].copy()
    buf = Buffers(c)
    eng.ppo_gradient(c.steps, **buf.args())
    eng.sync()
    buf.check("untouched")
    after = eng.snapshot(), eng.tick(), eng.stats(), eng.policy_fitness(), eng.get_policy()[0], eng.critic()[0]
    assert before[0] == after[0] and before[1] == after[1]
    for a, b in zip(before[2:], after[2:]):
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))
    # n_steps = 0 adds and writes nothing
    buf = Buffers(c)
    eng.ppo_gradient(0, **buf.args())
    eng.sync()
    got = buf.tables()
    assert (got[0] == np.uint64(GRAD_FILL % (1 << 64))).all() and (got[1] == np.uint64(EXCLUDED_FILL)).all() and (got[2] == np.uint64(COUNTS_FILL)).all()
    assert (buf.prob.cpu().numpy().view(np.uint32) == SENTINEL).all()
    buf.inputs_unchanged()
    eng.close()


def test_refusals(gymrs):
    c = ref.synthetic(0, 2, 2, 0)
    eng = engine_for(gymrs, c)
    buf = Buffers(c)
    before = eng.snapshot(), eng.tick()

    def refused(match, eng=eng, steps=2, **kw):
        args = buf.args(**kw)
        if "temperature" in kw:
            args.pop("scale", None)
        with pytest.raises(gymrs.GymrsError, match=match) as err:
            eng.ppo_gradient(steps, **args)
        assert err.value.status == EINVAL and "gymrs_ppo_gradient" in str(err.value)

    def record(**kw):
        r = dict(buf.args()["record"])
        r.update(kw)
        return r

    nan, inf = float("nan"), float("inf")
    refused("flag", flags=1)
    refused("flag", flags=2)
    for bad in (nan, -0.5, inf):
        refused("scale", scale=bad)
    for low, high in ((nan, 1.2), (0.8, nan), (-0.1, 1.2), (1.1, 1.2), (0.8, 0.9), (0.8, inf), (-inf, 1.2)):
        refused("clip", clip_low=low, clip_high=high)
    refused("record.obs", record=record(obs=0))
    refused("record.actions", record=record(actions=0))
    refused("start_obs", start_obs=0)
    refused("advantages is NULL", advantages=0)
    refused("old_prob is NULL", old_prob=0)
    refused("grad is NULL", grad=0)
    refused("excluded is NULL", excluded=0)
    refused("alias", prob=buf.dev["old_prob"].data_ptr())
    for name in ("start_obs", "advantages", "old_prob"):
        refused("16-byte aligned", **{name: buf.dev[name].data_ptr() + 4})
    refused("16-byte aligned", prob=buf.prob.data_ptr() + 8)
    for name in ("obs", "actions"):
        refused("16-byte aligned", record=record(**{name: buf.dev[name].data_ptr() + 8}))
    refused("8-byte aligned", grad=buf.grad.data_ptr() + 4)
    refused("8-byte aligned", excluded=buf.excluded.data_ptr() + 4)
    refused("8-byte aligned", counts=buf.counts.data_ptr() + 4)
    refused("lane_stride", record=record(lane_stride=c.n - 1 - (c.n - 1) % 16))
    refused("lane_stride", record=record(lane_stride=buf.stride + 8))
    lib = eng._lib
    traj = gymrs.engine.Trajectory(buf.dev["obs"].data_ptr(), buf.dev["actions"].data_ptr(), None, None, None, buf.stride)

    def desc(**kw):
        d = gymrs.PpoDesc(2, 0, c.scale, c.clip_low, c.clip_high, 0, traj, buf.dev["start_obs"].data_ptr(), buf.dev["advantages"].data_ptr(),
                          buf.dev["old_prob"].data_ptr(), None, buf.grad.data_ptr(), buf.excluded.data_ptr(), None, 0)
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    for d, word in ((desc(reserved=1), b"reserved"), (desc(pad_=1), b"pad_")):
        assert lib.gymrs_ppo_gradient(eng._h, C.byref(d)) == EINVAL and word in lib.gymrs_last_error()
    assert lib.gymrs_ppo_gradient(None, C.byref(desc())) == EINVAL and lib.gymrs_ppo_gradient(eng._h, None) == EINVAL
    # nothing was added so far
    eng.sync()
    got = buf.tables()
    assert (got[0] == np.uint64(GRAD_FILL % (1 << 64))).all() and (got[2] == np.uint64(COUNTS_FILL)).all()
    assert (buf.prob.cpu().numpy().view(np.uint32) == SENTINEL).all()
    d = desc()
    assert lib.gymrs_ppo_gradient(eng._h, C.byref(d)) == 0  # the minimal descriptor: no reward, done, truncated, prob, counts
    eng.sync()
    buf.check("minimal", prob=False, counts=False)
    # no policy
    eng.set_policy(None)
    refused("gymrs_set_policy")
    assert eng.snapshot() == before[0] and eng.tick() == before[1]
    eng.close()
    pend = gymrs.BatchedEngine(gymrs.PENDULUM, 256, flags=A | T)
    pend.reset(seed=1)
    refused("Pendulum", eng=pend)
    pend.close()
