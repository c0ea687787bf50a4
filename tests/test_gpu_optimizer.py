"""gymrs_apply_gradient on the device against the plain numpy restatement of tests/optimizer_ref.py, bit for bit: the rule of
include/gymrs_amd.h, "Optimizer", is defined to the bit, so nothing here has a tolerance.  The shapes meet every copy of the kernel:
S = 9 and 10 (a group of 16 lanes, four sets per wave), 114 (two slots per lane, ragged), 385 (the critic's: eight slots, the last
with one lane) and 450 (eight slots, a tail of two); n_sets = 1 (a lone group in a wave), 3 (a partly filled wave) and 67 (more than
one block with a ragged last one).  Every case is three consecutive calls, each with a table of its own: q uniform in +-2^40 with 0,
+-1 and +-2^62 planted in one set (which therefore clips; no other does at MAX_NORM), another set excluded, a -0.0f weight on top.

grad_scale is 2^-24 / 4096 = 2^-36, under which no integer q gives a denormal g (the smallest is 2^-36); the denormal has a test of
its own with a smaller scale, through the same run()."""
import ctypes as C
import functools
import itertools

import numpy as np
import optimizer_ref as ref
import pytest
import q_ref
import torch
from test_gpu_advantages import upload
from test_gpu_closed_loop_table import DEV
from test_gpu_ppo import _Floats
from test_gpu_q_gradient import Buffers, engine_for

pytestmark = pytest.mark.gpu
EINVAL = 1
GRAD_SCALE = 2.0**-24 / 4096
MAX_NORM = 1000.0
HYPER = dict(lr=0.01, beta1=0.9, beta2=0.999, eps=1e-8)
NETS = {9: (1, 0, False), 10: (0, 0, False), 114: (0, 16, False), 450: (0, 64, False), 385: (0, 64, True)}  # S: kind, hidden, the critic head
# S, n_sets, kind, max_norm, zero_grad, tau (the critic head has no target)
CASES = [c for c in itertools.product(NETS, (1, 3, 67), (ref.SGD, ref.ADAM), (np.inf, MAX_NORM), (False, True), (0.0, 0.25)) if not (NETS[c[0]][2] and c[5])]
assert len(CASES) == 4 * 3 * 2 * 2 * 2 * 2 + 3 * 2 * 2 * 2  # no case is dropped


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def tables(S, n_sets):
    """the weights, the target and the three calls' (q, excluded)"""
    rng = np.random.default_rng([S, n_sets])
    w, target = (rng.standard_normal((n_sets, S)).astype(np.float32) for _ in range(2))
    w[:, 0] = -0.0  # in the planted set under q = 0
    calls = []
    for call in range(3):
        q = rng.integers(-(1 << 40), (1 << 40) + 1, (n_sets, S), dtype=np.int64)
        q[call % n_sets, :5] = (0, 1, -1, 1 << 62, -(1 << 62))
        excluded = np.zeros(n_sets, np.uint64)
        if n_sets > 1 or call == 0:  # (a lone set is skipped once, then stepped twice)
            excluded[(call + 1) % n_sets] = 1
        calls.append((q, excluded))
    return w, target, calls


@functools.lru_cache(maxsize=None)
def expected(S, n_sets, kind, max_norm, zero_grad, tau, grad_scale):
    w, target, calls = tables(S, n_sets)
    state = dict(w=w, m=np.zeros_like(w), v=np.zeros_like(w), pw=np.ones((n_sets, 2), np.float32), target=target)
    out = []
    for q, excluded in calls:
        state = ref.apply(q, excluded, *(state[k] for k in ("w", "m", "v", "pw", "target")), kind=kind, grad_scale=grad_scale, max_norm=max_norm,
                          zero_grad=zero_grad, tau=tau, ascend=not NETS[S][2], **HYPER)
        if max_norm < np.inf and n_sets > 1:  # the reference alone: both sides of the clip among the sets that are stepped
            assert state["clipped"].any() and (~state["clipped"] & (excluded == 0)).any()
        out.append(state)
    return out


def run(gymrs, S, n_sets, kind, max_norm, zero_grad, tau, grad_scale=GRAD_SCALE):
    want = expected(S, n_sets, kind, max_norm, zero_grad, tau, grad_scale)  # and its checks of the inputs, before anything reaches the GPU
    env, hidden, critic = NETS[S]
    w, target, calls = tables(S, n_sets)
    eng = gymrs.BatchedEngine(env, 64, flags=7)
    eng.reset(seed=3)
    if critic:
        eng.set_critic(w, hidden=hidden, lanes_per_critic=1)
    else:
        if tau:
            eng.set_policy(target, hidden=hidden, lanes_per_policy=1)
            eng.q_target_sync()
        eng.set_policy(w, hidden=hidden, lanes_per_policy=1)
    skipped, n_skipped = upload(np.full(1, 5, np.int64)), 5  # ADDED to
    for call, ((q, excluded), exp) in enumerate(zip(calls, want)):
        grad, excl = upload(q), upload(excluded.view(np.int64))
        eng.apply_gradient(grad=grad.data_ptr(), excluded=excl.data_ptr(), skipped=skipped.data_ptr(), critic=critic, adam=kind == ref.ADAM,
                           grad_scale=grad_scale, max_norm=max_norm, tau=tau, ascend=not critic, zero_grad=zero_grad, **HYPER)
        eng.sync()
        n_skipped += exp["skipped"]
        got = dict(w=(eng.critic() if critic else eng.get_policy())[0])
        if kind == ref.ADAM:
            got["m"], got["v"], got["pw"] = eng.optimizer_state(critic)
        if tau:
            got["target"] = torch.as_tensor(_Floats(*eng.q_target_ptr()), device=DEV).cpu().numpy().reshape(n_sets, S)
        for name, g in got.items():
            assert np.array_equal(bits(g), bits(exp[name])), (name, call, np.argwhere(bits(g) != bits(exp[name]))[:4])
        assert np.array_equal(grad.cpu().numpy(), exp["grad"]) and np.array_equal(excl.cpu().numpy().view(np.uint64), exp["excluded"]), call
        assert int(skipped.cpu()[0]) == n_skipped, call
    if kind == ref.SGD:  # SGD allocates no state
        with pytest.raises(gymrs.GymrsError, match="no optimizer state"):
            eng.optimizer_state(critic)
    eng.close()


@pytest.mark.parametrize("S,n_sets,kind,max_norm,zero_grad,tau", CASES)
def test_three_calls_equal_the_reference(gymrs, S, n_sets, kind, max_norm, zero_grad, tau):
    run(gymrs, S, n_sets, kind, max_norm, zero_grad, tau)


@pytest.mark.parametrize("kind", [ref.SGD, ref.ADAM])
def test_denormal_gradients(gymrs, kind):
    """2^-140 takes q = +-1 to an f32 denormal and most of the table below 2^-100: g * g underflows, and the norm is far below MAX_NORM"""
    scale = 2.0**-140
    assert 0 < abs(float(ref.gradient(np.int64(1), scale))) < 2.0**-126
    run(gymrs, 10, 3, kind, np.inf, True, 0.25, grad_scale=scale)


def test_stream_order(gymrs):
    """q_gradient -> apply_gradient -> q_gradient with nothing in between equals the same calls with a sync after each"""
    c = q_ref.synthetic(0, 3, 7, 5, 0, 0.97, 1.0)
    results = []
    for synced in (False, True):
        shapes = dict(grad=(c.n_sets, q_ref.size_of(c.kind, c.hidden)), excluded=(c.n_sets,), counts=(c.n_sets, 2))
        eng, buf = engine_for(gymrs, c), Buffers(c, tables={k: torch.zeros(s, dtype=torch.int64, device=DEV) for k, s in shapes.items()})
        skipped = torch.zeros(1, dtype=torch.int64, device=DEV)
        torch.cuda.synchronize()
        t = buf.tables
        for step in (0, 1, 2):
            if step == 1:
                eng.apply_gradient(grad=t["grad"].data_ptr(), excluded=t["excluded"].data_ptr(), skipped=skipped.data_ptr(), adam=True, max_norm=0.5,
                                   grad_scale=2.0**-24 / (c.steps * c.n), tau=0.25, zero_grad=True, **HYPER)
            else:
                eng.q_gradient(c.steps, **buf.args())
            if synced:
                eng.sync()
        eng.sync()
        results.append([t[k].cpu().numpy() for k in shapes] + [buf.td.cpu().numpy(), skipped.cpu().numpy(), bits(eng.get_policy()[0])] +
                       [bits(a) for a in eng.optimizer_state()] + [torch.as_tensor(_Floats(*eng.q_target_ptr()), device=DEV).cpu().numpy().view(np.uint32)])
        eng.close()
    assert all(np.array_equal(a, b) for a, b in zip(*results))
    assert results[0][0].any() and not np.array_equal(results[0][5], bits(c.weights))  # a gradient of the NEW weights, which moved


REFUSALS = [("", dict(grad=0), "grad is NULL"), ("", dict(excluded=0), "excluded is NULL"), ("", dict(head=2), "head"), ("", dict(kind=2), "kind"),
            ("", dict(flags=4), "flag"), ("", dict(critic=True), "gymrs_set_critic"), ("", dict(lr=np.nan), "lr"), ("", dict(lr=np.inf), "lr"),
            ("", dict(grad_scale=np.nan), "grad_scale"), ("", dict(grad_scale=-np.inf), "grad_scale"), ("", dict(eps=np.inf), "eps"),
            ("", dict(eps=np.nan), "eps"), ("", dict(eps=-1.0), "eps"), ("", dict(beta1=1.0), "beta1"), ("", dict(beta1=-0.1), "beta1"),
            ("", dict(beta2=np.nan), "beta2"), ("", dict(beta2=1.5), "beta2"), ("", dict(max_norm=0.0), "max_norm"), ("", dict(max_norm=np.nan), "max_norm"),
            ("", dict(max_norm=-1.0), "max_norm"), ("", dict(tau=-0.1), "tau"), ("", dict(tau=1.5), "tau"), ("", dict(tau=np.nan), "tau"),
            ("", dict(tau=0.5), "gymrs_q_target_sync"), ("critic", dict(tau=0.5, critic=True), "policy head"), ("", dict(grad=4), "8-byte aligned"),
            ("", dict(excluded=4), "8-byte aligned"), ("", dict(skipped=4), "8-byte aligned"), ("no policy", {}, "gymrs_set_policy"),
            ("pendulum", {}, "Pendulum"), ("reserved", {}, "reserved"), ("NULL engine", {}, "NULL engine"), ("NULL desc", {}, "NULL desc")]


@pytest.mark.parametrize("setup,bad,cause", REFUSALS)
def test_refusals(gymrs, setup, bad, cause):
    eng = gymrs.BatchedEngine(gymrs.PENDULUM if setup == "pendulum" else gymrs.CARTPOLE, 64, flags=5 if setup == "pendulum" else 7)
    eng.reset(seed=1)
    w = np.ones((3, 10), np.float32)
    if setup not in ("pendulum", "no policy"):
        eng.set_policy(w, hidden=0, lanes_per_policy=1)
    if setup == "critic":
        eng.set_critic(np.ones((3, 5), np.float32), hidden=0, lanes_per_critic=1)
    grad, excluded, skipped = (torch.ones(n, dtype=torch.int64, device=DEV) for n in (32, 4, 2))
    torch.cuda.synchronize()
    args = dict(grad=grad.data_ptr(), excluded=excluded.data_ptr(), skipped=skipped.data_ptr(), lr=0.1, grad_scale=1.0, adam=True)
    args.update({k: (args[k] + v if k in ("grad", "excluded", "skipped") and v else v) for k, v in bad.items()})
    lib, desc = eng._lib, gymrs.OptimizerDesc(0, 0, 0, 0.1, 1.0, 0.9, 0.999, 1e-8, np.inf, 0.0, grad.data_ptr(), excluded.data_ptr(), None, setup == "reserved")
    if setup in ("reserved", "NULL engine", "NULL desc"):
        status = lib.gymrs_apply_gradient(None if setup == "NULL engine" else eng._h, None if setup == "NULL desc" else C.byref(desc))
        assert status == EINVAL and cause.encode() in lib.gymrs_last_error() and b"gymrs_apply_gradient" in lib.gymrs_last_error()
    else:
        with pytest.raises(gymrs.GymrsError, match=cause) as err:
            eng.apply_gradient(**args)
        assert err.value.status == EINVAL and "gymrs_apply_gradient" in str(err.value)
    eng.sync()
    assert (grad.cpu() == 1).all() and (excluded.cpu() == 1).all() and (skipped.cpu() == 1).all()  # a refused call touched nothing
    if setup not in ("pendulum", "no policy"):
        assert np.array_equal(eng.get_policy()[0], w)
    eng.close()
