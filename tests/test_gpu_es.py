"""gymrs_es_init / gymrs_es_step on the device against the numpy restatement of tests/test_es_host.py and tests/optimizer_ref.py, bit for
bit: the rule of include/gymrs_amd.h, "Evolution strategies", is defined to the bit, so nothing here has a tolerance.  The shapes meet
every path of the kernels: S = 9 / 10 (one slot per work-item of the update, many pairs per tile), 45 / 51, 387 / 450 (two slots, the
norm's eight terms per lane, a few pairs per tile); P = 2 (one pair: a ragged wave, a tail of the 16-byte stores), 130 (a ragged wave
in a full block's worth of lanes) and 1026 (a second chunk of the utilities with two policies, a third block of the gradient).  The
reference is fed the evaluation records read from the device: the evaluator has its own tests.  MountainCar never ends within 32
steps, so its table gives equal returns (sd = 0: every utility +0.0f); its second generation takes the caller's utilities instead."""
import ctypes as C

import numpy as np
import optimizer_ref as opt
import pytest
import test_es_host as es
import torch
from test_es_host import bits
from test_gpu_advantages import upload
from test_gpu_closed_loop_table import DEV
from test_gpu_ppo import _Floats

pytestmark = pytest.mark.gpu
EINVAL = 1
SEED, SIGMA, MAX_NORM = 0x1234567890ABCDEF, 0.125, 0.5
HYPER = dict(lr=0.05, beta1=0.9, beta2=0.999, eps=1e-8)
# kind, hidden, P, Adam with the clip (else SGD), what is special
CASES = [(0, 0, 2, False, ""), (1, 0, 130, True, ""), (0, 7, 1026, True, ""), (1, 7, 2, False, ""), (0, 64, 130, True, ""), (1, 64, 1026, False, ""),
         (0, 7, 130, True, "fewer lanes"), (0, 0, 130, True, "bad utilities"), (0, 64, 1026, False, "sigma_next")]


def device_floats(view):
    return torch.as_tensor(_Floats(*view), device=DEV).cpu().numpy()


def assert_state(eng, state, population, generation):
    got = dict(w=eng.es_state()["centre"], view=device_floats(eng.es_centre_ptr()), population=eng.get_policy()[0])
    got["m"], got["v"], got["pw"] = eng.es_optimizer_state()
    want = dict(w=state["w"][0], view=state["w"][0], m=state["m"][0], v=state["v"][0], pw=state["pw"][0], population=population)
    assert eng.es_state(centre=False)["generation"] == generation
    for name, w in want.items():
        assert np.array_equal(bits(got[name]), bits(w)), (name, generation, np.argwhere(bits(got[name]) != bits(w))[:4])


@pytest.mark.parametrize("kind,hidden,P,adam,special", CASES)
def test_two_generations_equal_the_reference(gymrs, kind, hidden, P, adam, special):
    S = gymrs.policy_size(kind, hidden)  # 10, 51, 450 (CartPole); 9, 45, 387 (MountainCar)
    rng = np.random.default_rng([kind, hidden, P])
    theta = (rng.standard_normal(S) * 0.5).astype(np.float32)
    missing = 40 if special == "fewer lanes" else 0  # policies without a lane: no episode
    eng = gymrs.BatchedEngine(kind, P - missing, flags=7)
    eng.reset(seed=3)
    eng.es_init(theta, n_policies=P, sigma=SIGMA, seed=SEED, hidden=hidden)
    state = dict(w=theta[None], m=np.zeros((1, S), np.float32), v=np.zeros((1, S), np.float32), pw=np.ones((1, 2), np.float32))
    sigma, max_norm = SIGMA, MAX_NORM if adam else np.inf
    skipped, n_skipped = upload(np.full(1, 5, np.int64)), 5  # ADDED to
    assert_state(eng, state, es.population(theta, sigma, SEED, 0, P), 0)
    for gen in (0, 1):
        eng.evaluate_policy(1, max_episode_steps=32, seed=gen)
        row, u = None, None
        if (special == "bad utilities" and gen == 0) or (kind == 1 and gen == 1):
            u = rng.standard_normal(P).astype(np.float32)
            if special:
                u[3], u[P - 1] = np.nan, np.inf
            row = upload(u)
        sigma_next = 0.25 if special == "sigma_next" and gen == 0 else 0.0
        grad_scale = 2.0**-24 / (P * sigma)
        eng.es_step(adam=adam, max_norm=max_norm, grad_scale=grad_scale, sigma_next=sigma_next, skipped=skipped.data_ptr(),
                    utilities=None if row is None else row.data_ptr(), **HYPER)
        eng.sync()
        if row is None:
            records = eng.policy_eval()
            u = es.utilities(records)
            assert (records[:P - missing, 2] == 1).all() and not records[P - missing:, 2].any() and not bits(u[P - missing:]).any()
            assert P == 2 or (len(np.unique(u)) > 1) == (kind == 0)  # CartPole's returns differ, MountainCar's are all -32
        G, excluded = es.gradient(u, SEED, gen, S)
        state = opt.apply(G[None], np.array([excluded], np.uint64), state["w"], state["m"], state["v"], state["pw"], np.zeros((1, S), np.float32),
                          kind=opt.ADAM if adam else opt.SGD, grad_scale=grad_scale, max_norm=max_norm, ascend=True, **HYPER)
        n_skipped += state["skipped"]
        sigma = sigma_next or sigma
        assert np.array_equal(bits(device_floats(eng.es_utilities_ptr())), bits(u))
        assert_state(eng, state, es.population(state["w"][0], sigma, SEED, gen + 1, P), gen + 1)  # written on a skipped step too
        assert int(skipped.cpu()[0]) == n_skipped
        if special == "bad utilities" and gen == 0:
            assert excluded > 0 and state["skipped"] == 1 and np.array_equal(bits(state["w"][0]), bits(theta))
        elif adam and kind == 0:
            assert state["clipped"].all()
    assert eng.es_state(centre=False)["sigma"] == sigma and not np.array_equal(bits(state["w"][0]), bits(theta))
    eng.close()


NAN, INF = float("nan"), float("inf")
REFUSALS = [("init", dict(n_policies=3), "n_policies"), ("init", dict(n_policies=0), "n_policies"), ("init", dict(n_policies=2**20 + 2), "n_policies"),
            ("init", dict(lanes_per_policy=0), "lanes_per_policy"), ("init", dict(sigma=0.0), "sigma"), ("init", dict(sigma=NAN), "sigma"),
            ("init", dict(sigma=INF), "sigma"), ("init", dict(hidden=65), "hidden"), ("init", dict(reserved=1), "reserved"),
            ("pendulum init", {}, "Pendulum"), ("step", dict(kind=2), "kind"), ("step", dict(flags=2), "flag"), ("step", dict(reserved=1), "reserved"),
            ("step", dict(lr=NAN), "lr"), ("step", dict(grad_scale=INF), "grad_scale"), ("step", dict(beta1=1.0), "beta1"), ("step", dict(eps=-1.0), "eps"),
            ("step", dict(max_norm=0.0), "max_norm"), ("step", dict(sigma_next=-1.0), "sigma_next"), ("step", dict(sigma_next=NAN), "sigma_next"),
            ("step", dict(sigma_next=INF), "sigma_next"), ("step", dict(utilities=2), "4-byte aligned"), ("step", dict(skipped=4), "8-byte aligned"),
            ("step", {}, "gymrs_evaluate_policy"), ("pendulum step", {}, "Pendulum"), ("no state step", {}, "gymrs_es_init"),
            ("NULL engine", {}, "NULL engine"), ("NULL desc", {}, "NULL desc")]


@pytest.mark.parametrize("call,bad,cause", REFUSALS)
def test_refusals(gymrs, call, bad, cause):
    pendulum = "pendulum" in call
    eng = gymrs.BatchedEngine(gymrs.PENDULUM if pendulum else gymrs.CARTPOLE, 64, flags=5 if pendulum else 7)
    eng.reset(seed=1)
    theta, has_state = np.linspace(-1, 1, 10, dtype=np.float32), call in ("init", "step")
    if has_state:
        eng.es_init(theta, n_policies=4, sigma=SIGMA, seed=SEED)
        before = (eng.es_state(), eng.get_policy()[0], eng.es_optimizer_state())
    buf = torch.ones(4, dtype=torch.int64, device=DEV)
    torch.cuda.synchronize()
    lib, name = eng._lib, "gymrs_es_init" if "init" in call else "gymrs_es_step"
    if call in ("NULL engine", "NULL desc"):
        desc = gymrs.EsStepDesc(0, 1, 0.1, 1.0, 0.9, 0.999, 1e-8, INF, 0.0, 0, None, None)
        status = lib.gymrs_es_step(None if call == "NULL engine" else eng._h, None if call == "NULL desc" else C.byref(desc))
        assert status == EINVAL and cause.encode() in lib.gymrs_last_error() and name.encode() in lib.gymrs_last_error()
    else:
        with pytest.raises(gymrs.GymrsError, match=cause) as err:
            if "init" in call:
                eng.es_init(theta, **{**dict(n_policies=4, sigma=SIGMA, seed=1), **bad})
            else:
                args = {**dict(lr=0.1, grad_scale=1.0, skipped=0), **bad}
                eng.es_step(**{k: (buf.data_ptr() + v if k in ("utilities", "skipped") else v) for k, v in args.items()})
        assert err.value.status == EINVAL and name in str(err.value)
    eng.sync()
    assert (buf.cpu() == 1).all()  # a refused call touched nothing
    if has_state:
        after = (eng.es_state(), eng.get_policy()[0], eng.es_optimizer_state())
        assert before[0].pop("centre").tobytes() == after[0].pop("centre").tobytes() and before[0] == after[0]
        assert before[1].tobytes() == after[1].tobytes() and all(b.tobytes() == a.tobytes() for b, a in zip(before[2], after[2]))
    eng.close()
