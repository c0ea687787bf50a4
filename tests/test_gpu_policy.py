"""Closed-loop rollouts (gymrs_set_policy / gymrs_policy_actions / gymrs_rollout_policy / _record) against a yardstick that does not
share code with them: the CPU f32 twin (oracle.bindings.TwinEngine) stepped with actions the TEST computes from the twin's
observations by its own restatement of the policy, tests/cpp/policy_ref.c (plain C, libm's fmaf, gcc -O2 -ffp-contract=off).
fmaf is correctly rounded and so is v_fma_f32: every comparison is bit for bit, no tolerance and no skipped lanes."""
import time

import closed_loop_ref
import numpy as np
import pytest
import torch
from closed_loop_ref import make_weights

from oracle.bindings import TwinEngine

pytestmark = pytest.mark.gpu

A, S, T, F = 1, 2, 4, 8
DIMS = {0: (4, 2), 1: (2, 3)}  # kind -> (observation size, number of actions)
SETS = [(1, 1), (7, 1), (5, 3), (4, 256), (3, 1024), (2, 10**6)]  # (n_policies, lanes_per_policy)
DEV = "cuda:0"


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def policy_ref():
    return closed_loop_ref.policy_ref  # (kind, hidden, weights, lanes_per_policy, gid0, obs) -> actions; built from cpp/policy_ref.c


def gpu_actions(eng, buf):
    eng.policy_actions(buf.data_ptr())
    eng.sync()
    return buf.cpu().numpy()


# ---- 1. gymrs_policy_actions == policy_ref on the engine's observations ------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("n", [777, 5000])
@pytest.mark.parametrize("vec", [4, 8])
def test_policy_actions_equal_the_reference(gymrs, policy_ref, kind, n, vec):
    gid0 = 12345
    eng = gymrs.BatchedEngine(kind, n, global_env_offset=gid0, flags=A, lanes_per_thread=vec)
    eng.reset(seed=21)
    buf = torch.zeros(n, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    obs = eng.get_obs()
    for hidden in (0, 1, 8, 64):
        for p, lpp in SETS:
            w = make_weights(kind, hidden, p, seed=100 * hidden + p)
            eng.set_policy(w, hidden=hidden, lanes_per_policy=lpp)
            got = gpu_actions(eng, buf)
            want = policy_ref(kind, hidden, w, lpp, gid0, obs)
            assert np.array_equal(got, want), (hidden, p, lpp, np.flatnonzero(got != want)[:8])
    eng.close()


@pytest.mark.parametrize("kind", [0, 1])
def test_policy_actions_with_non_finite_states_and_weights(gymrs, policy_ref, kind):
    n, gid0 = 5000, 12345
    d, a = DIMS[kind]
    eng = gymrs.BatchedEngine(kind, n, global_env_offset=gid0, flags=0)
    eng.reset(seed=22)
    buf = torch.zeros(n, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    rng = np.random.default_rng(5)
    st = eng.get_state()
    special = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, 0.0, -0.0, 1e-40], np.float32)
    mask = rng.random(st.shape) < 0.3
    st[mask] = rng.choice(special, size=int(mask.sum()))
    eng.set_state(st)
    assert np.array_equal(bits(eng.get_obs()), bits(st))
    for hidden in (0, 8):
        for p, lpp in ((5, 3), (3, 1024)):
            w = make_weights(kind, hidden, p, seed=7)
            for weird in (False, True):
                if weird:  # NaN and inf weights are legal: the definition says what they do
                    wm = rng.random(w.shape) < 0.1
                    w = w.copy()
                    w[wm] = rng.choice(np.array([np.nan, np.inf, -np.inf, -0.0], np.float32), size=int(wm.sum()))
                eng.set_policy(w, hidden=hidden, lanes_per_policy=lpp)
                got = gpu_actions(eng, buf)
                want = policy_ref(kind, hidden, w, lpp, gid0, st)
                assert np.array_equal(got, want), (hidden, p, lpp, weird)
                assert got.max() < a
    eng.close()


# ---- 2. gymrs_rollout_policy == the twin stepped with the reference's actions ------------------------------------------------
def assert_same(eng, tw, kind, flags):  # as tests/test_gpu_rollout.py
    assert np.array_equal(eng.get_state().view(np.uint32), tw.get_state().view(np.uint32))
    assert np.array_equal(eng.get_obs().view(np.uint32), tw.get_obs().view(np.uint32))
    gr, gd, gt = eng.get_step_result()
    tr, td, tt = tw.get_result()
    assert np.array_equal(gr.view(np.uint32), tr.view(np.uint32))
    assert np.array_equal(gd, td)
    if flags & T:
        assert np.array_equal(gt, tt)
    gs, ts = eng.stats(), tw.stats()
    assert np.array_equal(gs[1:], ts[1:])
    assert gs[0] == ts[0]


def twin_steps(tw, policy_ref, kind, hidden, w, lpp, gid0, steps, seen=None):
    """`steps` steps of the twin with the reference's actions.  seen (a dict): which actions occurred, and whether two policies of
    the set, asked alone about the same observations, ever disagreed."""
    for _ in range(steps):
        obs = tw.get_obs()
        act = policy_ref(kind, hidden, w, lpp, gid0, obs)
        if seen is not None:
            seen.setdefault("actions", set()).update(np.unique(act).tolist())
            alone = [policy_ref(kind, hidden, w[i:i + 1], 1, 0, obs) for i in range(len(w))]
            seen["disagree"] = seen.get("disagree", False) or any(not np.array_equal(alone[0], x) for x in alone[1:])
        tw.step(act)


# Seeds of the weights of test 2 per (kind, hidden, policy set): the first seed (searched on the CPU with the twin and policy_ref alone)
# for which requirement 6 below holds under every flag set and both sizes.  The 777 lanes at offset 12345 all lie in ONE block of 1024
# lanes, i.e. under one policy of the (3, 1024) set, and many a random policy only ever takes one action there.
CASE2_SEEDS = {(0, 0, 5): 1, (0, 0, 3): 1, (0, 8, 5): 1, (0, 8, 3): 7, (1, 0, 5): 1, (1, 0, 3): 14, (1, 8, 5): 1, (1, 8, 3): 2}


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("flags", [0, A, A | S, T, A | T, A | S | T])
@pytest.mark.parametrize("n,vec", [(5000, 4), (777, 8)])
def test_rollout_policy_equals_the_twin_loop(gymrs, twin, policy_ref, kind, flags, n, vec):
    gid0 = 12345
    p = gymrs.engine.default_params(kind)
    p.max_episode_steps = 17
    for hidden in (0, 8):
        for n_pol, lpp in ((5, 3), (3, 1024)):
            w = make_weights(kind, hidden, n_pol, seed=CASE2_SEEDS[kind, hidden, n_pol])
            eng = gymrs.BatchedEngine(kind, n, global_env_offset=gid0, flags=flags, params=p, lanes_per_thread=vec)
            tw = TwinEngine(twin, kind, n, p, flags=flags, gid0=gid0)
            eng.reset(seed=3)
            tw.reset(3)
            eng.set_policy(w, hidden=hidden, lanes_per_policy=lpp)
            seen = {}
            t = 0
            for steps in (1, 7, 40, 3):
                eng.rollout_policy(steps)
                twin_steps(tw, policy_ref, kind, hidden, w, lpp, gid0, steps, seen)
                t += steps
                assert_same(eng, tw, kind, flags)
                assert eng.tick()[0] == t + 1
            # 6. the policies must matter: two policies of the set disagree on the same observations, and more than one action occurs
            assert seen["disagree"] and len(seen["actions"]) >= 2
            eng.close()


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("flags", [A | F, A | S | T | F])
@pytest.mark.parametrize("n,vec", [(5000, 4), (777, 8)])
def test_rollout_policy_keeps_final_observations(gymrs, kind, flags, n, vec):
    """The twin keeps no final observations: here the fused launch is compared with a second engine driven by policy_actions + step
    (test 1 pins policy_actions, the existing suites pin the per-step rows)."""
    gid0 = 12345
    p = gymrs.engine.default_params(kind)
    p.max_episode_steps = 17
    buf = torch.zeros(n, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    for hidden in (0, 8):
        for n_pol, lpp in ((5, 3), (3, 1024)):
            w = make_weights(kind, hidden, n_pol, seed=CASE2_SEEDS[kind, hidden, n_pol])
            roll = gymrs.BatchedEngine(kind, n, global_env_offset=gid0, flags=flags, params=p, lanes_per_thread=vec)
            loop = gymrs.BatchedEngine(kind, n, global_env_offset=gid0, flags=flags, params=p, lanes_per_thread=vec)
            for e in (roll, loop):
                e.reset(seed=3)
                e.set_policy(w, hidden=hidden, lanes_per_policy=lpp)
            for steps in (1, 7, 40, 3):
                roll.rollout_policy(steps)
                for _ in range(steps):
                    loop.policy_actions(buf.data_ptr())
                    loop.step(buf.data_ptr())
                roll.sync()
                loop.sync()
                assert np.array_equal(bits(roll.get_final_obs()), bits(loop.get_final_obs()))
                assert np.array_equal(bits(roll.get_state()), bits(loop.get_state()))
                for x, y in zip(roll.get_step_result(), loop.get_step_result()):
                    assert np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8))
                assert np.array_equal(roll.stats(), loop.stats()) and roll.tick() == loop.tick()
            if kind == 0 or flags & T:  # (MountainCar without a time limit rarely finishes an episode in 51 steps)
                assert roll.get_final_obs().any()
            roll.close()
            loop.close()


# ---- 3. fused == per-step on the GPU at full size ----------------------------------------------------------------------------
def test_rollout_policy_matches_per_step_gpu_at_full_size(gymrs):
    n, steps, flags = 1 << 20, 200, A | S | T
    w = make_weights(0, 0, 1, seed=1)
    a = gymrs.BatchedEngine(0, n, flags=flags)
    b = gymrs.BatchedEngine(0, n, flags=flags)
    for e in (a, b):
        e.reset(seed=0)
        e.set_policy(w)
    a.rollout_policy(steps)
    buf = torch.zeros(n, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    for _ in range(steps):
        b.policy_actions(buf.data_ptr())
        b.step(buf.data_ptr())
    a.sync()
    b.sync()
    assert np.array_equal(bits(a.get_state()), bits(b.get_state()))
    assert np.array_equal(bits(a.get_obs()), bits(b.get_obs()))
    for x, y in zip(a.get_step_result(), b.get_step_result()):
        assert np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8))
    assert np.array_equal(a.stats(), b.stats()) and a.tick() == b.tick()
    sa = a.stats()
    assert sa[3] == n * steps and sa[2] > 0  # episodes keep ending under a random affine policy
    a.close()
    b.close()


@pytest.mark.parametrize("kind", [0, 1])
def test_rollout_policy_interleaves_with_the_other_stepping_paths(gymrs, twin, policy_ref, kind):
    """rollout_policy -> step -> rollout (random) -> rollout_policy on one engine matches the twin."""
    n, flags, gid0 = 6001, A | S | T, 64
    hidden, n_pol, lpp = 8, 4, 256
    p = gymrs.engine.default_params(kind)
    p.max_episode_steps = 11
    w = make_weights(kind, hidden, n_pol, seed=9)
    eng = gymrs.BatchedEngine(kind, n, global_env_offset=gid0, flags=flags, params=p)
    tw = TwinEngine(twin, kind, n, p, flags=flags, gid0=gid0)
    eng.reset(seed=8)
    tw.reset(8)
    eng.set_policy(w, hidden=hidden, lanes_per_policy=lpp)
    buf = torch.zeros(n, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    t = 0
    for phase in range(3):
        eng.rollout_policy(9)
        twin_steps(tw, policy_ref, kind, hidden, w, lpp, gid0, 9)
        for k in range(5):
            eng.fill_actions(buf.data_ptr(), seed=2, t=t + k)
            eng.step(buf.data_ptr())
            tw.step(tw.fill_actions(2, t + k))
        eng.rollout(6, action_seed=2, action_t0=t + 5)
        for k in range(6):
            tw.step(tw.fill_actions(2, t + 5 + k))
        t += 11
        eng.rollout_policy(4)
        twin_steps(tw, policy_ref, kind, hidden, w, lpp, gid0, 4)
        assert_same(eng, tw, kind, flags)
    assert eng.tick()[0] == 3 * 24 + 1
    eng.close()


# ---- 4. the recording variant ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("flags", [A | S, A | S | T, T])
def test_rollout_policy_record_keeps_what_per_step_stepping_shows(gymrs, policy_ref, kind, flags):
    n, steps, gid0 = 5001, 37, 64
    stride = 5008
    hidden, n_pol, lpp = 8, 5, 3
    p = gymrs.engine.default_params(kind)
    p.max_episode_steps = 9
    w = make_weights(kind, hidden, n_pol, seed=4)
    rec = gymrs.BatchedEngine(kind, n, flags=flags, params=p, global_env_offset=gid0)
    ref = gymrs.BatchedEngine(kind, n, flags=flags, params=p, global_env_offset=gid0)
    for e in (rec, ref):
        e.reset(seed=12)
        e.set_policy(w, hidden=hidden, lanes_per_policy=lpp)
    obs0 = rec.get_obs()
    obs = torch.full((steps, rec.obs_dim, stride), float("nan"), dtype=torch.float32, device=DEV)
    act = torch.full((steps, stride), 9, dtype=torch.uint8, device=DEV)
    rew = torch.full((steps, stride), float("nan"), dtype=torch.float32, device=DEV)
    done = torch.full((steps, stride), 9, dtype=torch.uint8, device=DEV)
    trunc = torch.full((steps, stride), 9, dtype=torch.uint8, device=DEV)
    buf = torch.zeros(n, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()  # torch filled these on its stream; the engine writes them on its own
    rec.rollout_policy_record(steps, obs=obs.data_ptr(), actions=act.data_ptr(), reward=rew.data_ptr(), done=done.data_ptr(),
                              truncated=trunc.data_ptr(), lane_stride=stride)
    rec.sync()
    obs_h, act_h, rew_h, done_h, trunc_h = (x.cpu().numpy() for x in (obs, act, rew, done, trunc))
    prev = obs0
    for k in range(steps):
        # the action of row k is the policy's answer to the observation of row k - 1 (the reset observation for row 0)
        assert np.array_equal(act_h[k, :n], policy_ref(kind, hidden, w, lpp, gid0, prev)), k
        ref.policy_actions(buf.data_ptr())
        ref.step(buf.data_ptr())
        ref.sync()
        assert np.array_equal(act_h[k, :n], buf.cpu().numpy()), k
        assert np.array_equal(bits(obs_h[k, :, :n]), bits(ref.get_obs())), k
        r, d, tr = ref.get_step_result()
        assert np.array_equal(bits(rew_h[k, :n]), bits(r)), k
        assert np.array_equal(done_h[k, :n], d), k
        if flags & T:
            assert np.array_equal(trunc_h[k, :n], tr), k
        prev = obs_h[k, :, :n]
    assert np.isnan(obs_h[:, :, n:]).all() and (done_h[:, n:] == 9).all() and (act_h[:, n:] == 9).all()  # row padding is never written
    assert np.array_equal(bits(rec.get_state()), bits(ref.get_state()))
    assert np.array_equal(rec.stats(), ref.stats()) and rec.tick() == ref.tick()
    rec.close()
    ref.close()


def test_rollout_policy_record_rejects_bad_buffers(gymrs):
    with gymrs.BatchedEngine(0, 100, flags=A) as eng:
        eng.reset(seed=1)
        eng.set_policy(make_weights(0, 0, 1, seed=1))
        good = torch.zeros(4 * 112 * 4, dtype=torch.float32, device=DEV).data_ptr()
        with pytest.raises(gymrs.GymrsError):
            eng.rollout_policy_record(1, obs=good, actions=good, reward=good, done=good, lane_stride=96)   # < n
        with pytest.raises(gymrs.GymrsError):
            eng.rollout_policy_record(1, obs=good, actions=good, reward=good, done=good, lane_stride=104)  # not a multiple of 16
        with pytest.raises(gymrs.GymrsError):
            eng.rollout_policy_record(1, obs=good + 4, actions=good, reward=good, done=good, lane_stride=112)  # misaligned
        with pytest.raises(gymrs.GymrsError):
            eng.rollout_policy_record(1, obs=good, actions=0, reward=good, done=good, lane_stride=112)  # missing buffer
        assert eng.tick()[0] == 1


# ---- 5. the surface around it ------------------------------------------------------------------------------------------------
class DeviceColumn:
    """A zero-copy torch view of an engine's device array"""

    def __init__(self, ptr, n, typestr):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (ptr, False), "version": 3}


def test_weights_rewritten_in_place_change_the_next_launch_only(gymrs, policy_ref):
    kind, n, hidden = 0, 40_000, 8
    w0, w1 = make_weights(kind, hidden, 3, seed=1), make_weights(kind, hidden, 3, seed=2)
    eng = gymrs.BatchedEngine(kind, n, flags=A)
    eng.reset(seed=6)
    eng.set_policy(w0, hidden=hidden, lanes_per_policy=1024)
    ptr, count = eng.policy_weights_ptr()
    assert count == w0.size
    before = torch.zeros(n, dtype=torch.uint8, device=DEV)
    after = torch.zeros(n, dtype=torch.uint8, device=DEV)
    new = torch.from_numpy(w1.reshape(-1)).to(DEV)
    torch.cuda.synchronize()
    obs = eng.get_obs()
    view = torch.as_tensor(DeviceColumn(ptr, count, "<f4"), device=DEV)
    eng.policy_actions(before.data_ptr())  # enqueued before the rewrite: the old weights
    with torch.cuda.stream(torch.cuda.ExternalStream(eng.stream, device=DEV)):
        view.copy_(new)
    eng.policy_actions(after.data_ptr())   # the next launch: the new ones
    eng.sync()
    assert np.array_equal(before.cpu().numpy(), policy_ref(kind, hidden, w0, 1024, 0, obs))
    assert np.array_equal(after.cpu().numpy(), policy_ref(kind, hidden, w1, 1024, 0, obs))
    assert not np.array_equal(before.cpu().numpy(), after.cpu().numpy())
    got, h, lpp = eng.get_policy()
    assert np.array_equal(bits(got), bits(w1)) and (h, lpp) == (hidden, 1024)
    eng.close()


def test_policy_set_get_remove_and_what_it_leaves_alone(gymrs, policy_ref):
    kind, n = 1, 3000
    eng = gymrs.BatchedEngine(kind, n, flags=A | S)
    eng.reset(seed=2)
    buf = torch.zeros(n, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    for call in (lambda: eng.policy_actions(buf.data_ptr()), lambda: eng.rollout_policy(1), eng.get_policy, eng.policy_weights_ptr):
        with pytest.raises(gymrs.GymrsError) as err:
            call()
        assert err.value.status == 1 and "no policy" in str(err.value)
    eng.rollout(5, action_seed=1)
    size0 = len(eng.snapshot())
    st, tick, stats = eng.get_state(), eng.tick(), eng.stats()
    w = make_weights(kind, 16, 7, seed=3)
    eng.set_policy(w, hidden=16, lanes_per_policy=5)
    got, h, lpp = eng.get_policy()  # round trip, bit for bit
    assert np.array_equal(bits(got), bits(w)) and (h, lpp) == (16, 5)
    assert np.array_equal(bits(eng.get_state()), bits(st)) and eng.tick() == tick and np.array_equal(eng.stats(), stats)
    assert len(eng.snapshot()) == size0  # the snapshot does not carry the policy
    clone = eng.clone()                  # ... nor does a clone
    with pytest.raises(gymrs.GymrsError):
        clone.rollout_policy(1)
    clone.close()
    for bad in (dict(hidden=65), dict(lanes_per_policy=0)):
        with pytest.raises((gymrs.GymrsError, ValueError)):
            eng.set_policy(w, **{**dict(hidden=16, lanes_per_policy=5), **bad})
    eng.rollout_policy(0)  # K == 0: a no-op
    assert eng.tick() == tick
    eng.set_policy(None)
    with pytest.raises(gymrs.GymrsError):
        eng.rollout_policy(1)
    with gymrs.BatchedEngine(2, 64) as pend:  # Pendulum takes a Box action: no policies
        with pytest.raises(gymrs.GymrsError):
            pend.set_policy(np.zeros(10, np.float32))
    eng.close()


@pytest.mark.parametrize("kind", [0, 1])
def test_parameter_table_refuses_the_fused_call_but_not_policy_actions(gymrs, policy_ref, kind):
    n = 2000
    rows = [gymrs.engine.default_params(kind), gymrs.engine.default_params(kind)]
    rows[1].gravity *= 1.25
    eng = gymrs.BatchedEngine(kind, n, flags=A, params=rows[0])
    eng.reset(seed=4)
    w = make_weights(kind, 0, 2, seed=8)
    eng.set_policy(w, lanes_per_policy=100)
    eng.set_param_table(rows)
    with pytest.raises(gymrs.GymrsError) as err:
        eng.rollout_policy(3)
    assert err.value.status == 1 and "parameter table" in str(err.value)
    buf = torch.zeros(n, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    assert np.array_equal(gpu_actions(eng, buf), policy_ref(kind, 0, w, 100, 0, eng.get_obs()))
    eng.step(buf.data_ptr())  # the per-step loop covers policy x table
    eng.set_param_table(None)
    eng.rollout_policy(3)
    eng.sync()
    eng.close()


# ---- speed -------------------------------------------------------------------------------------------------------------------
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
def test_closed_loop_in_one_launch_is_no_slower_than_the_open_loop_per_step_path(gymrs):
    """CartPole, 2^20 lanes, A|S, one affine policy with seeded normal weights (not a stabilising controller).  The yardstick is the best
    any per-step closed loop could be: gymrs_step_many over 8 pre-filled action buffers (HIP launches), where the policy costs nothing.
    rate(rollout_policy, K = 256) >= rate(step_many); no margin."""
    n, flags, k = 1 << 20, A | S, 256
    w = make_weights(0, 0, 1, seed=1)
    fused = gymrs.BatchedEngine(0, n, flags=flags)
    per_step = gymrs.BatchedEngine(0, n, flags=flags)
    for e in (fused, per_step):
        e.reset(seed=0)
    fused.set_policy(w)
    ring = torch.from_numpy(np.random.default_rng(0).integers(0, 2, (8, n)).astype(np.uint8)).to(DEV)
    torch.cuda.synchronize()

    def run_fused(calls):
        for _ in range(calls):
            fused.rollout_policy(k)
        fused.sync()

    def run_per_step(calls):
        for _ in range(calls):
            per_step.step_many(ring.data_ptr(), n, 8, k)
        per_step.sync()

    run_fused(2)
    run_per_step(2)
    fused.stats_clear()
    r_step = median_rate(run_per_step, n * k)
    r_fused = median_rate(run_fused, n * k)
    s = fused.stats()
    rearmed = s[2] / s[3]
    print(f"\nrollout_policy(K={k}): {r_fused:.4g} env-steps/s; step_many (8 pre-filled buffers): {r_step:.4g} env-steps/s; "
          f"ratio {r_fused / r_step:.3f}; share of lanes re-armed per step {rearmed:.4f}")
    assert rearmed > 0.001  # episodes keep ending (the twin at 20000 lanes: 0.0106 per lane-step, mean length 80)
    assert r_fused >= r_step
    fused.close()
    per_step.close()
