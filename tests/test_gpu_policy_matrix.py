"""Every copy of the closed-loop kernels against the CPU reference of tests/closed_loop_ref.py (the f32 twin stepped with the actions
of tests/cpp/policy_ref.c; neither shares code with the kernels).

rollout_policy_kernel compiles four copies of rollout_block per (env, lanes per work-item, flag set, recording or not) and each
wave picks one at run time: uniform weights (scalar loads) or gathered (per-lane vector loads) x full wave or the ragged wave that
holds the batch's tail.  The case table (closed_loop_ref.SHAPES) puts lanes into all four for both vector widths;
tests/test_closed_loop_ref.py shows on the CPU that inside each copy's lanes episodes end, actions vary and policies disagree.

Every comparison is bit for bit (uint32 views of floats, equal integers), no tolerance, no lane left out."""
from types import SimpleNamespace

import closed_loop_ref as ref
import numpy as np
import pytest
import torch
from closed_loop_ref import A, COPIES, DIMS, F, S, T, bits, make_weights, size_of

from oracle.bindings import TwinEngine

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SETS = [(1, 1), (7, 1), (5, 3), (4, 256), (3, 1024), (2, 10**6)]  # (n_policies, lanes_per_policy), as tests/test_gpu_policy.py


def where(got, want, classes):
    """For a failure message: how many lanes differ per copy of the kernel, and the first few"""
    g, w = np.ascontiguousarray(got), np.ascontiguousarray(want)
    bad = (g.view(np.uint32) if g.dtype == np.float32 else g) != (w.view(np.uint32) if w.dtype == np.float32 else w)
    while bad.ndim > 1:
        bad = bad.any(axis=0)
    lanes = np.flatnonzero(bad)
    return {COPIES[c]: int((classes[lanes] == c).sum()) for c in np.unique(classes[lanes])}, lanes[:8].tolist()


def same(what, got, want, classes, at, nan_equal=False):
    """nan_equal (tests/test_gpu_policy_slowpaths.py, whose states hold NaNs): a NaN equals any NaN, as in tests/test_gpu_slowpaths.py"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, at, got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype == np.float32:
        if nan_equal:
            both = np.isnan(got) & np.isnan(want)
            got, want = np.where(both, np.float32(0), got), np.where(both, np.float32(0), want)
        got, want = got.view(np.uint32), want.view(np.uint32)
    assert np.array_equal(got, want), (what, at) + where(got, want, classes)


def assert_launch(eng, want, flags, classes, at, first=0, nan_equal=False):
    """The engine after a launch == the reference's record of it (`want`), lanes [first, first + n_envs) of the reference's batch"""
    sl = slice(first, first + eng.n_envs)
    classes = classes[sl]
    same("state", eng.get_state(), want.state[:, sl], classes, at, nan_equal)
    same("obs", eng.get_obs(), want.obs[:, sl], classes, at, nan_equal)
    r, d, tr = eng.get_step_result()
    same("reward", r, want.reward[sl], classes, at, nan_equal)
    same("done", d, want.done[sl], classes, at)
    if flags & T:
        same("truncated", tr, want.truncated[sl], classes, at)
    if flags & F:
        same("final_obs", eng.get_final_obs(), want.final[:, sl], classes, at, nan_equal)
    assert eng.tick()[0] == want.tick, (at, eng.tick(), want.tick)


def assert_stats(eng, want, at):  # as assert_same of tests/test_gpu_policy.py
    gs = eng.stats()
    assert np.array_equal(gs[1:], want.stats[1:]) and gs[0] == want.stats[0], (at, gs, want.stats)


def make_engine(gymrs, c, first=0, count=None):
    """An engine for lanes [first, first + count) of case c's batch, reset, prepared and with c's policy set"""
    count = c.n - first if count is None else count
    eng = gymrs.BatchedEngine(c.kind, count, global_env_offset=c.gid0 + first, flags=c.flags, params=c.params, lanes_per_thread=c.vec)
    eng.reset(seed=c.reset_seed)
    if c.prepare is not None:
        eng.set_state(c.prepare(eng.get_state(), first))
    eng.set_policy(c.weights[0] if isinstance(c.weights, list) else c.weights, hidden=c.hidden, lanes_per_policy=c.lanes_per_policy)
    return eng


def final_rows_are_kept_in_every_copy(c, want):
    for copy in np.unique(c.classes):
        assert want.final[:, c.classes == copy].any(), COPIES[copy]  # an all-zero buffer cannot pass


# ---- a. every copy of the fused kernel ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,shape,flags,hidden", ref.cases(record=False))
def test_rollout_policy_equals_the_cpu_reference_in_every_copy(gymrs, kind, shape, flags, hidden):
    c = ref.case(kind, shape, flags, hidden, gymrs.engine.default_params(kind))
    want = ref.run_case(c)
    assert len(np.unique(c.classes)) == 3  # two full copies and the ragged wave's
    eng = make_engine(gymrs, c)
    same("start state", eng.get_state(), want[0].start_state, c.classes, 0)
    for k, steps in enumerate(c.schedule):
        eng.rollout_policy(steps)
        assert_launch(eng, want[k], flags, c.classes, k)
        assert_stats(eng, want[k], k)
    if flags & F:
        final_rows_are_kept_in_every_copy(c, want[-1])
    eng.close()


# ---- b. every copy of the recording kernel (4 lanes per work-item only) ------------------------------------------------------
@pytest.mark.parametrize("kind,shape,flags,hidden", ref.cases(record=True))
def test_rollout_policy_record_equals_the_cpu_reference_in_every_copy(gymrs, kind, shape, flags, hidden):
    c = ref.case(kind, shape, flags, hidden, gymrs.engine.default_params(kind))
    want = ref.run_case(c)
    n, d = c.n, DIMS[kind][0]
    stride = (n + 15) // 16 * 16 + 16  # > n: rows have padding columns
    rows = max(c.schedule)
    eng = make_engine(gymrs, c)
    for k, steps in enumerate(c.schedule):
        obs = torch.full((rows, d, stride), float("nan"), dtype=torch.float32, device=DEV)
        act = torch.full((rows, stride), 9, dtype=torch.uint8, device=DEV)
        rew = torch.full((rows, stride), float("nan"), dtype=torch.float32, device=DEV)
        done = torch.full((rows, stride), 9, dtype=torch.uint8, device=DEV)
        trunc = torch.full((rows, stride), 9, dtype=torch.uint8, device=DEV)
        torch.cuda.synchronize()  # torch filled these on its stream; the engine writes them on its own
        eng.rollout_policy_record(steps, obs=obs.data_ptr(), actions=act.data_ptr(), reward=rew.data_ptr(), done=done.data_ptr(),
                                  truncated=trunc.data_ptr(), lane_stride=stride)
        eng.sync()
        obs_h, act_h, rew_h, done_h, trunc_h = (x.cpu().numpy() for x in (obs, act, rew, done, trunc))
        w = want[k]
        for t in range(steps):
            same("recorded obs", obs_h[t, :, :n], w.rec_obs[t], c.classes, (k, t))
            same("recorded actions", act_h[t, :n], w.rec_actions[t], c.classes, (k, t))
            same("recorded reward", rew_h[t, :n], w.rec_reward[t], c.classes, (k, t))
            same("recorded done", done_h[t, :n], w.rec_done[t], c.classes, (k, t))
            if flags & T:
                same("recorded truncated", trunc_h[t, :n], w.rec_truncated[t], c.classes, (k, t))
        # padding columns and the rows beyond `steps` are never written
        assert np.isnan(obs_h[:, :, n:]).all() and np.isnan(rew_h[:, n:]).all()
        assert (act_h[:, n:] == 9).all() and (done_h[:, n:] == 9).all() and (trunc_h[:, n:] == 9).all()
        assert np.isnan(obs_h[steps:]).all() and np.isnan(rew_h[steps:]).all()
        assert (act_h[steps:] == 9).all() and (done_h[steps:] == 9).all() and (trunc_h[steps:] == 9).all()
        assert_launch(eng, w, flags, c.classes, k)
        assert_stats(eng, w, k)
    if flags & F:
        final_rows_are_kept_in_every_copy(c, want[-1])
    eng.close()


# ---- c. 64-bit lane ids --------------------------------------------------------------------------------------------------------
BIG_BLOCK = (1 << 32) + 1000  # lanes_per_policy beyond 2^32
# the engine's first wave starts 100 lanes before the end of block 5 (policy 5 % 3 = 2) and runs into block 6 (policy 0)
IDS = {"offset": ((1 << 40) + 12345, 1000), "block": (5 * BIG_BLOCK + BIG_BLOCK - 100, BIG_BLOCK)}


def straddles_with_a_high_remainder(gid0, lpp, vec):
    """The first wave's remainder in its block is >= 2^32, it has fewer than 64 * vec lanes left there (so it uses two policies),
    and the low 32 bits of the remainder alone would call it uniform."""
    r = gid0 % lpp
    return r >= 1 << 32 and lpp - r < 64 * vec and lpp - (r & 0xFFFFFFFF) >= 64 * vec


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("ids", list(IDS))
def test_policy_actions_with_64_bit_lane_ids(gymrs, kind, ids):
    n = 3000
    gid0, lpp = IDS[ids]
    classes = ref.wave_classes(n, 4, gid0, 3, lpp)
    if ids == "block":
        assert straddles_with_a_high_remainder(gid0, lpp, 4) and COPIES[classes[0]] == "gathered-full"
        assert (classes[256:] % 2 == 0).all()  # every later wave is uniform
    eng = gymrs.BatchedEngine(kind, n, global_env_offset=gid0, flags=A)
    eng.reset(seed=21)
    buf = torch.zeros(n, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    obs = eng.get_obs()
    for hidden in (0, 8):
        for seed in range(11, 31):
            w = make_weights(kind, hidden, 3, seed=seed)
            want = ref.policy_ref(kind, hidden, w, lpp, gid0, obs)
            if ids == "offset":
                break
            # "block": the first weights with which the first wave's first policy alone would be noticed in the lanes of its second
            first_only = ref.policy_ref(kind, hidden, w[2:3], 1, 0, obs)
            if not np.array_equal(first_only[100:256], want[100:256]):
                assert np.array_equal(first_only[:100], want[:100])
                break
        else:
            raise AssertionError("no seed tells the two policies of the first wave apart")
        eng.set_policy(w, hidden=hidden, lanes_per_policy=lpp)
        eng.policy_actions(buf.data_ptr())
        eng.sync()
        same("actions", buf.cpu().numpy(), want, classes, (hidden, seed))
    eng.close()


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("vec", [4, 8])
@pytest.mark.parametrize("ids", list(IDS))
def test_rollout_policy_with_64_bit_lane_ids(gymrs, kind, vec, ids):
    n, flags, hidden = 3000, A | S | T, 8
    gid0, lpp = IDS[ids]
    p = gymrs.engine.default_params(kind)
    p.max_episode_steps = ref.MAX_EPISODE_STEPS
    w = make_weights(kind, hidden, 3, seed=19)
    classes = ref.wave_classes(n, vec, gid0, 3, lpp)
    if ids == "block":
        assert straddles_with_a_high_remainder(gid0, lpp, vec) and COPIES[classes[0]] == "gathered-full"
    prepare = ref.mountain_car_prepare if kind == 1 else None
    want = ref.reference(kind, n, gid0, p, flags, w, hidden, lpp, 5, (3, 30), prepare)
    if ids == "block":  # the policies on the two sides of the block's end are told apart inside the first wave
        assert want[-1].disagree[100:64 * vec].any() and want[-1].episodes[:64 * vec].any()
    eng = gymrs.BatchedEngine(kind, n, global_env_offset=gid0, flags=flags, params=p, lanes_per_thread=vec)
    eng.reset(seed=5)
    if prepare is not None:
        eng.set_state(prepare(eng.get_state(), 0))
    eng.set_policy(w, hidden=hidden, lanes_per_policy=lpp)
    for k, steps in enumerate((3, 30)):
        eng.rollout_policy(steps)
        assert_launch(eng, want[k], flags, classes, k)
        assert_stats(eng, want[k], k)
    eng.close()


# ---- d. hidden widths: the remainder trip of the uniform copy's four-unit loop -------------------------------------------------
def without_the_remainder_trip(kind, hidden, w, lpp, gid0, obs):
    """The reference's actions if the policies w had only their first hidden & ~3 hidden units (none: the logits are b2)"""
    d, a = DIMS[kind]
    keep = hidden & ~3
    out = []
    for p in w:
        w1, b1 = p[:hidden * d].reshape(hidden, d), p[hidden * d:hidden * d + hidden]
        w2, b2 = p[hidden * d + hidden:hidden * d + hidden + a * hidden].reshape(a, hidden), p[-a:]
        out.append(np.concatenate([w1[:keep].ravel(), b1[:keep], w2[:, :keep].ravel(), b2] if keep else [np.zeros(a * d, np.float32), b2]))
    return ref.policy_ref(kind, keep, np.stack(out).astype(np.float32), lpp, gid0, obs)


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("n", [777, 5000])
@pytest.mark.parametrize("hidden", [2, 3, 5, 7, 63])
def test_policy_actions_at_hidden_widths_with_a_remainder_trip(gymrs, kind, n, hidden):
    gid0 = 12345
    eng = gymrs.BatchedEngine(kind, n, global_env_offset=gid0, flags=A)
    eng.reset(seed=21)
    buf = torch.zeros(n, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    obs = eng.get_obs()
    for p, lpp in SETS:
        # the first seed with which the units of the remainder trip matter: without them the reference answers differently somewhere
        for seed in range(100 * hidden + p, 100 * hidden + p + 20):
            w = make_weights(kind, hidden, p, seed=seed)
            want = ref.policy_ref(kind, hidden, w, lpp, gid0, obs)
            if not np.array_equal(without_the_remainder_trip(kind, hidden, w, lpp, gid0, obs), want):
                break
        assert not np.array_equal(without_the_remainder_trip(kind, hidden, w, lpp, gid0, obs), want), (p, lpp)
        classes = ref.wave_classes(n, 4, gid0, p, lpp)
        eng.set_policy(w, hidden=hidden, lanes_per_policy=lpp)
        eng.policy_actions(buf.data_ptr())
        eng.sync()
        same("actions", buf.cpu().numpy(), want, classes, (p, lpp, seed))
    eng.close()


# ---- e. constructed ties and zeros ---------------------------------------------------------------------------------------------
def tie_weights(kind, hidden):
    """CartPole: the two output rows are the same, y[0] == y[1] (the first wins: action 0).  MountainCar: rows 1 and 2 are the same
    and row 0 is theirs with a bias 1 lower, y[1] == y[2] > y[0] (action 1)."""
    d, a = DIMS[kind]
    w = make_weights(kind, hidden, 1, seed=31)[0]
    k = d if hidden == 0 else hidden  # length of an output row; the output layer is the last a * k + a floats
    rows, b = w[-(a * k + a):-a].reshape(a, k), w[-a:]
    rows[:] = rows[a - 1]
    b[:] = b[a - 1]
    if kind == 1:
        b[0] -= 1.0
    return w


def special_weights(kind, hidden, fan_out, seed=32):
    """Hidden unit 0: W1 row -1, b1 = -0.0: its pre-activation is exactly -0.0 on a lane whose observation is all +0.0.  Hidden unit 1:
    b1 = NaN, so its pre-activation is NaN everywhere.  By the definition the ReLU turns both into +0.  fan_out "inf": unit 0 feeds
    W2[1][0] = +inf and unit 1 W2[A-1][1] = +inf (inf * 0 makes those logits NaN); "finite": their W2 columns stay finite, so a ReLU
    that let the NaN through would turn every logit NaN where the right one leaves them as they are."""
    d, a = DIMS[kind]
    w = make_weights(kind, hidden, 1, seed=seed)[0]
    w1, b1 = w[:hidden * d].reshape(hidden, d), w[hidden * d:hidden * d + hidden]
    w2 = w[hidden * d + hidden:hidden * d + hidden + a * hidden].reshape(a, hidden)
    w1[0] = -1.0
    b1[:] = 0.0  # (no biases: the reset observations are small, and with biases a random policy answers the same everywhere)
    w[-a:] = 0.0
    b1[0] = -0.0
    b1[1] = np.nan
    if fan_out == "inf":
        w2[1, 0] = np.inf
        w2[a - 1, 1] = np.inf
    return w


def zero_every_fifth(state, first):
    state = state.copy()
    state[:, (-first) % 5::5] = 0.0
    return state


def occurred(kind, hidden, what, w, obs):
    """The reference side: the constructed tie or special value really occurs on these observations"""
    y, z = ref.policy_logits(kind, hidden, w, 1, 0, obs)
    act = ref.policy_ref(kind, hidden, w, 1, 0, obs)
    zero_lanes = ~obs.any(axis=0) & ~np.signbit(obs).any(axis=0)
    if what == "zero":
        assert not bits(y).any() and not act.any()
    elif what == "tie" and kind == 0:
        assert np.array_equal(bits(y[0]), bits(y[1])) and not act.any() and np.isfinite(y).all()
    elif what == "tie":
        assert np.array_equal(bits(y[1]), bits(y[2])) and (y[1] > y[0]).all() and (act == 1).all()
    else:
        assert zero_lanes.sum() >= 100
        assert (bits(z[0, zero_lanes]) == 0x80000000).all()  # exactly -0.0
        assert np.isnan(z[1]).all()
        if what == "inf":
            assert np.isnan(y[1, zero_lanes]).all() and np.isnan(y[DIMS[kind][1] - 1]).all()
            assert (act != DIMS[kind][1] - 1).all()  # a NaN never wins
        else:
            assert np.isfinite(y).all() and len(np.unique(act)) >= 2  # (a NaN let through would make every answer 0)


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("what,hidden", [("zero", 0), ("zero", 8), ("tie", 0), ("tie", 8), ("inf", 8), ("finite", 8), ("inf", 7), ("finite", 7)])
def test_constructed_ties_zeros_and_special_values(gymrs, twin, kind, what, hidden):
    n, gid0, flags, schedule = 1300, 12345, A | S | T, (1, 5)
    if what == "zero":
        w = np.zeros(size_of(kind, hidden), np.float32)
    elif what == "tie":
        w = tie_weights(kind, hidden)
    else:
        w = special_weights(kind, hidden, what)
    if what == "finite":  # the first seed with which the reference takes two different actions on the start state
        tw = TwinEngine(twin, kind, n, gymrs.engine.default_params(kind), flags=0, gid0=gid0)
        tw.reset(6)
        start = zero_every_fifth(tw.get_state(), 0)
        for seed in range(32, 52):
            w = special_weights(kind, hidden, what, seed)
            if len(np.unique(ref.policy_ref(kind, hidden, w, 1, 0, start))) >= 2:
                break
    p = gymrs.engine.default_params(kind)
    p.max_episode_steps = 4
    buf = torch.zeros(n, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    # one policy: the uniform copies; the same policy twice, 3 lanes each: the gathered copies
    for weights, lpp in ((w[None], 1), (np.stack([w, w]), 3)):
        classes = ref.wave_classes(n, 4, gid0, len(weights), lpp)
        assert set(classes) == ({0, 2} if len(weights) == 1 else {1, 3})
        want = ref.reference(kind, n, gid0, p, flags, weights, hidden, lpp, 6, schedule, zero_every_fifth)
        occurred(kind, hidden, what, w, want[0].start_state)
        if what in ("zero", "tie"):  # ... and on every later observation of the rollout
            for launch in want:
                occurred(kind, hidden, what, w, launch.obs)
        eng = gymrs.BatchedEngine(kind, n, global_env_offset=gid0, flags=flags, params=p)
        eng.reset(seed=6)
        eng.set_state(zero_every_fifth(eng.get_state(), 0))
        eng.set_policy(weights, hidden=hidden, lanes_per_policy=lpp)
        same("start state", eng.get_state(), want[0].start_state, classes, 0)
        eng.policy_actions(buf.data_ptr())
        eng.sync()
        same("actions", buf.cpu().numpy(), ref.policy_ref(kind, hidden, weights, lpp, gid0, want[0].start_state), classes, lpp)
        for k, steps in enumerate(schedule):
            eng.rollout_policy(steps)
            assert_launch(eng, want[k], flags, classes, k)
            assert_stats(eng, want[k], k)
        eng.close()


# ---- f. weights rewritten in place, fused path ---------------------------------------------------------------------------------
class DeviceColumn:
    """A zero-copy torch view of an engine's device array"""

    def __init__(self, ptr, n, typestr):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (ptr, False), "version": 3}


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("lpp", [1024, 3])  # the uniform copies (weights through the scalar cache); the gathered ones
def test_weights_rewritten_in_place_change_the_next_rollout_only(gymrs, kind, lpp):
    n, hidden, flags, k_steps, gid0 = 5000, 8, A | S | T, 12, 0
    w0, w1 = make_weights(kind, hidden, 3, seed=1), make_weights(kind, hidden, 3, seed=2)
    p = gymrs.engine.default_params(kind)
    p.max_episode_steps = ref.MAX_EPISODE_STEPS
    classes = ref.wave_classes(n, 4, gid0, 3, lpp)
    assert set(classes) == ({0, 2} if lpp == 1024 else {1, 3})  # uniform-full and uniform-ragged; the two gathered copies
    prepare = ref.mountain_car_prepare if kind == 1 else None
    want = ref.reference(kind, n, gid0, p, flags, [w0, w1], hidden, lpp, 6, (k_steps, k_steps), prepare)
    stale = ref.reference(kind, n, gid0, p, flags, [w0, w0], hidden, lpp, 6, (k_steps, k_steps), prepare)
    for copy in np.unique(classes):  # the old weights would be noticed in every copy's lanes
        m = classes == copy
        assert not np.array_equal(bits(want[1].state[:, m]), bits(stale[1].state[:, m])), COPIES[copy]
    eng = gymrs.BatchedEngine(kind, n, global_env_offset=gid0, flags=flags, params=p)
    eng.reset(seed=6)
    if prepare is not None:
        eng.set_state(prepare(eng.get_state(), 0))
    eng.set_policy(w0, hidden=hidden, lanes_per_policy=lpp)
    ptr, count = eng.policy_weights_ptr()
    assert count == w0.size
    new = torch.from_numpy(w1.reshape(-1)).to(DEV)
    torch.cuda.synchronize()
    view = torch.as_tensor(DeviceColumn(ptr, count, "<f4"), device=DEV)
    eng.rollout_policy(k_steps)  # enqueued before the rewrite: the old weights
    with torch.cuda.stream(torch.cuda.ExternalStream(eng.stream, device=DEV)):
        view.copy_(new)
    eng.rollout_policy(k_steps)  # the next launch: the new ones
    eng.sync()
    assert_launch(eng, want[1], flags, classes, "after the rewrite")
    assert_stats(eng, want[1], "after the rewrite")
    got, h, block = eng.get_policy()
    assert np.array_equal(bits(got), bits(w1)) and (h, block) == (hidden, lpp)
    eng.close()


# ---- g. cutting the batch ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("vec", [4, 8])
def test_engines_over_parts_of_a_batch_equal_one_reference_over_the_whole(gymrs, kind, vec):
    """include/gymrs_amd.h: the policy is keyed by the global id, "so the result does not depend on how a batch is cut into engines"."""
    n, gid0, lpp, hidden, flags = 9000, 12345, 1000, 8, A | S | T | F
    cuts = [0, 3001, 6202, n]
    for lo in cuts[1:-1]:
        assert all((gid0 + lo) % m for m in (4, 64, lpp))
    p = gymrs.engine.default_params(kind)
    p.max_episode_steps = ref.MAX_EPISODE_STEPS
    w = make_weights(kind, hidden, 3, seed=2)
    prepare = ref.mountain_car_prepare if kind == 1 else None
    c = SimpleNamespace(kind=kind, n=n, vec=vec, gid0=gid0, params=p, flags=flags, weights=w, hidden=hidden, lanes_per_policy=lpp,
                            reset_seed=4, schedule=ref.SCHEDULE, prepare=prepare)
    want = ref.run_case(c)
    assert want[-1].final.any() and want[-1].disagree.any()
    engines = [make_engine(gymrs, c, lo, hi - lo) for lo, hi in zip(cuts, cuts[1:])]
    for k, steps in enumerate(c.schedule):
        for eng in engines:
            eng.rollout_policy(steps)
        total = np.zeros(4)
        for eng, lo in zip(engines, cuts):
            classes = np.zeros(n, np.int8)  # a lane's copy depends on the cut: report the lanes of the engine's own launch
            classes[lo:lo + eng.n_envs] = ref.wave_classes(eng.n_envs, vec, gid0 + lo, 3, lpp)
            assert_launch(eng, want[k], flags, classes, (k, lo), first=lo)
            total += eng.stats()
        assert np.array_equal(total, want[k].stats), (k, total, want[k].stats)  # (returns and lengths are whole numbers: exact sums)
    for eng in engines:
        eng.close()
