"""Elided stores: every hand-over that can leave a stale array, on the device, against the CPU reference of
tests/elided_stores_ref.py (the f32 twin stepped with the same actions; it never loads the library).

Three places in the stepping path skip a store because "the array already holds the right value" -- the constant reward
(`wave_clean` words on the device, `clean_shape` on the host), Pendulum's uniform `truncated` value (`trunc_held`) and the CartPole
A | S | T launches that drop the time limit (`trunc_zero`).  A skipped store is only seen to be wrong while the array is dirty, so
every script here leaves it dirty across the call that has to invalidate the bookkeeping: reset, two valid steps at the starting
shape, a dirtying call (an invalid action, or a parameter index outside the table: the documented GYMRS_EACTION report), the
report consumed at sync, an event, one repairing step, two more steps.  After EVERY call state, reward, done, truncated, the tick
and, where kept, the statistics equal the reference bit for bit on all lanes.  Nothing writes into the engine's views.

tests/test_elided_stores_ref.py shows without a GPU that a case whose event relies on a clearing point would fail here if that
point were missing."""
import json
import os
from contextlib import contextmanager

import elided_stores_ref as ref
import lane_params_ref as lp
import numpy as np
import pytest
import torch
from elided_stores_ref import A, S
from test_gpu_time_limit_elision import Pair

from oracle.bindings import TwinEngine

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD = (ref.N + 15) // 16 * 16  # lane stride of the action ring and of the record buffers


@pytest.fixture
def elide_reward_forced(monkeypatch):
    """Engines created inside see GYMRS_DEV_ELIDE_REWARD (read at creation): CartPole's reward elision is a matter of size (from
    128 MiB per step on, 2^22 lanes); the knob puts it within reach of a 1300-lane test.  (Restated from tests/test_gpu_parity.py.)"""
    def force(value):
        monkeypatch.setenv("GYMRS_DEV_ELIDE_REWARD", value)
    return force


@contextmanager
def aql_opt_in(on):
    """GYMRS_AQL=1 (or unset) for the calls inside, as tests/test_gpu_lane_params_paths.py sets and restores it"""
    before = os.environ.get("GYMRS_AQL")
    os.environ.pop("GYMRS_AQL", None)
    if on:
        os.environ["GYMRS_AQL"] = "1"
    try:
        yield
    finally:
        os.environ.pop("GYMRS_AQL", None)
        if before is not None:
            os.environ["GYMRS_AQL"] = before


def device(a):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    torch.cuda.synchronize()  # torch copied on its stream; the engine reads on its own
    return t


def launched(eng):
    return json.loads(eng.env_json(0))["gymrs"]


def differing(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    bad = got.view(np.uint32) != want.view(np.uint32) if got.dtype == np.float32 else got != want
    return np.flatnonzero(bad.reshape(-1, bad.shape[-1]).any(axis=0))


def compare(eng, exp, flags, at, float_return=False):
    """the engine's getters == the reference, bit for bit, on all lanes"""
    reward, done, trunc = eng.get_step_result()
    for what, got, want in (("state", eng.get_state(), exp.state), ("reward", reward, exp.reward), ("done", done, exp.done),
                            ("truncated", trunc, exp.truncated)):
        lanes = differing(got, want)
        if len(lanes):
            raise AssertionError((what, at, f"{len(lanes)} lanes differ", lanes[:8].tolist(),
                                  np.asarray(got)[..., lanes[:8]].tolist(), np.asarray(want)[..., lanes[:8]].tolist()))
    if flags & S:
        got = eng.stats()
        if float_return:  # Pendulum's sum of returns is a float sum whose order differs; the integer counts are exact
            assert got[0] == pytest.approx(exp.stats[0], rel=1e-5, abs=1e-3) and np.array_equal(got[1:], exp.stats[1:]), (at, got, exp.stats)
        else:
            assert np.array_equal(got, exp.stats), ("stats", at, got, exp.stats)
    assert eng.tick()[0] == exp.tick, ("tick", at, eng.tick(), exp.tick)


def drain(eng):
    """a script that failed half-way may have left its report unconsumed"""
    try:
        eng.sync()
    except AssertionError:  # (InvalidActionError)
        pass


# ---- the engines of one (engine name, uniform | table): created once, every script starts with set_tuning and a reset ---------------
class Bench:
    def __init__(self, gymrs, name, table):
        self.gymrs, self.name, self.table = gymrs, name, table
        self.kind, self.flags, _ = ref.ENGINES[name]
        self.params_type = type(gymrs.engine.default_params(self.kind))
        self.rows = lp.rows_for(self.params_type, ref.rows_of(name, table))
        self.index = ref.index_of(name, table)
        self.eng = self.create()
        self.other = None
        self.extra = []
        d = lp.DIMS[self.kind][0]
        steps = max(ref.FUSED_STEPS.values())
        self.ring = torch.zeros((ref.RING, PAD), dtype=torch.uint8, device=DEV)
        self.actions = torch.zeros(PAD, dtype=torch.uint8, device=DEV)
        self.rec = dict(obs=torch.zeros((steps, d, PAD), dtype=torch.float32, device=DEV), actions=torch.zeros((steps, PAD), dtype=torch.uint8, device=DEV),
                        reward=torch.zeros((steps, PAD), dtype=torch.float32, device=DEV), done=torch.zeros((steps, PAD), dtype=torch.uint8, device=DEV),
                        truncated=torch.zeros((steps, PAD), dtype=torch.uint8, device=DEV))
        self.final = torch.zeros((steps, d, PAD), dtype=torch.float32, device=DEV)
        torch.cuda.synchronize()
        if table:  # the closed-loop launches: two affine policies, exploration and sampling settings
            import closed_loop_ref

            self.eng.set_policy(closed_loop_ref.make_weights(self.kind, 0, 2, seed=5), hidden=0, lanes_per_policy=100)
            self.eng.set_exploration(3, epsilon=0.25)
            self.eng.set_sampling(4, temperature=1.0)
        self.params_changed = self.table_changed = False

    def create(self):
        eng = self.gymrs.BatchedEngine(self.kind, ref.N, flags=self.flags, params=self.rows[0])
        assert launched(eng)["reward_store_elided"] == 1  # (MountainCar always; CartPole: GYMRS_DEV_ELIDE_REWARD=1 at creation)
        if self.table:
            self.set_table(eng)
        return eng

    def set_table(self, eng):
        eng.set_param_table(self.rows)
        eng.set_param_index(self.index)

    def record(self):
        return dict({k: v.data_ptr() for k, v in self.rec.items()}, lane_stride=PAD)

    def start(self, shape):
        """before a script: whatever the previous one left behind is put back"""
        for e in self.extra:
            e.close()
        self.extra = []
        drain(self.eng)
        self.eng.set_tuning(shape, 0)
        if self.params_changed:
            self.eng.set_params(self.rows[0])
        if self.table_changed:
            self.eng.set_param_table(self.rows)
        if self.table:
            self.eng.set_param_index(self.index)
        self.params_changed = self.table_changed = False

    def used_other(self, shape):
        """a second engine that has itself stepped: its own reward words are set, at the same launch shape"""
        if self.other is None:
            self.other = self.create()
        o = self.other
        drain(o)
        if self.table:
            self.set_table(o)
        o.set_tuning(shape, 0)
        o.reset(seed=ref.OTHER_SEED)
        keep = []
        for t in range(2):
            keep.append(device(lp.fill_actions(self.kind, ref.N, 0, ref.ACTION_SEED + 1, t)))
            o.step(keep[-1].data_ptr())
        o.sync()
        assert (o.get_step_result()[0] == np.float32(ref.CONST[self.kind])).all()
        return o

    def close(self):
        for e in self.extra + [self.eng] + ([self.other] if self.other is not None else []):
            e.close()


@pytest.fixture(scope="module")
def benches():
    """One Bench alive at a time: the cases are ordered by (engine, table), the previous one is closed when the key changes"""
    held = {}

    def get(gymrs, name, table):
        if (name, table) not in held:
            for b in held.values():
                b.close()
            held.clear()
            held[name, table] = Bench(gymrs, name, table)
        return held[name, table]
    yield get
    for b in held.values():
        b.close()


def policy_actions_now(b, which):
    """What the closed-loop launch `which` is about to play: the action kernel of the same source at the same tick (documented:
    `policy_actions(buf); step(buf)` is `rollout_closed_loop(1)`, likewise explore_actions and sample_actions)"""
    ptr = b.actions.data_ptr()
    if which == "cl-explore":
        b.eng.explore_actions(ptr)
    elif which == "cl-sample":
        b.eng.sample_actions(ptr)
    else:
        b.eng.policy_actions(ptr)
    b.eng.sync()
    act = b.actions.cpu().numpy()[:ref.N]
    assert (act < lp.DIMS[b.kind][1]).all()
    return act[None, :].copy()


def fused_launch(b, eng, which, t0):
    if which == "rollout":
        eng.rollout(ref.FUSED_STEPS[which], action_seed=ref.ACTION_SEED, action_t0=t0)
    elif which == "record":
        rec = b.record()
        stride = rec.pop("lane_stride")
        eng.rollout_record(ref.FUSED_STEPS[which], ref.ACTION_SEED, t0, lane_stride=stride, **rec)
    elif which == "transitions":
        eng.rollout_transitions(1, record=b.record(), final_obs=b.final.data_ptr(), lane_params=True)
    else:
        eng.rollout_closed_loop(1, lane_params=True, fitness=which == "cl-fitness", record=b.record() if which == "cl-record" else None,
                                explore=which == "cl-explore", sample=which == "cl-sample")


def run_script(b, c):
    gymrs = b.gymrs
    r = ref.Reference(c)
    calls, dirty_at, _ = ref.calls_of(c)
    b.start(c.shape)
    engines = [b.eng]
    keep = []  # device buffers stay alive until the script's last sync
    unpaid = 0  # lane-steps rejected since the last report: what the report must count
    reports = []
    for k, call in enumerate(calls):
        name, fused_actions = call[0], None
        if name == "reset":
            for e in engines:
                e.reset(seed=ref.RESET_SEED)
        elif name == "step":
            act = r.actions(call)
            if call[1] == "step":
                keep.append(device(act))
            for e in engines:
                if call[1] == "step":
                    e.step(keep[-1].data_ptr())
                elif call[2]:  # (step_host synchronises: the report comes out of the call itself)
                    with pytest.raises(gymrs.InvalidActionError) as ei:
                        e.step_host(act)
                    reports.append(str(ei.value))
                else:
                    e.step_host(act)
        elif name == "many":
            ring = r.actions(call)
            steps = len(ring)
            for e in engines:
                e.sync()  # (the ring is rewritten in place: nothing queued may still read it)
            b.ring[:steps, :ref.N] = torch.from_numpy(ring).to(DEV)
            torch.cuda.synchronize()
            with aql_opt_in(call[1] == "aql"):
                for e in engines:
                    e.step_many(b.ring.data_ptr(), PAD, steps, steps, use_graph=call[1] == "graph")
        elif name == "index":
            idx = b.index.copy()
            if call[1]:
                idx[list(ref.DIRTY)] = ref.BAD_INDEX
            for e in engines:
                e.set_param_index(idx)
        elif name == "fused":
            (eng,) = engines
            if call[1].startswith("cl-") or call[1] == "transitions":
                fused_actions = policy_actions_now(b, call[1])
            fused_launch(b, eng, call[1], r.r.t)
        elif name == "consume":
            for e in engines:
                if not reports:
                    with pytest.raises(gymrs.InvalidActionError) as ei:
                        e.sync()
                    reports.append(str(ei.value))
                assert f"lane {ref.DIRTY[0]} " in reports[-1] and f": {unpaid} invalid" in reports[-1], (unpaid, reports)
                e.sync()  # consumed
            unpaid = 0
        elif name == "tune":
            for e in engines:
                e.set_tuning(call[1], call[2])
        elif name == "restore":
            (eng,) = engines
            other = b.used_other(c.shape)
            other.restore(eng.snapshot())
            engines = [other]
        elif name == "clone":
            b.extra.append(engines[0].clone())
            engines = engines + b.extra[-1:]
        elif name == "stats-clear":
            for e in engines:
                e.stats_clear()
        elif name == "set-params":
            b.params_changed = True
            for e in engines:
                e.set_params(b.params_type.from_buffer_copy(bytes(ref.changed_row(b.kind, ref.rows_of(c.engine, False)[0]))))
        elif name == "set-state":
            for e in engines:
                e.set_state(r.new_state())
        elif name == "table":
            b.table_changed = True
            for e in engines:
                e.set_param_table(b.rows if call[1] else None)
                if call[1]:
                    e.set_param_index(b.index)
        else:
            raise AssertionError(call)
        exp = r.apply(call, actions=fused_actions)
        unpaid += sum(int((~paid).sum()) for _, _, paid in exp.launches)
        for which, e in enumerate(engines):
            compare(e, exp, b.flags, (ref.case_id(c), k, call, "engine" if which == 0 else "clone"))
    for e in engines:
        e.sync()
    del keep


CASES = sorted(ref.reward_cases(), key=lambda c: (list(ref.ENGINES).index(c.engine), ref.needs_table(c)))


@pytest.mark.parametrize("c", CASES, ids=[ref.case_id(c) for c in CASES])
def test_reward_array_equals_the_reference_after_every_call(gymrs, benches, elide_reward_forced, c):
    """The ids read engine-shape-source-event-repair (tests/elided_stores_ref.py lists them).  On the parent of the commit that
    added this file the fused sources at 4 lanes per work-item failed: the launch wrote 0.0 into the lanes whose index was outside
    the table, left their waves' words at "clean", and the repairing step skipped the store."""
    elide_reward_forced("1")
    run_script(benches(gymrs, c.engine, ref.needs_table(c)), c)


def test_params_rows_have_the_library_layout(gymrs):
    p = gymrs.engine.default_params(2)
    p.max_episode_steps = ref.P_LIMIT
    assert bytes(ref.pendulum_row(ref.P_LIMIT)) == bytes(p)
    assert [f for f, _ in ref.PendulumRow._fields_] == [f for f, _ in type(p)._fields_]


# ---- one case at natural size ---------------------------------------------------------------------------------------------------
def test_cartpole_at_the_size_that_elides_by_itself(gymrs, twin):
    """2^22 lanes, flag A, no developer knob: the engine elides the reward store by its size.  Invalid actions on lanes 300,
    2^21 + 1234 and n - 1 at 4 lanes per work-item (256-thread workgroups), set_tuning(8) -- which at this size also takes the
    launch to 512-thread workgroups -- one repairing step and two more against the twin."""
    n = 1 << 22
    lanes = [300, (1 << 21) + 1234, n - 1]
    eng = gymrs.BatchedEngine(0, n, flags=A)
    assert launched(eng)["reward_store_elided"] == 1
    tw = TwinEngine(twin, 0, n, eng.params, flags=A)
    eng.reset(seed=ref.RESET_SEED)
    tw.reset(ref.RESET_SEED)
    buf = torch.empty(n, dtype=torch.uint8, device=DEV)

    def step(t, bad=False):
        eng.fill_actions(buf.data_ptr(), seed=ref.ACTION_SEED, t=t)
        act = tw.fill_actions(ref.ACTION_SEED, t)
        if bad:
            eng.sync()
            buf[lanes] = ref.BAD_ACTION
            torch.cuda.synchronize()  # (torch wrote on its own stream)
            act[lanes] = ref.BAD_ACTION
        eng.step(buf.data_ptr())
        tw.step(act)
        got_r, got_d, got_t = eng.get_step_result()
        want_r, want_d, _ = tw.get_result()
        assert len(differing(eng.get_state(), tw.get_state())) == 0, t
        bad_lanes = differing(got_r, want_r)
        assert len(bad_lanes) == 0, (t, bad_lanes[:8], got_r[bad_lanes[:8]])
        assert np.array_equal(got_d, want_d) and not got_t.any(), t
        return got_r

    for t in range(2):
        assert (step(t) == 1.0).all()
    assert "256 work-items" in launched(eng)["last_launch"], launched(eng)["last_launch"]  # (512 only below 2^22 lanes at 4 lanes per work-item)
    r = step(2, bad=True)
    assert (r[lanes] == 0).all() and r.sum() == n - len(lanes)
    with pytest.raises(gymrs.InvalidActionError):
        eng.sync()
    eng.set_tuning(8)
    for t in range(3, 6):
        assert (step(t) == 1.0).all(), t
    assert ", 8, " in launched(eng)["last_launch"] and "512 work-items" in launched(eng)["last_launch"], launched(eng)["last_launch"]
    eng.close()


# ---- Pendulum's uniform `truncated` value ----------------------------------------------------------------------------------------
P_CASES = ref.pendulum_cases()


@pytest.fixture(scope="module")
def pendulums(gymrs):
    """{flags: (engine, second engine)} of Pendulum, limit 3: created once, every script starts with set_params, set_tuning, reset"""
    held = {}

    def get(flags):
        if flags not in held:
            p = type(gymrs.engine.default_params(2)).from_buffer_copy(bytes(ref.pendulum_row(ref.P_LIMIT)))
            held[flags] = [gymrs.BatchedEngine(2, ref.N, flags=flags, params=p) for _ in range(2)]
        return held[flags]
    yield get
    for pair in held.values():
        for e in pair:
            e.close()


@pytest.mark.parametrize("c", P_CASES, ids=[ref.pendulum_id(c) for c in P_CASES])
def test_pendulum_flags_equal_the_twin_around_every_event(gymrs, pendulums, c):
    """Limit 3, at least twelve steps; the event sits directly after a truncating step (the array holds 1) or directly before
    one.  done never changes, truncated is uniform: both compared after every call, with state, reward and statistics."""
    eng, other = pendulums(c.flags)
    P = type(eng.params)
    ring = torch.zeros((max(ref.P_MANY.values()), PAD), dtype=torch.float32, device=DEV)
    r = ref.PendulumReference(c)
    calls, _ = ref.pendulum_calls(c)
    for e in (eng, other):
        e.set_params(P.from_buffer_copy(bytes(ref.pendulum_row(ref.P_LIMIT))))
        e.set_tuning(c.shape, 0)
    engines, clones, keep = [eng], [], []
    for k, call in enumerate(calls):
        name = call[0]
        if name == "reset":
            eng.reset(seed=ref.RESET_SEED)
        elif name == "step":
            keep.append(device(r.actions(call)))
            for e in engines:
                e.step(keep[-1].data_ptr())
        elif name == "many":
            acts = r.actions(call)
            for e in engines:
                e.sync()
            ring[:len(acts), :ref.N] = torch.from_numpy(acts).to(DEV)
            torch.cuda.synchronize()
            with aql_opt_in(call[1] == "aql"):
                for e in engines:
                    e.step_many(ring.data_ptr(), PAD * 4, len(acts), len(acts))
        elif name == "rollout":
            for e in engines:
                e.rollout(call[1], action_seed=ref.ACTION_SEED, action_t0=r.t)
        elif name == "tune":
            for e in engines:
                e.set_tuning(call[1], 0)
        elif name == "clone":
            clones.append(eng.clone())
            engines = [eng, clones[-1]]
        elif name == "restore":  # into a used engine whose own array holds the opposite uniform value
            other.reset(seed=ref.OTHER_SEED)
            for t in range(ref.other_steps_before_restore(c)):
                keep.append(device(r.tw.fill_actions(ref.ACTION_SEED + 1, t)))
                other.step(keep[-1].data_ptr())
            held = other.get_step_result()[2]
            assert (held == (0 if c.after else 1)).all() and (eng.get_step_result()[2] == (1 if c.after else 0)).all()
            other.restore(eng.snapshot())
            engines = [other]
        elif name == "set-limit":
            for e in engines:
                e.set_params(P.from_buffer_copy(bytes(ref.pendulum_row(ref.P_NEW_LIMIT))))
        else:
            raise AssertionError(call)
        exp = r.apply(call)
        for e in engines:
            compare(e, exp, c.flags, (ref.pendulum_id(c), k, call), float_return=True)
            assert len(differing(e.get_obs(), exp.obs)) == 0, (k, call)
    for e in clones:
        e.close()


# ---- CartPole A | S | T: launches that drop the time limit ------------------------------------------------------------------------
@pytest.mark.parametrize("event", ["restore", "clone", "tune", "rollout"])
def test_limit_elision_goes_on_after_an_exact_launch_left_ones(gymrs, twin, event):
    """Limit 23: step until a launch that checked the limit has left ones in `truncated`, apply the event, step on.  Launches
    without the limit do not write the array: it must equal the twin after every step, and such launches must still happen.
    (Step 23 truncates every lane that survived since the reset.  No CartPole episode ends within its first seven steps, so no
    episode started at ticks 2 .. 8 and steps 24 .. 30 cannot reach the limit: those are the launches that can be elided after
    the event, which is why the fused rollout takes only two of them.  From step 31 on nearly every step truncates somebody.)"""
    p = Pair(gymrs, twin, 0, ref.N, limit=23, seed=6)
    for _ in range(60):
        p.step(1, check_flags=True)
        if p.tw.get_result()[2].any():
            break
    assert p.tw.get_result()[2].any() and p.eng.get_step_result()[2].any()  # the array holds ones now
    engines, spare = [p.eng], []
    if event == "restore":
        other = gymrs.BatchedEngine(0, ref.N, flags=1 | 2 | 4, params=p.p)
        other.reset(seed=1)
        for t in range(5):  # a used engine: launches without the limit, its own bound, `truncated` known to hold zeros
            other.fill_actions(p.buf.data_ptr(), seed=9, t=t)
            other.step(p.buf.data_ptr())
        other.sync()
        other.restore(p.eng.snapshot())
        spare, engines = [p.eng], [other]
        p.eng = other
    elif event == "clone":
        engines.append(p.eng.clone())
    elif event == "tune":
        p.eng.set_tuning(8)
    else:  # (two steps: see below)
        p.eng.rollout(2, action_seed=3, action_t0=p.t)
        for _ in range(2):
            p.tw.step(p.tw.fill_actions(3, p.t))
            p.t += 1
        p.check("after the rollout")
    before = [json.loads(e.env_json(0))["gymrs"]["time_limit_elided_launches"] for e in engines]
    seen_ones = False
    for _ in range(60):
        for e in engines[1:]:  # (the clone takes the same actions; Pair steps its own engine and the twin)
            e.fill_actions(p.buf.data_ptr(), seed=3, t=p.t)
            e.step(p.buf.data_ptr())
        p.step(1)
        want_r, want_d, want_t = p.tw.get_result()
        seen_ones |= bool(want_t.any())
        for e in engines:
            got_r, got_d, got_t = e.get_step_result()
            assert np.array_equal(got_t, want_t) and np.array_equal(got_d, want_d) and np.array_equal(got_r, want_r), (event, p.t)
    for e in engines:
        assert np.array_equal(e.get_state().view(np.uint32), p.tw.get_state().view(np.uint32)) and np.array_equal(e.stats(), p.tw.stats())
    after = [json.loads(e.env_json(0))["gymrs"]["time_limit_elided_launches"] for e in engines]
    assert all(a > b for a, b in zip(after, before)), (before, after)
    assert seen_ones  # and exact launches came back in between
    for e in engines[1:] + spare:
        e.close()
