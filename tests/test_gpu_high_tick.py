"""Every tick-keyed path at ticks the suite never reached: across tick 2^32 and at 3 * 2^32.

The engine tick is 64 bits wide, but the episode starts, the reset-log ring index and the tick the time-limit refresh sees are 32-bit,
and every random draw of a step (re-arm, epsilon-greedy, softmax sampling) puts tick bits 32 .. 47 into Philox counter word 3.
gymrs_reset restarts the tick at 0, so nothing else in the suite runs a kernel above a few thousand ticks.  Here a freshly reset
engine is moved forward by patching its snapshot (tests/time_shift.py) and its CPU f32 twin by TwinEngine.shift_time; from there
both step side by side.  tests/test_time_shift_ref.py shows without a GPU that the shifted twin deserves the trust.

  SMALL = 1000          checks the harness: no 32-bit quantity wraps, a disagreement is the helper's
  WRAP  = 2^32 - 30     the tick crosses 2^32 at step 29 of a run
  HIGH  = 3 * 2^32 + 5  steady state with tick bits in counter word 3, fill_actions' discrete slot t >> 1 beyond 32 bits

Every comparison is bit for bit (uint32 views of floats, equal integers); statistics integer for integer, except Pendulum's sum
of returns at rel = 1e-5 as in tests/test_gpu_rollout.py (f32 partial sums are grouped per wave on the GPU).  Every test ends by
comparing the engine's tick with the twin's, so a shift that silently did not happen cannot pass.  Ticks from 2^48 on alias in the
Philox counter by construction and are not tested."""
import closed_loop_ref as cl
import explore_ref as ex
import numpy as np
import pytest
import sample_ref as sr
import time_shift as ts
import torch
from closed_loop_ref import final_obs_after
from test_gpu_aql_chain import aql
from test_gpu_closed_loop_table import DEV, Recorder, compare
from test_gpu_explore import action_buffer
from test_gpu_explore import make_engine as make_explore_engine
from test_gpu_sample import make_engine as make_sample_engine
from test_gpu_sample import prob_buffer
from test_gpu_transitions import Sink

from oracle.bindings import TwinEngine

pytestmark = pytest.mark.gpu

A, S, T, F = 1, 2, 4, 8
DELTAS = [pytest.param(d, id=name) for name, d in ts.DELTAS.items()]
FAR = [pytest.param(ts.DELTAS[name], id=name) for name in ("WRAP", "HIGH")]
SHAPES = [(5000, 4, 12345), (777, 8, 64), (64, 4, 12345)]  # (n, lanes per work-item, global offset): full waves + a ragged one and the per-lane
#            action-block path; 8 lanes per work-item on the aligned path; an engine whose arrays live in mapped host memory
LIMIT = 17
ASEED = 6  # of fill_actions


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def same(what, got, want, at):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape, (what, at, got.shape, want.shape)
    bad = (bits(got) != bits(want)) if got.dtype == np.float32 else (got != want)
    if bad.any():
        where = np.argwhere(bad)[0]
        raise AssertionError((what, at, f"{int(bad.reshape(-1, bad.shape[-1]).any(axis=0).sum())} lanes differ", "first at", where.tolist(),
                              "got", got[tuple(where)].item(), "want", want[tuple(where)].item()))


def same_stats(kind, got, want, at):
    assert np.array_equal(got[1:], want[1:]), ("stats", at, got.tolist(), want.tolist())
    if kind == 2:
        assert got[0] == pytest.approx(want[0], rel=1e-5), ("stats", at, got.tolist(), want.tolist())
    else:
        assert got[0] == want[0], ("stats", at, got.tolist(), want.tolist())


class Pair:
    """An engine and its twin, reset with the same seed and moved `delta` ticks forward; the action counter t starts at the shifted
    tick.  With F the final-observation rows are tracked as tests/closed_loop_ref.py documents."""

    def __init__(self, gymrs, twin, kind, n, flags, delta, vec=4, gid0=12345, limit=LIMIT, seed=3, start=None, bounds=None):
        self.kind, self.n, self.flags, self.gymrs = kind, n, flags, gymrs
        p = gymrs.engine.default_params(kind)
        p.max_episode_steps = limit
        self.p = p
        self.eng = gymrs.BatchedEngine(kind, n, global_env_offset=gid0, flags=flags, params=p, lanes_per_thread=vec)
        self.tw = TwinEngine(twin, kind, n, p, flags=flags & ~F, gid0=gid0)
        self.tw0 = TwinEngine(twin, kind, n, p, flags=0) if flags & F else None
        self.eng.reset(seed=seed, options=bounds)  # (bounds: tests/test_gpu_reset_box.py)
        self.tw.reset(seed, bounds)
        if start is not None:
            self.eng.set_state(start)
            self.tw.set_state(start)
        if delta:
            ts.shift_engine(self.eng, delta)
            self.tw.shift_time(delta)
        self.t = self.tw.tick()
        self.final = np.zeros((self.eng.obs_dim, n), np.float32)
        self.buf = torch.empty(n, dtype=torch.float32 if kind == 2 else torch.uint8, device=DEV)

    def twin_step(self, a):
        last = final_obs_after(self.tw0, self.tw.get_state(), a) if self.tw0 is not None else None
        self.tw.step(a)
        if last is not None:
            _, d, tr = self.tw.get_result()
            ended = (d | tr) != 0
            self.final[:, ended] = last[:, ended]
        self.t += 1

    def step(self, k=1, stats=False, flags=False):
        for _ in range(k):
            self.eng.fill_actions(self.buf.data_ptr(), seed=ASEED, t=self.t)
            self.eng.step(self.buf.data_ptr())
            self.twin_step(self.tw.fill_actions(ASEED, self.t))
            if stats:
                same_stats(self.kind, self.eng.stats(), self.tw.stats(), ("tick", self.tw.tick()))
            if flags:
                self.check_flags()

    def check_flags(self, eng=None):
        at = ("tick", self.tw.tick())
        r, d, tr = (eng or self.eng).get_step_result()
        wr, wd, wtr = self.tw.get_result()
        same("reward", r, wr, at)
        same("done", d, wd, at)
        if self.flags & T:
            same("truncated", tr, wtr, at)

    def check(self, eng=None):
        eng = eng or self.eng
        at = ("tick", self.tw.tick())
        same("state", eng.get_state(), self.tw.get_state(), at)
        same("obs", eng.get_obs(), self.tw.get_obs(), at)
        self.check_flags(eng)
        if self.flags & F:
            same("final_obs", eng.get_final_obs(), self.final, at)
        same_stats(self.kind, eng.stats(), self.tw.stats(), at)
        assert eng.tick()[0] == self.tw.tick(), (eng.tick(), self.tw.tick())

    def ring(self, nbuf, seed=11):
        """nbuf action buffers on the device (filled by the engine) and on the host (by the twin), counted from the current t"""
        dev = torch.empty((nbuf, self.n), dtype=self.buf.dtype, device=DEV)
        host = []
        for b in range(nbuf):
            self.eng.fill_actions(dev[b].data_ptr(), seed=seed, t=self.t + b)
            host.append(self.tw.fill_actions(seed, self.t + b))
        return dev, host

    def step_many(self, steps, nbuf=4, **kw):
        dev, host = self.ring(nbuf)
        self.eng.step_many(dev.data_ptr(), dev.stride(0) * dev.element_size(), nbuf, steps, **kw)
        for k in range(steps):
            self.twin_step(host[k % nbuf])
        self.eng.sync()

    def close(self):
        self.eng.close()


# ---- the per-step kernel -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("delta", DELTAS)
@pytest.mark.parametrize("flags", [A | S, A | S | T, A | T, A | S | T | F, T])
@pytest.mark.parametrize("kind", [0, 1, 2])
def test_per_step_kernel(gymrs, twin, kind, flags, delta):
    """80 steps of fill_actions + step; everything an engine shows compared after steps 1, 29, 30, 31 (at WRAP: around the crossing) and 80."""
    for n, vec, gid0 in SHAPES:
        p = Pair(gymrs, twin, kind, n, flags, delta, vec=vec, gid0=gid0)
        done = 0
        for upto in (1, 29, 30, 31, 80):
            p.step(upto - done)
            done = upto
            p.check()
        assert p.eng.tick()[0] == 1 + delta + 80
        p.close()


# ---- the step paths, with the per-step statistics reads ---------------------------------------------------------------------------
@pytest.mark.parametrize("delta", DELTAS)
@pytest.mark.parametrize("kind,flags", [(0, A | S), (0, A | S | T), (1, A | S), (2, A | S | T)])
def test_statistics_read_after_every_step_a_clear_retuning_and_step_many(gymrs, twin, kind, flags, delta):
    """stats() after every single step (CartPole A|S: through the pending rows of the reset log, first_tick just below 2^32), one
    stats_clear 10 steps before the crossing, 8 lanes per work-item in mid-run, then step_many eager and as graph replays."""
    p = Pair(gymrs, twin, kind, 5000, flags, delta)
    p.step(19, stats=True)
    p.eng.stats_clear()
    p.tw.stats_clear()
    same_stats(kind, p.eng.stats(), p.tw.stats(), "after the clear")
    p.step(15, stats=True)  # across the crossing at WRAP
    p.check()
    p.eng.set_tuning(8)
    p.step(10, stats=True)
    p.eng.set_tuning(4)
    p.step(3, stats=True)
    p.step_many(24)
    p.check()
    p.step_many(24, use_graph=kind != 2)  # (graph replays are refused for Pendulum with the time limit: eager again)
    p.check()
    p.step(9, stats=True)
    p.check()
    assert p.eng.tick()[0] == 1 + delta + 104
    p.close()


@pytest.mark.parametrize("delta", FAR)
@pytest.mark.parametrize("kind", [0, 2])
def test_step_many_eager_and_graph_across_the_crossing(gymrs, twin, kind, delta):
    """The calls themselves span the crossing: 48 steps in one eager step_many, and on a second pair 48 graph replays."""
    for graph in ((False, True) if kind != 2 else (False,)):  # (graph replays are refused for Pendulum with the time limit)
        p = Pair(gymrs, twin, kind, 5000, A | S | T, delta)
        p.step_many(48, nbuf=8, use_graph=graph)
        p.check()
        p.step(5, stats=True)
        p.check()
        p.close()


@pytest.mark.parametrize("delta", FAR)
def test_chain_on_the_engines_own_queue_across_the_crossing(gymrs, twin, delta):
    """GYMRS_AQL=1: step_many as a chain on the engine's AQL dispatcher (HIP launches where that path is not available)."""
    with aql(True):
        p = Pair(gymrs, twin, 0, 5000, A | S, delta, gid0=64)
        p.step_many(48, nbuf=8)
        p.check()
        p.eng.stats_clear()
        p.tw.stats_clear()
        p.step_many(24)
    p.check()
    p.step(4, stats=True)
    assert p.eng.tick()[0] == p.tw.tick() == 1 + delta + 76
    p.close()


# ---- time-limit elision ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy,limit", [("alternate", 17), ("balance", 17), ("balance", 64), ("random", 17), ("random", 64)])
def test_time_limit_elision_across_the_crossing(gymrs, twin, policy, limit):
    """CartPole with all three flags drops the limit from a launch while no lane can reach it (the bound is refreshed from the age of
    the oldest episode, which sees 32 bits of the tick).  `alternate`: every lane starts upright at rest (by set_state: a reset box of
    width 0 is refused) and plays 0, 1, 0, 1, ...: upright for 17 steps, not for 64.  `balance`: every lane pushes towards the side its pole falls to (action =
    theta + theta_dot > 0, read from the twin).  Under both no lane terminates: all of them are truncated at every multiple of the limit.
    `random`: fill_actions, most episodes end before the limit.  Flags after every step, statistics around the crossing."""
    n = 5000
    p = Pair(gymrs, twin, 0, n, A | S | T, ts.WRAP, limit=limit, start=np.zeros((4, n), np.float32) if policy == "alternate" else None)
    steps = 2 * limit + 40
    if policy == "random":
        for k in range(steps):
            p.step(flags=True, stats=k in (27, 28, 29, 30))
    else:
        for k in range(1, steps + 1):
            st = p.tw.get_state()
            a = (st[2] + st[3] > 0).astype(np.uint8) if policy == "balance" else np.full(n, (k - 1) % 2, np.uint8)
            dev = torch.from_numpy(a).to(DEV)
            torch.cuda.synchronize()  # torch copied on its stream; the engine reads on its own
            p.eng.step(dev.data_ptr())
            p.twin_step(a)
            p.check_flags()
            _, d, tr = p.tw.get_result()
            assert not d.any() and (tr == (1 if k % limit == 0 else 0)).all(), k  # (the yardstick does what the test is about)
            if k in (28, 29, 30, 31):
                same_stats(0, p.eng.stats(), p.tw.stats(), ("tick", p.tw.tick()))
            p.eng.sync()  # `dev` is released below: the step has read it
    p.check()
    assert p.tw.tick() == 1 + ts.WRAP + steps
    p.close()


# ---- the fused rollouts -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("delta", DELTAS)
@pytest.mark.parametrize("flags", [A | S, A | S | T])
@pytest.mark.parametrize("kind", [0, 1, 2])
def test_rollout(gymrs, twin, kind, flags, delta):
    """rollout with action_t0 at the shifted tick: 1 + 7 + 40 + 3 steps (the 40 span the crossing at WRAP), then rollout -> step -> rollout"""
    for n, vec, gid0 in SHAPES[:2]:
        p = Pair(gymrs, twin, kind, n, flags, delta, vec=vec, gid0=gid0)
        for steps in (1, 7, 40, 3):
            p.eng.rollout(steps, action_seed=ASEED, action_t0=p.t)
            for _ in range(steps):
                p.twin_step(p.tw.fill_actions(ASEED, p.t))
            p.check()
        for steps in (9, 9):
            p.step(5)
            p.eng.rollout(steps, action_seed=ASEED, action_t0=p.t)
            for _ in range(steps):
                p.twin_step(p.tw.fill_actions(ASEED, p.t))
            p.check()
        assert p.eng.tick()[0] == 1 + delta + 79
        p.close()


@pytest.mark.parametrize("delta", FAR)
@pytest.mark.parametrize("kind", [0, 1, 2])
def test_rollout_record(gymrs, twin, kind, delta):
    """Row k of the record = what the per-step loop shows after step k on a second shifted engine (as tests/test_gpu_rollout.py does
    at low ticks), and both end where the twin ends."""
    n, steps, flags, stride = 5000, 37, A | S | T, 5008
    rec = Pair(gymrs, twin, kind, n, flags, delta, gid0=64)
    loop = Pair(gymrs, twin, kind, n, flags, delta, gid0=64)
    obs = torch.full((steps, rec.eng.obs_dim, stride), float("nan"), dtype=torch.float32, device=DEV)
    act = torch.zeros((steps, stride), dtype=rec.buf.dtype, device=DEV)
    rew = torch.full((steps, stride), float("nan"), dtype=torch.float32, device=DEV)
    done = torch.full((steps, stride), 9, dtype=torch.uint8, device=DEV)
    trunc = torch.full((steps, stride), 9, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()  # torch filled these on its stream; the engine writes them on its own
    rec.eng.rollout_record(steps, ASEED, rec.t, obs=obs.data_ptr(), actions=act.data_ptr(), reward=rew.data_ptr(), done=done.data_ptr(),
                           truncated=trunc.data_ptr(), lane_stride=stride)
    rec.eng.sync()
    obs_h, act_h, rew_h, done_h, trunc_h = (x.cpu().numpy() for x in (obs, act, rew, done, trunc))
    for k in range(steps):
        loop.step()
        loop.eng.sync()
        at = ("row", k)
        same("recorded action", act_h[k, :n], loop.buf.cpu().numpy(), at)
        same("recorded obs", obs_h[k, :, :n], loop.eng.get_obs(), at)
        r, d, tr = loop.eng.get_step_result()
        same("recorded reward", rew_h[k, :n], r, at)
        same("recorded done", done_h[k, :n], d, at)
        same("recorded truncated", trunc_h[k, :n], tr, at)
        same("recorded obs (twin)", obs_h[k, :, :n], loop.tw.get_obs(), at)
    assert np.isnan(obs_h[:, :, n:]).all() and (done_h[:, n:] == 9).all()  # the padding of a row is never written
    loop.check()
    for _ in range(steps):
        rec.twin_step(rec.tw.fill_actions(ASEED, rec.t))
    rec.check()
    assert rec.eng.tick() == loop.eng.tick()
    rec.close()
    loop.close()


# ---- the tick-keyed action sources ------------------------------------------------------------------------------------------------------
def shifted(make, gymrs, c, delta, vec=4, **kw):
    """make_engine of the explore / sample tests, moved `delta` ticks forward (the policy and the settings are installed again: they
    are in no snapshot)"""
    eng = make(gymrs, c, vec, **kw)
    ts.shift_engine(eng, delta)
    eng.set_policy(c.weights, hidden=c.hidden, lanes_per_policy=c.lanes_per_policy)
    if hasattr(c, "threshold"):
        eng.set_exploration(c.seed, threshold=c.threshold)
    else:
        eng.set_sampling(c.seed, scale=c.scale)
    return eng


@pytest.mark.parametrize("delta", DELTAS)
@pytest.mark.parametrize("kind", [0, 1])
def test_explore_actions_and_sample_actions_against_the_host_draws(gymrs, kind, delta):
    """explore_actions / sample_actions + step, 34 times (across the crossing at WRAP): every buffer equals gymrs.explore_draw /
    gymrs.sample_draw at the engine's tick, mixed with the plain-C policy's greedy action / fed with its logits."""
    full = A | S | T | F
    ce = ex.case(kind, full, False, 6, (3, 1), 8, (1,))
    cs = sr.case(kind, full, False, 6, (3, 1), 8, (1,))
    n, n_actions = ce.n, cl.DIMS[kind][1]
    gids = np.arange(n, dtype=np.uint64) + np.uint64(ce.gid0)
    e, s = shifted(make_explore_engine, gymrs, ce, delta), shifted(make_sample_engine, gymrs, cs, delta)
    buf, sbuf, pbuf = action_buffer(n), action_buffer(n), prob_buffer(n)  # (a buffer per engine: each works on its own stream)
    for k in range(34):
        tick = 1 + delta + k
        assert e.tick()[0] == s.tick()[0] == tick
        greedy = cl.policy_ref(kind, ce.hidden, ce.weights, ce.lanes_per_policy, ce.gid0, e.get_obs())
        explored, rnd = gymrs.explore_draw(ce.seed, ce.threshold, n_actions, gids, tick)
        e.explore_actions(buf.data_ptr())
        e.sync()
        same("explore_actions", buf.cpu().numpy()[:n], np.where(explored, rnd, greedy).astype(np.uint8), ("tick", tick))
        e.step(buf.data_ptr())
        _, _, _, logits = sr.sample_actions(kind, cs.hidden, cs.weights, cs.lanes_per_policy, cs.gid0, s.get_obs(), cs.seed, cs.scale, tick)
        want = [gymrs.sample_draw(cs.seed, cs.scale, logits[:, i], cs.gid0 + i, tick) for i in range(n)]
        s.sample_actions(sbuf.data_ptr(), pbuf.data_ptr())
        s.sync()
        same("sample_actions", sbuf.cpu().numpy()[:n], np.array([a for a, _ in want], np.uint8), ("tick", tick))
        same("prob", pbuf.cpu().numpy()[:n], np.array([pr[a] for a, pr in want], np.float32), ("tick", tick))
        s.step(sbuf.data_ptr())
    e.close()
    s.close()


@pytest.mark.parametrize("delta", DELTAS)
@pytest.mark.parametrize("hidden", [0, 8])
@pytest.mark.parametrize("kind", [0, 1])
def test_closed_loop_launches_of_40_steps(gymrs, kind, hidden, delta):
    """One launch of 40 steps from the shifted tick against the *_ref modules with tick0: rollout_closed_loop with explore (plain at 8
    lanes per work-item, recording at 4), with sample (plain, recording), and rollout_transitions with sample under a 3-row parameter
    table -- the snapshot patch has to carry the v5 tail -- checking final_obs[k] and start_obs."""
    full, tick0 = A | S | T | F, 1 + delta
    gid0, policy_set = (6, (3, 1)) if hidden else (0, (3, 512))
    ce = ex.case(kind, full, False, gid0, policy_set, hidden, (40,))
    cs = sr.case(kind, full, False, gid0, policy_set, hidden, (40,))
    ct = sr.case(kind, full, True, gid0, policy_set, hidden, (40,))
    rec = Recorder(kind, ce.n, 40)
    # epsilon-greedy
    want = ex.Run(ce, tick0=tick0).launch(40, (ce.seed, ce.threshold))
    eng = shifted(make_explore_engine, gymrs, ce, delta, vec=8)
    eng.rollout_closed_loop(40, explore=True)
    compare(eng, want, "explore", ce.classes[8])
    eng.close()
    eng = shifted(make_explore_engine, gymrs, ce, delta)
    eng.rollout_closed_loop(40, explore=True, record=rec.fresh())
    eng.sync()
    compare(eng, want, "explore, record", ce.classes[4])
    rec.check(want, 40, full, "explore", ce.classes[4])
    eng.close()
    # softmax sampling
    want = sr.Run(cs, tick0=tick0).launch(40, (cs.seed, cs.scale))
    eng = shifted(make_sample_engine, gymrs, cs, delta, vec=8)
    eng.rollout_closed_loop(40, sample=True)
    compare(eng, want, "sample", cs.classes[8])
    eng.close()
    eng = shifted(make_sample_engine, gymrs, cs, delta)
    eng.rollout_closed_loop(40, sample=True, record=rec.fresh())
    eng.sync()
    compare(eng, want, "sample, record", cs.classes[4])
    rec.check(want, 40, full, "sample", cs.classes[4])
    eng.close()
    # transitions, on a table
    want = sr.TransitionsRun(ct, tick0=tick0).launch(40)
    eng = shifted(make_sample_engine, gymrs, ct, delta)
    assert len(eng.param_table()) == ex.TABLE_ROWS and np.array_equal(eng.get_param_index(), ct.index)  # the tail came through
    sink = Sink(rec)
    eng.rollout_transitions(40, record=rec.fresh(), lane_params=True, sample=True, **sink.fresh())
    eng.sync()
    compare(eng, want, "transitions", ct.classes[4])
    rec.check(want, 40, full, "transitions", ct.classes[4])
    sink.check(want, 40, "transitions", ct.classes[4])
    assert want.ended.any() and eng.tick()[0] == tick0 + 40
    eng.close()


# ---- clone and snapshot at a high tick ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,flags", [(0, A | S), (0, A | S | T | F), (1, A | S | T), (2, A | S | T)])
def test_clone_and_snapshot_taken_5_steps_before_the_crossing(gymrs, twin, kind, flags):
    p = Pair(gymrs, twin, kind, 5000, flags, ts.WRAP)
    p.step(24)  # tick 2^32 - 5
    same_stats(kind, p.eng.stats(), p.tw.stats(), "before the copies")
    c = p.eng.clone()
    blob = p.eng.snapshot()
    r = gymrs.BatchedEngine(kind, 5000, global_env_offset=77, flags=flags, params=p.p)
    r.reset(seed=1)
    r.restore(blob)
    assert c.tick() == r.tick() == p.eng.tick() == ((1 << 32) - 5, 3)
    bufs = [torch.empty_like(p.buf) for _ in (c, r)]  # one per engine: each works on its own stream
    for k in range(30):
        for other, buf in zip((c, r), bufs):
            other.fill_actions(buf.data_ptr(), seed=ASEED, t=p.t)
            other.step(buf.data_ptr())
        p.step()
        if k in (3, 4, 5, 29):
            for other in (c, r):
                p.check(other)
    p.check()
    assert p.eng.tick()[0] == (1 << 32) + 25
    for e in (c, r):
        e.close()
    p.close()


def test_a_snapshot_written_before_the_read_out_changed_still_loads_and_continues(gymrs, twin):
    """tests/golden/snapshot_v4_cartpole_n300.bin was saved by the library as it was before the statistics read-out counted lengths
    from ages: CartPole, 300 lanes (one full wave and a ragged one), A|S|T, limit 17, offset 12345, reset(3), moved to WRAP and stepped
    20 times under fill_actions(6, .) -- tick 2^32 - 9.  The format did not change: it loads, shows the twin's state and statistics,
    and continues bit-identically across the crossing."""
    from pathlib import Path

    blob = (Path(__file__).resolve().parent / "golden" / "snapshot_v4_cartpole_n300.bin").read_bytes()
    n, flags = 300, A | S | T
    p = Pair(gymrs, twin, 0, n, flags, ts.WRAP)  # its own engine is the second witness
    p.step(20)
    r = gymrs.BatchedEngine(0, n, global_env_offset=5, flags=flags, params=p.p)
    r.reset(seed=9)
    r.restore(blob)
    assert r.tick() == ((1 << 32) - 9, 3)
    p.check(r)
    buf = torch.empty_like(p.buf)  # r works on its own stream
    for k in range(40):
        r.fill_actions(buf.data_ptr(), seed=ASEED, t=p.t)
        r.step(buf.data_ptr())
        p.step()
        same_stats(0, r.stats(), p.tw.stats(), ("tick", p.tw.tick()))
    p.check(r)
    p.check()
    r.close()
    p.close()
