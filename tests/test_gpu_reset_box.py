"""A custom reset box (`options` of reset) on every path that re-arms a lane.

gymrs_reset(bounds) replaces the engine's sampling box, and every later GYMRS_AUTO_RESET re-arm draws from it: the per-step kernels,
their copies for chains, captured graphs, the fused rollouts, every closed-loop kernel, the blocks of a sharded engine; clones and
snapshots carry it.  The default boxes cannot show a wrong read of it (CartPole's four components are equal, MountainCar samples
one); the boxes of tests/reset_box_ref.py can, and tests/test_reset_box_ref.py shows without a GPU that the yardsticks used here
deserve the trust: the f32 twin draws what the f64 oracle draws, a permuted or stale box moves every re-armed lane, and the
closed-loop cases re-arm lanes inside every kernel copy, into terminal states and into the general physics path.

Every comparison with the twin or a *_ref run is bit for bit (uint32 views of floats, equal integers and statistics; Pendulum's sum of
returns at rel = 1e-5 as in tests/test_gpu_rollout.py).  The oracle check uses reset_box_ref.tolerance.  Shapes, Pair, Recorder, Sink,
compare, aql and the make_engine functions are those of the existing modules.  The 127 tests of the file take 10 s on an MI355X, the
slowest 0.3 s."""
import explore_ref as ex
import numpy as np
import pytest
import reset_box_ref as rb
import test_gpu_policy_eval as pe
import test_gpu_policy_eval_table as pet
import torch
from test_gpu_aql_chain import aql
from test_gpu_closed_loop_table import DEV, Recorder, compare
from test_gpu_explore import make_engine as make_explore_engine
from test_gpu_high_tick import ASEED, SHAPES, A, F, Pair, S, T, bits, same, same_stats
from test_gpu_sample import make_engine as make_sample_engine
from test_gpu_transitions import Sink

pytestmark = pytest.mark.gpu

SEED = 3  # Pair's reset seed
NAMED = [pytest.param(kind, name, id=f"{kind}-{name}") for kind in (0, 1, 2) for name in rb.NAMED[kind]]
TWO = [pytest.param(kind, name, id=f"{kind}-{name}") for kind, name in ((0, "DISTINCT"), (0, "FAR"), (1, "GOAL"), (1, "FAR"), (2, "DISTINCT"))]


def check_oracle(oracle, p, gid0, bounds, tick, lanes=None, eng=None):
    """The lanes (default all) that the reset or the step from `tick` has just armed hold the f64 oracle's draw of that tick within
    tol_j, inside the box"""
    st = (eng or p.eng).get_state()
    lanes = np.ones(p.n, bool) if lanes is None else lanes
    want = oracle.reset_batch(p.kind, p.n, gid0, SEED, tick, rb.oracle_bounds(p.kind, bounds))
    err = np.abs(st.astype(np.float64) - want)[:, lanes]
    tol = rb.tolerance(p.kind, bounds)
    assert (err <= tol[:, None]).all(), ("oracle", tick, (err / np.maximum(tol[:, None], 1e-300)).max())
    assert rb.inside(p.kind, bounds, st[:, lanes]), ("outside the box", tick)


def ended(p):
    _, d, tr = p.tw.get_result()
    return (d | tr) != 0


def reset_again(p, seed=SEED, bounds=None):
    p.eng.reset(seed=seed, options=bounds)
    p.tw.reset(seed, bounds)
    p.t = p.tw.tick()
    p.final[:] = 0


# ---- 1. the per-step kernel -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [A, A | S, A | T, A | S | T, A | S | T | F])
@pytest.mark.parametrize("kind,name", NAMED)
def test_per_step_kernel(gymrs, twin, oracle, kind, name, flags):
    """60 x fill_actions + step; everything an engine shows against the twin after steps 1, 2, 17, 18 and 60 (the limit is 17), and at
    17 and 18 the lanes that re-armed against the oracle's draw of that tick"""
    bounds = rb.NAMED[kind][name]
    seen = 0
    for n, vec, gid0 in SHAPES:
        p = Pair(gymrs, twin, kind, n, flags, 0, vec=vec, gid0=gid0, bounds=bounds)
        same("state", p.eng.get_state(), p.tw.get_state(), "reset")
        check_oracle(oracle, p, gid0, bounds, 0)
        done = 0
        for upto in (1, 2, 17, 18, 60):
            p.step(upto - done)
            done = upto
            p.check()
            if upto in (17, 18):
                seen += int(ended(p).sum())
                check_oracle(oracle, p, gid0, bounds, p.tw.tick() - 1, ended(p))
        p.close()
    assert seen or (kind == 2 and not flags & T) or (kind == 1 and name == "WALL" and not flags & T)  # (lanes did re-arm there)


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_per_step_kernel_where_every_lane_rearms_on_every_step(gymrs, twin, oracle, kind):
    bounds = rb.NAMED[kind][rb.FIRST[kind]]
    for n, vec, gid0 in SHAPES:
        p = Pair(gymrs, twin, kind, n, A | T, 0, vec=vec, gid0=gid0, limit=1, bounds=bounds)
        done = 0
        for upto in (1, 2, 17, 18, 60):
            p.step(upto - done)
            done = upto
            p.check()
            assert ended(p).all()
            check_oracle(oracle, p, gid0, bounds, p.tw.tick() - 1)
        p.close()


# ---- 2. step_many: eager, graph replays, chains ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,first,second", [(0, "DISTINCT", "FAR"), (0, "TERMINAL", "DISTINCT"), (1, "GOAL", "FAR"), (1, "FAR", "WALL")])
def test_step_many_eager_and_as_graph_replays_across_a_second_reset(gymrs, twin, oracle, kind, first, second):
    """40 steps eager and 40 as graph replays under box B1; reset(same seed, options=B2); 34 graph replays: they follow a twin reset
    with B2 (the box is baked into a captured graph: a reset has to drop it)"""
    b1, b2 = rb.NAMED[kind][first], rb.NAMED[kind][second]
    n, vec, gid0 = SHAPES[0]
    p = Pair(gymrs, twin, kind, n, A | S | T, 0, vec=vec, gid0=gid0, bounds=b1)
    p.step_many(40)
    p.check()
    p.step_many(40, use_graph=True)
    p.check()
    check_oracle(oracle, p, gid0, b1, p.tw.tick() - 1, ended(p))
    reset_again(p, bounds=b2)
    same("state", p.eng.get_state(), p.tw.get_state(), "second reset")
    p.step_many(34, use_graph=True)  # 2 x 17: every lane that did not end on the way is truncated by the last replay
    p.check()
    assert ended(p).any()
    check_oracle(oracle, p, gid0, b2, p.tw.tick() - 1, ended(p))
    p.step(3, stats=True)
    p.check()
    p.close()


def test_step_many_eager_pendulum(gymrs, twin, oracle):
    """(graph replays are refused for Pendulum with the time limit, and without it no lane ever re-arms)"""
    bounds = rb.NAMED[2]["DISTINCT"]
    n, vec, gid0 = SHAPES[1]
    p = Pair(gymrs, twin, 2, n, A | S | T, 0, vec=vec, gid0=gid0, bounds=bounds)
    p.step_many(34)
    p.check()
    assert ended(p).all()  # step 34 = 2 x 17
    check_oracle(oracle, p, gid0, bounds, p.tw.tick() - 1)
    p.step_many(23)
    p.check()
    p.close()


@pytest.mark.parametrize("name", ["DISTINCT", "FAR"])
def test_chain_on_the_engines_own_queue(gymrs, twin, oracle, name):
    """GYMRS_AQL=1: step_many as a chain on the engine's AQL dispatcher, which fills the kernel-argument segment by hand"""
    bounds = rb.NAMED[0][name]
    with aql(True):
        p = Pair(gymrs, twin, 0, 5000, A | S, 0, gid0=64, bounds=bounds)
        p.step_many(48, nbuf=8)
        p.check()
        assert ended(p).any()
        check_oracle(oracle, p, 64, bounds, p.tw.tick() - 1, ended(p))
        p.step_many(24)
    p.check()
    p.step(4, stats=True)
    p.check()
    p.close()


# ---- 3. the fused rollouts --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,name", TWO)
def test_rollout_interleaved_with_the_per_step_kernel(gymrs, twin, oracle, kind, name):
    bounds = rb.NAMED[kind][name]
    for n, vec, gid0 in SHAPES[:2]:
        p = Pair(gymrs, twin, kind, n, A | S | T, 0, vec=vec, gid0=gid0, bounds=bounds)
        for steps in (1, 7, 40, 3):
            p.eng.rollout(steps, action_seed=ASEED, action_t0=p.t)
            for _ in range(steps):
                p.twin_step(p.tw.fill_actions(ASEED, p.t))
            p.check()
        assert ended(p).any()  # step 51 = 3 x 17
        check_oracle(oracle, p, gid0, bounds, p.tw.tick() - 1, ended(p))
        for steps in (9, 9):
            p.step(5)
            p.eng.rollout(steps, action_seed=ASEED, action_t0=p.t)
            for _ in range(steps):
                p.twin_step(p.tw.fill_actions(ASEED, p.t))
            p.check()
        p.close()


@pytest.mark.parametrize("kind,name", TWO)
def test_rollout_record(gymrs, twin, kind, name):
    """Row k of the record = what the twin shows after step k; the engine ends where the twin ends"""
    bounds = rb.NAMED[kind][name]
    n, steps, stride = 5000, 40, 5008
    rec = Pair(gymrs, twin, kind, n, A | S | T, 0, gid0=64, bounds=bounds)
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
        a = rec.tw.fill_actions(ASEED, rec.t)
        rec.twin_step(a)
        r, d, tr = rec.tw.get_result()
        at = ("row", k)
        same("recorded action", act_h[k, :n], a, at)
        same("recorded obs", obs_h[k, :, :n], rec.tw.get_obs(), at)
        same("recorded reward", rew_h[k, :n], r, at)
        same("recorded done", done_h[k, :n], d, at)
        same("recorded truncated", trunc_h[k, :n], tr, at)
    assert np.isnan(obs_h[:, :, n:]).all() and (done_h[:, n:] == 9).all()  # the padding of a row is never written
    rec.check()
    rec.close()


# ---- 4. the closed-loop kernels -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,ps,name,table", rb.closed_loop_cases())
def test_closed_loop_launches(gymrs, kind, ps, name, table):
    """Two launches of 40 steps against the explore_ref / sample_ref runs with `bounds`, launch by launch: rollout_closed_loop plain at 4
    and 8 lanes per work-item, with fitness, with explore, with sample, recording (under explore and under sample), and
    rollout_transitions with sample; with and without a parameter table"""
    full = rb.FULL
    c, greedy = rb.closed_loop_run(kind, ps, name, table, "greedy")
    _, explore = rb.closed_loop_run(kind, ps, name, table, "explore")
    cs, sample = rb.closed_loop_run(kind, ps, name, table, "sample")
    _, trans = rb.transitions_run(kind, ps, name, table)
    rec = Recorder(kind, c.n, max(c.schedule))
    engines = {"plain 4": (make_explore_engine(gymrs, c, 4, explore=False), greedy, {}, 4),
               "plain 8": (make_explore_engine(gymrs, c, 8, explore=False), greedy, {}, 8),
               "fitness": (make_explore_engine(gymrs, c, 4, explore=False), greedy, dict(fitness=True), 4),
               "explore": (make_explore_engine(gymrs, c, 8), explore, dict(explore=True), 8),
               "sample": (make_sample_engine(gymrs, cs, 8), sample, dict(sample=True), 8),
               "explore, record": (make_explore_engine(gymrs, c, 4), explore, dict(explore=True, record=True), 4),
               "sample, record": (make_sample_engine(gymrs, cs, 4), sample, dict(sample=True, record=True), 4)}
    for mode, (eng, want, _, vec) in engines.items():
        assert np.array_equal(bits(eng.get_state()), bits(want[0].start_state)), (mode, "start state")
    for k, steps in enumerate(c.schedule):
        for mode, (eng, want, kw, vec) in engines.items():
            kw = dict(kw)
            if kw.pop("record", False):
                kw["record"] = rec.fresh()
            eng.rollout_closed_loop(steps, lane_params=table, **kw)
            eng.sync()
            compare(eng, want[k], (mode, k), c.classes[vec])
            if "record" in kw:
                rec.check(want[k], steps, full, (mode, k), c.classes[vec])
            if mode == "fitness":
                got = eng.policy_fitness()
                assert np.array_equal(got, want[k].fitness), ("fitness", k, got.tolist(), want[k].fitness.tolist())
    for eng, _, _, _ in engines.values():
        eng.close()
    eng = make_sample_engine(gymrs, cs, 4)
    sink = Sink(rec)
    for k, steps in enumerate(cs.schedule):
        eng.rollout_transitions(steps, record=rec.fresh(), lane_params=table, sample=True, **sink.fresh())
        eng.sync()
        compare(eng, trans[k], ("transitions", k), cs.classes[4])
        rec.check(trans[k], steps, full, ("transitions", k), cs.classes[4])
        sink.check(trans[k], steps, ("transitions", k), cs.classes[4])
        assert trans[k].ended.any()
    eng.close()


# ---- 5. evaluate_policy ignores the box ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("table", [False, True])
@pytest.mark.parametrize("kind", [0, 1])
def test_evaluate_policy_ignores_the_box(gymrs, kind, table):
    """The records and lengths after reset(options=...) equal the existing reference's (the default box) and what the same engine
    returned before that reset"""
    bounds = rb.NAMED[kind][rb.FIRST[kind]]
    if table:
        shape, hidden, common = next(x[1:] for x in pet.tb.cases() if x[0] == kind)
        c, want = pet.reference_of(kind, shape, hidden, common)
        eng = pet.engine_of(gymrs, c)
        run = lambda: pet.evaluate(eng, common=common)  # noqa: E731
    else:
        shape, hidden, common = next(x[1:] for x in pe.ev.cases() if x[0] == kind)
        c, want = pe.reference_of(gymrs, kind, shape, hidden, common)
        eng = pe.engine_for(gymrs, kind, c.n, c.gid0, c.params, c.weights, hidden, c.lanes_per_policy)
        run = lambda: pe.evaluate(eng, pe.E, pe.M, pe.ev.SEED, common)  # noqa: E731
    before = run()
    eng.reset(seed=5, options=bounds)
    assert rb.inside(kind, bounds, eng.get_state())  # (the reset did take the box)
    after = run()
    for got in (before, after):
        assert np.array_equal(got[0], want.records) and np.array_equal(got[1], want.lengths)
    eng.close()


# ---- 6. where the box lives ------------------------------------------------------------------------------------------------------------
def step_both(p, others, steps, at=()):
    """p and the engines `others` (in p's place) `steps` steps forward, each compared with p's twin at the end and after the steps `at`"""
    bufs = [torch.empty_like(p.buf) for _ in others]  # one per engine: each works on its own stream
    for k in range(steps):
        for other, buf in zip(others, bufs):
            other.fill_actions(buf.data_ptr(), seed=ASEED, t=p.t)
            other.step(buf.data_ptr())
        p.step()
        if k in at or k == steps - 1:
            for other in others:
                p.check(other)
    p.check()


@pytest.mark.parametrize("kind,name", TWO)
def test_clone_and_snapshot_carry_the_box(gymrs, twin, oracle, kind, name):
    """clone after reset(options=B); snapshot + restore into an engine that was reset with another box and holds a captured graph of
    it (Pendulum: no graph with the time limit); 30 steps each, and then graph replays on the restored engine"""
    bounds = rb.NAMED[kind][name]
    other_box = rb.NAMED[kind][[x for x in rb.NAMED[kind] if x != name][0]] if kind != 2 else rb.box(2, c0=(-1.0, 0.0), c1=(2.0, 3.0))
    n, vec, gid0 = SHAPES[0]
    flags = A | S | T
    p = Pair(gymrs, twin, kind, n, flags, 0, vec=vec, gid0=gid0, bounds=bounds)
    p.step(4)
    c = p.eng.clone()
    blob = p.eng.snapshot()
    q = Pair(gymrs, twin, kind, n, flags, 0, vec=vec, gid0=gid0, bounds=other_box)
    q.step_many(8, use_graph=kind != 2)
    q.check()
    q.eng.restore(blob)
    step_both(p, (c, q.eng), 30, at=(12, 13))  # steps 17 and 18 since the reset
    check_oracle(oracle, p, gid0, bounds, p.tw.tick() - 1, ended(p), eng=q.eng)
    check_oracle(oracle, p, gid0, bounds, p.tw.tick() - 1, ended(p), eng=c)
    p.eng.close()
    p.eng = q.eng  # the restored engine in p's place: its graph was captured under the other box
    p.step_many(20, use_graph=kind != 2)
    p.check()
    c.close()
    p.close()


@pytest.mark.parametrize("kind,name", TWO)
def test_set_state_set_params_and_set_tuning_leave_the_box_alone_and_a_plain_reset_drops_it(gymrs, twin, oracle, kind, name):
    bounds = rb.NAMED[kind][name]
    n, vec, gid0 = SHAPES[0]
    p = Pair(gymrs, twin, kind, n, A | S | T | F, 0, vec=vec, gid0=gid0, bounds=bounds)
    p.step(3)
    st = p.tw.get_state()
    p.eng.set_state(st)
    p.tw.set_state(st)
    p.eng.set_params(p.p)
    p.tw.set_params(p.p)
    p.eng.set_tuning(8)
    p.step(31)  # step 34 = 2 x 17 since the reset
    p.check()
    assert ended(p).any()
    check_oracle(oracle, p, gid0, bounds, p.tw.tick() - 1, ended(p))
    reset_again(p)  # reset(seed) without options: back to the default box
    same("state", p.eng.get_state(), p.tw.get_state(), "plain reset")
    assert rb.inside(kind, rb.box(kind), p.eng.get_state())
    p.step(30)
    p.check()
    p.close()


@pytest.mark.parametrize("kind", [0, 1])
def test_reset_pcg64_leaves_the_f32_box_for_the_rearms(gymrs, twin, oracle, kind):
    """reset_pcg64(seed, options=B64), then 30 auto-reset steps, against a twin put in the same place with reset(seed, f32(B64)) +
    set_state(the engine's state)"""
    bounds = rb.NAMED[kind][rb.FIRST[kind]]
    n, vec, gid0 = SHAPES[0]
    p = Pair(gymrs, twin, kind, n, A | S | T, 0, vec=vec, gid0=gid0, bounds=bounds)
    p.eng.reset_pcg64(SEED, options=[float(x) for x in bounds])
    st = p.eng.get_state()
    assert not np.array_equal(bits(st), bits(p.tw.get_state())) and (st[0] >= bounds[0]).all() and (st[0] <= bounds[rb.STATE_DIM[kind]]).all()
    p.tw.set_state(st)
    for upto in (17, 13):
        p.step(upto)
        p.check()
    assert ended(p).any()
    check_oracle(oracle, p, gid0, bounds, p.tw.tick() - 1, ended(p))
    p.close()


# ---- 7. a sharded engine ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1])
def test_sharded_blocks_draw_from_the_box(gymrs, twin, oracle, kind):
    """ShardedEngine(kind, n, [0, 0, 0]) after reset(options=...): step, rollout and rollout_closed_loop against one engine (itself
    against the twin)"""
    bounds = rb.NAMED[kind][rb.FIRST[kind]]
    n, vec, gid0 = SHAPES[0]
    flags = A | S | T
    p = Pair(gymrs, twin, kind, n, flags, 0, vec=vec, gid0=gid0, bounds=bounds)
    sh = gymrs.ShardedEngine(kind, n, [0, 0, 0], global_env_offset=gid0, params=p.p, flags=flags)
    assert len(sh.shards) == 3
    sh.reset(seed=SEED, options=bounds)

    def agree(at):
        sh.sync()
        same("state", sh.get_state(), p.eng.get_state(), at)
        for name, x, y in zip(("reward", "done", "truncated"), sh.get_step_result(), p.eng.get_step_result()):
            same(name, x, y, at)
        same_stats(kind, sh.stats(), p.eng.stats(), at)
    agree("reset")
    bufs = [torch.empty(s.n_envs, dtype=torch.uint8, device=DEV) for s in sh.shards]
    torch.cuda.synchronize()
    for _ in range(20):
        sh.fill_actions([b.data_ptr() for b in bufs], seed=ASEED, t=p.t)
        sh.step([b.data_ptr() for b in bufs])
        p.step()
    p.check()
    agree("step")
    check_oracle(oracle, p, gid0, bounds, p.tw.tick() - 1, ended(p))
    sh.rollout(31, action_seed=ASEED, action_t0=p.t)
    p.eng.rollout(31, action_seed=ASEED, action_t0=p.t)
    for _ in range(31):
        p.twin_step(p.tw.fill_actions(ASEED, p.t))
    p.check()
    agree("rollout")
    w = ex.cl.make_weights(kind, 8, 3, ex.WEIGHTS_SEED)
    sh.set_policy(w, hidden=8, lanes_per_policy=1)
    p.eng.set_policy(w, hidden=8, lanes_per_policy=1)
    sh.rollout_closed_loop(40)
    p.eng.rollout_closed_loop(40)
    agree("rollout_closed_loop")
    st = p.eng.get_state()
    _, d, tr = p.eng.get_step_result()
    assert (d | tr).any() and rb.inside(kind, bounds, st[:, (d | tr) != 0])
    sh.close()
    p.close()


# ---- 8. edge boxes and refusals -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(rb.EDGES))
@pytest.mark.parametrize("kind", [0, 1, 2])
def test_edge_boxes(gymrs, twin, oracle, kind, name):
    """The reset, then two steps with max_episode_steps = 1: against the twin bit for bit, against the oracle within tol_j, inside the box"""
    bounds = rb.edge(kind, name)
    for n, vec, gid0 in SHAPES[1:]:
        p = Pair(gymrs, twin, kind, n, A | T, 0, vec=vec, gid0=gid0, limit=1, bounds=bounds)
        same("state", p.eng.get_state(), p.tw.get_state(), "reset")
        check_oracle(oracle, p, gid0, bounds, 0)
        for _ in range(2):
            p.step()
            p.check()
            assert ended(p).all()
            check_oracle(oracle, p, gid0, bounds, p.tw.tick() - 1)
        p.close()


@pytest.mark.parametrize("name", list(rb.REFUSED))
@pytest.mark.parametrize("kind", [0, 1, 2])
def test_degenerate_boxes_are_refused_and_the_engine_keeps_its_box(gymrs, twin, oracle, kind, name):
    """reset, reset_pcg64 and ShardedEngine.reset raise GymrsError; after each refusal 5 more steps against the twin under the previous box"""
    bounds, bad = rb.NAMED[kind][rb.FIRST[kind]], rb.refused(kind, name)
    n, vec, gid0 = SHAPES[1]
    flags = A | S | T
    p = Pair(gymrs, twin, kind, n, flags, 0, vec=vec, gid0=gid0, bounds=bounds)
    p.step(12)
    with pytest.raises(gymrs.GymrsError, match="bounds need finite low < high"):
        p.eng.reset(seed=9, options=bad)
    p.step(5)  # step 17: every lane that has not ended before is truncated and re-arms
    p.check()
    assert ended(p).any()
    check_oracle(oracle, p, gid0, bounds, p.tw.tick() - 1, ended(p))
    if kind != 2:  # (there is no PCG64 reset for Pendulum)
        with pytest.raises(gymrs.GymrsError, match="finite low < high"):
            p.eng.reset_pcg64(9, options=[float(x) for x in bad])
        p.step(5)
        p.check()
    sh = gymrs.ShardedEngine(kind, 5000, [0, 0, 0], global_env_offset=gid0, params=p.p, flags=flags)
    q = Pair(gymrs, twin, kind, 5000, flags, 0, gid0=gid0, bounds=bounds)
    sh.reset(seed=SEED, options=bounds)
    with pytest.raises(gymrs.GymrsError, match="bounds need finite low < high"):
        sh.reset(seed=9, options=bad)
    bufs = [torch.empty(s.n_envs, dtype=q.buf.dtype, device=DEV) for s in sh.shards]
    torch.cuda.synchronize()
    for _ in range(5):
        sh.fill_actions([b.data_ptr() for b in bufs], seed=ASEED, t=q.t)
        sh.step([b.data_ptr() for b in bufs])
        q.step()
    q.check()
    sh.sync()
    same("state", sh.get_state(), q.tw.get_state(), "sharded, after the refusal")
    sh.close()
    q.close()
    p.close()
