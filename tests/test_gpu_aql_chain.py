"""gymrs_step_many through the engine's own AQL dispatcher (gym-rs_amd/csrc/gymrs_aql.h): chains of per-step launches written
straight into an HSA queue, with the agent-scope release fence the HIP runtime puts on every launch only at the END of the
chain.  It is another SUBMISSION PATH for the same kernels, so everything must stay bit for bit what HIP launches produce
(GYMRS_AQL=0) and what the CPU f32 twin computes: states, rewards, flags, statistics -- at ragged and full sizes, with HIP
work on the engine's stream right before a chain (the hand-over into the chain) and right after it (the hand-over back:
the chain's stores must be visible to a copy, a statistics kernel, a HIP-launched step)."""
import json
import os

import numpy as np
import pytest
import torch

from oracle.bindings import TwinEngine

pytestmark = pytest.mark.gpu


class aql:
    """GYMRS_AQL for the calls inside the block (the library looks it up per gymrs_step_many call)."""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        self.before = os.environ.get("GYMRS_AQL")
        os.environ["GYMRS_AQL"] = "1" if self.on else "0"

    def __exit__(self, *exc):
        if self.before is None:
            os.environ.pop("GYMRS_AQL", None)
        else:
            os.environ["GYMRS_AQL"] = self.before


def extras(eng):
    return json.loads(eng.env_json(0))["gymrs"]


@pytest.fixture(autouse=True)
def _needs_the_dispatcher(gymrs):
    """These tests are ABOUT chains.  On a box where the dispatcher's own checks refuse the path (no CPU access to device memory
    through the BAR, a failed self-check) gymrs_step_many uses HIP launches -- covered by the rest of the suite -- and the tests
    here are skipped with the dispatcher's reason instead of failing."""
    with aql(True):
        with gymrs.BatchedEngine(0, 4096, flags=3) as eng:
            eng.reset(seed=1)
            ring = torch.zeros((2, 4096), dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()  # (torch's fill runs on torch's stream, the engine reads on its own)
            eng.step_many(ring.data_ptr(), 4096, 2, 8)
            eng.sync()
            how = extras(eng)["aql"]
    if how != "on":
        pytest.skip(f"AQL dispatcher not available on this box: {how}")


def ring_for(eng, kind, n, nbuf, seed=5):
    ring = torch.empty((nbuf, n), dtype=torch.float32 if kind == 2 else torch.uint8, device="cuda:0")
    for b in range(nbuf):
        eng.fill_actions(ring[b].data_ptr(), seed=seed, t=b)
    return ring  # NOT synchronised: the chain has to wait for these kernels itself


def flags_of(gymrs, kind):
    return gymrs.AUTO_RESET | gymrs.TRACK_STATS | (gymrs.TIME_LIMIT if kind == 2 else 0)


def same(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("n", [4099, 1 << 16])
def test_chain_equals_hip_launches_and_the_twin(gymrs, twin, kind, n):
    nbuf, steps = 5, 67
    flags = flags_of(gymrs, kind)
    engines = {}
    for on in (True, False):
        with aql(on):
            eng = gymrs.BatchedEngine(kind, n, flags=flags, global_env_offset=12345)
            eng.reset(seed=9)
            ring = ring_for(eng, kind, n, nbuf)
            eng.step_many(ring.data_ptr(), ring.stride(0) * ring.element_size(), nbuf, steps)  # no sync before: fills -> chain
            # no sync after either: the copies below ride the engine's stream, behind the chain's hand-over
            engines[on] = (eng, eng.get_state(), eng.get_step_result(), eng.get_obs(), eng.stats(), ring)
    e_on, e_off = engines[True][0], engines[False][0]
    x_on, x_off = extras(e_on), extras(e_off)
    assert x_on["aql"] == "on" and x_on["aql_launches"] == steps and x_on["aql_chains"] == 1, x_on
    assert x_off["aql_launches"] == 0
    for i in (1, 3):
        assert same(engines[True][i], engines[False][i])
    r_on, r_off = engines[True][2], engines[False][2]
    assert same(r_on[0], r_off[0]) and np.array_equal(r_on[1], r_off[1]) and np.array_equal(r_on[2], r_off[2])
    assert np.array_equal(engines[True][4], engines[False][4])
    # and the twin
    tw = TwinEngine(twin, kind, n, e_on.params, flags=flags, gid0=12345)
    tw.reset(9)
    bufs = [tw.fill_actions(5, b) for b in range(nbuf)]
    for t in range(steps):
        tw.step(bufs[t % nbuf])
    assert same(engines[True][1], tw.get_state()) and np.array_equal(engines[True][4], tw.stats())
    assert np.array_equal(r_on[1], tw.get_result()[1])
    for e in (e_on, e_off):
        e.close()


@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("flags", [0, 1, 3, 4, 5, 7])
def test_every_flag_set_has_its_chain(gymrs, twin, kind, flags):
    """Chains are not a fast path for the benchmarked flag sets only: every flag set of the launch table (at 4 lanes per
    work-item) has its kernels in the chain's code object.  A short episode cap, so that engines with GYMRS_TIME_LIMIT do
    truncate; without GYMRS_AUTO_RESET finished lanes stay finished (CartPole's steps_beyond_terminated bookkeeping)."""
    n, nbuf, steps = 20_003, 4, 61
    p = gymrs.engine.default_params(kind)
    p.max_episode_steps = 17
    got = {}
    for on in (True, False):
        with aql(on):
            eng = gymrs.BatchedEngine(kind, n, flags=flags, params=p, global_env_offset=77)
            eng.reset(seed=4)
            ring = ring_for(eng, kind, n, nbuf)
            eng.step_many(ring.data_ptr(), ring.stride(0) * ring.element_size(), nbuf, steps)
            stats = eng.stats() if flags & gymrs.TRACK_STATS else None
            got[on] = (eng, eng.get_state(), eng.get_step_result(), eng.get_obs(), stats, ring)
    x_on = extras(got[True][0])
    assert x_on["aql"] == "on" and x_on["aql_launches"] == steps, x_on
    assert extras(got[False][0])["aql_launches"] == 0
    assert same(got[True][1], got[False][1]) and same(got[True][3], got[False][3])
    for a, b in zip(got[True][2], got[False][2]):
        assert same(a, b) if a.dtype == np.float32 else np.array_equal(a, b)
    tw = TwinEngine(twin, kind, n, p, flags=flags, gid0=77)
    tw.reset(4)
    bufs = [tw.fill_actions(5, b) for b in range(nbuf)]
    for t in range(steps):
        tw.step(bufs[t % nbuf])
    assert same(got[True][1], tw.get_state())
    res = tw.get_result()
    assert same(got[True][2][0], res[0]) and np.array_equal(got[True][2][1], res[1]) and np.array_equal(got[True][2][2], res[2])
    if got[True][4] is not None:
        if kind == 2:  # (Pendulum's returns are float sums taken per wavefront: the twin adds them in another order)
            assert np.allclose(got[True][4], got[False][4], rtol=1e-5) and np.allclose(got[True][4], tw.stats(), rtol=1e-5)
        else:
            assert np.array_equal(got[True][4], got[False][4]) and np.array_equal(got[True][4], tw.stats())
    for on in (True, False):
        got[on][0].close()


def test_chains_interleaved_with_hip_launches_statistics_and_copies(gymrs, twin):
    """chain -> gymrs_step (HIP) -> statistics -> chain -> set_state -> chain -> clone -> chain on both: every boundary between
    the two submission paths, at a size whose reset-log ring is folded inside chains and by the stand-alone kernel."""
    kind, n, nbuf = 0, 70_001, 8
    flags = flags_of(gymrs, kind)
    with aql(True):
        eng = gymrs.BatchedEngine(kind, n, flags=flags)
        tw = TwinEngine(twin, kind, n, eng.params, flags=flags)
        eng.reset(seed=3)
        tw.reset(3)
        ring = ring_for(eng, kind, n, nbuf)
        bufs = [tw.fill_actions(5, b) for b in range(nbuf)]
        stride = ring.stride(0)
        t_dev = 0

        def both(k):
            nonlocal t_dev
            eng.step_many(ring.data_ptr(), stride, nbuf, k)
            for t in range(k):
                tw.step(bufs[t % nbuf])
            t_dev += k

        both(13)                                # a chain that ends in mid-ring (5 rows pending)
        eng.step(ring[0].data_ptr())            # one HIP launch right behind it
        tw.step(bufs[0])
        assert np.array_equal(eng.stats(), tw.stats())   # folds the pending rows with the stand-alone kernel
        both(40)
        assert same(eng.get_state(), tw.get_state())
        st = eng.get_state()
        st[:, :100] = 0.01
        eng.set_state(st)
        tw.set_state(st)
        both(9)
        twin_clone_state = tw.get_state().copy()
        clone = eng.clone()
        both(24)
        clone.step_many(ring.data_ptr(), stride, nbuf, 24)   # the clone builds its own chain object
        assert same(clone.get_state(), eng.get_state()) and np.array_equal(clone.stats(), eng.stats())
        assert same(eng.get_state(), tw.get_state()) and np.array_equal(eng.stats(), tw.stats())
        assert not same(twin_clone_state, tw.get_state())
        x = extras(eng)
        assert x["aql"] == "on" and x["aql_chains"] == 4 and x["aql_launches"] == 13 + 40 + 9 + 24
        assert extras(clone)["aql_chains"] == 1
        clone.close()
        eng.close()


@pytest.mark.parametrize("n,auto_reset", [(1000, True), (64, False)])
def test_pendulum_episode_clock_crosses_every_submission_path(gymrs, twin, n, auto_reset):
    """Pendulum's uniform episode clock is host bookkeeping every submission path shares: gymrs_step -> eager gymrs_step_many -> a
    chain -> the fused rollout -> gymrs_step -> eager again, with a limit of 7 steps reached in mid-call and at the end of a call.  1000 lanes: ragged,
    under one workgroup row; 64 lanes without auto-reset: the mapped host pool (its gymrs_step_many stays with HIP launches), and a
    clock that never restarts."""
    flags = gymrs.TIME_LIMIT | ((gymrs.AUTO_RESET | gymrs.TRACK_STATS) if auto_reset else 0)
    p = gymrs.engine.default_params(2)
    p.max_episode_steps = 7
    nbuf, seed = 4, 5
    eng = gymrs.BatchedEngine(2, n, flags=flags, params=p)
    tw = TwinEngine(twin, 2, n, p, flags=flags)
    eng.reset(seed=3)
    tw.reset(3)
    ring = ring_for(eng, 2, n, nbuf, seed=seed)
    bufs = [tw.fill_actions(seed, b) for b in range(nbuf)]
    stride = ring.stride(0) * ring.element_size()
    truncations = []

    def check(twin_actions):
        for a in twin_actions:
            tw.step(a)
        want, got = tw.get_result(), eng.get_step_result()
        assert same(eng.get_state(), tw.get_state())
        assert same(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
        assert len(np.unique(got[2])) == 1  # the clock is uniform
        truncations.append(int(got[2][0]))

    eng.step(ring[0].data_ptr())
    check(bufs[:1])
    with aql(False):
        eng.step_many(ring.data_ptr(), stride, nbuf, 3)
    check([bufs[t % nbuf] for t in range(3)])
    with aql(True):
        eng.step_many(ring.data_ptr(), stride, nbuf, 9)
    check([bufs[t % nbuf] for t in range(9)])
    eng.rollout(5, action_seed=seed, action_t0=2)
    check([tw.fill_actions(seed, 2 + k) for k in range(5)])
    eng.step(ring[1].data_ptr())
    check(bufs[1:2])
    with aql(False):
        eng.step_many(ring.data_ptr(), stride, nbuf, 2)  # (to the third limit: the last step of the call is the 21st)
    check(bufs[:2])
    # the calls end after 1, 4, 13, 18, 19 and 21 steps; with auto-reset steps 7, 14 and 21 truncate and restart the clock, without
    # it every step from the seventh on truncates
    assert truncations == ([0, 0, 0, 0, 0, 1] if auto_reset else [0, 0, 1, 1, 1, 1])
    assert extras(eng)["aql_launches"] == (9 if n > 64 else 0)
    assert eng.stats()[3] == 21 * n
    assert eng.tick()[0] == 1 + 21  # (the reset took tick 0)
    eng.close()


def test_short_calls_graphs_small_engines_and_other_launch_shapes_keep_to_hip_launches(gymrs):
    n = 5000
    with aql(True):
        with gymrs.BatchedEngine(0, n, flags=gymrs.AUTO_RESET | gymrs.TRACK_STATS) as eng:
            eng.reset(seed=1)
            ring = ring_for(eng, 0, n, 4)
            eng.step_many(ring.data_ptr(), n, 4, 3)      # shorter than a chain is worth
            assert extras(eng)["aql_launches"] == 0
            eng.step_many(ring.data_ptr(), n, 4, 40, use_graph=True)   # graph replays are HIP's
            assert extras(eng)["aql_launches"] == 0
        with gymrs.BatchedEngine(0, 48, flags=gymrs.AUTO_RESET | gymrs.TRACK_STATS) as eng:   # a small engine's arrays are mapped host memory
            eng.reset(seed=1)
            ring = ring_for(eng, 0, 48, 4)
            eng.step_many(ring.data_ptr(), 48, 4, 40)
            assert extras(eng)["aql_launches"] == 0
        # 8 lanes per work-item (a tuning knob): the chain's code object holds the 4-lane kernels only
        with gymrs.BatchedEngine(0, n, flags=gymrs.AUTO_RESET | gymrs.TRACK_STATS, lanes_per_thread=8) as eng:
            eng.reset(seed=1)
            ring = ring_for(eng, 0, n, 4)
            eng.step_many(ring.data_ptr(), n, 4, 40)
            assert extras(eng)["aql_launches"] == 0


def test_invalid_action_inside_a_chain_is_reported(gymrs):
    n = 10_000
    with aql(True):
        with gymrs.BatchedEngine(0, n, flags=gymrs.AUTO_RESET | gymrs.TRACK_STATS) as eng:
            eng.reset(seed=1)
            ring = ring_for(eng, 0, n, 4)
            torch.cuda.synchronize()
            ring[2, 777] = 9
            torch.cuda.synchronize()
            eng.step_many(ring.data_ptr(), n, 4, 16)
            with pytest.raises(gymrs.GymrsError, match="invalid action"):
                eng.sync()
            assert extras(eng)["aql_launches"] == 16


def _full_size_both_ways(gymrs, steps, repetitions):
    n, nbuf = 1 << 20, 32
    flags = flags_of(gymrs, 0)
    out = {}
    for on in (True, False):
        with aql(on):
            eng = gymrs.BatchedEngine(0, n, flags=flags)
            eng.reset(seed=0)
            ring = ring_for(eng, 0, n, nbuf, seed=1)
            eng.step_many(ring.data_ptr(), n, nbuf, 300)
            eng.sync()
            stream = torch.cuda.ExternalStream(eng.stream, device=torch.device("cuda", 0))
            times = []
            for _ in range(repetitions):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                eng.step_many(ring.data_ptr(), n, nbuf, steps)
                e1.record(stream)
                eng.sync()
                times.append(e0.elapsed_time(e1) * 1e3 / steps)
            out[on] = (eng.get_state(), eng.stats(), sorted(times)[len(times) // 2], extras(eng))
            eng.close()
    return out


def test_full_size_chain_is_bit_identical(gymrs):
    """2^20 lanes (BASELINE configs[1]): 1000-step chains against 1000 HIP launches -- same bits, same statistics."""
    steps = 1000
    out = _full_size_both_ways(gymrs, steps, 2)
    assert same(out[True][0], out[False][0]) and np.array_equal(out[True][1], out[False][1])
    assert out[True][3]["aql_launches"] == 300 + 2 * steps and out[False][3]["aql_launches"] == 0


@pytest.mark.perf
def test_full_size_chain_is_faster(gymrs):
    """The reason the path exists: the chain is faster (the HIP runtime's per-launch release fence costs this kernel > 1 us).  A timing
    relation: runs after every correctness test (conftest.GPU_ORDER)."""
    out = _full_size_both_ways(gymrs, 1000, 5)
    print(f"us per 2^20-lane step: AQL chain {out[True][2]:.3f}, HIP launches {out[False][2]:.3f}")
    assert out[True][2] < out[False][2]


def test_a_chain_launch_on_an_unexpected_xcd_is_loud(gymrs, twin):
    """The launches of a chain carry no release fence, which is only right while workgroup i runs on the same XCD in every launch.  The
    FIRST launch of every chain records, per residue class of the workgroup index (mod 8), the XCC it runs on (HW_REG_XCC_ID) into the chain
    object's own table, tagged with the chain's number (StepArgs::xcc_table); every later launch of that chain compares.  A table nobody's
    XCC matches -- and no recording launch -- (test hook gymrs_dev_set_hooks bit 0: the table is overwritten on the stream ahead of the chain)
    stands in for a deal that changed under the engine: gymrs_sync must fail with GYMRS_EHIP, the chain object is DISCARDED (not parked for the
    next engine) and the engine goes on through HIP launches (VERDICT r3 "next" #3)."""
    n, nbuf = 20_000, 4
    flags = flags_of(gymrs, 0)
    with aql(True):
        with gymrs.BatchedEngine(0, n, flags=flags) as eng:
            eng.reset(seed=4)
            ring = ring_for(eng, 0, n, nbuf)
            eng.step_many(ring.data_ptr(), n, nbuf, 16)
            eng.sync()  # the true table: silent
            assert extras(eng)["aql"] == "on" and extras(eng)["aql_launches"] == 16
            import ctypes as C

            lib = gymrs.load_library()
            lib.gymrs_dev_set_hooks.argtypes = [C.c_void_p, C.c_uint32]
            assert lib.gymrs_dev_set_hooks(eng._h, 1) == 0
            try:
                eng.step_many(ring.data_ptr(), n, nbuf, 16)
                # EVERY read-out that synchronises reports it, not only gymrs_sync: here the first one after the chain is a host copy
                with pytest.raises(gymrs.GymrsError, match="another XCD") as info:
                    eng.get_state()
                assert info.value.status == 2  # GYMRS_EHIP
                eng.sync()  # reported once
            finally:
                assert lib.gymrs_dev_set_hooks(eng._h, 0) == 0
            x = extras(eng)
            assert x["aql"] != "on" and "XCD" in x["aql"] and x["aql_launches"] == 32, x
            eng.step_many(ring.data_ptr(), n, nbuf, 16)  # HIP launches from here on
            eng.sync()
            assert extras(eng)["aql_launches"] == 32
            # (the deal had not really changed: the values are what the twin computes)
            tw = TwinEngine(twin, 0, n, eng.params, flags=flags)
            tw.reset(4)
            bufs = [tw.fill_actions(5, b) for b in range(nbuf)]
            for t in range(48):
                tw.step(bufs[t % nbuf])
            assert same(eng.get_state(), tw.get_state()) and np.array_equal(eng.stats(), tw.stats())


def test_three_engines_in_one_process_alternate_chains(gymrs, twin):
    """Several engines = several chain queues next to several stream queues.  On some placements of a stream's queue and its
    chain's queue the asynchronous hand-over (a one-wave kernel in flight on the stream while the chain runs) slows the chain
    by a factor of 3-6 (profiles/r03_two_engines.log); every engine therefore times both hand-overs on its own stream once and
    keeps the synchronous one where the asynchronous one costs.  Whatever each engine picked: same bits as the twin, and no
    engine's chains are slower than twice the fastest engine's."""
    import time

    n, nbuf, steps = 1 << 18, 4, 400
    flags = flags_of(gymrs, 0)
    with aql(True):
        engines = []
        for k in range(3):
            eng = gymrs.BatchedEngine(0, n, flags=flags, global_env_offset=k * n)
            eng.reset(seed=11)
            engines.append((eng, ring_for(eng, 0, n, nbuf)))
        rates = [[] for _ in engines]
        for rnd in range(4):
            for k, (eng, ring) in enumerate(engines):
                eng.sync()
                t0 = time.perf_counter()
                eng.step_many(ring.data_ptr(), n, nbuf, steps)
                eng.sync()
                rates[k].append((time.perf_counter() - t0) * 1e6 / steps)
        best = [min(r[1:]) for r in rates]  # (the first round includes the calibration)
        for k, (eng, ring) in enumerate(engines):
            x = extras(eng)
            assert x["aql"] == "on" and x["aql_launches"] == 4 * steps and x["aql_handover"], x
            tw = TwinEngine(twin, 0, n, eng.params, flags=flags, gid0=k * n)
            tw.reset(11)
            bufs = [tw.fill_actions(5, b) for b in range(nbuf)]
            for _ in range(4):
                for t in range(steps):
                    tw.step(bufs[t % nbuf])
            assert same(eng.get_state(), tw.get_state()) and np.array_equal(eng.stats(), tw.stats())
            eng.close()
        assert max(best) < 2.0 * min(best), rates  # (a coarse timing relation, checked after the bits: a factor of 2, not a rate)


def test_engines_beyond_the_queue_budget_keep_to_hip_launches(gymrs):
    """Every chain object is a hardware queue of its own: a process drives at most 8 engines per device through chains
    (gymrs_aql.hip: kMaxChainsPerDevice); the others say so and step through HIP launches -- with the same results -- and an
    engine created after some of the first were closed gets a chain again."""
    n, nbuf, steps = 8192, 2, 16
    flags = flags_of(gymrs, 0)
    with aql(True):
        engines, states = [], []
        for k in range(11):
            eng = gymrs.BatchedEngine(0, n, flags=flags)
            eng.reset(seed=2)
            ring = ring_for(eng, 0, n, nbuf)
            eng.step_many(ring.data_ptr(), n, nbuf, steps)
            engines.append(eng)
            states.append(eng.get_state())
        how = [extras(e)["aql"] for e in engines]
        assert how[:8] == ["on"] * 8 and all("already drives" in h for h in how[8:]), how
        assert [extras(e)["aql_launches"] for e in engines] == [steps] * 8 + [0] * 3
        assert all(same(states[0], st) for st in states[1:])
        for e in engines[:4]:
            e.close()
        with gymrs.BatchedEngine(0, n, flags=flags) as late:
            late.reset(seed=2)
            ring = ring_for(late, 0, n, nbuf)
            late.step_many(ring.data_ptr(), n, nbuf, steps)
            assert extras(late)["aql"] == "on" and same(late.get_state(), states[0])
        for e in engines[4:]:
            e.close()


@pytest.mark.parametrize("kind,steps", [(2, 450), (0, 300), (1, 450)])
def test_long_chains_forced_hints_reset_and_restore(gymrs, twin, kind, steps):
    """Chains that cross Pendulum's 200-step time limit twice (the host-computed truncate_all argument changes inside a chain), with
    the memory hint forced both ways (gymrs_set_tuning: the `_nt` and `_pl` kernel variants), a seeded reset, stats_clear and a
    snapshot restore between chains: bits and statistics of the twin every time."""
    n, nbuf = 9001, 6
    flags = flags_of(gymrs, kind)
    with aql(True):
        eng = gymrs.BatchedEngine(kind, n, flags=flags, global_env_offset=77)
        tw = TwinEngine(twin, kind, n, eng.params, flags=flags, gid0=77)
        eng.reset(seed=21)
        tw.reset(21)
        ring = ring_for(eng, kind, n, nbuf)
        bufs = [tw.fill_actions(5, b) for b in range(nbuf)]
        stride = ring.stride(0) * ring.element_size()

        def both(k):
            eng.step_many(ring.data_ptr(), stride, nbuf, k)
            for t in range(k):
                tw.step(bufs[t % nbuf])

        def stats_equal(gs, ts):  # Pendulum's sum of returns is a float sum over waves: the order differs from the twin's
            return (np.array_equal(gs[1:], ts[1:]) and gs[0] == pytest.approx(ts[0], rel=1e-5)) if kind == 2 else np.array_equal(gs, ts)

        def check(what):
            assert same(eng.get_state(), tw.get_state()), what
            assert stats_equal(eng.stats(), tw.stats()), (what, eng.stats(), tw.stats())
            r, d, tr = eng.get_step_result()
            tr_, td, tt = tw.get_result()
            assert np.array_equal(d, td) and np.array_equal(tr, tt) and same(r, tr_), what

        both(steps)
        check("automatic hints")
        eng.set_tuning(4, 1)   # every access hinted
        both(steps // 2)
        check("forced non-temporal")
        eng.set_tuning(4, 2)   # none
        both(steps // 2)
        check("forced plain")
        eng.set_tuning(4, 0)
        blob = eng.snapshot()
        tw_state, tw_stats = tw.get_state().copy(), tw.stats().copy()
        both(40)
        eng.restore(blob)      # back to the snapshot: the twin is rebuilt to the same point by replaying
        tw2 = TwinEngine(twin, kind, n, eng.params, flags=flags, gid0=77)
        tw2.reset(21)
        for k in (steps, steps // 2, steps // 2):
            for t in range(k):
                tw2.step(bufs[t % nbuf])
        assert same(tw2.get_state(), tw_state) and np.array_equal(tw2.stats(), tw_stats)
        assert same(eng.get_state(), tw_state) and stats_equal(eng.stats(), tw_stats)
        tw = tw2
        both(33)
        check("after the restore")
        eng.stats_clear()
        tw.stats_clear()
        eng.reset(seed=5)
        tw.reset(5)
        both(64)
        check("after stats_clear + reset")
        x = extras(eng)
        assert x["aql"] == "on" and x["aql_launches"] == steps + 2 * (steps // 2) + 40 + 33 + 64, x
        eng.close()
