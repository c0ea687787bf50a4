"""gymrs_rollout_transitions against the CPU reference of tests/transitions_ref.py (which never loads the library;
tests/test_transitions_ref.py shows without a GPU that its cases are worth comparing with), against gymrs_rollout_closed_loop on an
identically prepared engine, and against the per-step loop on an engine with GYMRS_FINAL_OBS.

The kernels (gym-rs_amd/csrc/gymrs_transitions.hip, gymrs_table_transitions_<env>.hip) are built per env, with and without a parameter
table, for the eight flag sets with auto-reset at 4 lanes per work-item, and each holds four copies of rollout_block that a wave picks
from at run time.  The matrix meets every family under every flag set, 4200 and 5000 lanes (all four copies), H = 0 and 8, greedy
and exploring, launches of 1, 7, 40 and 4 steps.  Every comparison is bit for bit; final_obs and start_obs are pre-filled with a
NaN sentinel so that an element written where none should be shows."""
import numpy as np
import pytest
import torch
import transitions_ref as ref
from test_gpu_closed_loop_table import DEV, INVALID_ACTION, Recorder, compare, same
from test_gpu_explore import action_buffer, make_engine
from transitions_ref import A, DIMS, F, S, T, bits

pytestmark = pytest.mark.gpu


class Sink:
    """final_obs [rows][D][stride] and start_obs [D][stride] on the device, every word the sentinel"""

    def __init__(self, rec):
        self.rec = rec

    def fresh(self):
        r = self.rec
        self.final = torch.full((r.rows, r.d, r.stride), ref.SENTINEL, dtype=torch.int32, device=DEV)
        self.start = torch.full((r.d, r.stride), ref.SENTINEL, dtype=torch.int32, device=DEV)
        torch.cuda.synchronize()  # torch filled these on its stream; the engine writes them on its own
        return dict(final_obs=self.final.data_ptr(), start_obs=self.start.data_ptr())

    def host(self):
        return self.final.cpu().numpy().view(np.uint32), self.start.cpu().numpy().view(np.uint32)

    def check(self, want, steps, at, classes):
        """The elements under `ended` equal the reference, every other one is still the sentinel; start_obs is the pre-launch observation"""
        n = self.rec.n
        final, start = self.host()
        written = np.zeros(final.shape, bool)
        written[:steps, :, :n] = want.ended[:, None, :]
        assert (final[~written] == ref.SENTINEL).all(), ("final_obs written outside the ended lane-steps", at,
                                                         np.argwhere((final != ref.SENTINEL) & ~written)[:4].tolist())
        got = np.where(written[:steps, :, :n], final[:steps, :, :n], 0).view(np.float32)
        exp = np.where(written[:steps, :, :n], bits(want.final_obs), 0).view(np.float32)
        for t in range(steps):
            same("final_obs", got[t], exp[t], (at, t), classes, want.index)
        same("start_obs", start[:, :n].view(np.float32), want.start_obs, at, classes, want.index)
        assert (start[:, n:] == ref.SENTINEL).all()
        return final


def launch(eng, c, steps, rec, sink, **kw):
    eng.rollout_transitions(steps, record=rec.fresh(), lane_params=c.table, explore=c.explore, **sink.fresh(), **kw)


@pytest.mark.parametrize("kind,table,flags,shape,hidden,explore", ref.matrix())
def test_transitions_equal_the_reference_the_closed_loop_call_and_the_per_step_loop(gymrs, kind, table, flags, shape, hidden, explore):
    c = ref.case(kind, shape, flags, hidden, table, explore)
    want = ref.run_case(c)
    cls = c.classes[4]
    eng, twin = make_engine(gymrs, c, 4, explore=explore), make_engine(gymrs, c, 4, explore=explore)
    c_f = ref.case(kind, shape, flags | F, hidden, table, explore)
    loop = make_engine(gymrs, c_f, 4, explore=explore)
    rec, rec2 = Recorder(kind, c.n, max(c.schedule)), Recorder(kind, c.n, max(c.schedule))
    sink = Sink(rec)
    buf = action_buffer(c.n)
    for k, steps in enumerate(c.schedule):
        launch(eng, c, steps, rec, sink)
        twin.rollout_closed_loop(steps, lane_params=table, explore=explore, record=rec2.fresh())
        eng.sync()
        twin.sync()
        # the reference
        compare(eng, want[k], ("transitions", k), cls)
        rows = rec.check(want[k], steps, flags, ("transitions", k), cls)
        final = sink.check(want[k], steps, k, cls)
        # the existing call on an identically prepared engine: record rows, state, results, statistics, tick, final observations
        rows2 = rec2.check(want[k], steps, flags, ("closed loop", k), cls)
        for a, b in zip(rows, rows2):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), ("record rows differ from rollout_closed_loop's", k)
        assert np.array_equal(bits(eng.get_state()), bits(twin.get_state())) and eng.tick() == twin.tick()
        assert np.array_equal(eng.stats(), twin.stats())
        for a, b in zip(eng.get_step_result(), twin.get_step_result()):
            assert np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))
        if flags & F:
            assert np.array_equal(bits(eng.get_final_obs()), bits(twin.get_final_obs()))
        # the per-step loop on an engine with GYMRS_FINAL_OBS, read after every step
        for t in range(steps):
            (loop.explore_actions if explore else loop.policy_actions)(buf.data_ptr())
            loop.step(buf.data_ptr())
            loop.sync()
            e = want[k].ended[t]
            got = bits(loop.get_final_obs())[:, e]
            assert np.array_equal(got, final[t, :, :c.n][:, e]), ("the per-step loop's final observations differ", k, t)
    for x in (eng, twin, loop):
        x.close()


@pytest.mark.parametrize("kind", [0, 1])
def test_out_of_table_lanes_write_nothing_and_are_reported(gymrs, kind):
    c = ref.case(kind, 0, A | S | T, 0, True, False)
    eng = make_engine(gymrs, c, 4, explore=False)
    bad = [5, 300, c.n - 1]
    index = np.array(c.index, np.uint16)
    index[bad] = ref.K
    eng.set_param_index(index)
    rec = Recorder(kind, c.n, 40)
    sink = Sink(rec)
    launch(eng, c, 40, rec, sink)
    with pytest.raises(gymrs.InvalidActionError) as err:
        eng.sync()
    assert err.value.status == INVALID_ACTION and f"lane {bad[0]} " in str(err.value)
    final, start = sink.host()
    done, trunc = rec.done.cpu().numpy(), rec.trunc.cpu().numpy()
    assert (final[:, :, bad] == ref.SENTINEL).all() and not done[:40, bad].any() and not trunc[:40, bad].any()
    ended = ((done[:40, :c.n] | trunc[:40, :c.n]) != 0)
    written = final[:40, :, :c.n] != ref.SENTINEL
    assert np.array_equal(written, np.broadcast_to(ended[:, None, :], written.shape)) and ended.any()
    eng.close()


def test_refusals_leave_state_and_tick_untouched(gymrs):
    c = ref.case(0, 0, A | S | T, 0, True, False)
    eng = make_engine(gymrs, c, 4, explore=False)
    rec = Recorder(0, c.n, 4)
    sink = Sink(rec)
    before = bits(eng.get_state()).copy(), eng.tick()

    def refused(match, eng=eng, **kw):
        args = dict(record=rec.fresh(), lane_params=True, **sink.fresh())
        args.update(kw)
        with pytest.raises(gymrs.GymrsError, match=match) as err:
            eng.rollout_transitions(4, **args)
        assert err.value.status == 1  # GYMRS_EINVAL

    refused("GYMRS_CLOSED_LOOP_FITNESS", flags=4 | 1)
    refused("unknown flag bits", flags=4 | 2)
    refused("gymrs_set_exploration", explore=True)
    refused("GYMRS_CLOSED_LOOP_LANE_PARAMS", lane_params=False)
    refused("final_obs", final_obs=0)
    refused("16-byte aligned", final_obs=sink.fresh()["final_obs"] + 4)
    refused("16-byte aligned", start_obs=sink.fresh()["start_obs"] + 8)
    broken = rec.fresh()
    broken["lane_stride"] = c.n + 1
    refused("lane_stride", record=broken)
    broken = rec.fresh()
    broken["obs"] = 0
    refused("required", record=broken)
    desc = gymrs.TransitionsDesc(4, 4, gymrs.engine.Trajectory(*[rec.fresh()[f] for f in ("obs", "actions", "reward", "done", "truncated", "lane_stride")]),
                                 sink.fresh()["final_obs"], None, 1)
    lib = eng._lib
    import ctypes as C
    assert lib.gymrs_rollout_transitions(eng._h, C.byref(desc)) == 1 and b"reserved" in lib.gymrs_last_error()
    assert lib.gymrs_rollout_transitions(None, C.byref(desc)) == 1 and lib.gymrs_rollout_transitions(eng._h, None) == 1
    assert np.array_equal(bits(eng.get_state()), before[0]) and eng.tick() == before[1]
    final, start = sink.host()
    assert (final == ref.SENTINEL).all() and (start == ref.SENTINEL).all()
    # n_steps == 0: a no-op after the checks, start_obs included
    eng.rollout_transitions(0, record=rec.fresh(), lane_params=True, **sink.fresh())
    eng.sync()
    final, start = sink.host()
    assert (final == ref.SENTINEL).all() and (start == ref.SENTINEL).all() and eng.tick() == before[1]
    eng.close()
    # engines that cannot take the call
    plain = ref.case(0, 0, A, 0, False, False)
    plain.flags = T  # no auto-reset
    no_auto = make_engine(gymrs, plain, 4, explore=False)
    refused("GYMRS_AUTO_RESET", eng=no_auto, lane_params=False)
    no_auto.close()
    plain.flags = A
    rows = make_engine.__globals__["rows_of"](gymrs, plain)
    no_policy = gymrs.BatchedEngine(0, plain.n, flags=A, params=rows[0])
    no_policy.reset(seed=1)
    refused("gymrs_set_policy", eng=no_policy, lane_params=False)
    no_policy.close()
    pend = gymrs.BatchedEngine(gymrs.PENDULUM, 256, flags=A | T)
    pend.reset(seed=1)
    refused("Pendulum", eng=pend, lane_params=False)
    pend.close()
