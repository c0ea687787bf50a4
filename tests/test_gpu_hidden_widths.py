"""Hidden widths 1, 7 and 64 in every exploring, sampling, recording and transitions kernel, in the per-step explore_actions and
sample_actions and in evaluate_policy, against the CPU references that tests/hidden_width_ref.py borrows (explore_ref, sample_ref,
transitions_ref, policy_eval_ref, policy_eval_table_ref: the f32 twin, tests/cpp/policy_ref.c, tests/cpp/sample_ref.c, a numpy
Philox).  The other GPU modules meet these kernels with H = 0 and 8, which never enter the remainder of the four-unit loop over the
hidden layer; tests/test_hidden_width_ref.py shows on the CPU that every case here would notice a kernel that dropped its last units.

One test per family instance (family, env, with or without a parameter table, lanes per work-item): its widths run on ONE engine,
with set_policy, a seeded reset and (MountainCar) set_state in between.  Every comparison is bit for bit (uint32 views of floats, equal
integers, statistics and records with ==; for `prob` on non-finite observations a NaN equals any NaN, as elsewhere in the suite)."""
import hidden_width_ref as hw
import lane_params_ref as lp
import numpy as np
import policy_eval_ref as ev
import pytest
from test_gpu_closed_loop_table import Recorder, compare, same
from test_gpu_explore import action_buffer
from test_gpu_explore import make_engine as explore_engine
from test_gpu_policy_eval import assert_lengths, assert_records, engine_for, evaluate
from test_gpu_policy_eval_table import evaluate as evaluate_table
from test_gpu_policy_eval_table import table_engine
from test_gpu_sample import make_engine as sample_engine
from test_gpu_sample import prob_buffer
from test_gpu_transitions import Sink

pytestmark = pytest.mark.gpu

ROLLOUTS = [inst for group in ("closed", "record", "transitions") for inst in hw.instances(group)]


def at_width(gymrs, eng, c):
    """The instance's one engine with case c on it: built for the first width (the make_engine of the family's own module), for
    the next ones given c's policy set, reset with the seed and prepared again; the settings of c's action source either way"""
    if eng is None:
        return (sample_engine if c.source == "sample" else explore_engine)(gymrs, c, c.vec, c.source != "policy")
    eng.set_policy(c.weights, hidden=c.hidden, lanes_per_policy=c.lanes_per_policy)
    eng.reset(seed=c.reset_seed)
    if c.prepare is not None:
        eng.set_state(c.prepare(eng.get_state()))
    if c.source == "sample":
        eng.set_sampling(c.seed, scale=c.scale)
    elif c.source == "explore":
        eng.set_exploration(c.seed, threshold=c.threshold)
    return eng


def greedy_is_policy_actions(eng, c, want_action, want_greedy, at):
    """policy_actions (policy_eval, the argmax copy of the layer) gives the action the sampling reference reports as `greedy`, and
    sample_actions (policy_logits) the reference's sampled one, on the engine's current observations"""
    greedy, sampled = action_buffer(c.n), action_buffer(c.n)
    eng.policy_actions(greedy.data_ptr())
    eng.sample_actions(sampled.data_ptr())
    eng.sync()
    same("policy_actions against the sampling reference's greedy action", greedy.cpu().numpy()[:c.n], want_greedy, at, c.copies, c.index)
    same("sample_actions", sampled.cpu().numpy()[:c.n], want_action, at, c.copies, c.index)
    assert (greedy.cpu().numpy()[c.n:] == 9).all() and (sampled.cpu().numpy()[c.n:] == 9).all()


@pytest.mark.parametrize("inst", ROLLOUTS, ids=lambda i: i.id)
def test_rollouts_equal_the_cpu_reference_at_every_width(gymrs, inst):
    """The fused launch (with the fitness records where the family counts them), the recording launch (its rows) or
    rollout_transitions (its rows, final_obs on the ended lane-steps only, start_obs), launch by launch: state, observations, last
    results, final observations, statistics and tick after each.  The sampling recorders at width 7 also tie the layer's two copies."""
    eng = None
    for hidden in hw.WIDTHS:
        c = hw.case(inst, hidden)
        ref = hw.run_case(c)
        want = ref.out
        eng = at_width(gymrs, eng, c)
        same("start state", eng.get_state(), want[0].start_state, hidden, c.copies, c.index)
        if hidden == 7 and c.source == "sample" and c.group != "closed":
            greedy_is_policy_actions(eng, c, ref.actions[0], ref.greedy[0], hidden)
        rec = Recorder(c.kind, c.n, max(c.schedule))
        sink = Sink(rec)
        how = dict(lane_params=c.table, explore=c.source == "explore", sample=c.source == "sample")
        fitness = c.family.endswith("_fitness")
        for k, steps in enumerate(c.schedule):
            at = (hidden, k)
            if c.group == "transitions":
                eng.rollout_transitions(steps, record=rec.fresh(), **sink.fresh(), **how)
            else:
                eng.rollout_closed_loop(steps, fitness=fitness, record=rec.fresh() if c.group == "record" else None, **how)
            eng.sync()
            compare(eng, want[k], at, c.copies)
            if c.group != "closed":
                rec.check(want[k], steps, c.flags, at, c.copies)
            if c.group == "transitions":
                sink.check(want[k], steps, at, c.copies)
            if fitness:
                got = eng.policy_fitness()
                assert np.array_equal(got, want[k].fitness), ("fitness", at, got.tolist(), want[k].fitness.tolist())
        assert fitness or not eng.policy_fitness().any()  # the other calls count nothing
    eng.close()


@pytest.mark.parametrize("inst", hw.instances("step"), ids=lambda i: i.id)
def test_per_step_calls_equal_the_cpu_reference_at_every_width(gymrs, inst):
    """explore_actions, and sample_actions with a `prob` buffer (it depends on every unit of the layer), on the reset observations
    and on observations with NaNs, infinities, huge and denormal values; nothing beyond n_envs is written"""
    eng = None
    for hidden in hw.WIDTHS:
        c = hw.case(inst, hidden)
        eng = at_width(gymrs, eng, c)
        for j, want in enumerate(hw.run_case(c)):
            at = (hidden, j)
            if j:
                eng.set_state(want.obs)
            same("observations", eng.get_obs(), want.obs, at, c.copies, c.index, nan_equal=True)
            buf, pbuf = action_buffer(c.n), prob_buffer(c.n)
            if c.source == "sample":
                eng.sample_actions(buf.data_ptr(), pbuf.data_ptr())
            else:
                eng.explore_actions(buf.data_ptr())
            eng.sync()
            got, gp = buf.cpu().numpy(), pbuf.cpu().numpy()
            same("actions", got[:c.n], want.actions, at, c.copies, c.index)
            assert (got[c.n:] == 9).all() and (gp[c.n if c.source == "sample" else 0:] == -7.0).all()
            if c.source == "sample":
                same("prob", gp[:c.n], want.prob, at, c.copies, c.index, nan_equal=True)
                if hidden == 7:
                    greedy_is_policy_actions(eng, c, want.actions, want.greedy, at)
    eng.close()


@pytest.mark.parametrize("inst", hw.instances("eval"), ids=lambda i: i.id)
def test_evaluate_policy_equals_the_cpu_reference_at_widths_1_and_64(gymrs, inst):
    """All eight fields of every policy's record and the whole `lengths` buffer, with == on integers"""
    eng = None
    for hidden in hw.EVAL_WIDTHS:
        c = hw.case(inst, hidden)
        want = hw.run_case(c)
        if eng is not None:
            eng.set_policy(c.weights, hidden=hidden, lanes_per_policy=c.lanes_per_policy)
        elif c.table:
            eng = table_engine(gymrs, c.kind, c.n, c.gid0, c.rows, c.index, c.weights, hidden, c.lanes_per_policy)
        else:
            params = lp.rows_for(type(gymrs.engine.default_params(c.kind)), c.rows)[0]
            eng = engine_for(gymrs, c.kind, c.n, c.gid0, params, c.weights, hidden, c.lanes_per_policy)
        got, lengths = evaluate_table(eng, common=c.common) if c.table else evaluate(eng, ev.EPISODES, ev.MAX_STEPS, ev.SEED, c.common)
        assert_lengths(lengths, want.lengths, c.copies, (hidden, c.common))
        assert_records(got, want.records, (hidden, c.common))
    eng.close()
