"""The CPU reference of closed-loop rollouts under a parameter table (tests/closed_loop_table_ref.py) and the case table of
tests/test_gpu_closed_loop_table.py, checked without a GPU: the cases reach every copy of every TableT closed-loop kernel, and the
reference alone shows that a wrong kernel would be noticed there -- episodes end, more than one action, policies that disagree,
and after every launch a lane stepped with its neighbour's row would differ."""
import closed_loop_ref as cl
import closed_loop_table_ref as ref
import numpy as np
import pytest
from closed_loop_table_ref import A, COPIES, F, S, T


def test_the_schedule_avoids_the_multiples_of_the_limit():
    totals = np.cumsum(ref.SCHEDULE)
    assert ref.SCHEDULE == (1, 7, 40, 4) and all(t % ref.MAX_EPISODE_STEPS for t in totals), totals
    assert sum(cl.SCHEDULE) % cl.MAX_EPISODE_STEPS == 0  # why closed_loop_ref's own schedule is not used
    assert totals[-1] > 3 * ref.MAX_EPISODE_STEPS  # several episodes per lane under a time limit


def test_every_kernel_of_the_matrix_steps_lanes_in_all_four_copies():
    table = ref.coverage()
    # 2 envs x 10 flag sets x (fused and fitness at 4 and 8 lanes per work-item + recording at 4)
    assert len(table) == 2 * 10 * 5
    assert {k[:2] + k[3:] for k in table} == {(kind, vec, mode) for kind in (0, 1)
                                              for vec, mode in ((4, "fused"), (8, "fused"), (4, "fitness"), (8, "fitness"), (4, "record"))}
    assert {k[2] for k in table} == set(ref.FLAG_SETS) and len(set(ref.FLAG_SETS)) == 10
    for key, lanes in table.items():
        assert lanes.min() >= 64, (key, dict(zip(COPIES, lanes)))  # at least a wavefront's worth of lanes


def test_the_cases_are_the_ones_the_matrix_names():
    assert len(ref.cases()) == 2 * 4 * 10 * 3 and len(ref.cases(record=True)) == 2 * 2 * 10 * 2
    assert all(ref.records_too(shape, hidden) for _, shape, _, hidden in ref.cases(record=True))
    assert [s[0] for s in ref.SHAPES] == [4200, 5000, 4200, 2900] and [s[1] for s in ref.SHAPES] == [4, 4, 8, 8]
    assert {s[2] for s in ref.SHAPES} == {(1 << 40) + 12345, 12345}
    c = ref.case(1, 1, A | S, 7)
    assert len(c.rows) == 5 and c.index.shape == (5000,) and set(c.index.tolist()) == set(range(5))
    assert all(r.max_episode_steps == 17 for r in c.rows) and c.weights.shape == (3, cl.size_of(1, 7))
    assert np.array_equal(c.policies[:3], [(12345 + i) // 1024 % 3 for i in range(3)])


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("shape", range(len(ref.SHAPES)))
@pytest.mark.parametrize("hidden", ref.HIDDEN)
def test_every_case_is_worth_comparing(kind, shape, hidden):
    """Under every flag set: inside each copy's lanes an episode ended (sets with A or T), two different actions occurred and two
    policies of the set disagreed; after every launch a neighbouring row would show in >= 0.9 of the lanes."""
    lowest = 1.0
    for flags in ref.FLAG_SETS:
        c = ref.case(kind, shape, flags, hidden)
        out = ref.run_case(c)
        assert ref.worth_comparing(c, out) == [], (flags, ref.worth_comparing(c, out))
        lowest = min(lowest, min(launch.told_apart for launch in out))
        last = out[-1]
        assert last.tick == 1 + sum(ref.SCHEDULE) and last.rec_obs.shape == (ref.SCHEDULE[-1], ref.DIMS[kind][0], c.n)
        assert [launch.rec_reward.shape[0] for launch in out] == list(ref.SCHEDULE)
        if not flags & A:
            assert not last.final.any()
        if flags & F:
            assert all(last.final[:, c.classes == copy].any() for copy in np.unique(c.classes))
        assert last.stats[3] == c.n * sum(ref.SCHEDULE)
        if flags & A and flags & S:
            assert last.stats[2] == last.episodes.sum()
        # the fitness records are the recorded rows, folded: column sums against the rows' own totals
        assert last.fitness[:, 1].sum() == last.episodes.sum() and last.fitness[:, 1:].min() >= 0
        if not flags & T:
            assert not last.fitness[:, 3].any() and np.array_equal(last.fitness[:, 1], last.fitness[:, 2])
        assert (last.fitness[:, 1] > 0).all() or not flags & (A | T)  # every policy ended episodes
    print(f"kind {kind} shape {shape} hidden {hidden}: lowest told-apart fraction {lowest:.3f}")


@pytest.mark.parametrize("kind", [0, 1])
def test_reference_rows_getters_and_fitness_are_consistent(kind):
    """The reference against itself: the last recording row of a launch is what the getters show after it, and the fitness records
    are sums of the rows per policy (recounted here lane by lane)."""
    c = ref.case(kind, 1, A | S | T | F, 8)
    out = ref.run_case(c)
    total = np.zeros((ref.N_POLICIES, 4), np.int64)
    for launch in out:
        assert np.array_equal(ref.bits(launch.rec_obs[-1]), ref.bits(launch.obs))
        assert np.array_equal(ref.bits(launch.rec_reward[-1]), ref.bits(launch.reward))
        assert np.array_equal(launch.rec_done[-1], launch.done) and np.array_equal(launch.rec_truncated[-1], launch.truncated)
        for lane in range(0, c.n, 37):
            p = (c.gid0 + lane) // c.lanes_per_policy % ref.N_POLICIES
            assert p == c.policies[lane]
        for p in range(ref.N_POLICIES):
            m = c.policies == p
            total[p] += [int(launch.rec_reward[:, m].sum()), int(((launch.rec_done | launch.rec_truncated)[:, m] != 0).sum()),
                         int(launch.rec_done[:, m].sum()), int(launch.rec_truncated[:, m].sum())]
        assert np.array_equal(launch.fitness, total)
    # every policy ended episodes; over the set, lanes terminated and lanes were truncated (one policy may do only one of the two)
    assert (out[-1].fitness[:, 1] > 0).all() and out[-1].fitness[:, 2].sum() > 0 and out[-1].fitness[:, 3].sum() > 0


@pytest.mark.parametrize("kind", [0, 1])
def test_a_wrong_row_or_a_uniform_engine_would_be_noticed(kind):
    """The same case stepped with every lane on row 0 (what the uniform kernels would do) ends elsewhere"""
    c = ref.case(kind, 0, A | S | T, 7)
    out = ref.run_case(c)
    flat = ref.case(kind, 0, A | S | T, 7)
    flat.index = np.zeros_like(c.index)
    other = ref.run_case(flat)
    differs = (ref.bits(out[-1].state) != ref.bits(other[-1].state)).any(axis=0)
    assert differs[c.index != 0].mean() >= ref.TOLD_APART
    assert not np.array_equal(out[-1].fitness, other[-1].fitness)
