"""The CPU closed-loop reference (tests/closed_loop_ref.py) and the case table of tests/test_gpu_policy_matrix.py, checked without a
GPU: the cases reach every copy of the rollout kernel, and inside each copy's lanes the reference alone shows that a wrong kernel
would be noticed there (episodes end, more than one action, policies that disagree, final observations kept)."""
import closed_loop_ref as ref
import numpy as np
import pytest
from closed_loop_ref import A, COPIES, F, S, T


def waves_per_copy(n, vec, gid0, n_policies, lpp):
    first = ref.wave_classes(n, vec, gid0, n_policies, lpp)[::64 * vec]  # one lane per wave
    return {COPIES[c]: int(k) for c, k in enumerate(np.bincount(first, minlength=4)) if k}


def test_wave_classes_on_the_shapes_of_test_gpu_policy():
    """Pins the restatement of the selection rule: the waves of tests/test_gpu_policy.py's fused cases, classified by hand from
    policy_select and the `full` test when the matrix was written."""
    assert waves_per_copy(5000, 4, 12345, 5, 3) == {"gathered-full": 19, "gathered-ragged": 1}
    assert waves_per_copy(5000, 4, 12345, 3, 1024) == {"uniform-full": 15, "gathered-full": 4, "gathered-ragged": 1}
    assert waves_per_copy(777, 8, 12345, 5, 3) == {"gathered-full": 1, "gathered-ragged": 1}
    assert waves_per_copy(777, 8, 12345, 3, 1024) == {"uniform-full": 1, "gathered-ragged": 1}
    assert waves_per_copy(6001, 4, 64, 4, 256) == {"gathered-full": 23, "gathered-ragged": 1}
    assert waves_per_copy(5001, 4, 64, 5, 3) == {"gathered-full": 19, "gathered-ragged": 1}
    assert waves_per_copy(1 << 20, 4, 0, 1, 1) == {"uniform-full": 4096}


def test_wave_classes_lane_counts():
    big = (1 << 40) + 12345
    assert ref.lanes_per_copy(5000, 4, 12345, 3, 1000) == {"uniform-full": 3584, "gathered-full": 1280, "uniform-ragged": 136}
    assert ref.lanes_per_copy(4200, 4, big, 3, 1000) == {"uniform-full": 3072, "gathered-full": 1024, "uniform-ragged": 104}
    assert ref.lanes_per_copy(4200, 8, big, 3, 1000) == {"uniform-full": 2048, "gathered-full": 2048, "uniform-ragged": 104}
    assert ref.lanes_per_copy(2900, 8, 12345, 3, 1000) == {"uniform-full": 1536, "gathered-full": 1024, "gathered-ragged": 340}
    assert ref.lanes_per_copy(5000, 4, 12345, 3, 1024) == {"uniform-full": 3840, "gathered-full": 1024, "gathered-ragged": 136}
    # a wave is one class; exact multiples of a wave have no ragged wave; one policy is always uniform
    assert ref.lanes_per_copy(512, 4, 7, 1, 1) == {"uniform-full": 512}
    assert ref.lanes_per_copy(513, 8, 0, 2, 1 << 40) == {"uniform-full": 512, "uniform-ragged": 1}
    assert ref.lanes_per_copy(100, 4, 0, 2, 1) == {"gathered-ragged": 100}
    # lanes_per_policy beyond 2^32: the block's remainder needs all 64 bits
    lpp = (1 << 32) + 1000
    assert ref.lanes_per_copy(600, 4, lpp - 100, 3, lpp) == {"gathered-full": 256, "uniform-full": 256, "uniform-ragged": 88}


@pytest.mark.parametrize("vec", [4, 8])
def test_the_case_table_reaches_all_four_copies(vec):
    lanes = np.zeros(4, np.int64)
    shapes = [s for s in ref.SHAPES if s[1] == vec]
    assert len(shapes) == 2
    for n, _, gid0, lpp in shapes:
        per_shape = np.bincount(ref.wave_classes(n, vec, gid0, ref.N_POLICIES, lpp), minlength=4)
        assert (per_shape > 0).sum() == 3 and per_shape[2:].min() == 0  # one ragged wave with lanes per launch
        lanes += per_shape
    assert lanes.min() >= 64, dict(zip(COPIES, lanes))  # every copy steps at least a wavefront's worth of lanes


def test_every_kernel_of_the_matrix_steps_lanes_in_all_four_copies():
    table = ref.coverage()
    # 2 envs x (2 vector widths + the recording kernel at 4 lanes per work-item) x 10 flag sets
    assert len(table) == 2 * 3 * 10
    assert {k[:2] + k[3:] for k in table} == {(kind, vec, rec) for kind in (0, 1) for vec, rec in ((4, False), (8, False), (4, True))}
    for key, lanes in table.items():
        assert lanes.min() > 0, (key, dict(zip(COPIES, lanes)))


def test_the_flag_sets_are_the_ten_the_kernels_are_built_for():
    assert len(set(ref.FLAG_SETS)) == 10
    assert set(ref.FLAG_SETS) == {0, A, A | S, T, A | T, A | S | T, A | F, A | S | F, A | T | F, A | S | T | F}


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("shape", range(len(ref.SHAPES)))
@pytest.mark.parametrize("hidden", ref.HIDDEN)
def test_every_case_is_worth_comparing(gymrs, kind, shape, hidden):
    """Under every flag set, inside each copy's lanes: an episode ended (sets with A or T), two different actions occurred, two
    policies of the set disagreed, and with F a final observation was kept.  MountainCar is not exempt."""
    for flags in ref.FLAG_SETS:
        c = ref.case(kind, shape, flags, hidden, gymrs.engine.default_params(kind))
        out = ref.run_case(c)
        assert ref.worth_comparing(c, out) == [], (flags, ref.worth_comparing(c, out))
        last = out[-1]
        assert last.tick == 1 + sum(ref.SCHEDULE) and last.rec_obs.shape == (ref.SCHEDULE[-1], ref.DIMS[kind][0], c.n)
        if not flags & A:
            assert not last.final.any()
        if flags & S:
            assert last.stats[3] == c.n * sum(ref.SCHEDULE) and last.stats[2] == last.episodes.sum()


def test_seeds_are_the_first_that_qualify(gymrs):
    """SEEDS says 'the first seed': spot-check one entry above 1 (CartPole, hidden 7, shape 0: seeds 1 .. 16 each miss a condition)."""
    kind, hidden, shape = 0, 7, 0
    want = ref.SEEDS[kind, hidden, shape]
    assert want > 1
    saved = dict(ref.SEEDS)
    try:
        for seed in range(1, want):
            ref.SEEDS[kind, hidden, shape] = seed
            missed = False
            for flags in ref.FLAG_SETS:
                c = ref.case(kind, shape, flags, hidden, gymrs.engine.default_params(kind))
                if ref.worth_comparing(c, ref.run_case(c)):
                    missed = True
                    break
            assert missed, seed
    finally:
        ref.SEEDS.clear()
        ref.SEEDS.update(saved)


@pytest.mark.parametrize("kind", [0, 1])
def test_reference_final_rows_and_recording_rows_are_consistent(gymrs, kind):
    """The reference against itself: the last recording row of a launch is what the getters show after it; a lane's final row
    changes exactly when its step ended an episode; the logits behind policy_ref give policy_ref's actions."""
    c = ref.case(kind, 1, A | S | T | F, 8, gymrs.engine.default_params(kind))
    out = ref.run_case(c)
    prev_final = np.zeros_like(out[0].final)
    prev_episodes = np.zeros(c.n, np.int64)
    for launch in out:
        assert np.array_equal(ref.bits(launch.rec_obs[-1]), ref.bits(launch.obs))
        assert np.array_equal(ref.bits(launch.rec_reward[-1]), ref.bits(launch.reward))
        assert np.array_equal(launch.rec_done[-1], launch.done) and np.array_equal(launch.rec_truncated[-1], launch.truncated)
        ended = ((launch.rec_done | launch.rec_truncated) != 0).sum(axis=0)
        assert np.array_equal(launch.episodes - prev_episodes, ended)
        changed = np.any(ref.bits(launch.final) != ref.bits(prev_final), axis=0)
        assert not changed[ended == 0].any()
        prev_final, prev_episodes = launch.final, launch.episodes
    y, z = ref.policy_logits(kind, 8, c.weights, c.lanes_per_policy, c.gid0, out[-1].obs)
    assert z.shape == (8, c.n) and np.isfinite(y).all()
    assert np.array_equal(np.argmax(y, axis=0), ref.policy_ref(kind, 8, c.weights, c.lanes_per_policy, c.gid0, out[-1].obs))


def test_mountain_car_prepare_follows_the_batch_not_the_engine():
    whole = ref.mountain_car_prepare(np.zeros((2, 100), np.float32), 0)
    for first in (0, 1, 6, 7, 33):
        part = ref.mountain_car_prepare(np.zeros((2, 100 - first), np.float32), first)
        assert np.array_equal(part, whole[:, first:])
    assert (whole[0] != 0).sum() == 15
