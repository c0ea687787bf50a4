"""The CPU per-policy fitness reference (tests/policy_fitness_ref.py) on the case table of tests/test_gpu_policy_fitness.py, checked
without a GPU: the expected records are worth comparing with.  In every case every policy ends episodes and at least two policies
have different records (a kernel that credits the wrong policy, or nobody, is noticed), and every instantiation with a time limit
sees truncations."""
import ctypes as C
from functools import lru_cache

import closed_loop_ref as ref
import numpy as np
import policy_fitness_ref as fit
import pytest
from closed_loop_ref import T



def columns(gymrs):
    """The columns of a record array by name: the field order of the library's record (what `policy_fitness()` returns rows of) and
    of the reference must be one and the same, or the GPU comparison would compare one counter with another."""
    names = [name for name, _ in gymrs.engine.PolicyFitness._fields_]
    assert names == list(fit.FIELDS)
    return {name: i for i, name in enumerate(names)}


@lru_cache(maxsize=None)
def final_records(gymrs, kind, shape, hidden):
    """{flag set: the records after the whole schedule} of the ten cases of (kind, shape, hidden); computed once per session"""
    EPISODES = columns(gymrs)["episodes"]
    out = {}
    for flags in ref.FLAG_SETS:
        c = ref.case(kind, shape, flags, hidden, gymrs.engine.default_params(kind))
        launches = ref.run_case(c)
        per_launch = fit.of_case(c, launches)
        assert len(per_launch) == len(ref.SCHEDULE)
        for before, after in zip(per_launch, per_launch[1:]):  # cumulative: the counters never go down
            assert (after[:, EPISODES:] >= before[:, EPISODES:]).all()
        out[flags] = per_launch[-1]
    return out


def test_the_record_has_the_four_fields_of_the_header(gymrs):
    assert [name for name, _ in gymrs.engine.PolicyFitness._fields_] == list(fit.FIELDS)
    assert C.sizeof(gymrs.engine.PolicyFitness) == 32


def test_policy_of_lane_is_the_formula_of_the_header():
    assert fit.policy_of_lane(0, 1, 3) == 0 and fit.policy_of_lane(5, 1, 3) == 2 and fit.policy_of_lane(2999, 1000, 3) == 2
    assert fit.policy_of_lane(3000, 1000, 3) == 0
    big = (1 << 40) + 12345
    assert fit.policy_of_lane(big, 1000, 3) == (big // 1000) % 3
    pol = fit.policies_of(4200, big, 1000, 3)
    assert set(pol) == {0, 1, 2} and np.count_nonzero(np.diff(pol)) == 4  # five blocks, cut by the odd offset


def test_fold_rows_counts_what_the_rows_say(gymrs):
    col = columns(gymrs)
    pol = np.array([0, 0, 1, 2])
    reward = np.array([[1, 1, 0, -1], [1, 0, 0, -1]], np.float32)
    done = np.array([[0, 1, 1, 0], [0, 1, 0, 0]], np.uint8)
    trunc = np.array([[0, 1, 0, 1], [0, 0, 0, 0]], np.uint8)
    got = fit.fold_rows(pol, 4, reward, done, trunc)
    # policy 0: lanes 0 and 1; done and truncated in one step count as ONE episode
    assert got[:, col["reward_sum"]].tolist() == [3, 0, -2, 0]
    assert got[:, col["episodes"]].tolist() == [2, 1, 1, 0]
    assert got[:, col["done"]].tolist() == [2, 1, 0, 0]
    assert got[:, col["truncated"]].tolist() == [1, 0, 1, 0]
    assert got.dtype == np.int64


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("shape", range(len(ref.SHAPES)))
@pytest.mark.parametrize("hidden", ref.HIDDEN)
def test_every_policy_ends_episodes_and_two_policies_differ(gymrs, kind, shape, hidden):
    col = columns(gymrs)
    EPISODES, DONE, TRUNCATED = col["episodes"], col["done"], col["truncated"]
    for flags, rec in final_records(gymrs, kind, shape, hidden).items():
        assert rec.shape == (ref.N_POLICIES, 4)
        assert (rec[:, EPISODES] > 0).all(), (flags, rec)  # 1. every policy's counters move
        distinct = {tuple(row) for row in rec.tolist()}
        assert len(distinct) >= 2, (flags, rec)  # 2. crediting another policy would be noticed
        if not (kind == 1 and shape == 3):  # (MountainCar, SHAPES[3]: policies 1 and 2 own 1000 lanes each and tie)
            assert len(distinct) == 3, (flags, rec)
        if not flags & T:
            assert not rec[:, TRUNCATED].any() and np.array_equal(rec[:, EPISODES], rec[:, DONE])
        assert (rec[:, EPISODES] <= rec[:, DONE] + rec[:, TRUNCATED]).all()


def test_every_instantiation_with_a_time_limit_truncates(gymrs):
    """3. per (kind, lanes per work-item, flag set with T), summed over its cases.  Not per case: CartPole SHAPES[3] with hidden 7 or
    8 under A | T truncates nothing (every episode ends before 17 steps), which the GPU must reproduce."""
    TRUNCATED = columns(gymrs)["truncated"]
    total = {}
    for kind, shape, flags, hidden in ref.cases(record=False):
        if flags & T:
            key = (kind, ref.SHAPES[shape][1], flags)
            total[key] = total.get(key, 0) + int(final_records(gymrs, kind, shape, hidden)[flags][:, TRUNCATED].sum())
    assert len(total) == 2 * 2 * 5
    for key, count in total.items():
        assert count > 0, key
