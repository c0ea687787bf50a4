"""The per-policy fitness records of include/gymrs_amd.h ("per-policy fitness") computed on the CPU alone: the rows a recording
launch keeps, as tests/closed_loop_ref.py computes them (f32 twin + tests/cpp/policy_ref.c), summed per policy with Python ints.
Like closed_loop_ref this module never imports the library: what it returns is the yardstick of tests/test_gpu_policy_fitness.py,
and tests/test_policy_fitness_ref.py shows without a GPU that it is worth comparing with.

The case table is closed_loop_ref's, unchanged (SHAPES, SEEDS, SCHEDULE, MAX_EPISODE_STEPS, N_POLICIES, mountain_car_prepare).

A plain module, imported by test files; no fixtures, no pytest hooks."""
import closed_loop_ref as ref
import numpy as np

FIELDS = ("reward_sum", "episodes", "done", "truncated")  # the columns of a record, in gymrs_policy_fitness order


def policy_of_lane(gid, lanes_per_policy, n_policies):
    """include/gymrs_amd.h: lane i of the engine uses policy ((global_env_offset + i) / lanes_per_policy) % n_policies"""
    return (int(gid) // int(lanes_per_policy)) % int(n_policies)


def policies_of(n, gid0, lanes_per_policy, n_policies):
    """The policy of each of the n lanes of an engine at global offset gid0 (python ints: ids go beyond 2^32)"""
    return np.array([policy_of_lane(gid0 + i, lanes_per_policy, n_policies) for i in range(n)], np.int64)


def fold_rows(pol, n_policies, reward, done, truncated):
    """What one launch adds: (n_policies, 4) int64 from the rows [steps][n] a recording launch keeps.  The rewards are whole
    numbers (0, 1, -1): converted one by one, so the sum is an integer sum."""
    reward = np.asarray(reward)
    r = reward.astype(np.int64)
    assert np.array_equal(r.astype(reward.dtype), reward)  # the conversion is exact
    d, t = np.asarray(done).astype(np.int64), np.asarray(truncated).astype(np.int64)
    assert ((d | 1) == 1).all() and ((t | 1) == 1).all()
    e = ((d | t) != 0).astype(np.int64)
    out = np.zeros((n_policies, 4), np.int64)
    for col, rows in enumerate((r, e, d, t)):
        per_lane = rows.sum(axis=0)
        for p in range(n_policies):
            out[p, col] = int(per_lane[pol == p].sum())
    return out


def cumulative(launches, n, gid0, lanes_per_policy, n_policies, first=0, count=None):
    """The records after each launch of closed_loop_ref.reference(...)'s result `launches`, for an engine that holds lanes
    [first, first + count) of the reference's batch: a list of (n_policies, 4) int64, one per launch."""
    count = n - first if count is None else count
    pol = policies_of(count, gid0 + first, lanes_per_policy, n_policies)
    sl = slice(first, first + count)
    total = np.zeros((n_policies, 4), np.int64)
    out = []
    for w in launches:
        total = total + fold_rows(pol, n_policies, w.rec_reward[:, sl], w.rec_done[:, sl], w.rec_truncated[:, sl])
        out.append(total)
    return out


def of_case(c, launches):
    """`cumulative` for a case of closed_loop_ref.case and its run_case result"""
    return cumulative(launches, c.n, c.gid0, c.lanes_per_policy, ref.N_POLICIES)
