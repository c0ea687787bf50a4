"""The CPU reference of gymrs_evaluate_policy (tests/policy_eval_ref.py) on the case table of tests/test_gpu_policy_eval.py, checked
without a GPU: every case of the GPU matrix is worth comparing.  In the lanes of each copy of the kernel's two paths a case reaches
(uniform / gathered x full / ragged waves, by closed_loop_ref.wave_classes at 4 lanes per work-item) some episode ends by done
before the limit and some at the limit, and some wave holds lanes with different step totals (lanes park while others play); the
records of two policies differ, and some record has return_min != return_max."""
import ctypes as C
from functools import lru_cache

import closed_loop_ref as ref
import numpy as np
import policy_eval_ref as ev
import pytest


@lru_cache(maxsize=None)
def run(gymrs, kind, shape, hidden, common):
    c = ev.case(kind, shape, hidden, common, gymrs.engine.default_params(kind))
    return c, ev.run_case(c)


def test_the_record_has_the_eight_fields_of_the_header(gymrs):
    assert [name for name, _ in gymrs.engine.PolicyEval._fields_] == list(ev.FIELDS)
    assert C.sizeof(gymrs.engine.PolicyEval) == 64 and C.sizeof(gymrs.engine.EvalDesc) == 32


def test_records_count_what_the_episodes_say():
    length = np.array([[3, 17, 5, 2], [17, 1, 5, 9]], np.int64)
    done = np.array([[1, 0, 1, 1], [1, 1, 1, 0]], bool)  # (lane 0's second episode: done AND at the limit)
    pol = np.array([0, 0, 2, 2])
    cp = ev.records(0, length, done, pol, 4, 17)
    assert cp[0].tolist() == [38, 9 + 289 + 289 + 1, 4, 3, 2, 38, 1, 17]
    assert cp[2].tolist() == [21, 25 + 4 + 25 + 81, 4, 3, 0, 21, 2, 9]
    assert cp[1].tolist() == list(ev.IDENTITY) == cp[3].tolist()
    mc = ev.records(1, length, done, pol, 4, 17)
    assert mc[0].tolist() == [-38, 588, 4, 3, 2, 38, -17, -1] and mc[2].tolist() == [-21, 135, 4, 3, 0, 21, -9, -2]
    assert ev.packed(length, done)[1].tolist() == [17 | 0x80000000, 1 | 0x80000000, 5 | 0x80000000, 9]
    both = ev.merge([cp, ev.records(0, length[:, :2], done[:, :2], pol[:2], 4, 17)])
    assert both[0].tolist() == [76, 1176, 8, 6, 4, 76, 1, 17] and both[2].tolist() == cp[2].tolist() and both[1].tolist() == list(ev.IDENTITY)
    assert ev._wrap(2**64 - 5) == -5 and ev._wrap(2**63) == -2**63


def test_the_matrix_reaches_all_four_copies():
    seen = set()
    for shape in range(len(ev.SHAPES)):
        n, vec, gid0, lpp = ev.SHAPES[shape]
        assert vec == 4
        seen |= set(ref.lanes_per_copy(n, 4, gid0, ev.N_POLICIES, lpp))
    assert seen == set(ref.COPIES)


@pytest.mark.parametrize("kind,shape,hidden,common", ev.cases())
def test_every_case_is_worth_comparing(gymrs, kind, shape, hidden, common):
    c, r = run(gymrs, kind, shape, hidden, common)
    assert ev.worth_comparing(c, r) == []
    assert r.records.shape == (ev.N_POLICIES, 8) and r.records.dtype == np.int64 and r.lengths.shape == (ev.EPISODES, c.n)
    rec = r.records
    assert (rec[:, 2] == ev.EPISODES * np.bincount(r.pol, minlength=ev.N_POLICIES)).all()  # every lane plays E episodes
    assert (rec[:, 0] == ev.SIGN[kind] * rec[:, 5]).all() and (rec[:, 3] + rec[:, 4] >= rec[:, 2]).all()
    assert (rec[:, 6] >= -ev.MAX_STEPS).all() and (rec[:, 7] <= ev.MAX_STEPS).all() and (rec[:, 6] <= rec[:, 7]).all()


@pytest.mark.parametrize("kind", [0, 1])
def test_common_starts_give_every_policy_the_same_states(gymrs, kind):
    c, r = run(gymrs, kind, 0, 0, True)
    n, _, gid0, lpp = ev.SHAPES[0]
    g = np.array([(gid0 + i) % lpp for i in range(n)])
    first = {}
    for i in range(n):  # two lanes with the same g % lanes_per_policy start every episode from the same state
        j = first.setdefault(int(g[i]), i)
        if j != i:
            assert all(np.array_equal(st[:, i].view(np.uint32), st[:, j].view(np.uint32)) for st in r.starts)
    assert len(first) == lpp and len(set(r.pol)) == 3
    _, plain = run(gymrs, kind, 0, 0, False)
    assert not np.array_equal(plain.starts[0], r.starts[0])  # and they are not the per-lane states
    assert not np.array_equal(r.starts[0], r.starts[1])  # episode e + 1 draws afresh
