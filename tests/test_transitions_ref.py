"""No GPU: the cases tests/test_gpu_transitions.py compares gymrs_rollout_transitions with are worth comparing with.  For every case of
the matrix, inside the lanes of every kernel copy present: an episode ends by done, one by truncation (flag sets with the time
limit), a lane ends two episodes inside one launch -- which the engine's own final-observation array cannot represent -- and on
every ended lane-step the final observation differs bitwise from the recorded, re-armed one."""
import numpy as np
import pytest
import transitions_ref as ref
from transitions_ref import A, T


def test_the_matrix_meets_every_family_flag_set_and_axis_value():
    m = ref.matrix()
    assert {(kind, table, flags) for kind, table, flags, *_ in m} == {(k, t, f) for k in (0, 1) for t in (False, True) for f in ref.FLAG_SETS}
    assert len(ref.FLAG_SETS) == 8 and all(f & A for f in ref.FLAG_SETS)
    for kind in (0, 1):
        for table in (False, True):
            mine = [x for x in m if x[0] == kind and x[1] == table]
            assert {x[3] for x in mine} == {0, 1} and {x[4] for x in mine} == set(ref.HIDDEN) and {x[5] for x in mine} == {False, True}


def test_both_shapes_put_lanes_into_all_four_copies():
    seen = set()
    for shape in (0, 1):
        seen |= set(np.unique(ref.case(0, shape, A, 0, False, False).classes[4]).tolist())
    assert seen == {0, 1, 2, 3}


@pytest.mark.parametrize("kind,table,flags,shape,hidden,explore", ref.matrix())
def test_the_case_is_worth_comparing(kind, table, flags, shape, hidden, explore):
    c = ref.case(kind, shape, flags, hidden, table, explore)
    out = ref.run_case(c)
    assert ref.worth_comparing(c, out) == []
    total = sum(c.schedule)
    assert sum(x.final_obs.shape[0] for x in out) == total and out[0].start_obs.shape == (ref.DIMS[kind][0], c.n)
    assert np.array_equal(ref.bits(out[0].start_obs), ref.bits(out[0].start_state))
    if flags & T:
        assert any(x.rec_truncated.any() for x in out)
