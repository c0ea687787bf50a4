"""No GPU: the cases tests/test_gpu_hidden_widths.py compares the kernels with at hidden widths 1, 7 and 64 are worth comparing with.
The table of tests/hidden_width_ref.py puts every width on every family instance and every flag set on every width in every group (per family as far as its four or eight instances reach);
every case meets hidden_width_ref.worth_comparing under its seed; and the reference computed without the units that the four-unit
loop leaves to its remainder differs from the true one inside the lanes of every kernel copy -- so a kernel that dropped, misread or
overran those units could not pass the GPU comparison, which the last test shows by making that comparison here."""
import closed_loop_ref as cl
import explore_ref as ex
import hidden_width_ref as hw
import numpy as np
import pytest
import transitions_ref as tr
from closed_loop_ref import S
from hidden_width_ref import A, FLAG_SETS, bits
from test_gpu_closed_loop_table import same  # the GPU tests' comparison: numpy only, but its module imports torch (no GPU needed for that)

INSTANCES = [inst for group in hw.GROUPS for inst in hw.instances(group)]


def test_every_width_meets_every_family_instance_and_every_flag_set():
    per_group = {group: hw.instances(group) for group in hw.GROUPS}
    assert {g: len(x) for g, x in per_group.items()} == {"closed": 32, "record": 12, "transitions": 12, "step": 8, "eval": 8}
    assert len({inst.key for inst in INSTANCES}) == len(INSTANCES) == 72 and set(hw.SEEDS) == {inst.key for inst in INSTANCES}
    assert sum(len(hw.widths_of(inst)) for inst in INSTANCES) == 208  # the cases
    for inst in INSTANCES:  # one seed per width; a temperature where the family samples
        seeds, temperature = hw.SEEDS[inst.key]
        assert len(seeds) == len(hw.widths_of(inst)) and all(0 < s < 200 for s in seeds) and (temperature is not None) == (inst.source == "sample")
        assert hw.widths_of(inst) == ((1, 64) if inst.group == "eval" else (1, 7, 64))
    both, lanes = [(k, t) for k in (0, 1) for t in (False, True)], (4, 8)
    for family in hw.GROUPS["closed"]:
        assert {(i.kind, i.table, i.vec) for i in per_group["closed"] if i.family == family} == {(k, t, v) for k, t in both for v in lanes}
    for group in ("record", "transitions"):
        for family in hw.GROUPS[group]:
            mine = [i for i in per_group[group] if i.family == family]
            assert {(i.kind, i.table, i.vec) for i in mine} == {(k, t, 4) for k, t in both} and {i.shape for i in mine} == {0, 1}
    for family in hw.GROUPS["step"]:
        assert {(i.kind, i.table, i.vec) for i in per_group["step"] if i.family == family} == {(k, False, v) for k in (0, 1) for v in lanes}
    assert {(i.kind, i.table, i.shape) for i in per_group["eval"]} == {(k, t, s) for k, t in both for s in (0, 1)}
    # an instance runs all its widths under its one flag set: every flag set the group's kernels are built for occurs in the group
    for group, sets in (("closed", FLAG_SETS), ("record", FLAG_SETS), ("transitions", tr.FLAG_SETS)):
        assert {i.flags for i in per_group[group]} == set(sets), group
    assert len(tr.FLAG_SETS) == 8 and all(f & A for f in tr.FLAG_SETS)
    # per family, as far as four or eight engines reach: a closed family misses two sets; every recording and transitions family
    # meets four different sets, with and without each of T, S and F; sample_transitions takes the four transitions_policy leaves
    sets_of = lambda group, family: {i.flags for i in per_group[group] if i.family == family}  # noqa: E731
    assert all(len(sets_of("closed", family)) == 8 for family in hw.GROUPS["closed"])
    for group in ("record", "transitions"):
        for family in hw.GROUPS[group]:
            mine = sets_of(group, family)
            assert len(mine) == 4 and all({bool(f & bit) for f in mine} == {False, True} for bit in (hw.T, S, hw.F)), (family, mine)
    assert sets_of("transitions", "transitions_policy") | sets_of("transitions", "sample_transitions") == set(tr.FLAG_SETS)
    assert not sets_of("record", "record_policy") <= {f for f in FLAG_SETS if f & A} and not sets_of("record", "record_sample") <= {f for f in FLAG_SETS if f & A}
    for family in hw.GROUPS["closed"]:  # ... and the light axes take turns inside every family
        cases = [hw.case(i, h) for i in per_group["closed"] if i.family == family for h in hw.WIDTHS]
        assert {c.gid0 for c in cases} == set(ex.OFFSETS) and {c.schedule for c in cases} == set(ex.SPLITS)
        for h in hw.WIDTHS:
            assert {(c.n_policies, c.lanes_per_policy) for c in cases if c.hidden == h} == set(ex.POLICY_SETS)


@pytest.mark.parametrize("inst", [i for i in INSTANCES if i.group != "eval"], ids=lambda i: i.id)
def test_the_widths_of_an_instance_reach_every_kind_of_wave(inst):
    """Across the instance's three widths a uniform and a gathered wave and a full and a ragged wave carry lanes; where a case of
    64 units has a gathered wave, lanes of one use the set's last policy (a read past the set would leave the table)"""
    cases = [hw.case(inst, h) for h in hw.WIDTHS]
    seen = set(np.concatenate([np.unique(c.copies) for c in cases]).tolist())
    assert seen & {0, 2} and seen & {1, 3} and seen & {0, 1} and seen & {2, 3}, seen
    assert all(c.n == (ex.N if inst.group in ("closed", "step") else tr.SHAPES[inst.shape][0]) and max(c.schedule) <= 40 for c in cases)
    wide = cases[-1]
    assert wide.hidden == 64 and wide.weights.shape[1] == (450 if inst.kind == 0 else 387)
    if set(np.unique(wide.copies)) & {1, 3}:
        assert hw.last_policy_in_a_gathered_wave(wide)
    if inst.group in ("record", "transitions") or wide.n_policies > wide.lanes_per_policy:  # the shapes of 4200 and 5000 lanes; (3, 1)
        assert set(np.unique(wide.copies)) & {1, 3}


@pytest.mark.parametrize("inst", INSTANCES, ids=lambda i: i.id)
def test_every_case_would_notice_the_remainder(inst):
    for hidden in hw.widths_of(inst):
        c = hw.case(inst, hidden)
        ref, zeroed = hw.run_case(c), hw.run_case(hw.without_remainder(c))
        assert hw.worth_comparing(c, ref, zeroed) == [], (hidden, c.weights_seed)
        shows = hw.remainder_shows(c, ref, zeroed)
        assert set(shows) == {cl.COPIES[k] for k in np.unique(c.copies)} and min(shows.values()) > 0, (hidden, shows)
        r = hidden % 4 or 4  # what without_remainder removes, and nothing else
        a, b = c.weights.reshape(-1), hw.without_remainder(c).weights.reshape(-1)
        assert (a != b).sum() == c.n_policies * r * (1 + cl.DIMS[c.kind][1]) and (b[a != b] == 0).all()
        if c.group == "step" and c.source == "sample":  # the two textual copies agree in the reference: greedy == the argmax policy
            for call in ref:
                assert np.array_equal(call.greedy, cl.policy_ref(c.kind, hidden, c.weights, c.lanes_per_policy, c.gid0, call.obs))
            assert np.isnan(ref[1].obs).any() and not np.isnan(ref[0].obs).any()


@pytest.mark.parametrize("family,hidden", [("sample", 7), ("explore", 1), ("sample_actions", 64)])
def test_the_gpu_comparison_fails_against_the_reference_without_the_remainder(family, hidden):
    """The assertion of the GPU test (`same`, bit for bit) with the reference without the last units in the kernel's place: it
    passes on the true reference and fails on that one, naming the copies"""
    inst = next(i for i in INSTANCES if i.family == family)
    c = hw.case(inst, hidden)
    ref, zeroed = hw.run_case(c), hw.run_case(hw.without_remainder(c))
    what, pick = ("prob", lambda r: r[0].prob) if c.group == "step" else ("recorded actions", lambda r: r.actions)
    same(what, pick(ref), pick(ref), hidden, c.copies, c.index)
    with pytest.raises(AssertionError) as err:
        same(what, pick(zeroed), pick(ref), hidden, c.copies, c.index)
    print(family, err.value)
    assert "lanes differ" in str(err.value) and not np.array_equal(bits(pick(zeroed)), bits(pick(ref)))
    if c.group != "step":  # ... and so do the lanes themselves
        with pytest.raises(AssertionError):
            same("state", zeroed.out[-1].state, ref.out[-1].state, hidden, c.copies, c.index)
