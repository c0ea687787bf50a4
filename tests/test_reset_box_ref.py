"""No GPU: the yardsticks of tests/test_gpu_reset_box.py deserve trust.

The f32 twin shares make_sample_box / uniform_in_box with the library (gym-rs_amd/csrc/gymrs_philox.h), so a twin-against-GPU comparison
cannot see a defect of the draw itself; the f64 oracle (oracle/gymrs_oracle.c) restates it independently.  Here: under every box of
tests/reset_box_ref.py the twin's reset and re-arm draws are the oracle's within a derived tolerance and lie in the box; the boxes
the library must refuse are refused by its own check and the others are not; a permuted or a stale box would show; the optional
`bounds` of the *_ref modules changes nothing at its default; and the closed-loop cases reach what they are for."""
import importlib
from itertools import combinations

import numpy as np
import pytest
import reset_box_ref as rb
import test_time_shift_ref as tsr
from reset_box_ref import A, S, T

from oracle.bindings import TwinEngine

GID0S = ((1 << 33) + 5, 12347)  # beyond 2^32; neither is a multiple of 4
N, SEED, STEPS = 200, 21, 6


@pytest.fixture(scope="module")
def gymrs_params():
    return importlib.import_module("gym-rs_amd").engine.default_params


def rearming_twin(twin, gymrs_params, kind, gid0, bounds):
    """A twin whose every lane re-arms on every step: max_episode_steps = 1 with A | T"""
    p = gymrs_params(kind)
    p.max_episode_steps = 1
    tw = TwinEngine(twin, kind, N, p, flags=A | T, gid0=gid0)
    tw.reset(SEED, bounds)
    return tw


def draws(twin, gymrs_params, kind, gid0, bounds):
    """[(tick of the draw, state [D][N])]: the reset (tick 0) and STEPS re-arms"""
    tw = rearming_twin(twin, gymrs_params, kind, gid0, bounds)
    out = [(0, tw.get_state())]
    for _ in range(STEPS):
        t = tw.tick()
        tw.step(tw.fill_actions(4, t))
        _, done, trunc = tw.get_result()
        assert trunc.all()
        out.append((t, tw.get_state()))
    return out


BOXES = [(kind, name, rb.NAMED[kind][name]) for kind in (0, 1, 2) for name in rb.NAMED[kind]] + \
        [(kind, name, rb.edge(kind, name)) for kind in (0, 1, 2) for name in rb.EDGES]


@pytest.mark.parametrize("kind,name,bounds", BOXES, ids=[f"{k}-{n}" for k, n, _ in BOXES])
def test_the_twin_draws_what_the_oracle_draws_inside_the_box(twin, oracle, gymrs_params, kind, name, bounds):
    """Reset and six re-arm ticks, 200 lanes at two offsets: every component within tol_j (reset_box_ref.tolerance) of
    Oracle.reset_batch(..., tick, bounds) and lo_j <= v < hi_j.  Largest err / tol_j seen (printed by the test), per box:
      CartPole DISTINCT 0.344, TERMINAL 0.250, FAR 0.285;  MountainCar GOAL 0.278, WALL 0.333, FAR 0.320;  Pendulum DISTINCT 0.364
      edge boxes, on the varied component (the same in the three envs): [-1, 0) 0.000, [-1, -0) 0.000, [0, 2^24) 0.000 (the f32 draws
      are exact), [1e5, 1e5 + 1) 0.616, [-1.5e38, 1.5e38) 0.095, and [1, nextafter 1) 1.000 (0.99999994: the oracle spreads over the
      one-ulp box, every f32 draw is 1); over CartPole's three default components 0.099 each time."""
    tol = rb.tolerance(kind, bounds)
    worst = 0.0
    for gid0 in GID0S:
        for tick, st in draws(twin, gymrs_params, kind, gid0, bounds):
            assert rb.inside(kind, bounds, st), (name, gid0, tick)
            want = oracle.reset_batch(kind, N, gid0, SEED, tick, rb.oracle_bounds(kind, bounds))
            err = np.abs(st.astype(np.float64) - want)
            for j in range(rb.SAMPLED[kind]):
                worst = max(worst, err[j].max() / tol[j])
            assert (err <= tol[:, None]).all(), (name, gid0, tick, (err / np.maximum(tol[:, None], 1e-300)).max())
    print(f"kind {kind} {name}: largest err / tol = {worst:.3f}")
    if name not in ("[1, nextafter 1)",):  # (there every draw is 1)
        assert len(np.unique(st[0])) > N // 4  # the draws spread: not one value for every lane


def test_the_librarys_check_refuses_the_degenerate_boxes_and_no_other(twin):
    """twin_sample_range_ok is the check gymrs_reset and gymrs_reset_pcg64 apply per sampled component.  What the refused boxes would do
    is shown with the library's own uniform_in_box: one value for every random word."""
    for name, (lo, hi) in rb.REFUSED.items():
        values = {twin.lib.twin_uniform_in_box(r << 8, lo, hi) for r in (0, 1, 12345, (1 << 23), (1 << 24) - 1)}
        assert len({v for v in values if v == v}) == 1, (name, values)  # (a NaN for word 0 at an infinite width is what the select hides)
        assert not twin.sample_range_ok(lo, hi), name
    for name, (lo, hi) in rb.EDGES.items():
        assert twin.sample_range_ok(lo, hi), name
    for kind in (0, 1, 2):
        d = rb.STATE_DIM[kind]
        for b in [rb.box(kind)] + list(rb.NAMED[kind].values()):
            assert all(twin.sample_range_ok(b[j], b[d + j]) for j in range(rb.SAMPLED[kind])), (kind, b)
    for lo, hi in ((0.0, 0.0), (1.0, 0.5), (0.0, float("inf")), (float("-inf"), 0.0), (float("nan"), 1.0), (0.0, float("nan"))):
        assert not twin.sample_range_ok(lo, hi), (lo, hi)  # what was refused before stays refused
    assert twin.sample_range_ok(0.0, 2.0 ** -102) and not twin.sample_range_ok(0.0, float(np.nextafter(np.float32(2.0 ** -102), np.float32(0))))


@pytest.mark.parametrize("kind", [0, 2])
def test_a_permuted_or_a_stale_box_would_be_noticed(twin, gymrs_params, kind):
    """DISTINCT with two components transposed, or replaced by the default box: at the reset and at every re-arm some lane moves by more
    than the oracle tolerance (in fact every lane does: the intervals are disjoint)"""
    bounds = rb.NAMED[kind]["DISTINCT"]
    tol = rb.tolerance(kind, bounds)
    d = rb.STATE_DIM[kind]
    others = [rb.swapped(kind, bounds, i, j) for i, j in combinations(range(d), 2)] + [None]
    assert len(others) == (7 if kind == 0 else 2)
    for gid0 in GID0S:
        real = draws(twin, gymrs_params, kind, gid0, bounds)
        for other in others:
            for (tick, st), (_, wrong) in zip(real, draws(twin, gymrs_params, kind, gid0, other)):
                moved = (np.abs(st.astype(np.float64) - wrong) > tol[:, None]).any(axis=0)
                assert moved.all(), (kind, gid0, tick, other)


# ---- the optional `bounds` of the reference modules ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(tsr.PINNED))
def test_bounds_none_leaves_every_reference_what_it_was(gymrs_params, name):
    """The digests of tests/test_time_shift_ref.py, taken before the modules had a `bounds`: unchanged at the default, unchanged with
    the env's own box passed explicitly (the argument does reach the twin), and different under another box."""
    assert tsr.digest(tsr.run_module(name, gymrs_params)) == tsr.PINNED[name]
    kind = 1 if name in ("sample", "closed_loop") else 0
    assert tsr.digest(run_with(name, gymrs_params, rb.box(kind))) == tsr.PINNED[name]
    assert tsr.digest(run_with(name, gymrs_params, rb.NAMED[kind][rb.FIRST[kind]])) != tsr.PINNED[name]


def run_with(name, gymrs_params, bounds):
    full = A | S | T | rb.F
    if name == "explore":
        return tsr.ex.run_case(tsr.ex.case(0, full, True, 6, (3, 1), 8, tsr.ex.SPLITS[1], bounds=bounds))
    if name == "sample":
        return tsr.sr.run_case(tsr.sr.case(1, full, False, 6, (3, 512), 0, tsr.sr.SPLITS[1], bounds=bounds))
    if name == "transitions":
        return tsr.tr.run_case(tsr.tr.case(0, 0, A | S | T, 8, False, True, bounds=bounds))
    return tsr.cl.run_case(tsr.cl.case(1, 1, full, 8, gymrs_params(1), bounds=bounds))


# ---- the closed-loop cases -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,ps,name,table", rb.closed_loop_cases())
def test_the_closed_loop_cases_reach_what_they_are_for(kind, ps, name, table):
    """Greedy, exploring and sampling run of every case (the transitions launch replays the sampling run): lanes of every kernel copy
    re-arm in both launches; TERMINAL / GOAL: lanes end on two consecutive steps; FAR: re-armed lanes start their next step outside
    the fast range, in waves that also hold lanes inside it.  And the greedy run under the default box differs in state and statistics."""
    for source in rb.SOURCES:
        c, launches = rb.closed_loop_run(kind, ps, name, table, source)
        assert rb.missing(kind, name, c, launches) == [], source
        assert rb.inside(kind, c.bounds, launches[0].start_state) or kind == 1  # (MountainCar: every 7th lane starts prepared)
    _, other = rb.closed_loop_run(kind, ps, name, table, "greedy", default_box=True)
    _, launches = rb.closed_loop_run(kind, ps, name, table, "greedy")
    for x, y in zip(launches, other):
        assert not np.array_equal(rb.cl.bits(x.state), rb.cl.bits(y.state))
        if (kind, name, table) == (1, "WALL", False):
            # the one case whose statistics cannot tell: from the left wall, as from the valley, no lane reaches the default goal inside
            # the 17-step limit, so under both boxes the same lanes end on the same steps (the prepared ones, then everybody at the
            # limit).  Its states and observations differ in every lane; with a table the low-goal rows tell the boxes apart.
            assert np.array_equal(x.stats, y.stats) and (rb.cl.bits(x.state)[0] != rb.cl.bits(y.state)[0]).mean() > 0.99
        else:
            assert not np.array_equal(x.stats, y.stats)
    if kind == 1 and name == "GOAL":
        ended = np.concatenate([(x.rec_done | x.rec_truncated) != 0 for x in launches])
        after = np.concatenate([x.rec_obs for x in launches])
        assert ended.any() and (after[:, 1][ended] == 0).all()  # the velocity bounds are ignored: a re-armed lane is at rest
