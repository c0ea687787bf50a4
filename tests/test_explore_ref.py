"""The CPU epsilon-greedy reference (tests/explore_ref.py) and the case table of tests/test_gpu_explore.py, checked without a GPU: the
Philox restatement against Random123's known answers and the oracle's draws, the cases against what makes a comparison with them mean
something, both ends of the threshold, and the library's host-only gymrs_explore_draw against the reference's draw."""
import ctypes as C

import closed_loop_ref as cl
import explore_ref as ref
import lane_params_ref as lp
import numpy as np
import pytest
from explore_ref import A, COPIES, DIMS, F, S, T, bits


# ---- the generator ---------------------------------------------------------------------------------------------------------------
def test_philox_known_answers():
    """Random123's kat_vectors for philox4x32-10 (recomputed from the constants of gym-rs_amd/csrc/gymrs_philox.h)"""
    zero = ref.philox4x32_10((0, 0, 0, 0), (0, 0))
    assert [int(x) for x in zero] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    ones = ref.philox4x32_10((ref.M32,) * 4, (ref.M32,) * 2)
    assert [int(x) for x in ones] == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]


def test_philox_is_the_oracles_on_every_stream(oracle):
    rng = np.random.default_rng(1)
    for stream in (ref.STREAM_RESET, ref.STREAM_ACTION, ref.STREAM_EXPLORE):
        for _ in range(20):
            seed, gid, tick = (int(x) for x in rng.integers(0, 2**64, 3, dtype=np.uint64))
            ctr = [gid & ref.M32, gid >> 32, tick & ref.M32, ((tick >> 32) & 0xFFFF) | (stream << 16)]
            want = oracle.philox(ctr, [seed & ref.M32, seed >> 32])
            assert [int(x) for x in ref.draw4(seed, gid, tick, stream)] == want, (stream, seed, gid, tick)
    # vectorised == one at a time
    gids = np.arange(7, dtype=np.uint64) + np.uint64(2**40)
    many = ref.draw4(5, gids, 9, 2)
    for i, g in enumerate(gids):
        assert [int(x[i]) for x in many] == [int(x) for x in ref.draw4(5, int(g), 9, 2)]


def test_stream_0_is_the_oracles_reset_draw(oracle):
    """CartPole's reset samples x, x_dot, theta, theta_dot from the four words of block (seed, gid, tick, stream 0)"""
    n, gid0, seed, tick = 64, (1 << 33) + 5, 77, 3
    got = oracle.reset_batch(0, n, gid0, seed, tick)
    words = ref.draw4(seed, [gid0 + i for i in range(n)], tick, ref.STREAM_RESET)
    for j in range(4):
        want = (words[j] >> np.uint32(8)).astype(np.float64) * (1.0 / 16777216.0) * (0.05 - -0.05) + -0.05
        assert np.array_equal(got[j], want), j


@pytest.mark.parametrize("gid0", ref.OFFSETS)
@pytest.mark.parametrize("kind", [0, 1])
def test_stream_1_is_the_twins_action_stream(kind, gid0):
    """word (g & 3) of block (g >> 2, slot), the 16-bit halves and the scaling: the layout the exploration stream shares"""
    n = 37
    gids = [gid0 + i for i in range(n)]
    for t in (0, 1, 2, 7, (1 << 33) + 1):
        assert np.array_equal(ref.random_policy_actions(11, DIMS[kind][1], gids, t), lp.fill_actions(kind, n, gid0, 11, t)), t


def test_draw_by_hand():
    """One draw spelled out with Python integers only"""
    seed, gid, tick = ref.SEED, (1 << 32) + 6, (1 << 32) + 9
    ctr = [(gid >> 2) & ref.M32, (gid >> 2) >> 32, tick & ref.M32, ((tick >> 32) & 0xFFFF) | (2 << 16)]
    w = int(ref.philox4x32_10(ctr, (seed & ref.M32, seed >> 32))[gid & 3])
    for n_actions in (2, 3):
        for threshold in (0, 1, 16384, 65535, 65536):
            explored, random = ref.draw(seed, threshold, n_actions, gid, tick)
            assert bool(explored) == ((w & 0xFFFF) < threshold) and int(random) == ((w >> 16) * n_actions) >> 16


# ---- the library's host-only draw ------------------------------------------------------------------------------------------------
def test_gymrs_explore_draw_equals_the_reference(gymrs):
    lib = gymrs.load_library()
    big = 1 << 32
    gids = [0, 1, 2, 3, 4, 5, 6, 7, 1023, big - 1, big, big + 1, big + 2, big + 3, (1 << 40) + 12345, 2**64 - 1]
    ticks = [0, 1, 2, 40, big - 1, big, big + 7, (1 << 47) + 3, 2**64 - 1]
    assert {g & 3 for g in gids} == {0, 1, 2, 3} and max(gids) > big and max(ticks) > big
    g, t = np.meshgrid(ref.as_u64(gids), ref.as_u64(ticks), indexing="ij")
    e, a = C.c_uint8(), C.c_uint8()
    for seed in (0, 1, ref.SEED, 2**64 - 1):
        for threshold in (0, 1, 6554, 16384, 65535, 65536):
            for n_actions in (2, 3):
                x = gymrs.Exploration(seed, threshold, 0)
                want_e, want_a = ref.draw(seed, threshold, n_actions, g, t)
                for i in np.ndindex(g.shape):
                    assert lib.gymrs_explore_draw(C.byref(x), n_actions, int(g[i]), int(t[i]), C.byref(e), C.byref(a)) == 0
                    assert (e.value, a.value) == (int(want_e[i]), int(want_a[i])), (seed, threshold, n_actions, int(g[i]), int(t[i]))
    # the module function: scalars and arrays
    got_e, got_a = gymrs.explore_draw(ref.SEED, ref.THRESHOLD, 3, g, t)
    want_e, want_a = ref.draw(ref.SEED, ref.THRESHOLD, 3, g, t)
    assert got_e.dtype == np.bool_ and got_a.dtype == np.uint8 and np.array_equal(got_e, want_e) and np.array_equal(got_a, want_a)
    assert want_e.any() and not want_e.all() and set(want_a.ravel()) == {0, 1, 2}
    one = gymrs.explore_draw(ref.SEED, ref.THRESHOLD, 3, gids[5], ticks[3])
    assert one == (bool(want_e[5, 3]), int(want_a[5, 3]))


def test_gymrs_explore_draw_refusals(gymrs):
    lib = gymrs.load_library()
    e, a = C.c_uint8(), C.c_uint8()
    ok = gymrs.Exploration(1, 16384, 0)
    assert lib.gymrs_explore_draw(None, 2, 0, 0, C.byref(e), C.byref(a)) == 1 and b"gymrs_explore_draw" in lib.gymrs_last_error()
    assert lib.gymrs_explore_draw(C.byref(gymrs.Exploration(1, 65537, 0)), 2, 0, 0, C.byref(e), C.byref(a)) == 1
    assert b"threshold" in lib.gymrs_last_error()
    assert lib.gymrs_explore_draw(C.byref(gymrs.Exploration(1, 5, 1)), 2, 0, 0, C.byref(e), C.byref(a)) == 1 and b"reserved" in lib.gymrs_last_error()
    assert lib.gymrs_explore_draw(C.byref(ok), 0, 0, 0, C.byref(e), C.byref(a)) == 1 and b"n_actions" in lib.gymrs_last_error()
    assert lib.gymrs_explore_draw(C.byref(ok), 2, 0, 0, None, None) == 0  # either output may be NULL


# ---- the case table -------------------------------------------------------------------------------------------------------------
def test_the_matrix_crosses_what_it_says():
    m = ref.matrix()
    assert len(m) == 40 and {(k, f, t) for k, f, t, _ in m} == {(k, f, t) for k in (0, 1) for f in ref.FLAG_SETS for t in (False, True)}
    combos = {ref.axes(i) for _, _, _, i in m}
    assert len(combos) == 36 and len({ref.axes(i) for i in range(36)}) == 36  # every offset x policy set x hidden x split
    for kind in (0, 1):  # each env meets every value of every lighter axis, with and without a table
        for table in (False, True):
            seen = [ref.axes(i) for k, _, t, i in m if k == kind and t == table]
            assert {a[0] for a in seen} == set(ref.OFFSETS) and {a[1] for a in seen} == set(ref.POLICY_SETS)
            assert {a[2] for a in seen} == set(ref.HIDDEN) and {a[3] for a in seen} == set(ref.SPLITS)
    assert all(sum(s) == ref.STEPS for s in ref.SPLITS)


def test_the_shapes_reach_all_four_copies_at_both_lane_counts():
    assert ref.N == 5 * 256 + 20 == 2 * 512 + 276
    for vec in (4, 8):
        lanes = np.zeros(4, np.int64)
        for gid0 in ref.OFFSETS:
            for n_policies, lpp in ref.POLICY_SETS:
                per = cl.lanes_per_copy(ref.N, vec, gid0, n_policies, lpp)
                assert sum(per.values()) == ref.N
                lanes += np.array([per.get(c, 0) for c in COPIES])
        assert lanes.min() >= 20 * 3, dict(zip(COPIES, lanes))
        assert cl.lanes_per_copy(ref.N, vec, 0, 1, 1) == {"uniform-full": ref.N - (20 if vec == 4 else 276), "uniform-ragged": 20 if vec == 4 else 276}
        assert set(cl.lanes_per_copy(ref.N, vec, 6, 3, 1)) == {"gathered-full", "gathered-ragged"}
    # whole waves uniform: at 4 lanes per work-item every wave of an aligned engine; at an offset of 6 every second wave (the ragged
    # one among them: it starts at lane 1286 of the batch, 250 lanes before a block of 512 ends) straddles two policies
    assert set(cl.lanes_per_copy(ref.N, 4, 0, 3, 512)) == {"uniform-full", "uniform-ragged"}
    assert set(cl.lanes_per_copy(ref.N, 4, 6, 3, 512)) == {"uniform-full", "gathered-full", "gathered-ragged"}


@pytest.mark.parametrize("kind,flags,table,i", ref.matrix())
def test_every_case_is_worth_comparing(kind, flags, table, i):
    """Threshold 16384: the explored share of the lane-steps lies within 5 binomial standard deviations of 0.25; explored actions
    differ from the argmax in some lane-steps and agree in others; every action of the env occurs among explored steps; episodes
    end inside the window; under a table the rows are told apart."""
    c = ref.matrix_case(kind, flags, table, i)
    assert c.threshold == 16384 and c.n == 1300 and sum(c.schedule) == 40
    out = ref.run_case(c)
    w = ref.whole(out)
    total = w.explored.size
    assert total == 40 * 1300
    sd = np.sqrt(0.25 * 0.75 / total)
    assert abs(w.explored.mean() - 0.25) <= 5 * sd, (w.explored.mean(), sd)
    ex = w.explored
    assert (w.actions[ex] != w.greedy[ex]).any() and (w.actions[ex] == w.greedy[ex]).any()
    assert np.array_equal(w.actions[~ex], w.greedy[~ex]) and (w.greedy < DIMS[kind][1]).all()
    assert set(w.actions[ex]) == set(range(DIMS[kind][1]))
    assert w.ended.any(), "no episode ended inside the window"
    if flags & (A | T):  # ... in the ragged wave of both lane counts too (auto-reset or a time limit: every lane's episode ends)
        assert w.ended[:, -20:].any() and w.ended[:, :256].any()
    assert out[-1].tick == 41 and out[-1].rec_obs.shape == (c.schedule[-1], DIMS[kind][0], c.n)
    if flags & F:
        assert out[-1].final.any()
    if flags & S:
        assert out[-1].stats[3] == 40 * c.n and out[-1].stats[2] == w.ended.sum()
    if table:
        assert len(set(c.index)) == ref.TABLE_ROWS
        run = ref.Run(c)
        run.launch(40, (c.seed, c.threshold))
        assert run.ref.told_apart((c.index.astype(np.int64) + 1) % ref.TABLE_ROWS) >= lp.TOLD_APART
    assert out[-1].fitness.any() and out[-1].fitness[:, 1].sum() == w.ended.sum()


def test_the_split_does_not_matter():
    for kind in (0, 1):
        a = ref.run_case(ref.case(kind, A | S | T | F, True, 6, (3, 1), 8, ref.SPLITS[0]))
        b = ref.run_case(ref.case(kind, A | S | T | F, True, 6, (3, 1), 8, ref.SPLITS[1]))
        assert np.array_equal(bits(a[-1].state), bits(b[-1].state)) and np.array_equal(a[-1].stats, b[-1].stats)
        assert np.array_equal(a[-1].fitness, b[-1].fitness)
        assert np.array_equal(ref.whole(a).actions, ref.whole(b).actions)


# ---- both ends of the threshold --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, A | S | T | F])
@pytest.mark.parametrize("kind", [0, 1])
def test_threshold_0_is_closed_loop_ref_bit_for_bit(kind, flags):
    c = ref.case(kind, flags, False, 6, (3, 512), 8, ref.SPLITS[1], threshold=0)
    out = ref.run_case(c)
    want = cl.reference(kind, c.n, c.gid0, lp.default_row(kind, ref.MAX_EPISODE_STEPS), flags, c.weights, c.hidden, c.lanes_per_policy,
                        c.reset_seed, c.schedule, (lambda state, first: cl.mountain_car_prepare(state, first)) if kind == 1 else None)
    assert not ref.whole(out).explored.any()
    for got, w in zip(out, want):
        for f in ("state", "obs", "reward", "final", "rec_obs", "rec_reward"):
            assert np.array_equal(bits(getattr(got, f)), bits(getattr(w, f))), f
        for f in ("done", "truncated", "rec_actions", "rec_done", "rec_truncated"):
            assert np.array_equal(getattr(got, f), getattr(w, f)), f
        assert got.tick == w.tick
        if flags & S:
            assert np.array_equal(got.stats, w.stats)
    # ... and the greedy launch (no settings at all) is the same thing
    run = ref.Run(c)
    plain = [run.launch(steps) for steps in c.schedule]
    assert np.array_equal(bits(plain[-1].state), bits(out[-1].state)) and np.array_equal(ref.whole(plain).actions, ref.whole(out).actions)


@pytest.mark.parametrize("kind", [0, 1])
def test_threshold_65536_never_consults_the_policy(kind):
    c = ref.case(kind, A | S | T | F, True, 0, (3, 1), 8, threshold=ref.EXPLORE_ONE)
    out = ref.run_case(c)
    w = ref.whole(out)
    assert w.explored.all() and (w.greedy == 255).all() and set(w.actions.ravel()) == set(range(DIMS[kind][1]))
    broken = c.weights.copy()
    broken[:, ::2] = np.nan
    broken[:, 1::4] = np.inf
    other = ref.run_case(c, weights=broken)
    assert np.array_equal(bits(other[-1].state), bits(out[-1].state)) and np.array_equal(ref.whole(other).actions, w.actions)
    assert np.array_equal(other[-1].fitness, out[-1].fitness)
    # the action is the random policy's formula on this stream's high half: uniform over the actions
    share = np.bincount(w.actions.ravel(), minlength=DIMS[kind][1]) / w.actions.size
    assert np.abs(share - 1.0 / DIMS[kind][1]).max() < 0.01, share
