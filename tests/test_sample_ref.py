"""The sampling rule of include/gymrs_amd.h ("sampling") without a GPU: the library's host-side gymrs_sample_draw against the plain-C
restatement tests/cpp/sample_ref.c, bit for bit; the polynomial's error against f64 exp2 over its whole domain; the frequencies of
2^20 draws against the f64 softmax; and that the cases of tests/sample_ref.py (the yardstick of tests/test_gpu_sample.py) are worth
comparing with."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest
import sample_ref as ref
from sample_ref import DIMS, bits

ROOT = Path(__file__).resolve().parent.parent
POLY_BOUND = 6.71e-8  # what the header states ("6.7e-8 (measured: 6.704e-8, below 6.71e-8)")
F32 = np.float32
NAN, INF = F32(np.nan), F32(np.inf)


def library_draws(gymrs, logits, scale, seed, gids, tick):
    """gymrs_sample_draw row by row: (actions uint8 [n], probs f32 [n][A])"""
    lib = gymrs.load_library()
    y = np.ascontiguousarray(logits, F32)
    n, a = y.shape
    x = gymrs.Sampling(seed, float(scale), 0)
    act, probs = np.empty(n, np.uint8), np.empty((n, a), F32)
    out = C.c_uint8()
    fp = C.POINTER(C.c_float)
    for i in range(n):
        st = lib.gymrs_sample_draw(C.byref(x), a, y[i].ctypes.data_as(fp), int(gids[i]), int(tick), C.byref(out), probs[i].ctypes.data_as(fp))
        assert st == 0, lib.gymrs_last_error()
        act[i] = out.value
    return act, probs


def assert_same(gymrs, logits, scale, seed=0xABCDEF0123, tick=77, first=0):
    y = np.ascontiguousarray(logits, F32)
    gids = ref.ex.as_u64([first + i for i in range(len(y))])
    got_a, got_p = library_draws(gymrs, y, scale, seed, gids, tick)
    want_a, _, want_p = ref.draw_many(y, float(F32(scale)), ref.words(seed, gids, tick))
    bad = np.flatnonzero((got_a != want_a) | (bits(got_p) != bits(want_p)).any(axis=1))
    assert bad.size == 0, (scale, y[bad[:3]].tolist(), got_a[bad[:3]], want_a[bad[:3]], got_p[bad[:3]], want_p[bad[:3]])
    return want_a, want_p


# ---- (a) the library's host draw == the plain-C reference, bit for bit ------------------------------------------------------------
@pytest.mark.parametrize("n_actions", [3, 2])
def test_sample_draw_equals_the_c_reference_on_random_logits(gymrs, n_actions):
    rng = np.random.default_rng(20 + n_actions)
    y = (rng.standard_normal((100000, n_actions)) * rng.choice([0.01, 1.0, 30.0], size=(100000, 1))).astype(F32)
    scale = ref.LOG2E
    act, probs = assert_same(gymrs, y, scale, first=(1 << 32) - 50000)
    assert set(act) == set(range(n_actions)) and np.abs(probs.sum(axis=1) - 1).max() < 1e-6


def corner_logits():
    tiny = F32(1e-45)  # the smallest denormal
    rows = [
        (0, 0, 0), (1.5, 1.5, 1.5), (2, 2, -1), (-1, 2, 2),  # ties
        (0.0, -0.0, 0.0), (-0.0, 0.0, -0.0),  # signed zeros
        (tiny, 0, -tiny), (0, -tiny, F32(-3e-39)), (1, F32(np.nextafter(F32(1), F32(0))), 1),  # denormal / one-ulp differences
        (0, -126, -126), (0, F32(np.nextafter(F32(-126), F32(-200))), -126), (0, -125.99999, -127), (0, -149, -1000),  # the cut at -126
        (0, -INF, 1), (-INF, -INF, 0), (-INF, -INF, -INF), (INF, 0, 1), (0, INF, INF), (INF, INF, INF), (-INF, INF, 0),
        (NAN, 0, 1), (0, NAN, 1), (0, 1, NAN), (NAN, NAN, 0), (NAN, NAN, NAN), (1, NAN, INF), (NAN, INF, 0),
        (3e38, -3e38, 0), (-3e38, 3e38, 3e38), (0.3, -0.2, 1.1),
    ]
    return np.array(rows, F32)


@pytest.mark.parametrize("scale", [ref.LOG2E, 1.0, 0.0, 1e30, 1e-30, 126.0])
def test_sample_draw_equals_the_c_reference_on_the_corners(gymrs, scale):
    """Every corner row under 64 draws (64 consecutive global ids), as triples and as pairs (the first two columns)"""
    rows = corner_logits()
    y = np.repeat(rows, 64, axis=0)
    assert_same(gymrs, y, scale)
    assert_same(gymrs, y[:, :2], scale)
    assert_same(gymrs, y[:, 1:], scale)


def test_what_the_header_says_follows_from_the_rule():
    lib = ref.lib()
    w = lambda d: float(lib.sample_ref_weight(C.c_float(d)))  # noqa: E731
    assert w(0.0) == 1.0 and w(-0.0) == 1.0 and w(-1.0) == 0.5 and w(-126.0) == 2.0 ** -126  # c0 == 1: exact at the integers
    below = float(np.nextafter(F32(-126), F32(-200)))
    assert w(below) == 0.0 and w(float("nan")) == 0.0 and w(float("-inf")) == 0.0 and w(-1e30) == 0.0
    assert w(-1e-45) == float(F32(lib.sample_ref_poly(C.c_float(1.0))) * F32(0.5))  # f rounds up to 1.0 for a denormal d
    # every weight is 0 or a normal number; the greedy action weighs 1 whenever its logit is finite
    rng = np.random.default_rng(3)
    y = (rng.standard_normal((4096, 3)) * 40).astype(F32)
    for scale in (ref.LOG2E, 3.0, 1e30):
        wd = np.zeros(len(y), np.uint32)
        weights = np.empty((len(y), 3), F32)
        for i, row in enumerate(y):
            a = C.c_uint8()
            g = lib.sample_ref_draw(3, row.ctypes.data, C.c_float(scale), int(wd[i]), C.byref(a), weights[i].ctypes.data, None)
            assert weights[i, g] == 1.0
        assert ((weights == 0) | (weights >= np.finfo(F32).tiny)).all()
    # an action of weight zero is never taken; all weights zero (NaN / infinite maximum) plays the greedy action
    words = np.arange(0, 1 << 32, 1 << 20, dtype=np.uint64).astype(np.uint32)
    for row, allowed in (((0, -INF, 0), {0, 2}), ((0, -1000, -1000), {0}), ((NAN, 5, 7), {0}), ((1, INF, INF), {1}), ((-INF, -INF, -INF), {0}),
                         ((0, 0, NAN), {0, 1})):
        act, greedy, probs = ref.draw_many(np.tile(np.array(row, F32), (len(words), 1)), ref.SCALE, words)
        assert set(act) == allowed, (row, set(act))
        assert (probs[0][sorted(set(range(3)) - allowed)] == 0).all() and probs[0].sum() == 1.0


# ---- (b) the polynomial ------------------------------------------------------------------------------------------------------------------
def test_polynomial_error_over_all_fractions_is_within_the_stated_bound():
    """P(f) with true fmaf against f64 exp2 over all f = i / 2^23: at most the bound of the header (which names the same figure)"""
    err = ref.lib().sample_ref_poly_max_rel_err()
    print(f"max relative error of P over [0, 1): {err:.4e}")
    assert err <= POLY_BOUND, err
    text = (ROOT / "include" / "gymrs_amd.h").read_text()
    assert "is 6.7e-8 (measured: 6.704e-8, below 6.71e-8" in text and round(err * 1e8, 3) == 6.704
    assert ref.lib().sample_ref_poly(C.c_float(0.0)) == 1.0


# ---- (c) frequencies --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logits,scale", [((0.3, -0.2, 1.1), ref.LOG2E), ((0.7, 0.7, 0.7), ref.LOG2E), ((2.0, -5.0), 0.0)])
def test_frequencies_of_2_to_20_draws_match_the_f64_softmax(gymrs, logits, scale):
    n = 1 << 20
    gids = np.arange(n, dtype=np.uint64)
    w = ref.words(ref.SEED, gids, 9)
    y = np.tile(np.array(logits, F32), (n, 1))
    act, _, probs = ref.draw_many(y, float(F32(scale)), w)
    p = ref.softmax64(np.array(logits, F32), F32(scale))
    freq = np.bincount(act, minlength=len(logits)) / n
    bound = 6 * np.sqrt(p * (1 - p) / n)
    print("frequencies", freq, "softmax", p, "bounds", bound)
    assert (np.abs(freq - p) <= bound).all(), (freq, p, bound)
    assert np.abs(probs[0].astype(np.float64) - p).max() < 3e-7
    # the library draws the same actions (a sample of the ids: the ctypes loop is the slow part)
    some = np.arange(0, n, 257)
    got, _ = library_draws(gymrs, y[some], scale, ref.SEED, gids[some], 9)
    assert np.array_equal(got, act[some])


# ---- (d) the matrix is worth comparing with ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,flags,table,i", ref.matrix())
def test_every_case_is_worth_comparing(kind, flags, table, i):
    """In every main case at least one lane-step in eight takes a non-greedy action and at least one in eight the greedy one; every
    action occurs; episodes end inside the window; the probability row is a probability."""
    c = ref.matrix_case(kind, flags, table, i)
    assert c.scale == ref.SCALE and c.n == 1300 and sum(c.schedule) == 40
    out = ref.run_case(c)
    w = ref.whole(out)
    other = w.explored.mean()
    assert w.explored.size == 40 * 1300 and 1 / 8 <= other <= 7 / 8, other
    assert set(w.actions.ravel()) == set(range(DIMS[kind][1])) and (w.greedy < DIMS[kind][1]).all()
    prob = np.concatenate([x.prob for x in out])
    assert ((prob > 0) & (prob <= 1)).all() and prob.min() < 0.5
    assert w.ended.any(), "no episode ended inside the window"
    assert out[-1].tick == 41 and out[-1].fitness.any() and out[-1].fitness[:, 1].sum() == w.ended.sum()


def test_the_split_and_the_greedy_launch():
    for kind in (0, 1):
        full = ref.A | ref.S | ref.T | ref.F
        a = ref.run_case(ref.case(kind, full, True, 6, (3, 1), 8, ref.SPLITS[0]))
        b = ref.run_case(ref.case(kind, full, True, 6, (3, 1), 8, ref.SPLITS[1]))
        assert np.array_equal(bits(a[-1].state), bits(b[-1].state)) and np.array_equal(a[-1].stats, b[-1].stats)
        assert np.array_equal(ref.whole(a).actions, ref.whole(b).actions)
        # a launch without the flag is explore_ref's greedy launch
        c = ref.case(kind, full, True, 6, (3, 1), 8)
        g, e = ref.Run(c).launch(40, None), ref.ex.Run(c).launch(40, None)
        assert np.array_equal(bits(g.state), bits(e.state)) and np.array_equal(g.rec_actions, e.rec_actions) and not g.explored.any()
        # scale 1e30 is greedy wherever the logits have no exact tie
        hard = ref.Run(c).launch(40, (c.seed, 1e30))
        assert np.array_equal(hard.rec_actions, g.rec_actions) and (hard.prob == 1).all()
