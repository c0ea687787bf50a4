"""gymrs_entropy_log2 and gymrs_entropy_lane (host only, no GPU) against tests/entropy_ref.py: bit for bit against the numpy restatement
of the rule, within a stated tolerance of the f64 calculus, the degenerate lane-steps of the header's selects, and the refusals."""
import ctypes as C

import entropy_ref as ref
import numpy as np
import pytest
from entropy_ref import DIMS, F32, LOG2E

K = 5
NAN, INF = float("nan"), float("inf")


def case(kind, hidden, n=6, seed=1):
    """n lanes with their own networks, observations, in-range actions and old probabilities near the new ones"""
    d, a = DIMS[kind]
    rng = np.random.default_rng([seed, kind, hidden])
    w = ref.make_weights(kind, hidden, n, seed) * F32(3.0)
    x = rng.standard_normal((K, d, n)).astype(F32)
    actions = rng.integers(0, a, (K, n)).astype(np.uint8)
    old = rng.uniform(0.2, 0.9, (K, n)).astype(F32)
    return w, x, actions, old


def by_library(gymrs, kind, hidden, w, x, actions, old, coef=0.01, scale=LOG2E):
    out = [gymrs.entropy_lane(kind, hidden, w[i], x[:, :, i], None if actions is None else actions[:, i], None if old is None else old[:, i],
                              coef=coef, scale=scale) for i in range(w.shape[0])]
    return tuple(np.stack([np.asarray(o[j]) for o in out]) for j in range(4))


def test_log2_equals_the_restatement_on_every_mantissa_and_keeps_the_stated_bound(gymrs):
    lib = gymrs.load_library()
    m = (np.arange(1 << 23, dtype=np.uint32) + np.uint32(0x3F800000)).view(F32)
    want = ref.log2(m)
    err = float(np.abs(want.astype(np.float64) - np.log2(m.astype(np.float64))).max())
    print(f"max |entropy_log2 - log2| over [1, 2): {err:.4e}")
    assert err <= ref.LOG2_BOUND
    out = C.c_float()
    fn, ref_out = lib.gymrs_entropy_log2, C.byref(out)
    got = np.empty(1 << 23, F32)
    for i, v in enumerate(m.tolist()):
        fn(v, ref_out)
        got[i] = out.value
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert gymrs.entropy_log2(1.0) == 0.0 and np.signbit(F32(gymrs.entropy_log2(1.0))) == False  # noqa: E712
    assert all(gymrs.entropy_log2(2.0**e) == float(e) for e in range(-126, 128))
    for bad in (0.0, 2.0**-127, -1.0, NAN, INF):
        assert lib.gymrs_entropy_log2(bad, ref_out) == 1 and b"gymrs_entropy_log2" in lib.gymrs_last_error()
    assert lib.gymrs_entropy_log2(1.0, None) == 1


@pytest.mark.parametrize("hidden", [0, 1, 7, 64])
@pytest.mark.parametrize("kind", [0, 1])
def test_the_lane_equals_the_restatement_and_the_calculus(gymrs, kind, hidden):
    """Bit for bit against entropy_ref.lanes, with and without old_prob.  Against f64: the tolerance tests/test_gradient_ref.py applies to
    gymrs_gradient_lane, (K + 16) * 2^-22 * B + 2^-25 per parameter with |coef * beta| as the coefficient in B, is kept as it is: the
    factor p[b] * (log2 p[b] + h2) this head puts in the place of 1{a = b} - p[b] stays below 1.5 in magnitude and adds the log2's
    absolute error of 1.41e-7 < 3 * 2^-24, which cancels to first order between l[b] and h2; the largest error / bound measured here
    of every case is printed (0.14 .. 0.92 over the eight cases, the largest at H = 64), so no wider bound was needed.  The sums: K lane-steps of at most ln 3, each
    within 16 * 2^-24 (the log2, the weights' 6.7e-8, six roundings), and half a fixed-point unit."""
    coef = 0.01
    w, x, actions, old = case(kind, hidden)
    got = by_library(gymrs, kind, hidden, w, x, actions, old, coef)
    want = ref.lanes(kind, hidden, LOG2E, coef, w, x, actions, old)
    for g, v, name in zip(got, want, ("q", "excluded", "sums", "counts")):
        assert np.array_equal(g, v), name
    assert got[0].any() and not got[1].any() and (got[3] == K).all()
    plain = by_library(gymrs, kind, hidden, w, x, None, None, coef)
    assert np.array_equal(plain[0], got[0]) and np.array_equal(plain[2][:, 0], got[2][:, 0]) and not plain[2][:, 1].any() and not plain[3][:, 1].any()
    worst = 0.0
    for i in range(w.shape[0]):
        g64, bound, ent, kl, zmin = ref.reference64(kind, hidden, LOG2E, coef, w[i], x[:, :, i], actions[:, i], old[:, i])
        assert zmin > 1e-6
        tol = (K + 16) * 2.0**-22 * bound + 2.0**-25
        err = np.abs(got[0][i] * 2.0**-24 - g64)
        worst = max(worst, float((err / tol).max()))
        assert (err <= tol).all(), (i, float((err / tol).max()))
        assert abs(got[2][i, 0] * 2.0**-24 - ent) <= K * 16 * 2.0**-24 + 2.0**-25
        assert abs(got[2][i, 1] * 2.0**-24 - kl) <= K * 16 * 2.0**-24 * max(1.0, float((1.0 / old[:, i]).max())) + 2.0**-25
    print(f"calculus: kind {kind} H {hidden}: largest error / bound = {worst:.4f}")


@pytest.mark.parametrize("kind", [0, 1])
def test_degenerate_lane_steps_follow_the_selects(gymrs, kind):
    d, a = DIMS[kind]
    w, x, actions, old = case(kind, 0, n=1)
    # step 0: every logit NaN (total == 0); steps 1 ..: planted old_prob and an action out of range
    x[0, 0, 0] = NAN
    old[1:, 0] = [0.0, INF, NAN, 0.5]
    actions[4, 0] = a
    got = by_library(gymrs, kind, 0, w, x, actions, old)
    want = ref.lanes(kind, 0, LOG2E, 0.01, w, x, actions, old)
    for g, v in zip(got, want):
        assert np.array_equal(g, v)
    assert got[1][0] == 0 and tuple(got[3][0]) == (K - 1, 0) and got[2][0, 1] == 0 and got[2][0, 0] > 0
    # a weight of 0: the bias of action 0 leads by more than 126 / scale; p = (1, 0, ..), the entropy and its gradient are +0
    w[:] = 0
    w[0, a * d] = 1000.0
    got = by_library(gymrs, kind, 0, w, x[1:], actions[1:], np.ones_like(old[1:]))
    assert not got[0].any() and not got[2].any() and tuple(got[3][0]) == (K - 1, int((actions[1:, 0] == 0).sum()))
    assert np.array_equal(got[0], ref.lanes(kind, 0, LOG2E, 0.01, w, x[1:], actions[1:], np.ones_like(old[1:]))[0])


@pytest.mark.parametrize("kind", [0, 1])
def test_the_logit_gradients_of_a_lane_step_sum_to_zero(gymrs, kind):
    """db of an affine network after ONE step is g itself.  sum_b p[b] * (l[b] + h2) is 0 in exact arithmetic and the log2's error
    cancels in it, so what is left is rounding: with |l[b]| < 8 here, l[b] and l[b] + h2 round to within 2^-22 each, p and the product
    to 2 * 2^-24 relative of at most 8: below 16 * 2^-24 per action before ck, 64 * 2^-24 * |ck| for A <= 3 with the sum's own
    roundings; the fixed point adds half a unit per action."""
    d, a = DIMS[kind]
    w, x, _, _ = case(kind, 0, n=8)
    coef = 1.0
    q = by_library(gymrs, kind, 0, w, x[:1], None, None, coef)[0]
    g = q[:, a * d:] * 2.0**-24
    ck = coef * LOG2E * float(ref.LN2) ** 2
    assert (np.abs(g).max(axis=1) > 1e-2).sum() >= 4  # (a lane near the uniform policy has a small g of its own)
    assert (np.abs(g.sum(axis=1)) <= 64 * 2.0**-24 * ck + a * 2.0**-25).all()


def test_lane_refusals(gymrs):
    lib = gymrs.load_library()
    f, b = (C.c_float * 10)(), (C.c_uint8 * 1)()
    q, ex, sums = (C.c_int64 * 10)(), C.c_uint64(), (C.c_int64 * 2)()
    good = [0, 0, 1.0, 0.01, f, 1, f, b, f, q, C.pointer(ex), sums, None]  # kind, hidden, scale, coef, weights, K, x, actions, old_prob, outputs
    assert lib.gymrs_entropy_lane(*good) == 0  # counts is optional
    no_kl = list(good)
    no_kl[7] = no_kl[8] = None
    assert lib.gymrs_entropy_lane(*no_kl) == 0  # and so are actions and old_prob together
    bad = [(0, 2, b"Pendulum"), (1, 65, b"hidden"), (2, NAN, b"scale"), (2, -1.0, b"scale"), (2, INF, b"scale"), (3, NAN, b"coef"), (3, INF, b"coef"),
           (7, None, b"actions")] + [(i, None, b"NULL") for i in (4, 6, 9, 10, 11)]
    for i, value, word in bad:
        args = list(good)
        args[i] = value
        assert lib.gymrs_entropy_lane(*args) == 1 and b"gymrs_entropy_lane" in lib.gymrs_last_error() and word in lib.gymrs_last_error(), (i, value)
