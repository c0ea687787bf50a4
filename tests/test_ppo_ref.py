"""The CPU reference of gymrs_ppo_gradient (tests/ppo_ref.py, tests/cpp/ppo_ref.c) equals the library's host-only gymrs_ppo_lane
integer for integer, equals gymrs_gradient_lane fed the coefficient row of the rule, agrees with the calculus of the clipped objective,
and its cases hold what makes them worth comparing.  No GPU: the library is loaded for the two host-only lanes alone."""
import numpy as np
import ppo_ref as ref
import pytest
from ppo_ref import bits

CASES = [(kind, shape, hidden) for kind, shape, hidden in ref.matrix() if shape in (0, 1, 2)]  # 1, 5 and 257 lanes: every lane is compared


def same_bits(a, b):
    return ((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all()  # a NaN equals any NaN, as elsewhere in the suite


def lanes_by_library(gymrs, c):
    """(grad, excluded, counts, prob) of the case, every lane through gymrs.ppo_lane, summed here modulo 2^64"""
    grad = np.zeros((c.n_sets, ref.size_of(c.kind, c.hidden)), np.uint64)
    excluded, counts = np.zeros(c.n_sets, np.uint64), np.zeros((c.n_sets, 2), np.uint64)
    pr = np.zeros((c.steps, c.n), np.float32)
    idx = ref.set_index(c)
    for i in range(c.n):
        x, a, adv = ref.inputs_of(c, i)
        q, ex, cnt, p = gymrs.ppo_lane(c.kind, c.hidden, c.weights[idx[i]], x, a, adv, c.old_prob[:, i], clip_low=c.clip_low, clip_high=c.clip_high,
                                       scale=c.scale, prob=True)
        grad[idx[i]] += q.view(np.uint64)
        excluded[idx[i]] += np.uint64(ex)
        counts[idx[i]] += cnt
        pr[:, i] = p
    return grad.view(np.int64), excluded, counts, pr


@pytest.mark.parametrize("kind,shape,hidden", CASES)
def test_the_c_restatement_equals_gymrs_ppo_lane(gymrs, kind, shape, hidden):
    for steps in ref.STEPS:
        c = ref.synthetic(kind, shape, steps, hidden)
        want = ref.reference(c)
        got = lanes_by_library(gymrs, c)
        at = (kind, shape, hidden, steps)
        for name, g, w in zip(("grad", "excluded", "counts"), got, want):
            assert np.array_equal(g, w), (name, at)
        assert same_bits(got[3], want[3]), at
        if c.n >= 64:  # (a handful of lane-steps may all be cut, or all out of range)
            assert want[0].any() and want[2].all() and want[1].sum() > 0, at


@pytest.mark.parametrize("kind,shape,hidden", CASES)
def test_ppo_lane_equals_gradient_lane_fed_the_rules_coefficient(gymrs, kind, shape, hidden):
    """by definition the call equals gymrs_policy_gradient with coef[k][i] = c: the coefficient row is computed here in numpy f32 from
    the prob row gymrs_gradient_lane gives, and the two host lanes agree integer for integer; the counters are those of the rule"""
    for steps in ref.STEPS:
        c = ref.synthetic(kind, shape, steps, hidden)
        idx = ref.set_index(c)
        for i in range(c.n):
            x, a, adv = ref.inputs_of(c, i)
            w = c.weights[idx[i]]
            _, _, pa = gymrs.gradient_lane(c.kind, c.hidden, w, x, a, np.zeros(steps, np.float32), scale=c.scale, prob=True)
            one = ref.SimpleNamespace(kind=kind, advantages=adv[:, None], old_prob=c.old_prob[:, i:i + 1], actions=a[:, None], clip_low=c.clip_low,
                                      clip_high=c.clip_high)
            _, cut, coef, on = ref.rule(one, pa[:, None])
            q1, ex1, p1 = gymrs.gradient_lane(c.kind, c.hidden, w, x, a, coef[:, 0], scale=c.scale, prob=True)
            q2, ex2, cnt, p2 = gymrs.ppo_lane(c.kind, c.hidden, w, x, a, adv, c.old_prob[:, i], clip_low=c.clip_low, clip_high=c.clip_high, scale=c.scale,
                                              prob=True)
            at = (kind, shape, hidden, steps, i)
            assert np.array_equal(q1, q2) and ex1 == ex2 and same_bits(p1, p2), at
            assert cnt.tolist() == [int(on.sum()), int(cut.sum())], at


@pytest.mark.parametrize("kind,shape,hidden", [case for case in ref.matrix() if ref.SHAPES[case[1]][0] >= 64])
def test_every_case_of_64_lanes_or_more_is_worth_comparing(kind, shape, hidden):
    for steps in ref.STEPS:
        c = ref.synthetic(kind, shape, steps, hidden)
        assert ref.worth_comparing(c) == [], (kind, shape, hidden, steps, c.seed)
        assert len(c.planted) == 12


def test_small_shapes_use_the_plain_bounds():
    for shape in (0, 1):
        c = ref.synthetic(0, shape, 7, 5)
        assert (c.clip_low, c.clip_high) == ref.PLAIN_BOUNDS == (float(np.float32(0.8)), float(np.float32(1.2))) and not c.planted


@pytest.mark.parametrize("kind,shape,hidden", [(0, 2, 0), (1, 2, 0), (0, 2, 5), (1, 2, 5), (0, 2, 64), (1, 2, 64), (0, 1, 1)])
@pytest.mark.parametrize("steps", [1, 7])
def test_against_calculus(kind, shape, hidden, steps):
    """|grad * 2^-24 - G64| <= (K + 16) * 2^-22 * B + lanes * 2^-25 per parameter: the project's bound for gymrs_policy_gradient
    (tests/test_gradient_ref.py derives the constant), with B built the same way from the coefficient |adv * ratio * beta| of the lane-
    steps that are not cut.  G64 is the gradient of  sum min(ratio * adv, clip(ratio, low, high) * adv)  in f64
    (ppo_ref.reference64).  The objective has a kink where a ratio meets a bound, and a hidden unit one at z = 0: the cases use the
    bounds 0.8 / 1.2 with ratios near 0.5, 0.91, 1, 1.11 and 2, and it is asserted on the reference that every ratio stays at least
    1e-3 from both bounds and every |z| above 1e-6.  No lane is planted (`specials=False`).  The test prints the largest error / bound
    of every case."""
    c = ref.synthetic(kind, shape, steps, hidden, specials=False, boundary=False)
    grad, excluded, counts, _, _ = ref.reference(c)
    assert not excluded.any()
    g64, bound, zmin, margin = ref.reference64(c)
    assert zmin > 1e-6 and margin >= 1e-3
    err = np.abs(grad.astype(np.float64) * 2.0**-24 - g64)
    tol = (steps + 16) * 2.0**-22 * bound + c.n * 2.0**-25
    worst = float((err / tol).max())
    print(f"calculus: kind {kind} shape {shape} H {hidden} K {steps}: largest error / bound = {worst:.4f}, cut {int(counts[:, 1].sum())} of {int(counts[:, 0].sum())}")
    assert (err <= tol).all(), (worst, np.unravel_index(np.argmax(err / tol), err.shape))
    if c.n >= 64:
        assert np.abs(g64).max() > 1e-3 and counts[:, 1].sum() > 0


@pytest.mark.parametrize("kind,hidden", [(0, 0), (1, 5), (0, 64)])
def test_additivity_over_lanes_and_launches(kind, hidden):
    c = ref.synthetic(kind, 2, 7, hidden)
    whole = ref.reference(c)
    for cut in (1, 100, 129, 256):
        g, e, n, _, _ = ref.reference(c, lanes=slice(0, cut))
        ref.reference(c, lanes=slice(cut, c.n), grad=g, excluded=e, counts=n)
        assert np.array_equal(g, whole[0]) and np.array_equal(e, whole[1]) and np.array_equal(n, whole[2]), cut
    g, e, n, _, _ = ref.reference(c)
    ref.reference(c, grad=g, excluded=e, counts=n)
    assert np.array_equal(g, 2 * whole[0]) and np.array_equal(e, 2 * whole[1]) and np.array_equal(n, 2 * whole[2])


@pytest.mark.parametrize("kind,shape,hidden", [(0, 2, 0), (1, 2, 5), (0, 5, 64)])
def test_the_planted_lanes_do_what_the_rule_says(kind, shape, hidden):
    c = ref.synthetic(kind, shape, 7, hidden)
    idx = ref.set_index(c)
    out = {}
    for name, i in c.planted.items():
        x, a, adv = ref.inputs_of(c, i)
        out[name] = ref.lane(kind, hidden, c.scale, c.clip_low, c.clip_high, c.weights[idx[i]], x, a, adv, c.old_prob[:, i])
    a_out = ref.DIMS[kind][1]
    # old_prob = 0 under a negative advantage: ratio = +inf is not below clip_low, c = -inf; a NaN old_prob: c = NaN: pairs are excluded
    for name in ("po_zero", "po_nan", "adv_nan", "nan"):  # a non-finite c reaches every bias sum of the last layer at least
        assert out[name][1] >= a_out, name
    for name in ("adv_nbig", "big"):  # ratio 1, never cut: the sums pass 2^30
        assert out[name][1] >= 1 and out[name][2].tolist() == [7, 0], name
    assert np.isneginf(out["po_zero"][4][0]) and np.isnan(out["po_nan"][4][0])
    # old_prob = +inf: ratio = +0, which a negative advantage cuts and a positive one multiplies to 0: nothing is excluded by it
    assert out["po_inf"][4][0] == 0.0
    # a negative old_prob is arithmetic like any other: ratio < 0, cut exactly when the advantage is negative
    i = c.planted["po_neg"]
    assert (out["po_neg"][4][0] == 0.0) == bool(c.advantages[0, i] < 0) and out["po_neg"][1] == 0
    # an advantage of either zero is never cut, counts, and adds nothing
    for name in ("adv_pzero", "adv_nzero"):
        q, ex, cnt, _, cf = out[name]
        assert not q.any() and ex == 0 and cnt.tolist() == [7, 0] and not cf.any(), name
    # every action out of range: nothing added, nothing excluded, nothing counted
    q, ex, cnt, pr, _ = out["off"]
    assert not q.any() and ex == 0 and cnt.tolist() == [0, 0] and not pr.any()
    # ratio == the bound is not cut; one ulp further it is
    for (k, i), side in zip(c.boundary, ("high", "low")):
        x, a, adv = ref.inputs_of(c, i)
        args = (kind, hidden, c.scale)
        at = ref.lane(*args, c.clip_low, c.clip_high, c.weights[idx[i]], x[k:k + 1], a[k:k + 1], adv[k:k + 1], c.old_prob[k:k + 1, i])
        low, high = np.float32(c.clip_low), np.float32(c.clip_high)
        low, high = (low, np.nextafter(high, np.float32(0))) if side == "high" else (np.nextafter(low, np.float32(2)), high)
        past = ref.lane(*args, float(low), float(high), c.weights[idx[i]], x[k:k + 1], a[k:k + 1], adv[k:k + 1], c.old_prob[k:k + 1, i])
        assert at[2].tolist() == [1, 0] and at[0].any() and past[2].tolist() == [1, 1] and not past[0].any(), side
