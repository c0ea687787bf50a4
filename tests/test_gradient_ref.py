"""The CPU reference of gymrs_policy_gradient (tests/gradient_ref.py, tests/cpp/gradient_ref.c) equals the library's host-only
gymrs_gradient_lane integer for integer, agrees with calculus, is additive, and excludes what the rule excludes.  No GPU: the library
is loaded for gymrs_gradient_lane alone."""
import gradient_ref as ref
import numpy as np
import pytest
from gradient_ref import bits

CASES = [(kind, shape, hidden) for kind, shape, hidden in ref.matrix() if shape in (0, 1, 2)]  # 1, 5 and 257 lanes: every lane is compared


def lanes_by_library(gymrs, c, prob):
    """(grad, excluded, prob) of the case, every lane through gymrs.gradient_lane, summed here modulo 2^64"""
    grad = np.zeros((c.n_sets, ref.size_of(c.kind, c.hidden, c.critic)), np.uint64)
    excluded = np.zeros(c.n_sets, np.uint64)
    pr = np.zeros((c.steps, c.n), np.float32)
    idx = ref.set_index(c)
    for i in range(c.n):
        x, a, cf = ref.inputs_of(c, i)
        out = gymrs.gradient_lane(c.kind, c.hidden, c.weights[idx[i]], x, a, cf, critic=c.critic, scale=None if c.critic else c.scale, prob=prob)
        grad[idx[i]] += out[0].view(np.uint64)
        excluded[idx[i]] += np.uint64(out[1])
        if prob:
            pr[:, i] = out[2]
    return grad.view(np.int64), excluded, pr


@pytest.mark.parametrize("kind,shape,hidden", CASES)
def test_the_c_restatement_equals_gymrs_gradient_lane(gymrs, kind, shape, hidden):
    for critic in (False, True):
        for steps in ref.STEPS:
            c = ref.synthetic(kind, shape, steps, hidden, critic)
            want = ref.reference(c, prob=not critic)
            got = lanes_by_library(gymrs, c, prob=not critic)
            at = (kind, shape, hidden, critic, steps)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), at
            if not critic:
                same = (bits(got[2]) == bits(want[2])) | (np.isnan(got[2]) & np.isnan(want[2]))  # a NaN equals any NaN, as elsewhere in the suite
                assert same.all(), at
                assert want[0].any(), at


@pytest.mark.parametrize("kind,shape,hidden,critic", [(0, 2, 0, False), (1, 2, 0, False), (0, 2, 5, False), (1, 2, 5, True), (0, 2, 64, False),
                                                       (1, 2, 64, False), (0, 2, 64, True), (0, 1, 1, False), (1, 2, 0, True)])
@pytest.mark.parametrize("steps", [1, 7])
def test_against_calculus(kind, shape, hidden, critic, steps):
    """|grad * 2^-24 - G64| <= (K + 16) * 2^-22 * B + lanes * 2^-25 per parameter, G64 and B by gradient_ref.reference64.

    Where the constant comes from (u = 2^-24, the f32 unit roundoff; B = the sum over the parameter's terms of |c * beta| * m with
    m = |x_j|, |r|, sum_b |W2[b][h]| or their product, i.e. the magnitude a term can have when |1{a = b} - p| <= 1):
      * accumulation: K roundings (the fma's own, or the add's), each at most u times a partial sum <= B:  K * u * B;
      * a term: beta and c * beta round once each, the subtraction and the product with cb once each (4u); with a hidden layer, e
        adds A roundings and r (D + 1) roundings of z: at most 4 + 3 + 5 = 12 u relative to |c * beta| * m;
      * p: its absolute error enters a term with weight |c * beta| * m.  The weights 2^d come from a degree-6 polynomial with a
        relative error of 6.7e-8 < 2^-23 (profiles/policy_sample.md); d = (y[b] - y[greedy]) * scale carries the rounding of the
        logits, at most (D + H + 2) u * L * scale with L = the f64 sum of |w| |x| behind a logit, and dp <= p * ln 2 * dd; the sum and the
        divide add (A + 1) u.  With the cases' weights (unit normals over sqrt(fan-in)) and observations (unit normals) L * scale
        stays below 2^4 and (D + H + 2) <= 70, so the logits' share is below 2^4 * 70 * ln 2 u < 2^10 u in the worst case -- but that
        worst case multiplies p <= 1 of an action whose weight is then ~2^-16 of the total; for actions with p of order 1 the logit
        differences are of order 1 and the share is below (D + H + 2) * 4 u * ln 2 / 8 < 28 u for H = 64.  Together below 48 u.
    4 + 12 + 48 = 64 = 16 * 4 units of u, hence (K + 16) * 4u = (K + 16) * 2^-22: the constant the issue states, kept as stated.  Every
    lane's rounding to the fixed point adds at most half a unit of 2^-24: lanes * 2^-25.  Lanes planted to be excluded are left out of the
    case (`specials=False`); a hidden unit within 1e-6 of its kink has no derivative to compare with: asserted not to occur.  The test
    prints the largest error / bound of every case (on the CPU reference they are between 0.001 and 0.13)."""
    c = ref.synthetic(kind, shape, steps, hidden, critic, specials=False)
    grad, excluded, _ = ref.reference(c)
    assert not excluded.any()
    g64, bound, zmin = ref.reference64(c)
    assert zmin > 1e-6
    err = np.abs(grad.astype(np.float64) * 2.0**-24 - g64)
    tol = (steps + 16) * 2.0**-22 * bound + c.n * 2.0**-25
    worst = float((err / tol).max())
    print(f"calculus: kind {kind} shape {shape} H {hidden} critic {critic} K {steps}: largest error / bound = {worst:.4f}")
    assert (err <= tol).all(), (worst, np.unravel_index(np.argmax(err / tol), err.shape))
    assert np.abs(g64).max() > 1e-3


@pytest.mark.parametrize("kind,hidden,critic", [(0, 0, False), (1, 5, False), (0, 64, True), (1, 1, True)])
def test_additivity_over_lanes_and_launches(kind, hidden, critic):
    c = ref.synthetic(kind, 2, 7, hidden, critic)
    whole = ref.reference(c)
    for cut in (1, 100, 129, 256):
        g, e, _ = ref.reference(c, lanes=slice(0, cut))
        ref.reference(c, lanes=slice(cut, c.n), grad=g, excluded=e)
        assert np.array_equal(g, whole[0]) and np.array_equal(e, whole[1]), cut
    g, e, _ = ref.reference(c)
    ref.reference(c, grad=g, excluded=e)
    assert np.array_equal(g, 2 * whole[0]) and np.array_equal(e, 2 * whole[1])


@pytest.mark.parametrize("kind,shape,hidden", [(0, 2, 0), (1, 2, 5), (0, 5, 64), (1, 3, 1), (0, 4, 5)])
@pytest.mark.parametrize("critic", [False, True])
def test_exclusions(kind, shape, hidden, critic):
    """the planted lanes are counted and add nothing where they are excluded, their neighbours are unchanged, an out-of-range action
    adds nothing and is not counted, and no other lane is excluded anywhere"""
    c = ref.synthetic(kind, shape, 7, hidden, critic)
    idx = ref.set_index(c)
    s = ref.size_of(kind, hidden, critic)
    per_lane = {}
    counts = np.zeros(c.n, np.int64)
    for i in range(c.n):
        x, a, cf = ref.inputs_of(c, i)
        q, ex, _ = ref.lane(kind, hidden, critic, c.scale, c.weights[idx[i]], x, a, cf)
        counts[i] = ex
        if i in c.planted.values():
            per_lane[i] = q
    planted = sorted(c.planted.values())
    others = np.setdiff1d(np.arange(c.n), planted)
    assert len(planted) == 4 and not counts[others].any()  # away from the planted lanes nothing is excluded
    for name in ("inf", "nan", "big"):
        i = c.planted[name]
        assert counts[i] >= 1, name
    if not critic:
        i = c.planted["off"]  # every action out of range, every observation infinite: nothing added, nothing counted
        assert counts[i] == 0 and not per_lane[i].any()
    i = c.planted["nan"]  # a NaN coefficient reaches every bias sum of the last layer at least
    assert counts[i] >= ref.outputs_of(kind, critic) and not per_lane[i][s - ref.outputs_of(kind, critic):].any()
    # the table is the sum of the lanes that are not planted plus what the planted lanes add: their neighbours are unchanged
    whole, excluded, _ = ref.reference(c)
    clean = ref.synthetic(kind, shape, 7, hidden, critic)
    for i in planted:  # the planted lanes made harmless: coefficient 0, finite observations, valid actions
        clean.coef[:, i], clean.start_obs[:, i], clean.obs[:, :, i], clean.actions[:, i] = 0.0, 0.0, 0.0, 0
    base, base_excluded, _ = ref.reference(clean)
    assert not base_excluded.any()
    extra = np.zeros_like(base)
    for i in planted:
        extra[idx[i]] += per_lane[i]
    assert np.array_equal(whole, base + extra)
    assert np.array_equal(excluded, np.bincount(idx, weights=counts, minlength=c.n_sets).astype(np.uint64))
    # an out-of-range action on a lane that is not planted: the step adds nothing
    lane = int(others[np.argmax((c.actions[:, others] >= ref.outputs_of(kind, critic)).any(axis=0))]) if not critic else None
    if lane is not None and (c.actions[:, lane] >= ref.outputs_of(kind, critic)).any():
        x, a, cf = ref.inputs_of(c, lane)
        keep = a < ref.outputs_of(kind, critic)
        q_all, _, _ = ref.lane(kind, hidden, critic, c.scale, c.weights[idx[lane]], x, a, cf)
        q_kept, _, _ = ref.lane(kind, hidden, critic, c.scale, c.weights[idx[lane]], x[keep], a[keep], cf[keep])
        assert np.array_equal(q_all, q_kept)
