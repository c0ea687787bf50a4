"""gymrs_value_lane and gymrs_normalize_host (host only, no GPU) against tests/value_ref.py, bit for bit; one calculus check each."""
import advantages_ref as adv
import gradient_ref as ref
import numpy as np
import pytest
import value_ref as vr
from types import SimpleNamespace

F = np.float32
CLIP = 0.25


def case(gymrs, kind, hidden, steps, clipped, seed=3):
    """one lane with every edge planted where the arithmetic allows it: dl == +clip, dl == -clip, e2^2 == e1^2"""
    w = adv.make_critics(kind, hidden, 1, 40 + hidden)[0]
    x, rn, on = (a[..., 0] for a in vr.draw(kind, hidden, 1, steps, seed))
    v = gymrs.value_lane(kind, hidden, w, x, np.zeros(steps, F))[4]
    R, vo, j = (v + rn).astype(F), (v + on).astype(F), None
    if clipped and steps >= 6:
        vo[4] = np.nan                                      # compares false: plain on this step
        # dl == +clip and dl == -clip at the first steps where the subtraction is exact: not clipped
        up = next(int(k) for k in range(5, steps) if F(v[k] - F(v[k] - F(CLIP))) == F(CLIP))
        dn = next(int(k) for k in range(up + 1, steps) if F(v[k] - F(v[k] + F(CLIP))) == F(-CLIP))
        vo[up], vo[dn] = v[up] - F(CLIP), v[dn] + F(CLIP)
        # vc == -v exactly and R == 0: clipped, e2 == -e1, the squares are equal: not cut (the first step where vo -+ clip is exact)
        s = np.where(v > 0, F(1.0), F(-1.0)).astype(F)
        mirror = (-v - s * F(CLIP)).astype(F)
        j = next(int(k) for k in range(dn + 1, steps) if F(mirror[k] + s[k] * F(CLIP)) == -v[k] and v[k] != 0)
        vo[j], R[j] = mirror[j], 0.0
        j = (up, dn, j)
    return w, x, R, (vo if clipped else None), j


@pytest.mark.parametrize("clipped", [False, True])
@pytest.mark.parametrize("hidden", [0, 1, 7, 64])
@pytest.mark.parametrize("kind", [0, 1])
def test_value_lane_equals_the_rule_and_the_critic_head_fed_c(gymrs, kind, hidden, clipped):
    steps = 24
    w, x, R, vo, j = case(gymrs, kind, hidden, steps, clipped)
    q, ex, sums, counts, values = gymrs.value_lane(kind, hidden, w, x, R, vo, clip=CLIP)
    wq, wex, wsums, wcounts, wvalues, c = vr.lane(kind, hidden, w, x, R, vo, CLIP)
    assert np.array_equal(values.view(np.uint32), wvalues.view(np.uint32))
    assert np.array_equal(q, wq) and ex == wex == 0 and [int(s) for s in sums] == wsums and [int(n) for n in counts] == wcounts
    q2, ex2 = gymrs.gradient_lane(kind, hidden, w, x, None, c, critic=True)
    assert np.array_equal(q, q2) and ex2 == 0 and q.any()
    if clipped:
        dl = (values - vo).astype(F)
        up, dn, j = j
        assert dl[up] == F(CLIP) and dl[dn] == F(-CLIP) and all(c[k] == F(values[k] - R[k]) for k in (up, dn)), "dl == +-clip is not clipped"
        assert abs(dl[j]) > CLIP and c[j] == values[j] != 0 and R[j] == 0, "clipped to -v with R = 0: e2^2 == e1^2 is not cut"
        assert c[4] == F(values[4] - R[4]), "a NaN old value is neither clipped nor cut"
        assert 0 < counts[1] < steps


@pytest.mark.parametrize("hidden", [0, 7])
def test_a_nan_return_excludes_the_lane(gymrs, hidden):
    w, x, R, vo, _ = case(gymrs, 0, hidden, 24, True)
    R[3] = np.nan
    q, ex, sums, counts, _ = gymrs.value_lane(0, hidden, w, x, R, vo, clip=CLIP)
    wq, wex, wsums, wcounts, _, _ = vr.lane(0, hidden, w, x, R, vo, CLIP)
    assert ex == wex and ex >= 2 and not np.asarray(sums).any() and np.array_equal(q, wq) and [int(n) for n in counts] == wcounts
    assert counts[0] == 24


@pytest.mark.parametrize("kind,hidden", [(0, 0), (1, 7), (0, 64)])
def test_value_lane_against_calculus(gymrs, kind, hidden):
    """q * 2^-24 against the f64 gradient of sum 0.5 * max(e1^2, e2^2) at points at least 1e-3 away from the clip boundary and from
    e2^2 == e1^2, under gradient_ref's bound for the critic head, unchanged: (K + 16) * 2^-22 * B + lanes * 2^-25 with B from the f64
    coefficient.  Measured largest error / bound: 0.0015 (H = 0), 0.0073 (H = 7), 0.076 (H = 64)."""
    lanes, steps, clip = 64, 7, 0.2
    w = adv.make_critics(kind, hidden, 1, 7)
    x, rn, on = vr.draw(kind, hidden, lanes, steps, 11)
    grad, coef = np.zeros(w.shape[1], object), np.zeros((steps, lanes))
    for i in range(lanes):
        v64 = np.array([vr.forward64(kind, hidden, w[0], x[k, :, i]) for k in range(steps)])
        R, vo = (v64 + rn[:, i]).astype(F), (v64 + on[:, i]).astype(F)
        vc = np.clip(v64, vo.astype(np.float64) - clip, vo.astype(np.float64) + clip)
        e1, e2 = v64 - R, vc - R
        near = (np.abs(np.abs(v64 - vo) - clip) < 1e-3) | ((vc != v64) & (np.abs(e2 * e2 - e1 * e1) < 1e-3))
        vo[near] = v64[near].astype(F)  # move such a point inside the range: not clipped
        vc = np.clip(v64, vo.astype(np.float64) - clip, vo.astype(np.float64) + clip)
        coef[:, i] = np.where((vc != v64) & ((vc - R) ** 2 > e1 * e1), 0.0, e1)
        q, ex = gymrs.value_lane(kind, hidden, w[0], x[:, :, i], R, vo, clip=clip)[:2]
        assert ex == 0
        grad += q.astype(object)
    c = SimpleNamespace(kind=kind, hidden=hidden, critic=True, scale=0.0, n=lanes, gid0=0, lanes_per_set=lanes, n_sets=1, steps=steps, weights=w,
                        start_obs=x[0], obs=x[1:], actions=np.zeros((steps, lanes), np.uint8), coef=coef)
    g64, bound, zmin = ref.reference64(c)
    assert zmin > 1e-6 and (coef == 0).mean() > 0.1
    err = np.abs(grad.astype(np.float64) * 2.0**-24 - g64[0])
    tol = (steps + 16) * 2.0**-22 * bound[0] + lanes * 2.0**-25
    print(f"value calculus: kind {kind} H {hidden}: largest error / bound = {float((err / tol).max()):.4f}")
    assert (err <= tol).all(), float((err / tol).max())


def special(rng, count):
    a = (3.0 * rng.standard_normal(count) + 1.5).astype(F)
    if count >= 8:
        a[[1, 2, 3, 4]] = [np.nan, 8192.0, -np.inf, np.nextafter(F(8192.0), F(0.0))]  # non-members, and the largest member
    return a


@pytest.mark.parametrize("count", [0, 1, 2, 5, 1000])
def test_normalize_host_equals_the_integer_restatement(gymrs, count):
    a = special(np.random.default_rng(count), count)
    out, st = gymrs.normalize_host(a, eps=1e-6)
    wout, wst = vr.normalize(a, 1e-6)
    assert np.array_equal(out.view(np.uint32), wout.view(np.uint32))
    assert (int(st["s1"]), int(st["n"]), int(st["s2"]), int(st["non_members"])) == wst[:4]
    assert st["mean"].view(np.uint32) == wst[4].view(np.uint32) and st["inv"].view(np.uint32) == wst[5].view(np.uint32)
    if count >= 8:
        assert st["non_members"] == 3 and np.isnan(out[1]) and out[4] > 0
    if count == 0:
        assert st["n"] == 0 and st["mean"] == 0 and st["inv"] == F(1.0 / np.float64(F(1e-6)))


def test_normalize_host_edges(gymrs):
    one, st1 = gymrs.normalize_host([2.5, np.nan], eps=0.5)
    assert st1["n"] == 1 and st1["mean"] == 2.5 and st1["inv"] == 2.0 and one[0] == 0.0 and np.isnan(one[1])  # n = 1: sd = 0
    same, st = gymrs.normalize_host([0.75] * 9, eps=0.5)
    assert st["s2"] == 0 and st["inv"] == 2.0 and not same.any()  # all-equal members: sd = 0
    none, st0 = gymrs.normalize_host([np.inf, 8192.0], eps=0.5)
    assert st0["n"] == 0 and st0["non_members"] == 2 and none[0] == np.inf and none[1] == F(16384.0)  # n = 0: mean = 0, inv = 1 / eps
    for eps in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(gymrs.GymrsError, match="eps"):
            gymrs.normalize_host([1.0], eps=eps)


def test_normalize_host_against_f64(gymrs):
    """Against numpy's f64 mean and std (ddof = 1) of the same f32 data.  The rule's resolution is 2^-24 per element and per square,
    rounded to nearest: the mean is off by at most 2^-25 (the elements' roundings average) plus its f32 rounding 2^-24 |mean|; the
    squares are taken about the f32 mean in f32 (2^-24 relative each) and fixed (2^-25 each), so var is off by at most 2^-23 var +
    2^-25 + 2 |dmean| sd, and sd by that over 2 sd.  Measured error / tolerance: 0.45 (mean), 0.26 (sd)."""
    a = special(np.random.default_rng(5), 4096)
    out, st = gymrs.normalize_host(a, eps=1e-6)
    m = a[np.isfinite(a) & (np.abs(a) < 8192)].astype(np.float64)
    mean, sd = m.mean(), m.std(ddof=1)
    tol_mean = 2.0**-25 + 2.0**-24 * abs(mean)
    tol_sd = (2.0**-23 * sd * sd + 2.0**-25 + 2 * tol_mean * sd) / (2 * sd) + 2.0**-24 * sd  # + the f32 rounding of inv
    got_sd = 1.0 / float(st["inv"]) - float(F(1e-6))
    print(f"normalize: error / tolerance = {abs(float(st['mean']) - mean) / tol_mean:.3f} (mean), {abs(got_sd - sd) / tol_sd:.3f} (sd)")
    assert abs(float(st["mean"]) - mean) <= tol_mean and abs(got_sd - sd) <= tol_sd
