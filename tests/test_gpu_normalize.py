"""gymrs_normalize_advantages on the device against gymrs_normalize_host (host only; tests/test_value_host.py holds it to the integer
restatement of the rule) per set, bit for bit, for `out` and `stats`.  Rows are wider than n_envs and keep their padding bytes."""
import numpy as np
import pytest
import torch
from advantages_ref import SENTINEL

pytestmark = pytest.mark.gpu
DEV, EINVAL, GID0, LPP, EPS = "cuda:0", 1, 11, 7, 1e-6
F = np.float32
# (n_envs, K): a ragged wave in the one-launch path; full and ragged waves in it; the smallest pairs above its 512 row items of 4 lanes
SHAPES = [(5, 1), (259, 3), (2049, 1), (1025, 2)]


def rows(n, steps, seed):
    a = (2.0 * np.random.default_rng([seed, n, steps]).standard_normal((steps, n)) + 0.5).astype(F)
    a[0, 1], a[steps - 1, n - 2] = np.nan, 8192.0  # a NaN and a non-member
    stride = (n + 15) // 16 * 16 + 16
    dev = torch.full((steps, stride), SENTINEL, dtype=torch.int32, device=DEV)
    dev[:, :n] = torch.from_numpy(a.view(np.int32)).to(DEV)
    return a, dev, stride


def launch(gymrs, a, dev, stride, n_sets, in_place, lanes=None, lpp=LPP):
    """(out bits [K][stride], stats [n_sets]) of one engine over the lanes `lanes` (default: all)"""
    steps, n = a.shape
    lo, hi = lanes or (0, n)
    eng = gymrs.BatchedEngine(gymrs.PENDULUM, hi - lo, global_env_offset=GID0 + lo, flags=5)  # every env kind is served
    eng.reset(seed=1)
    out = dev if in_place else torch.full_like(dev, SENTINEL)
    stats = torch.full((n_sets, 5), -1, dtype=torch.int64, device=DEV)  # the launch zeroes it itself
    torch.cuda.synchronize()
    eng.normalize_advantages(steps, adv=dev.data_ptr() + 4 * lo, out=out.data_ptr() + 4 * lo, stats=stats.data_ptr(), lane_stride=stride,
                             lanes_per_policy=lpp, n_sets=n_sets, eps=EPS)
    eng.sync()
    eng.close()
    return out.cpu().numpy().view(np.uint32), stats.cpu().numpy().view(gymrs.ADVANTAGE_STATS_DTYPE).reshape(-1)


@pytest.mark.parametrize("in_place", [False, True])
# one set: whole workgroups add through LDS; 7 lanes per set: gathered waves; 512: waves with one set each that differ within a workgroup
@pytest.mark.parametrize("n_sets,lpp", [(1, LPP), (3, LPP), (3, 512)])
@pytest.mark.parametrize("n,steps", SHAPES)
def test_out_and_stats_equal_the_host_rule_per_set(gymrs, n, steps, n_sets, lpp, in_place):
    a, dev, stride = rows(n, steps, 1)
    out, stats = launch(gymrs, a, dev, stride, n_sets, in_place, lpp=lpp)
    sets = np.array([((GID0 + i) // lpp) % n_sets for i in range(n)])
    for m in range(n_sets):
        wout, wst = gymrs.normalize_host(a[:, sets == m], eps=EPS)
        assert stats[m].tobytes() == wst.tobytes(), (m, stats[m], wst)
        assert np.array_equal(out[:, :n][:, sets == m].ravel(), wout.view(np.uint32)), m
    assert (out[:, n:] == SENTINEL).all() and stats["non_members"].sum() == 2 and stats["n"].sum() == n * steps - 2


def test_two_engines_that_cut_one_batch_add_up_to_one(gymrs):
    n, steps, cut = 2064, 2, 1040  # (the second part takes the one-launch path, the first and the whole the four launches) the second block's rows start 16-byte aligned inside the first one's
    a, dev, stride = rows(n, steps, 2)
    whole = launch(gymrs, a, dev, stride, 3, False)[1]
    parts = [launch(gymrs, a, dev, stride, 3, False, lanes)[1] for lanes in ((0, cut), (cut, n))]
    for name in ("s1", "n", "non_members"):
        assert np.array_equal(parts[0][name] + parts[1][name], whole[name]), name
    # S2 is taken about the mean of the engine's OWN members, so the parts' S2 do not add up to the whole's: they differ by the
    # parallel-axis term n_p * (mean_p - mean)^2.  Tolerance from the rule: per element 2^-25 (the fixed point) + 3 * 2^-24 * sq (dm
    # and the square round once each in f32), on both sides, + 3 n d^2 for a mean off by d <= 2^-23 (|mean| < 1 here).
    s2 = lambda st: st["s2"].astype(np.float64) * 2.0**-24  # noqa: E731
    shift = sum(p["n"] * (p["mean"].astype(np.float64) - whole["mean"]) ** 2 for p in parts)
    tol = 2 * (whole["n"] * 2.0**-25 + 3 * 2.0**-24 * s2(whole)) + 3 * whole["n"] * 2.0**-46
    assert (np.abs(s2(parts[0]) + s2(parts[1]) + shift - s2(whole)) <= tol).all() and (shift > 0).all()


def test_refusals_and_no_steps(gymrs):
    a, dev, stride = rows(259, 3, 3)
    eng = gymrs.BatchedEngine(gymrs.CARTPOLE, 259, flags=1)
    eng.reset(seed=1)
    stats = torch.full((3, 5), -1, dtype=torch.int64, device=DEV)
    good = dict(adv=dev.data_ptr(), out=dev.data_ptr(), stats=stats.data_ptr(), lane_stride=stride, lanes_per_policy=LPP, n_sets=3, eps=EPS)
    cases = [("flag", dict(flags=1)), ("eps", dict(eps=0.0)), ("eps", dict(eps=float("nan"))), ("eps", dict(eps=float("inf"))), ("n_sets", dict(n_sets=0)),
             ("lanes_per_policy", dict(lanes_per_policy=0)), ("adv is NULL", dict(adv=0)), ("out is NULL", dict(out=0)), ("stats is NULL", dict(stats=0)),
             ("16-byte aligned", dict(out=dev.data_ptr() + 4)), ("8-byte aligned", dict(stats=stats.data_ptr() + 4)), ("lane_stride", dict(lane_stride=256)),
             ("lane_stride", dict(lane_stride=stride + 8))]
    for word, change in cases:
        with pytest.raises(gymrs.GymrsError, match=word) as err:
            eng.normalize_advantages(3, **dict(good, **change))
        assert err.value.status == EINVAL and "gymrs_normalize_advantages" in str(err.value), word
    eng.normalize_advantages(0, **good)  # a no-op after the checks
    eng.sync()
    assert (stats == -1).all()
    eng.close()
