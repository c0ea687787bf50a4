"""The CPU reference of gymrs_advantages (tests/advantages_ref.py, tests/cpp/advantages_ref.c) is right, and the cases
tests/test_gpu_advantages.py compares the kernel on are worth comparing.  No GPU: the library is loaded for the host-only
gymrs_critic_value alone.

Exact properties of the rule: plain returns, independence of A[k] from the rows above k at lambda = 0, and the three poisoning
properties the selects give.  One accuracy check against an f64 numpy restatement of the same formulas: the largest absolute
difference over ACCURACY_CASES measured on the CPU is 3.814697265625e-06 (profiles/advantages.md); the bound is four times that --
the margin only absorbs libm / compiler differences between machines, not algorithmic error."""
import advantages_ref as ref
import numpy as np
import pytest
from advantages_ref import DIMS, bits

MEASURED_F64_DIFFERENCE = 3.814697265625e-06
ACCURACY_CASES = [(kind, shape, 17, hidden, gl) for kind in (0, 1) for shape, hidden, gl in ((3, 8, (0.97, 0.9)), (4, 7, (1.0, 1.0)), (2, 0, (0.5, 0.0)))]


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def outputs(c, **kw):
    return np.stack(ref.reference(c, **kw))


@pytest.mark.parametrize("shape,steps", [(2, 17), (3, 17), (1, 2), (0, 1)])
def test_plain_returns_are_the_integer_reward_sums(shape, steps):
    """no critic, gamma = lambda = 1, CartPole's 0 / 1 rewards: R[k] = the sum of the rewards up to and including the first ended step
    at or after k, or to the window's end"""
    c = ref.synthetic(0, shape, steps, 0, critic=False, gamma=1.0, lam=1.0)
    adv, ret, val = ref.reference(c)
    want = np.zeros((steps, c.n), np.int64)
    run = np.zeros(c.n, np.int64)
    for k in range(steps - 1, -1, -1):
        run = c.reward[k].astype(np.int64) + np.where(c.ended[k], 0, run)
        want[k] = run
    assert np.array_equal(ret, want.astype(np.float32)) and same(adv, ret) and not val.any() and not np.signbit(val).any()


@pytest.mark.parametrize("kind", [0, 1])
def test_lambda_zero_keeps_a_row_when_the_rows_above_are_rewritten(kind):
    c = ref.synthetic(kind, 2, 17, 8, gamma=0.5, lam=0.0, specials=False)
    adv = ref.reference(c)[0]
    other = ref.synthetic(kind, 2, 17, 8, gamma=0.5, lam=0.0, seed=99, specials=False)
    for k in (0, 5, 15):
        mixed = {f: np.concatenate([getattr(c, f)[:k + 1], getattr(other, f)[k + 1:]]) for f in ("obs", "reward", "done", "truncated", "final_obs")}
        assert same(ref.reference(c, **mixed)[0][k], adv[k]), k


@pytest.mark.parametrize("kind,hidden", [(0, 8), (1, 0), (0, 7)])
def test_poisoning_unselected_inputs_changes_no_output_bit(kind, hidden):
    c = ref.synthetic(kind, 2, 17, hidden, specials=False)
    base = outputs(c)
    assert np.isfinite(base).all()
    done, trunc = c.done != 0, c.truncated != 0
    # every final_obs element that is not truncated && !done
    fin = np.where((trunc & ~done)[:, None, :], c.final_obs, np.float32(np.nan))
    assert same(outputs(c, final_obs=fin), base) and (trunc & ~done).any()
    # the obs[K-1] column of a done step when final_obs is given
    obs = c.obs.copy()
    obs[-1][:, done[-1]] = np.nan
    assert same(outputs(c, obs=obs), base) and done[-1].any()
    # every row behind an ended step, as seen from the steps before it: per lane, poison everything above its first end after row k0
    for k0 in (0, 6):
        obs, rew, fin = c.obs.copy(), c.reward.copy(), c.final_obs.copy()
        first_end = np.where(c.ended[k0:].any(axis=0), k0 + c.ended[k0:].argmax(axis=0), c.steps)
        behind = np.arange(c.steps)[:, None] > first_end[None, :]  # rows strictly above the end
        rew[behind] = np.nan
        fin[np.broadcast_to(behind[:, None, :], fin.shape)] = np.nan
        obs[np.broadcast_to((np.arange(c.steps)[:, None] >= first_end[None, :])[:, None, :], obs.shape)] = np.nan  # the end's own obs row: a done step never reads it,
        # a truncated-only step reads final_obs in its place
        got = outputs(c, obs=obs, reward=rew, final_obs=fin)
        seen = np.arange(c.steps)[:, None] <= first_end[None, :]
        assert behind.any() and same(np.where(seen, got, 0), np.where(seen, base, 0)), k0


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("hidden", [0, 7, 8])
def test_host_call_equals_the_c_reference(gymrs, kind, hidden):
    d = DIMS[kind][0]
    assert gymrs.critic_size(kind, hidden) == ref.critic_size(kind, hidden)
    rng = np.random.default_rng(5 + hidden)
    w = ref.make_critics(kind, hidden, 4, 77)
    xs = [rng.standard_normal(d).astype(np.float32) for _ in range(8)]
    for value in (np.nan, np.inf, -np.inf, -0.0, 1e30):
        x = rng.standard_normal(d).astype(np.float32)
        x[rng.integers(d)] = value
        xs.append(x)
    xs.append(np.full(d, -0.0, np.float32))
    poisoned = w[0].copy()
    poisoned[1] = np.nan
    for crit in list(w) + [poisoned, np.zeros_like(w[0]), -np.zeros_like(w[0])]:
        for x in xs:
            assert bits(gymrs.critic_value(kind, hidden, crit, x)) == bits(ref.critic_value(kind, hidden, crit, x)), (crit, x)


def test_c_reference_is_close_to_the_f64_restatement():
    worst = 0.0
    for kind, shape, steps, hidden, (gamma, lam) in ACCURACY_CASES:
        c = ref.synthetic(kind, shape, steps, hidden, gamma=gamma, lam=lam, specials=False)
        got, want = ref.reference(c), ref.reference64(c)
        for a, b in zip(got, want):
            assert np.isfinite(a).all()
            worst = max(worst, float(np.abs(a.astype(np.float64) - b).max()))
    print("largest |f32 reference - f64 restatement| =", repr(worst))
    assert worst <= 4 * MEASURED_F64_DIFFERENCE


@pytest.mark.parametrize("kind,shape,steps,hidden,critic,final,trunc,returns,values,gl", ref.matrix())
def test_matrix_cases_are_worth_comparing(kind, shape, steps, hidden, critic, final, trunc, returns, values, gl):
    c = ref.synthetic(kind, shape, steps, hidden, critic, final, trunc, *gl)
    assert ref.worth_comparing(c) == []
    if c.final_obs is not None:  # unwritten elements are the sentinel
        assert (bits(c.final_obs)[~np.broadcast_to(c.ended[:, None, :], c.final_obs.shape)] == ref.SENTINEL).all()
    adv, ret, val = ref.reference(c)
    if not critic:
        assert not val.any()
    elif c.n >= 64:
        assert len(np.unique(bits(val[0]))) > c.n // 2  # the critic does vary over the lanes


def test_matrix_reaches_every_kernel_copy_and_every_axis_value():
    cov = ref.coverage()
    assert set(cov) == {(kind, critic) for kind in (0, 1) for critic in (False, True)}
    for (kind, critic), lanes in cov.items():
        assert (lanes > 0).all() if critic else (lanes[[0, 2]] > 0).all() and not lanes[[1, 3]].any(), (kind, critic, lanes)
    m = ref.matrix()
    for kind in (0, 1):
        rows = [r for r in m if r[0] == kind]
        assert {r[2] for r in rows} == set(ref.STEPS) and {r[3] for r in rows if r[4]} == set(ref.HIDDEN) and {r[9] for r in rows} == set(ref.GAMMA_LAMBDA)
        for axis in (4, 5, 6, 7, 8):
            assert {r[axis] for r in rows} == {False, True}, axis
        assert {r[1] for r in rows} == set(range(len(ref.SHAPES)))
        # the large shapes meet the critic with and without final_obs at K = 17
        assert {(r[4], r[5]) for r in rows if r[1] in (3, 4) and r[2] == 17} >= {(True, True)}
