"""CartPole's per-step fast path -- the scale-free division behind its two guards, the done-masks taken from the termination
compares -- bit for bit against the CPU f32 twin (which divides with `/` and knows none of it).

Every case compares state, observation, reward / done / truncated, statistics and the tick after 40 single HIP launches, after 40
more through gymrs_step_many (HIP launches), and after a 40-step chain on the engine's own queue (HIP launches again where the
dispatcher is not available: the kernels are the same templates):

  * sizes 256 (exactly one wave), 257 and 9001 (a ragged tail: the general per-lane code next to fast waves), 2^14 (many workgroups);
  * flag sets 0, A, A|S, A|S|T with max_episode_steps = 45: truncations from step 45 on, inside the 120 steps;
  * both integrators;
  * the default parameters (host guard on), a custom set inside the guard's interval (on) and one outside it (off: the kernel divides
    with `/`) -- the same bits in all three, because the twin never changes.

One more run starts from a POISONED state, written through set_state: a few lanes per wave with theta_dot = 1e30 (theta_dot^2
overflows: the numerator is infinite or NaN), 3e-30, theta = +-0 with theta_dot = +-0, NaN and infinite velocities and positions, and
an angle of 2.5 rad (which takes its wave off the fast path altogether).  Every third wave holds such lanes, so that
some waves trip the device guard and recompute their quotients with `/` and some do not.  Bit equality with the twin is the check:
nothing exposes the guard.

NaNs in that run.  Under auto-reset a poisoned lane ends on its first step and is re-armed, and the comparison is bit for bit as
everywhere else.  Without auto-reset (flag set 0) the poison stays and the arithmetic MAKES NaNs (inf - inf in xacc one step after
theta_dot = 1e30, and so on).  IEEE 754 leaves the sign and payload of a NaN that an operation makes, or picks among NaN operands, to
the implementation, and the two machines differ: from the second step on the GPU holds 0xffc00000 where the twin holds 0x7fc00000, in
25-40 lanes of 9001, NaN on both sides in every one of them.  That is a property of the two machines, not of any kernel (the parent
commit's library shows the same lanes and bits on these inputs: profiles/cartpole_fastpath_ab.log), so in the flag set 0 run a lane
must be NaN on both sides or on neither, and every value that is not a NaN must still have the twin's bits."""
import numpy as np
import pytest
from test_gpu_aql_chain import aql
from test_gpu_high_tick import A, Pair, S, T, same, same_stats

pytestmark = pytest.mark.gpu

SIZES = [256, 257, 9001, 1 << 14]
LIMIT = 45
FLAG_SETS = [pytest.param(f, id=name) for name, f in (("0", 0), ("A", A), ("AS", A | S), ("AST", A | S | T))]
# gravity, masscart, masspole, length, force_mag: tests/test_div_in_range.py shows what the host guard says to each
PARAMS = {"default": None, "inside": (3.7, 2.5, 0.4, 0.3, 6.0), "outside": (9.8, 1.0, 1.0, 10.0, 10.0)}


def make_pair(gymrs, twin, n, flags, integrator, which):
    p = Pair(gymrs, twin, 0, n, flags, 0, vec=4, limit=LIMIT)
    q = gymrs.engine.default_params(0)
    if PARAMS[which] is not None:
        q.gravity, q.masscart, q.masspole, q.length, q.force_mag = PARAMS[which]
    q.kinematics_integrator = integrator
    q.max_episode_steps = LIMIT
    p.eng.set_params(q)
    p.tw.set_params(q)
    return p


def run_three_ways(p, steps=40, check=None):
    check = check or p.check
    p.step(steps)
    check()
    with aql(False):
        p.step_many(steps)
    check()
    with aql(True):
        p.step_many(steps)
    check()


@pytest.mark.parametrize("which", list(PARAMS))
@pytest.mark.parametrize("integrator", [0, 1])
@pytest.mark.parametrize("flags", FLAG_SETS)
def test_fast_path_equals_the_twin(gymrs, twin, flags, integrator, which):
    for n in SIZES:
        p = make_pair(gymrs, twin, n, flags, integrator, which)
        run_three_ways(p)
        if flags & T:
            assert p.tw.stats()[2] > 0  # episodes did end (and, from step 45 on, by the limit)
        p.close()


def canonical(x):
    """`x` with every NaN replaced by the one quiet NaN 0x7fc00000 (see the module docstring: NaNs the arithmetic makes)"""
    x = np.array(x, np.float32, copy=True)
    x[np.isnan(x)] = np.uint32(0x7FC00000).view(np.float32)
    return x


def check_nan_as_nan(p):
    """Pair.check with NaNs compared as NaNs: NaN on both sides or on neither, every other value bit for bit"""
    at = ("tick", p.tw.tick())
    same("state", canonical(p.eng.get_state()), canonical(p.tw.get_state()), at)
    same("obs", canonical(p.eng.get_obs()), canonical(p.tw.get_obs()), at)
    p.check_flags()
    same_stats(0, p.eng.stats(), p.tw.stats(), at)
    assert p.eng.tick()[0] == p.tw.tick()


def poisoned(state):
    """`state` (4, n) with poisoned lanes in every third wave of 256 lanes; returns the lanes' wave indices that hold one"""
    st = state.copy()
    n = st.shape[1]
    nan, inf = np.float32("nan"), np.float32("inf")
    poison = [  # (lane inside the wave, {row: value})
        (3, {3: np.float32(1e30)}), (64, {3: np.float32(-1e30)}),
        (7, {3: np.float32(3e-30)}), (130, {3: np.float32(-3e-30)}),
        (11, {2: np.float32(0.0), 3: np.float32(0.0)}), (12, {2: np.float32(-0.0), 3: np.float32(-0.0)}),
        (13, {2: np.float32(0.0), 3: np.float32(-0.0)}), (200, {2: np.float32(-0.0), 3: np.float32(0.0)}),
        (17, {3: nan}), (18, {1: nan}), (255, {3: inf}), (254, {3: -inf}), (100, {1: inf}), (101, {0: nan}),
    ]
    waves = []
    for w in range(0, (n + 255) // 256, 3):
        for lane, values in poison:
            i = w * 256 + lane
            if i < n:
                for row, v in values.items():
                    st[row, i] = v
                waves.append(w)
        if w % 6 == 0 and w * 256 + 33 < n:
            st[2, w * 256 + 33] = np.float32(2.5)  # an angle beyond pi/4: the wave leaves the fast path (the general per-lane code)
    return st, sorted(set(waves))


@pytest.mark.parametrize("integrator", [0, 1])
@pytest.mark.parametrize("flags", [pytest.param(0, id="0"), pytest.param(A | S, id="AS"), pytest.param(A | S | T, id="AST")])
def test_poisoned_lanes_trip_the_device_guard_in_some_waves(gymrs, twin, flags, integrator):
    """Without auto-reset the poisoned lanes stay poisoned: their waves take the `/` branch on every step; with it they end and are
    re-armed after the first."""
    for n in (9001, 1 << 14):
        p = make_pair(gymrs, twin, n, flags, integrator, "default")
        st, waves = poisoned(p.tw.get_state())
        assert 0 < len(waves) < (n + 255) // 256 - len(waves)  # most waves stay clean
        p.eng.set_state(st)
        p.tw.set_state(st)
        check = p.check if flags & A else (lambda: check_nan_as_nan(p))
        for _ in range(4):  # every one of the first steps on its own, then the three submission forms
            p.step(1)
            check()
        run_three_ways(p, steps=12, check=check)
        p.close()
