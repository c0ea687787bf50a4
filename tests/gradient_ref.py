"""gymrs_policy_gradient computed on the CPU alone (include/gymrs_amd.h, "gradients").

The rule is restated in tests/cpp/gradient_ref.c from the header's text (plain C, libm's fmaf, gcc -O2 -ffp-contract=off) and once
more here in f64 numpy (the calculus yardstick of tests/test_gradient_ref.py).  The synthetic records are built in numpy, so the
kernels are tested independently of the rollout kernels.  This module never imports the library: what it returns is the yardstick of
tests/test_gpu_gradient.py.

A plain module like advantages_ref.py, imported by test files; no fixtures, no pytest hooks."""
import ctypes as C
import tempfile
from pathlib import Path
from types import SimpleNamespace

import advantages_ref as adv
import closed_loop_ref as cl
import numpy as np
import spawn_server
from advantages_ref import SHAPES  # noqa: F401  (n, global offset, lanes per set, n_sets)
from closed_loop_ref import COPIES, DIMS, bits  # noqa: F401  (re-exported to the test files)

SENTINEL = adv.SENTINEL
HIDDEN = (0, 1, 5, 64)  # affine; 1 and 5: a chunk of the hidden layer with a remainder; 64: the widest
STEPS = (1, 2, 7)
LOG2E = float(np.float32(1.4426950408889634))
SCALES = (LOG2E, float(np.float32(LOG2E / 8.0)))  # temperature 1 and 8
BIG = np.float32(3.0e10)  # a coefficient that takes a lane's sums past 2^30

_lib = None
_dir = None


def lib():
    global _lib, _dir
    if _lib is None:
        _dir = tempfile.TemporaryDirectory(prefix="gradient_ref")  # removed when the interpreter exits
        out = Path(_dir.name) / "libgradient_ref.so"
        src = Path(__file__).resolve().parent / "cpp" / "gradient_ref.c"
        spawn_server.run(["gcc", "-O2", "-ffp-contract=off", "-shared", "-fPIC", str(src), "-o", str(out), "-lm"], check=True)
        _lib = C.CDLL(str(out))
        _lib.gradient_ref_lane.restype = None
        _lib.gradient_ref_lane.argtypes = [C.c_int, C.c_int, C.c_uint32, C.c_int, C.c_float, C.c_void_p, C.c_uint32] + [C.c_void_p] * 6
        _lib.gradient_ref.restype = None
        _lib.gradient_ref.argtypes = [C.c_int, C.c_int, C.c_uint32, C.c_int, C.c_float, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32] + \
            [C.c_void_p] * 8
    return _lib


def size_of(kind, hidden, critic):
    return adv.critic_size(kind, hidden) if critic else cl.size_of(kind, hidden)


def outputs_of(kind, critic):
    return 1 if critic else DIMS[kind][1]


def make_sets(kind, hidden, critic, n_sets, seed):
    return adv.make_critics(kind, hidden, n_sets, seed) if critic else cl.make_weights(kind, hidden, n_sets, seed)


def lane(kind, hidden, critic, scale, w, x, actions, coef, prob=False):
    """(q [S] int64, excluded, prob [K] or None) of ONE lane under ONE set, by the C reference"""
    w, x, coef = (np.ascontiguousarray(a, np.float32) for a in (w, x, coef))
    k = coef.size
    a = np.ascontiguousarray(actions if actions is not None else np.zeros(k), np.uint8)
    assert w.size == size_of(kind, hidden, critic) and x.size == k * DIMS[kind][0] and a.size == k
    q = np.zeros(w.size, np.int64)
    ex = C.c_uint64()
    pr = np.zeros(k, np.float32) if prob else None
    lib().gradient_ref_lane(DIMS[kind][0], outputs_of(kind, critic), hidden, int(critic), scale, w.ctypes.data, k, x.ctypes.data, a.ctypes.data,
                            coef.ctypes.data, q.ctypes.data, C.addressof(ex), pr.ctypes.data if prob else None)
    return q, ex.value, pr


def reference(c, lanes=None, grad=None, excluded=None, prob=False):
    """(grad [n_sets][S] int64, excluded [n_sets] uint64, prob [K][n] f32 or None) of the case by the C reference, over the lanes
    `lanes` (a slice; default all), ADDED to grad / excluded when given"""
    sl = lanes if lanes is not None else slice(0, c.n)
    lo, hi = sl.start, sl.stop
    n = hi - lo
    obs, start, coef = (np.ascontiguousarray(a[..., lo:hi], np.float32) for a in (c.obs, c.start_obs, c.coef))
    actions = np.ascontiguousarray(c.actions[:, lo:hi], np.uint8)
    w = np.ascontiguousarray(c.weights, np.float32)
    s = size_of(c.kind, c.hidden, c.critic)
    grad = np.zeros((c.n_sets, s), np.int64) if grad is None else grad
    excluded = np.zeros(c.n_sets, np.uint64) if excluded is None else excluded
    pr = np.zeros((c.steps, n), np.float32) if prob else None
    lib().gradient_ref(DIMS[c.kind][0], outputs_of(c.kind, c.critic), c.hidden, int(c.critic), c.scale, c.n_sets, c.lanes_per_set, c.gid0 + lo, n,
                       c.steps, w.ctypes.data, obs.ctypes.data, start.ctypes.data, actions.ctypes.data, coef.ctypes.data, grad.ctypes.data,
                       excluded.ctypes.data, pr.ctypes.data if prob else None)
    return grad, excluded, pr


def set_index(c):
    return np.array([((c.gid0 + i) // c.lanes_per_set) % c.n_sets for i in range(c.n)], np.int64)  # python ints: ids go beyond 2^32


def inputs_of(c, i):
    """x [K][D], actions [K], coef [K] of lane i"""
    x = np.concatenate([c.start_obs[None, :, i], c.obs[:c.steps - 1, :, i]]).astype(np.float32)
    return x, c.actions[:, i], c.coef[:, i]


def synthetic(kind, shape, steps, hidden, critic, seed=1, specials=True):
    """A record of `steps` rows over the lanes of SHAPES[shape]: normal observations and coefficients, actions uniform over the A
    actions.  With `specials` (and at least 64 lanes) four lanes are planted, listed in c.planted: one with an infinite observation,
    one with a NaN coefficient, one whose coefficients take its sums past 2^30, and one whose every action is out of range (A or
    200) AND whose observations are infinite: it must add nothing and count nothing.  About one other lane-step in fifty has an
    out-of-range action too."""
    n, gid0, lps, n_sets = SHAPES[shape]
    d, a = DIMS[kind]
    rng = np.random.default_rng([seed, kind, shape, steps, hidden, int(critic)])
    obs = rng.standard_normal((steps, d, n)).astype(np.float32)
    start_obs = rng.standard_normal((d, n)).astype(np.float32)
    coef = rng.standard_normal((steps, n)).astype(np.float32)
    actions = rng.integers(0, a, (steps, n)).astype(np.uint8)
    planted = {}
    if specials:
        bad = rng.random((steps, n)) < 0.02
        actions[bad] = np.where(rng.random(int(bad.sum())) < 0.5, a, 200).astype(np.uint8)
        if n >= 64:
            i_inf, i_nan, i_big, i_off = (int(v) for v in rng.choice(np.arange(1, n - 1), 4, replace=False))
            start_obs[0, i_inf] = np.inf
            actions[0, i_inf] = 0
            coef[steps - 1, i_nan] = np.nan
            actions[steps - 1, i_nan] = 1
            coef[:, i_big] = BIG
            actions[:, i_big] = 0
            start_obs[:, i_off] = np.inf
            obs[:, :, i_off] = -np.inf
            actions[:, i_off] = np.where(np.arange(steps) % 2 == 0, a, 200).astype(np.uint8)
            planted = dict(inf=i_inf, nan=i_nan, big=i_big, off=i_off)
    c = SimpleNamespace(kind=kind, shape=shape, n=n, gid0=gid0, lanes_per_set=lps, n_sets=n_sets, steps=steps, hidden=hidden, critic=critic,
                        scale=SCALES[(shape + kind) % 2], obs=obs, start_obs=start_obs, coef=coef, actions=actions, planted=planted,
                        weights=make_sets(kind, hidden, critic, n_sets, 200 + 10 * kind + hidden + int(critic)),
                        classes=cl.wave_classes(n, 4, gid0, n_sets, lps))
    return c


def matrix():
    """[(kind, shape, hidden)]: both envs x every shape x every hidden width; every entry is run with both heads and every K"""
    return [(kind, shape, hidden) for kind in (0, 1) for shape in range(len(SHAPES)) for hidden in HIDDEN]


# ---- the f64 restatement: calculus, not the rule ------------------------------------------------------------------------------------
def reference64(c):
    """(G [n_sets][S], B [n_sets][S], zmin): the gradient in f64 with an exact softmax at temperature 1 / beta (beta = scale * ln 2 as
    the rule rounds it), B = the sum of the magnitudes the error bound is stated in, zmin = the smallest |z| of a hidden unit met
    (a unit that close to its kink has no derivative to compare with).  Lane-steps with an action out of range add nothing."""
    d, a = DIMS[c.kind][0], outputs_of(c.kind, c.critic)
    h, s = c.hidden, size_of(c.kind, c.hidden, c.critic)
    beta = float(np.float32(c.scale) * np.float32(float.fromhex("0x1.62e430p-1"))) if not c.critic else 1.0
    grad, bound = np.zeros((c.n_sets, s)), np.zeros((c.n_sets, s))
    idx = set_index(c)
    zmin = np.inf
    for i in range(c.n):
        w = np.asarray(c.weights[idx[i]], np.float64)
        x_all, act, coef = inputs_of(c, i)
        for k in range(c.steps):
            x, cf = x_all[k].astype(np.float64), float(coef[k])
            if not c.critic and act[k] >= a:
                continue
            if h == 0:
                y = w[a * d:] + w[:a * d].reshape(a, d) @ x
            else:
                w1, b1 = w[:h * d].reshape(h, d), w[h * d:h * d + h]
                w2, b2 = w[h * d + h:h * d + h + a * h].reshape(a, h), w[h * d + h + a * h:]
                z = b1 + w1 @ x
                zmin = min(zmin, np.abs(z).min())
                r = np.where(z > 0, z, 0.0)
                y = b2 + w2 @ r
            if c.critic:
                g = np.array([cf])
            else:
                e = np.exp((y - y.max()) * beta)
                g = cf * beta * ((np.arange(a) == act[k]) - e / e.sum())
            m = abs(cf * beta)
            if h == 0:
                grad[idx[i]] += np.concatenate([np.outer(g, x).ravel(), g])
                bound[idx[i]] += np.concatenate([np.tile(m * np.abs(x), a), np.full(a, m)])
            else:
                dz = np.where(z > 0, w2.T @ g, 0.0)
                mz = m * np.abs(w2).sum(axis=0)
                grad[idx[i]] += np.concatenate([np.outer(dz, x).ravel(), dz, np.outer(g, r).ravel(), g])
                bound[idx[i]] += np.concatenate([np.outer(mz, np.abs(x)).ravel(), mz, np.tile(m * np.abs(r), a), np.full(a, m)])
    return grad, bound, zmin
