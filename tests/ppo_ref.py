"""gymrs_ppo_gradient computed on the CPU alone (include/gymrs_amd.h, "clipped surrogate").

The rule is restated in tests/cpp/ppo_ref.c from the header's text (plain C, libm's fmaf, gcc -O2 -ffp-contract=off) and once more here
in f64 numpy (the calculus yardstick of tests/test_ppo_ref.py: the gradient of the clipped objective).  The cases are built on
gradient_ref.synthetic, which is imported and not modified: its coefficient row is the advantages row, and the old probabilities are
the reference's own new p[a] times a factor per lane-step.  This module never imports the library: what it returns is the yardstick
of tests/test_gpu_ppo.py.

A plain module like gradient_ref.py, imported by test files; no fixtures, no pytest hooks."""
import ctypes as C
import tempfile
from pathlib import Path
from types import SimpleNamespace  # noqa: F401  (re-exported to the test files)

import gradient_ref as gref
import numpy as np
import spawn_server
from gradient_ref import BIG, DIMS, HIDDEN, SENTINEL, SHAPES, STEPS, bits, inputs_of, set_index  # noqa: F401  (re-exported to the test files)

FACTORS = np.array([0.5, 0.9, 1.0, 1.1, 2.0], np.float32)  # old_prob = new p[a] * factor: ratios near 2, 1.11, 1, 0.91 and 0.5
PLAIN_BOUNDS = (float(np.float32(0.8)), float(np.float32(1.2)))  # shapes below 64 lanes, and cases that keep away from the boundary
# Seed of `synthetic` per (kind, shape, K, H): 1 unless an entry here replaces it -- the next seed, searched with this module alone,
# for which worth_comparing holds (tests/test_ppo_ref.py asserts it for every case of at least 64 lanes).  None was needed.
SEEDS = {}

_lib = None
_dir = None


def lib():
    global _lib, _dir
    if _lib is None:
        _dir = tempfile.TemporaryDirectory(prefix="ppo_ref")  # removed when the interpreter exits
        out = Path(_dir.name) / "libppo_ref.so"
        src = Path(__file__).resolve().parent / "cpp" / "ppo_ref.c"
        spawn_server.run(["gcc", "-O2", "-ffp-contract=off", "-shared", "-fPIC", str(src), "-o", str(out), "-lm"], check=True)
        _lib = C.CDLL(str(out))
        _lib.ppo_ref_lane.restype = None
        _lib.ppo_ref_lane.argtypes = [C.c_int, C.c_int, C.c_uint32, C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_uint32] + [C.c_void_p] * 9
        _lib.ppo_ref.restype = None
        _lib.ppo_ref.argtypes = [C.c_int, C.c_int, C.c_uint32, C.c_float, C.c_float, C.c_float, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64,
                                 C.c_uint32] + [C.c_void_p] * 11
    return _lib


def size_of(kind, hidden):
    return gref.size_of(kind, hidden, False)


def lane(kind, hidden, scale, low, high, w, x, actions, adv, old_prob):
    """(q [S] int64, excluded, counts [2] uint64, prob [K], coef [K]) of ONE lane under ONE policy, by the C reference"""
    w, x, adv, old_prob = (np.ascontiguousarray(a, np.float32) for a in (w, x, adv, old_prob))
    k = adv.size
    a = np.ascontiguousarray(actions, np.uint8)
    assert w.size == size_of(kind, hidden) and x.size == k * DIMS[kind][0] and a.size == k and old_prob.size == k
    q = np.zeros(w.size, np.int64)
    ex = C.c_uint64()
    counts = np.zeros(2, np.uint64)
    pr, cf = np.zeros(k, np.float32), np.zeros(k, np.float32)
    lib().ppo_ref_lane(DIMS[kind][0], DIMS[kind][1], hidden, scale, low, high, w.ctypes.data, k, x.ctypes.data, a.ctypes.data, adv.ctypes.data,
                       old_prob.ctypes.data, q.ctypes.data, C.addressof(ex), counts.ctypes.data, pr.ctypes.data, cf.ctypes.data)
    return q, ex.value, counts, pr, cf


def reference(c, lanes=None, grad=None, excluded=None, counts=None):
    """(grad [n_sets][S] int64, excluded [n_sets] uint64, counts [n_sets][2] uint64, prob [K][n] f32, coef [K][n] f32) of the case by
    the C reference, over the lanes `lanes` (a slice; default all), ADDED to grad / excluded / counts when given"""
    sl = lanes if lanes is not None else slice(0, c.n)
    lo, hi = sl.start, sl.stop
    n = hi - lo
    obs, start, adv, old = (np.ascontiguousarray(a[..., lo:hi], np.float32) for a in (c.obs, c.start_obs, c.advantages, c.old_prob))
    actions = np.ascontiguousarray(c.actions[:, lo:hi], np.uint8)
    w = np.ascontiguousarray(c.weights, np.float32)
    grad = np.zeros((c.n_sets, size_of(c.kind, c.hidden)), np.int64) if grad is None else grad
    excluded = np.zeros(c.n_sets, np.uint64) if excluded is None else excluded
    counts = np.zeros((c.n_sets, 2), np.uint64) if counts is None else counts
    pr, cf = np.zeros((c.steps, n), np.float32), np.zeros((c.steps, n), np.float32)
    lib().ppo_ref(DIMS[c.kind][0], DIMS[c.kind][1], c.hidden, c.scale, c.clip_low, c.clip_high, c.n_sets, c.lanes_per_set, c.gid0 + lo, n, c.steps,
                  w.ctypes.data, obs.ctypes.data, start.ctypes.data, actions.ctypes.data, adv.ctypes.data, old.ctypes.data, grad.ctypes.data,
                  excluded.ctypes.data, counts.ctypes.data, pr.ctypes.data, cf.ctypes.data)
    return grad, excluded, counts, pr, cf


def rule(c, pa):
    """(ratio, cut, coef, on) [K][n] of the case by the rule in numpy f32, from the new probabilities pa: one divide, the compares, a
    select, one multiply"""
    adv, old = c.advantages.astype(np.float32), c.old_prob.astype(np.float32)
    with np.errstate(all="ignore"):
        ratio = pa.astype(np.float32) / old
        cut = ((adv > 0) & (ratio > np.float32(c.clip_high))) | ((adv < 0) & (ratio < np.float32(c.clip_low)))
        coef = np.where(cut, np.float32(0.0), adv * ratio).astype(np.float32)
    on = c.actions < DIMS[c.kind][1]
    return ratio, cut & on, coef, on


def synthetic(kind, shape, steps, hidden, seed=None, specials=True, boundary=True):
    """gradient_ref.synthetic's policy-head case as a PPO case: c.advantages is its coefficient row, c.old_prob the reference's own new
    p[a] times a factor drawn from FACTORS per lane-step.  With `specials` and at least 64 lanes eight more lanes are planted on top of
    gradient_ref's (c.planted gains their names): old_prob of 0 (with a negative advantage: c is -inf), NaN, +inf and negative at step
    0; advantages of +0, -0 and NaN on every step; advantages of -BIG on every step (gradient_ref plants +BIG).  Bounds: with `boundary`
    and at least 64 lanes clip_high is the f32 ratio of one lane-step with adv > 0 and 1 < ratio < 1.5, clip_low that of one with
    adv < 0 and 0.75 < ratio < 1 (c.boundary lists the two (k, i)): the strict compare sits on the boundary.  Otherwise 0.8 / 1.2."""
    seed = SEEDS.get((kind, shape, steps, hidden), 1) if seed is None else seed
    c = gref.synthetic(kind, shape, steps, hidden, False, seed=seed, specials=specials)
    c.seed = seed
    c.advantages = c.coef
    a = DIMS[kind][1]
    rng = np.random.default_rng([seed, 77, kind, shape, steps, hidden])
    if specials and c.n >= 64:
        free = np.setdiff1d(np.arange(1, c.n - 1), list(c.planted.values()))
        names = ("po_zero", "po_nan", "po_inf", "po_neg", "adv_pzero", "adv_nzero", "adv_nan", "adv_nbig")
        lanes = dict(zip(names, (int(v) for v in rng.choice(free, len(names), replace=False))))
        for name in names:  # valid actions where the planted value is to be met
            i = lanes[name]
            c.actions[:, i] = np.arange(steps) % a
        c.advantages[0, lanes["po_zero"]] = -1.0
        c.advantages[:, lanes["adv_pzero"]] = 0.0
        c.advantages[:, lanes["adv_nzero"]] = -0.0
        c.advantages[:, lanes["adv_nan"]] = np.nan
        c.advantages[:, lanes["adv_nbig"]] = -BIG
        c.planted.update(lanes)
    _, _, pa = gref.reference(c, prob=True)  # the new p[a] (+0 where the action is out of range)
    factor = FACTORS[rng.integers(0, len(FACTORS), (steps, c.n))]
    c.old_prob = (pa * factor).astype(np.float32)
    if specials and c.n >= 64:
        c.old_prob[0, c.planted["po_zero"]] = 0.0
        c.old_prob[0, c.planted["po_nan"]] = np.nan
        c.old_prob[0, c.planted["po_inf"]] = np.inf
        c.old_prob[0, c.planted["po_neg"]] = -0.25
        c.old_prob[:, c.planted["adv_nbig"]] = pa[:, c.planted["adv_nbig"]]  # ratio 1: never cut, the sums pass 2^30
        c.old_prob[:, c.planted["big"]] = pa[:, c.planted["big"]]
    c.clip_low, c.clip_high = PLAIN_BOUNDS
    c.boundary = []
    if boundary and c.n >= 64:
        ratio, _, _, on = rule(c, pa)
        ok = on & np.isfinite(ratio) & np.isfinite(c.advantages)
        ok[:, list(c.planted.values())] = False
        high = np.argwhere(ok & (c.advantages > 0) & (ratio > 1.0) & (ratio < 1.5))
        low = np.argwhere(ok & (c.advantages < 0) & (ratio < 1.0) & (ratio > 0.75))
        if len(high) and len(low):
            kh, ih = (int(v) for v in high[rng.integers(len(high))])
            kl, il = (int(v) for v in low[rng.integers(len(low))])
            c.clip_high, c.clip_low = float(ratio[kh, ih]), float(ratio[kl, il])
            c.boundary = [(kh, ih), (kl, il)]
    return c


def matrix():
    """[(kind, shape, hidden)]: both envs x every shape x every hidden width; every entry is run with every K of STEPS"""
    return [(kind, shape, hidden) for kind in (0, 1) for shape in range(len(SHAPES)) for hidden in HIDDEN]


def worth_comparing(c):
    """What is missing for the case to show anything (empty: nothing), on the CPU reference alone: a lane-step cut high, one cut low,
    one that is not cut with a ratio other than 1, and the two boundary steps (ratio == the bound on the side the advantage pushes to),
    which the strict compares must not cut."""
    _, _, _, pa, coef = reference(c)
    ratio, cut, _, on = rule(c, pa)
    ok = on & np.isfinite(ratio) & np.isfinite(c.advantages)
    missing = []
    if not (cut & ok & (c.advantages > 0)).any():
        missing.append("cut high")
    if not (cut & ok & (c.advantages < 0)).any():
        missing.append("cut low")
    if not (~cut & ok & (ratio != 1.0) & (c.advantages != 0)).any():
        missing.append("uncut off 1")
    if len(c.boundary) != 2:
        missing.append("boundary")
    else:
        (kh, ih), (kl, il) = c.boundary
        if not (ratio[kh, ih] == np.float32(c.clip_high) and c.advantages[kh, ih] > 0 and not cut[kh, ih] and coef[kh, ih] != 0):
            missing.append("boundary high")
        if not (ratio[kl, il] == np.float32(c.clip_low) and c.advantages[kl, il] < 0 and not cut[kl, il] and coef[kl, il] != 0):
            missing.append("boundary low")
    if not (0.0 <= c.clip_low <= 1.0 <= c.clip_high < np.inf):
        missing.append("bounds in range")
    return missing


# ---- the f64 restatement: calculus, not the rule ------------------------------------------------------------------------------------
def reference64(c):
    """(G [n_sets][S], B [n_sets][S], zmin, margin): the gradient of  sum over k of min(ratio * adv, clip(ratio, low, high) * adv)  in
    f64 with an exact softmax at temperature 1 / beta: where the clipped term is the smaller one (and the ratio is strictly outside
    the range) the objective is constant and adds nothing; elsewhere it is ratio * adv, whose gradient is adv * ratio * grad log p[a].
    B = the sum of the magnitudes the error bound is stated in (gradient_ref.reference64's, with |adv * ratio| as the coefficient),
    zmin = the smallest |z| of a hidden unit met, margin = the smallest distance of an f64 ratio from either bound."""
    d, a = DIMS[c.kind]
    h, s = c.hidden, size_of(c.kind, c.hidden)
    beta = float(np.float32(c.scale) * np.float32(float.fromhex("0x1.62e430p-1")))
    grad, bound = np.zeros((c.n_sets, s)), np.zeros((c.n_sets, s))
    idx = set_index(c)
    zmin, margin = np.inf, np.inf
    for i in range(c.n):
        w = np.asarray(c.weights[idx[i]], np.float64)
        x_all, act, adv = inputs_of(c, i)
        for k in range(c.steps):
            x, ad, po = x_all[k].astype(np.float64), float(adv[k]), float(c.old_prob[k, i])
            if act[k] >= a:
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
            e = np.exp((y - y.max()) * beta)
            p = e / e.sum()
            ratio = p[act[k]] / po
            margin = min(margin, abs(ratio - c.clip_low), abs(ratio - c.clip_high))
            clipped = min(max(ratio, c.clip_low), c.clip_high)
            if clipped * ad < ratio * ad:  # the clipped term is the minimum: constant in theta
                continue
            cf = ad * ratio
            g = cf * beta * ((np.arange(a) == act[k]) - p)
            m = abs(cf * beta)
            if h == 0:
                grad[idx[i]] += np.concatenate([np.outer(g, x).ravel(), g])
                bound[idx[i]] += np.concatenate([np.tile(m * np.abs(x), a), np.full(a, m)])
            else:
                dz = np.where(z > 0, w2.T @ g, 0.0)
                mz = m * np.abs(w2).sum(axis=0)
                grad[idx[i]] += np.concatenate([np.outer(dz, x).ravel(), dz, np.outer(g, r).ravel(), g])
                bound[idx[i]] += np.concatenate([np.outer(mz, np.abs(x)).ravel(), mz, np.tile(m * np.abs(r), a), np.full(a, m)])
    return grad, bound, zmin, margin
