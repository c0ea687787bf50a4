"""gymrs_q_gradient restated as calculus in f64 numpy (include/gymrs_amd.h, "Q-learning"): exact max, exact clamp, the gradient of
sum huber_kappa(delta) per lane and parameter, with a running error bound carried alongside.  This module never imports the library:
what it returns is the yardstick of tests/test_q_lane.py and tests/test_gpu_q_gradient.py.

The bound.  An f32 chain of m fused multiply-adds errs by at most m * 2^-24 * sum|terms|.  `e` below carries m * sum|terms| (without
the 2^-24), propagated to first order: logits (a hidden unit's error passes the 1-Lipschitz ReLU and is weighted by |W2|) -> target =
fma(gamma, boot, r) -> delta = q_a - target (its own rounding: |delta|).  The clamp is 1-Lipschitz, so d errs by no more than delta.
Into the table: bound = sum over k of (|d| + e(delta)) * |dQ/dtheta|.  A comparison uses (K + 16) * 2^-22 * bound + n * 2^-25, the form
of tests/test_gradient_ref.py: 2^-22 = four times the unit roundoff covers e, K + 16 the K accumulations of a sum, and the last term
the fixed-point rounding of n lanes.  td is compared within 2^-22 * e(delta).

The argmax, the ReLU's kink and the clamp's corners are not continuous (not differentiable): a lane-step within the bound of one would
differ legitimately.  reference() asserts that a case has none; a case that fails takes its next seed from SEEDS.

A plain module, imported by test files; no fixtures, no pytest hooks."""
from types import SimpleNamespace

import numpy as np

DIMS = {0: (4, 2), 1: (2, 3)}  # kind -> (D, A)
DOUBLE = 1
SENTINEL = 0x7FC0BEEF  # a NaN: the bytes of final_obs no step wrote
BIG = np.float32(3.0e10)  # a reward that takes a lane's sums past 2^30 (unclamped)
SHAPES = ((1, 0, 1, 1), (5, 12345, 2, 3), (257, 0, 1 << 20, 1), (300, 7, 1, 7), (64, 0, 64, 1))  # n, global offset, lanes per set, n_sets
# (kind, shape, steps, hidden, flags): the first seed whose case is tie-free, where that is not 1 (the cases of
# tests/test_gpu_q_gradient.py; seed 1 met an argmax tie or a clamp corner at H = 64, once at H = 5)
SEEDS = {(0, 2, 7, 64, 0): 2, (0, 3, 7, 5, 0): 2, (0, 3, 7, 64, 0): 3, (1, 2, 2, 64, 0): 3, (1, 2, 1, 64, 1): 2, (1, 2, 7, 64, 1): 2, (1, 3, 7, 64, 0): 2}


def size_of(kind, hidden):
    d, a = DIMS[kind]
    return a * (d + 1) if hidden == 0 else hidden * (d + 1) + a * (hidden + 1)


def set_index(c):
    return np.array([((c.gid0 + i) // c.lanes_per_set) % c.n_sets for i in range(c.n)], np.int64)


def synthetic(kind, shape, steps, hidden, flags, gamma, kappa):
    """Normal observations, rewards and weights; about 10 % done and 10 % truncated (some both); final_obs holds the sentinel except on
    ended lane-steps; about 2 % of the actions out of range; with at least 64 lanes one lane each with an infinite observation, a NaN
    reward and rewards that take |delta| sums past 2^30 (c.planted)."""
    n, gid0, lps, n_sets = SHAPES[shape]
    d, a = DIMS[kind]
    rng = np.random.default_rng([SEEDS.get((kind, shape, steps, hidden, flags), 1), kind, shape, steps, hidden, flags])
    f32 = lambda *s: rng.standard_normal(s).astype(np.float32)  # noqa: E731
    obs, start_obs, reward = f32(steps, d, n), f32(d, n), f32(steps, n)
    done, truncated = ((rng.random((steps, n)) < 0.1).astype(np.uint8) for _ in range(2))
    ended = (done | truncated) != 0
    final_obs = np.full((steps, d, n), SENTINEL, np.uint32).view(np.float32)
    final_obs[np.broadcast_to(ended[:, None, :], final_obs.shape)] = f32(int(ended.sum()) * d)
    actions = rng.integers(0, a, (steps, n)).astype(np.uint8)
    bad = rng.random((steps, n)) < 0.02
    actions[bad] = np.where(rng.random(int(bad.sum())) < 0.5, a, 200).astype(np.uint8)
    planted = {}
    if n >= 64:
        i_inf, i_nan, i_big = (int(v) for v in rng.choice(np.arange(1, n - 1), 3, replace=False))
        start_obs[0, i_inf] = np.inf
        reward[steps - 1, i_nan] = np.nan
        reward[:, i_big] = BIG
        actions[0, i_inf], actions[steps - 1, i_nan], actions[:, i_big] = 0, 1, 0
        planted = dict(inf=i_inf, nan=i_nan, big=i_big)
    s = size_of(kind, hidden)
    return SimpleNamespace(kind=kind, shape=shape, n=n, gid0=gid0, lanes_per_set=lps, n_sets=n_sets, steps=steps, hidden=hidden, flags=flags,
                           gamma=float(np.float32(gamma)), kappa=float(np.float32(kappa)), obs=obs, start_obs=start_obs, final_obs=final_obs,
                           reward=reward, done=done, truncated=truncated, actions=actions, planted=planted, weights=f32(n_sets, s),
                           target=f32(n_sets, s))


def transitions(c):
    """x [K][D][n] the observation every step started from, x_next [K][D][n] the selected successor"""
    x = np.concatenate([c.start_obs[None], c.obs[:c.steps - 1]])
    ended = ((c.done | c.truncated) != 0)[:, None, :]
    return x, np.where(ended, c.final_obs, c.obs)


def _net(w, kind, h):
    d, a = DIMS[kind]
    n = len(w)
    if h == 0:
        return w[:, :a * d].reshape(n, a, d), w[:, a * d:]
    o = np.cumsum([h * d, h, a * h])
    return w[:, :o[0]].reshape(n, h, d), w[:, o[0]:o[1]], w[:, o[1]:o[2]].reshape(n, a, h), w[:, o[2]:]


def _logits(net, x):
    """(y [n][A], e [n][A], z [n][H] or None, r) of x [n][D]"""
    if len(net) == 2:
        w, b = net
        return b + np.einsum("nad,nd->na", w, x), x.shape[1] * (abs(b) + np.einsum("nad,nd->na", abs(w), abs(x))), None, None
    w1, b1, w2, b2 = net
    z = b1 + np.einsum("nhd,nd->nh", w1, x)
    ez = x.shape[1] * (abs(b1) + np.einsum("nhd,nd->nh", abs(w1), abs(x)))
    r = np.where(z > 0, z, 0.0)
    return b2 + np.einsum("nah,nh->na", w2, r), z.shape[1] * (abs(b2) + np.einsum("nah,nh->na", abs(w2), r)) + np.einsum("nah,nh->na", abs(w2), ez), z, r


def reference(c):
    """td [K][n], e [K][n] (its bound), on [K][n], cut [K][n], and per lane and parameter the f64 sum L [n][S] with its bound B [n][S].
    Lane-steps that are not finite are exempt from the tie checks: their pairs are excluded by the rule."""
    d, a = DIMS[c.kind]
    h, idx, rows = c.hidden, set_index(c), np.arange(c.n)
    online, target = (_net(np.asarray(w, np.float64)[idx], c.kind, h) for w in (c.weights, c.target))
    x_all, xn_all = (v.astype(np.float64) for v in transitions(c))
    shape = (c.steps, c.n)
    td, err, on, cut = np.zeros(shape), np.zeros(shape), np.zeros(shape, bool), np.zeros(shape, bool)
    L, B = np.zeros((c.n, size_of(c.kind, h))), np.zeros((c.n, size_of(c.kind, h)))
    with np.errstate(all="ignore"):
        for k in range(c.steps):
            x, xn = x_all[k].T, xn_all[k].T
            y, ey, z, r = _logits(online, x)
            yt, et, _, _ = _logits(target, xn)
            ysel, es = _logits(online, xn)[:2] if c.flags & DOUBLE else (yt, et)
            best = np.nanargmax(np.where(np.isnan(ysel), -np.inf, ysel), axis=1)
            dn = c.done[k] != 0
            v, ev = np.where(dn, 0.0, yt[rows, best]), np.where(dn, 0.0, et[rows, best])
            act = np.minimum(c.actions[k], a - 1)
            on[k] = c.actions[k] < a
            rew = c.reward[k].astype(np.float64)
            delta = y[rows, act] - (rew + c.gamma * v)
            e = abs(delta) + ey[rows, act] + abs(c.gamma * v) + abs(rew) + c.gamma * ev
            dd = np.clip(delta, -c.kappa, c.kappa)
            ok = on[k] & np.isfinite(delta) & np.isfinite(e)
            # none of what the calculus cannot decide: a tie of the two largest deciding logits, a clamp corner, a unit on its kink
            top = np.sort(ysel, axis=1)[:, -2:]
            assert not (ok & ~dn & (top[:, 1] - top[:, 0] <= 2.0**-22 * 2 * es.max(axis=1))).any(), ("argmax tie", k)
            assert not (ok & (abs(abs(delta) - c.kappa) <= 2.0**-22 * e)).any(), ("clamp corner", k)
            assert z is None or not (ok[:, None] & (abs(z) < 1e-6)).any(), ("ReLU kink", k)
            td[k], err[k], cut[k] = np.where(on[k], delta, 0.0), np.where(on[k], e, 0.0), on[k] & (abs(delta) > c.kappa)
            g = np.where(on[k][:, None] & (np.arange(a) == act[:, None]), dd[:, None], 0.0)  # [n][A]
            m = np.where(on[k][:, None] & (np.arange(a) == act[:, None]), (abs(dd) + e)[:, None], 0.0)
            if h == 0:
                parts = [(g[:, :, None] * x[:, None, :], m[:, :, None] * abs(x)[:, None, :]), (g, m)]
            else:
                w2 = online[2]
                live = z > 0  # a unit that is off adds exactly nothing, whatever the lane-step holds
                dz, mz = np.where(live, np.einsum("na,nah->nh", g, w2), 0.0), np.where(live, np.einsum("na,nah->nh", m, abs(w2)), 0.0)
                parts = [(dz[:, :, None] * x[:, None, :], mz[:, :, None] * abs(x)[:, None, :]), (dz, mz),
                         (g[:, :, None] * r[:, None, :], np.where(live[:, None, :], m[:, :, None] * r[:, None, :], 0.0)), (g, m)]
            keep = on[k][:, None]
            L += np.where(keep, np.concatenate([p[0].reshape(c.n, -1) for p in parts], axis=1), 0.0)
            B += np.where(keep, np.concatenate([p[1].reshape(c.n, -1) for p in parts], axis=1), 0.0)
    return SimpleNamespace(td=td, err=err, on=on, cut=cut, L=L, B=B)


def table(c, r):
    """(grad [n_sets][S] f64, bound [n_sets][S], excluded [n_sets], counts [n_sets][2]) from reference(c): a (lane, parameter) pair
    whose sum is not finite or not below 2^30 is excluded, as the rule has it"""
    idx = set_index(c)
    out = ~(np.abs(r.L) < 2.0**30)
    grad, bound = (np.zeros((c.n_sets, r.L.shape[1])) for _ in range(2))
    np.add.at(grad, idx, np.where(out, 0.0, r.L))
    np.add.at(bound, idx, np.where(out, 0.0, r.B))
    excluded, counts = np.zeros(c.n_sets, np.uint64), np.zeros((c.n_sets, 2), np.uint64)
    np.add.at(excluded, idx, out.sum(axis=1).astype(np.uint64))
    np.add.at(counts, idx, np.stack([r.on.sum(axis=0), r.cut.sum(axis=0)], axis=1).astype(np.uint64))
    return grad, bound, excluded, counts


def tolerance(c, bound):
    return (c.steps + 16) * 2.0**-22 * bound + c.n * 2.0**-25
