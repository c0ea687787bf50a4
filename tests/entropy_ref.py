"""gymrs_entropy_gradient computed in numpy alone (include/gymrs_amd.h, "Entropy").

`lanes` restates the rule from the header's text in f32 numpy, operation by operation, for N lanes side by side (one fmaf with a single
rounding: optimizer_ref.fmaf); `reference64` is the calculus in f64: H = -sum p ln p with an exact softmax, its gradient by the chain
rule through the network, k3 with np.log.  This module never imports the library.

A plain module like gradient_ref.py, imported by test files; no fixtures, no pytest hooks."""
import numpy as np
from optimizer_ref import fmaf

F32, F64 = np.float32, np.float64
DIMS = {0: (4, 2), 1: (2, 3)}  # kind: (D, A)
LN2 = F32(float.fromhex("0x1.62e430p-1"))
LOG2E = float(F32(1.4426950408889634))
P = [F32(float.fromhex(h)) for h in ("0x1p+0", "0x1.62e430p-1", "0x1.ebfc40p-3", "0x1.c69f6ap-5", "0x1.3c4a8ap-7", "0x1.4ca4ccp-10", "0x1.b4d1e4p-13")]
Q = [F32(float.fromhex(h)) for h in ("0x1.715466p+0", "-0x1.714ef8p-1", "0x1.ebcb78p-2", "-0x1.6c7e8ep-2", "0x1.1255d2p-2", "-0x1.76f800p-3",
                                     "0x1.925438p-4", "-0x1.19ef3ap-5", "0x1.739d30p-8")]
LOG2_BOUND = 1.41e-7  # the header's figure for max |entropy_log2 - log2| over [1, 2)


def size_of(kind, hidden):
    d, a = DIMS[kind]
    return a * (d + 1) if hidden == 0 else hidden * (d + 1) + a * hidden + a


def make_weights(kind, hidden, n_sets, seed):
    d, a = DIMS[kind]
    rng = np.random.default_rng([seed, kind, hidden])
    return rng.standard_normal((n_sets, size_of(kind, hidden))).astype(F32) / F32(np.sqrt(max(hidden, d)))


def horner(coefs, t):
    acc = np.full_like(t, coefs[-1])
    for c in coefs[-2::-1]:
        acc = fmaf(acc, t, c)
    return acc


def log2(v):
    u = np.ascontiguousarray(v, F32).view(np.uint32)
    e = ((u >> 23) & 0xFF).astype(np.int32) - 127
    t = ((u & 0x007FFFFF) | 0x3F800000).view(F32) - F32(1.0)
    return e.astype(F32) + t * horner(Q, t)


def weight(d):
    ok = d >= F32(-126.0)  # false for a NaN
    ds = np.where(ok, d, F32(0.0))
    fl = np.floor(ds)
    return np.where(ok, np.ldexp(horner(P, ds - fl), fl.astype(np.int32)), F32(0.0)).astype(F32)


def forward(w, hidden, d, a, x):
    """(y [A] of [N], z [H], r [H]) under per-lane weights w [N][S]"""
    if hidden == 0:
        y = []
        for b in range(a):
            acc = w[:, a * d + b]
            for j in range(d):
                acc = fmaf(w[:, b * d + j], x[j], acc)
            y.append(acc)
        return y, [], []
    o_b1, o_w2 = hidden * d, hidden * d + hidden
    o_b2 = o_w2 + a * hidden
    y, zs, rs = [w[:, o_b2 + b] for b in range(a)], [], []
    for h in range(hidden):
        z = w[:, o_b1 + h]
        for j in range(d):
            z = fmaf(w[:, h * d + j], x[j], z)
        r = np.where(z > 0, z, F32(0.0))
        y = [fmaf(w[:, o_w2 + b * hidden + h], r, y[b]) for b in range(a)]
        zs.append(z)
        rs.append(r)
    return y, zs, rs


def lanes(kind, hidden, scale, coef, w, x, actions=None, old_prob=None):
    """The rule for N lanes: w [N][S] (every lane's own network), x [K][D][N], actions / old_prob [K][N] or None.
    Returns (q [N][S] int64, excluded [N], sums [N][2] int64, counts [N][2] uint64)."""
    d, a = DIMS[kind]
    w, x = np.ascontiguousarray(w, F32), np.ascontiguousarray(x, F32)
    k_steps, n = x.shape[0], x.shape[2]
    scale, coef = F32(scale), F32(coef)
    beta = scale * LN2
    ck = (coef * beta) * LN2
    acc = np.zeros((n, size_of(kind, hidden)), F32)
    s_h, s_kl = np.zeros(n, F32), np.zeros(n, F32)
    n_h, n_kl = np.zeros(n, np.uint64), np.zeros(n, np.uint64)

    def add(s, on, new):
        acc[:, s] = np.where(on, new, acc[:, s])

    with np.errstate(all="ignore"):
        for k in range(k_steps):
            xs = [x[k, j] for j in range(d)]
            y, zs, rs = forward(w, hidden, d, a, xs)
            greedy, m = np.zeros(n, np.int64), y[0]
            for b in range(1, a):
                up = y[b] > m
                m, greedy = np.where(up, y[b], m), np.where(up, b, greedy)
            dd = [(y[b] - m) * scale for b in range(a)]
            wt = [weight(v) for v in dd]
            total = wt[0]
            for b in range(1, a):
                total = total + wt[b]
            on = total > 0
            lt = log2(total)
            l = [dd[b] - lt for b in range(a)]
            p = [np.where(on, wt[b] / total, np.where(greedy == b, F32(1.0), F32(0.0))).astype(F32) for b in range(a)]
            t = [np.where(wt[b] > 0, p[b] * l[b], F32(0.0)) for b in range(a)]
            tot = t[0]
            for b in range(1, a):
                tot = tot + t[b]
            h2 = -tot
            hn = h2 * LN2
            g = [-(ck * np.where(wt[b] > 0, p[b] * (l[b] + h2), F32(0.0))) for b in range(a)]
            s_h = np.where(on, s_h + hn, s_h)
            n_h += on.astype(np.uint64)
            if old_prob is not None:
                act = actions[k]
                pa = np.zeros(n, F32)
                for b in range(a):
                    pa = np.where(act == b, p[b], pa)
                ratio = pa / old_prob[k].astype(F32)
                ok = (ratio >= F32(2.0**-126)) & (ratio <= np.finfo(F32).max)
                kl = (ratio - F32(1.0)) - log2(ratio) * LN2
                take = on & (act < a) & ok
                s_kl = np.where(take, s_kl + kl, s_kl)
                n_kl += take.astype(np.uint64)
            if hidden == 0:
                for b in range(a):
                    for j in range(d):
                        add(b * d + j, on, fmaf(g[b], xs[j], acc[:, b * d + j]))
                    add(a * d + b, on, acc[:, a * d + b] + g[b])
            else:
                o_b1, o_w2 = hidden * d, hidden * d + hidden
                o_b2 = o_w2 + a * hidden
                for b in range(a):
                    add(o_b2 + b, on, acc[:, o_b2 + b] + g[b])
                for h in range(hidden):
                    for b in range(a):
                        add(o_w2 + b * hidden + h, on, fmaf(g[b], rs[h], acc[:, o_w2 + b * hidden + h]))
                    e = g[0] * w[:, o_w2 + h]
                    for b in range(1, a):
                        e = fmaf(g[b], w[:, o_w2 + b * hidden + h], e)
                    dz = np.where(zs[h] > 0, e, F32(0.0))
                    add(o_b1 + h, on, acc[:, o_b1 + h] + dz)
                    for j in range(d):
                        add(h * d + j, on, fmaf(dz, xs[j], acc[:, h * d + j]))

        def fixed(v):
            ok = np.abs(v) < F32(2.0**30)  # false for NaN and the infinities
            return np.rint(np.where(ok, v, 0).astype(F64) * 16777216.0).astype(np.int64), ~ok

        q, bad = fixed(acc)
        (qh, bad_h), (qk, bad_k) = fixed(s_h), fixed(s_kl)
    excluded = bad.sum(axis=1) + bad_h + bad_k
    return q, excluded.astype(np.uint64), np.stack([qh, qk], axis=1), np.stack([n_h, n_kl], axis=1)


def reference64(kind, hidden, scale, coef, w, x, actions=None, old_prob=None):
    """ONE lane in f64: (G [S] the gradient of coef * sum Hn, B [S] the magnitudes the error bound is stated in -- gradient_ref's with
    |coef * beta| as the coefficient --, sum of Hn, sum of k3, zmin = the smallest |z| of a hidden unit met)."""
    d, a = DIMS[kind]
    w, x = np.asarray(w, F64), np.asarray(x, F64)
    beta = float(F32(scale) * LN2)
    grad, bound = np.zeros(w.size), np.zeros(w.size)
    ent = kl = 0.0
    zmin = np.inf
    m = abs(coef * beta)
    for k in range(x.shape[0]):
        xk = x[k]
        if hidden == 0:
            y = w[a * d:] + w[:a * d].reshape(a, d) @ xk
        else:
            h = hidden
            w1, b1 = w[:h * d].reshape(h, d), w[h * d:h * d + h]
            w2, b2 = w[h * d + h:h * d + h + a * h].reshape(a, h), w[h * d + h + a * h:]
            z = b1 + w1 @ xk
            zmin = min(zmin, np.abs(z).min())
            r = np.where(z > 0, z, 0.0)
            y = b2 + w2 @ r
        e = np.exp((y - y.max()) * beta)
        p = e / e.sum()
        hk = -(p * np.log(p)).sum()
        ent += hk
        g = -coef * beta * p * (np.log(p) + hk)
        if old_prob is not None:
            ratio = p[actions[k]] / float(old_prob[k])
            kl += (ratio - 1.0) - np.log(ratio)
        if hidden == 0:
            grad += np.concatenate([np.outer(g, xk).ravel(), g])
            bound += np.concatenate([np.tile(m * np.abs(xk), a), np.full(a, m)])
        else:
            dz = np.where(z > 0, w2.T @ g, 0.0)
            mz = m * np.abs(w2).sum(axis=0)
            grad += np.concatenate([np.outer(dz, xk).ravel(), dz, np.outer(g, r).ravel(), g])
            bound += np.concatenate([np.outer(mz, np.abs(xk)).ravel(), mz, np.tile(m * np.abs(r), a), np.full(a, m)])
    return grad, bound, ent, kl, zmin
