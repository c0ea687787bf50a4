"""The rules of include/gymrs_amd.h, "Value loss" and "Advantage normalisation", restated on the CPU: the value rule in numpy f32 (the
critic forward is advantages_ref's C reference, the backward pass and the fixed point of the table gradient_ref's), the
normalisation in Python integers.  This module never imports the library.  A plain module like gradient_ref.py."""
import math
from fractions import Fraction

import advantages_ref as adv
import gradient_ref as ref
import numpy as np
from closed_loop_ref import DIMS

F = np.float32


def fma32(a, b, c):
    """fmaf for finite f32 inputs: the exact rational a * b + c rounded once (to nearest even) to f32; NaN and inf as IEEE has them"""
    a, b, c = float(a), float(b), float(c)
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        return F(a * b + c)
    t = Fraction(a) * Fraction(b) + Fraction(c)
    lo = F(float(t))  # may be double-rounded: pick the nearer of lo and its neighbours exactly
    best = min((F(lo), np.nextafter(lo, F(-np.inf)), np.nextafter(lo, F(np.inf))),
               key=lambda v: (abs(Fraction(float(v)) - t), int(v.view(np.uint32)) & 1) if np.isfinite(v) else (Fraction(10) ** 60, 0))
    return F(best)


def fixed(L):
    """(q, ok) of gradient_fixed"""
    L = float(L)
    if not abs(L) < 2.0**30:  # false for NaN and the infinities
        return 0, False
    return int(np.rint(np.float64(L) * 16777216.0)), True


def coefficient(v, R, vo, clip):
    """(c, e1, es, cut) of one lane-step in f32; vo None: plain"""
    with np.errstate(all="ignore"):
        v, R = F(v), F(R)
        e1 = F(v - R)
        if vo is None:
            return e1, e1, e1, False
        vo, clip = F(vo), F(clip)
        dl = F(v - vo)
        hi, lo = bool(dl > clip), bool(dl < -clip)
        vc = F(vo + clip) if hi else (F(vo - clip) if lo else v)
        e2 = F(vc - R)
        cut = (hi or lo) and bool(F(e2 * e2) > F(e1 * e1))
        return (F(0.0) if cut else e1), e1, (e2 if cut else e1), cut


def lane(kind, hidden, w, x, returns, old_values=None, clip=0.0):
    """(q, excluded, sums, counts, values, c) of ONE lane under ONE critic, as gymrs_value_lane defines them"""
    k = len(returns)
    values = np.array([adv.critic_value(kind, hidden, w, x[j]) for j in range(k)], F)
    c, s0, s1, ncut = np.zeros(k, F), F(0.0), F(0.0), 0
    for j in range(k):
        c[j], e1, es, cut = coefficient(values[j], returns[j], None if old_values is None else old_values[j], clip)
        s0, s1, ncut = fma32(e1, e1, s0), fma32(es, es, s1), ncut + int(cut)
    q, excluded, _ = ref.lane(kind, hidden, True, 0.0, w, x, None, c)
    sums = []
    for s in (s0, s1):
        f, ok = fixed(s)
        sums.append(f)
        excluded += 0 if ok else 1
    return q, excluded, sums, [k, ncut], values, c


def forward64(kind, hidden, w, x):
    """V(x) in f64"""
    d, w, x = DIMS[kind][0], np.asarray(w, np.float64), np.asarray(x, np.float64)
    if hidden == 0:
        return w[d] + w[:d] @ x
    z = w[hidden * d:hidden * d + hidden] + w[:hidden * d].reshape(hidden, d) @ x
    return w[-1] + w[hidden * d + hidden:hidden * d + 2 * hidden] @ np.where(z > 0, z, 0.0)


def normalize(a, eps):
    """(out f32, (s1, n, s2, non_members, mean, inv)) of one set: the integers in Python, each f64 step one numpy f64 operation"""
    a = np.asarray(a, F)
    member = np.array([bool(np.isfinite(v)) and abs(float(v)) < 8192.0 for v in a], bool)
    s1 = sum(int(np.rint(np.float64(v) * 16777216.0)) for v in a[member])
    n = int(member.sum())
    mean = F(np.float64(s1) / (np.float64(n) * 16777216.0)) if n else F(0.0)
    s2 = 0
    for v in a[member]:
        dm = F(v - mean)
        s2 += int(np.rint(np.float64(F(dm * dm)) * 16777216.0))
    var = np.float64(s2) / 16777216.0 / np.float64(n - 1) if n >= 2 else np.float64(0.0)
    inv = F(np.float64(1.0) / (np.sqrt(var) + np.float64(F(eps))))
    with np.errstate(all="ignore"):
        out = ((a - mean).astype(F) * inv).astype(F)
    wrap = lambda v: v - (1 << 64) if v >= 1 << 63 else v  # noqa: E731  (s1 as the int64 the record holds)
    return out, (wrap(s1 % (1 << 64)), n, s2 % (1 << 64), len(a) - n, mean, inv)


def draw(kind, hidden, lanes, steps, seed):
    """critic-independent inputs of `lanes` lanes: x [K][D][lanes], and the two noise rows returns / old_values are made from once V
    is known: R = V + r_noise, vo = V + o_noise.  Every second lane-step has vo at least 0.3 away from V on the side opposite to R (a
    clip of 0.2 moves V away from R: cut), the others have vo half way towards R (clipped or not, never cut): nearly half are cut."""
    rng = np.random.default_rng([seed, kind, hidden, lanes, steps])
    d = DIMS[kind][0]
    x, rn, z = rng.standard_normal((steps, d, lanes)), rng.standard_normal((steps, lanes)), rng.standard_normal((steps, lanes))
    odd = (np.arange(steps * lanes).reshape(steps, lanes) % 2) == 1
    on = np.where(odd, -np.sign(rn) * (0.3 + np.abs(z)), 0.5 * rn)
    return x.astype(F), rn.astype(F), on.astype(F)
