"""gymrs_apply_gradient restated in plain numpy (include/gymrs_amd.h, "Optimizer"): f32 arrays with the operations in the order of the
rule, f64 for the norm with the explicit 64-slot butterfly, one fmaf with a single rounding.  Every set is a row; the module knows
nothing of groups, waves or packing, and never imports the library.

fmaf.  a * b is exact in f64 (24 x 24 bits).  The f64 sum with c is rounded to ODD (the error of the addition, from TwoSum, decides
whether the sum was exact; an inexact even sum moves to its odd neighbour on the error's side), and rounding an odd-rounded f64 to
f32 equals rounding the exact value once (53 >= 2 * 24 + 2 bits).

A plain module, imported by test files; no fixtures, no pytest hooks."""
import numpy as np

SGD, ADAM = 0, 1
F32, F64 = np.float32, np.float64


def fmaf(a, b, c):
    p, c = np.asarray(a, F32).astype(F64) * np.asarray(b, F32).astype(F64), np.asarray(c, F32).astype(F64)
    with np.errstate(invalid="ignore", over="ignore"):
        s = p + c
        t = s - p
        err = (p - (s - t)) + (c - t)
        move = np.isfinite(s) & (err != 0) & ((s.view(np.int64) & 1) == 0)
        s = np.where(move, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
        return s.astype(F32)


def gradient(q, grad_scale):
    with np.errstate(over="ignore"):
        return (np.asarray(q, np.int64).astype(F64) * F64(F32(grad_scale))).astype(F32)


def norms(g):
    """(float)sqrt(slot[0]) per row of g [n_sets][S]: 64 slots filled in ascending s, then the butterfly 32, 16, .. 1"""
    sq = g.astype(F64) * g.astype(F64)
    slot = np.zeros((g.shape[0], 64), F64)
    with np.errstate(over="ignore", invalid="ignore"):
        for s0 in range(0, g.shape[1], 64):
            part = sq[:, s0:s0 + 64]
            slot[:, :part.shape[1]] = slot[:, :part.shape[1]] + part
        for mask in (32, 16, 8, 4, 2, 1):
            slot = slot + slot[:, np.arange(64) ^ mask]
        return np.sqrt(slot[:, 0]).astype(F32)


def apply(q, excluded, w, m, v, pw, target, *, kind, lr, grad_scale, beta1=0.9, beta2=0.999, eps=1e-8, max_norm=np.inf, tau=0.0,
          ascend=False, zero_grad=False):
    """One call.  q int64 [n_sets][S], excluded uint64 [n_sets], w / m / v / target f32 [n_sets][S], pw f32 [n_sets][2] (m, v, pw
    are ignored by SGD, target with tau == 0).  Returns dict(w, m, v, pw, target, grad, excluded, skipped, clipped): new arrays,
    `skipped` the number of sets left alone, `clipped` a bool per set (False where skipped)."""
    lr, beta1, beta2, eps, max_norm, tau, one = (F32(x) for x in (lr, beta1, beta2, eps, max_norm, tau, 1))
    w, m, v, pw, target = (np.array(a, F32) for a in (w, m, v, pw, target))
    skip = np.asarray(excluded) != 0
    with np.errstate(over="ignore", invalid="ignore", divide="ignore", under="ignore"):
        g = gradient(q, grad_scale)
        clipped = np.zeros(len(g), bool)
        if max_norm < np.inf:
            norm = norms(g)
            clipped = norm > max_norm
            cs = max_norm / norm
            g = np.where(clipped[:, None], g * cs[:, None], g)
        if kind == ADAM:
            p1, p2 = pw[:, 0] * beta1, pw[:, 1] * beta2
            c1, c2 = (one - p1)[:, None], (one - p2)[:, None]
            mo = fmaf(beta1, m, (one - beta1) * g)
            vo = fmaf(beta2, v, (one - beta2) * (g * g))
            step = lr * ((mo / c1) / (np.sqrt(vo / c2) + eps))
            pw_new = np.stack([p1, p2], axis=1)
        else:
            step, mo, vo, pw_new = lr * g, m, v, pw
        wn = w + step if ascend else w - step
        tn = fmaf(tau, wn - target, target) if tau > 0 else target
    keep = skip[:, None]
    out = dict(w=np.where(keep, w, wn), m=np.where(keep, m, mo), v=np.where(keep, v, vo), pw=np.where(keep, pw, pw_new),
               target=np.where(keep, target, tn), skipped=int(skip.sum()), clipped=clipped & ~skip)
    out["grad"] = np.zeros_like(q) if zero_grad else np.array(q)
    out["excluded"] = np.zeros_like(excluded) if zero_grad else np.array(excluded)
    assert all(out[k].dtype == F32 for k in ("w", "m", "v", "pw", "target")), "an operation left f32"
    return out
