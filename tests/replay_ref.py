"""Prioritized replay restated (include/gymrs_amd.h, "Replay"): the draw in Python integers over numpy Philox words, the priority
rule in f32 numpy from the log2 / 2^d restatements of entropy_ref.py, the flattening of a record into the ring with numpy indexing.
This module never imports the library.  A plain module imported by test files; no fixtures, no pytest hooks."""
import numpy as np
from entropy_ref import F32, log2, weight
from explore_ref import stream_word

NONE, MAX_P, TILE, STREAM = 0xFFFFFFFF, 1 << 24, 4096, 5


def priority(td, alpha, eps, cap):
    td, alpha, eps, cap = np.atleast_1d(np.asarray(td, F32)), F32(alpha), F32(eps), F32(cap)
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.abs(td) + eps
        v = np.where(~(v <= cap), cap, v).astype(F32)
        d = alpha * (log2(v) - log2(np.full_like(v, cap)))
        d = np.where(d > 0, F32(0.0), d).astype(F32)
        p = np.rint(weight(d) * F32(16777216.0)).astype(np.uint32)
    return np.maximum(p, 1).astype(np.uint32)


def strata(total, n_samples):
    """[(lo, width)] of the n_samples strata of [0, total)"""
    q, rem = divmod(total, n_samples)
    return [(j * q + min(j, rem), q + (j < rem)) for j in range(n_samples)]


def draw(prio, n_samples, seed, counter):
    """(idx uint32 [n_samples], total)"""
    prefix = np.cumsum(np.asarray(prio, np.uint64), dtype=np.uint64)
    total = int(prefix[-1])
    if total == 0:
        return np.full(n_samples, NONE, np.uint32), 0
    r = stream_word(seed, np.arange(n_samples, dtype=np.uint64), counter, STREAM)
    u = [min(lo + (int(rj) * w >> 32), total - 1) for (lo, w), rj in zip(strata(total, n_samples), r)]
    return np.searchsorted(prefix, np.array(u, np.uint64), side="right").astype(np.uint32), total


def patterns(count, seed=7):
    """name -> priorities [count]: what a tiled prefix sum can get wrong"""
    rng = np.random.default_rng([seed, count])
    out = {"ones": np.ones(count, np.uint32), "max": np.full(count, MAX_P, np.uint32), "zero": np.zeros(count, np.uint32),
           "random": rng.integers(0, MAX_P + 1, count).astype(np.uint32)}
    edges = np.ones(count, np.uint32)  # zeros on both sides of every tile boundary
    for b in range(TILE, count + TILE, TILE):
        edges[max(b - 2, 0):min(b + 2, count)] = 0
    out["edges"] = edges
    for name, at in (("last_of_tile0", min(TILE, count) - 1), ("first_of_tile1", TILE)):
        if at < count:
            out[name] = np.zeros(count, np.uint32)
            out[name][at] = MAX_P
    return out


def flatten(c, n, steps, head, capacity, store):
    """push of record c (arrays [K][..][n], start_obs [D][n]) into `store` (dict of arrays over capacity), in place"""
    ended = (c["done"] != 0) | (c["truncated"] != 0)
    for k in range(steps):
        at = (head + k * n + np.arange(n)) % capacity
        store["s"][:, at] = c["start_obs"] if k == 0 else c["obs"][k - 1]
        store["s_next"][:, at] = np.where(ended[k], c["final_obs"][k], c["obs"][k])
        store["action"][at], store["reward"][at], store["done"][at] = c["actions"][k], c["reward"][k], (c["done"][k] != 0)
        store["priority"][at] = c["priority"]
    return store
