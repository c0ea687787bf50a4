"""gymrs_advantages computed on the CPU alone (include/gymrs_amd.h, "advantages").

The rule is restated in tests/cpp/advantages_ref.c from the header's text (plain C, libm's fmaf, gcc -O2 -ffp-contract=off) and once
more here in f64 numpy (the accuracy yardstick of tests/test_advantages_ref.py).  The synthetic records are built in numpy, so the
kernel is tested independently of the rollout kernels.  This module never imports the library: what it returns is the yardstick of
tests/test_gpu_advantages.py, and tests/test_advantages_ref.py shows without a GPU that its cases are worth comparing with.

A plain module like transitions_ref.py, imported by test files; no fixtures, no pytest hooks."""
import ctypes as C
import tempfile
from pathlib import Path
from types import SimpleNamespace

import closed_loop_ref as cl
import numpy as np
import spawn_server
from closed_loop_ref import COPIES, DIMS, bits  # noqa: F401  (re-exported to the test files)

SENTINEL = 0x7FC0BEEF  # transitions_ref.SENTINEL: the NaN bit pattern unwritten buffers are pre-filled with
HIDDEN = (0, 7, 8)  # affine; one trip of the uniform copy's four-unit loop plus a remainder of three; two trips
STEPS = (1, 2, 17)
GAMMA_LAMBDA = ((1.0, 1.0), (0.97, 0.9), (0.5, 0.0), (0.0, 1.0))
# (n, global offset, lanes_per_critic, n_critics).  The two 4-lane shapes of closed_loop_ref.SHAPES reach all four kernel copies
# between them; 257 lanes are one full wave and a ragged wave of one lane; the last has lanes_per_critic = 1 (every wave gathers).
SHAPES = [(1, 0, 1, 1), (5, 12345, 2, 3), (257, 3, 100, 3), (cl.SHAPES[0][0], cl.SHAPES[0][2], cl.SHAPES[0][3], 3),
          (cl.SHAPES[1][0], cl.SHAPES[1][2], cl.SHAPES[1][3], 3), (300, 5, 1, 3)]
P_DONE, P_TRUNC = 0.10, 0.10
# Seed of `synthetic` per (kind, shape, K): 1 unless an entry here replaces it -- the next seed, searched with this module alone, for
# which worth_comparing holds (tests/test_advantages_ref.py asserts it).
SEEDS = {(1, 2, 1): 2, (0, 3, 2): 2, (1, 3, 1): 2}

_lib = None
_dir = None


def lib():
    global _lib, _dir
    if _lib is None:
        _dir = tempfile.TemporaryDirectory(prefix="advantages_ref")  # removed when the interpreter exits
        out = Path(_dir.name) / "libadvantages_ref.so"
        src = Path(__file__).resolve().parent / "cpp" / "advantages_ref.c"
        spawn_server.run(["gcc", "-O2", "-ffp-contract=off", "-shared", "-fPIC", str(src), "-o", str(out), "-lm"], check=True)
        _lib = C.CDLL(str(out))
        _lib.advantages_ref_critic.restype = C.c_float
        _lib.advantages_ref_critic.argtypes = [C.c_int, C.c_uint32, C.c_void_p, C.c_void_p]
        _lib.advantages_ref_values.restype = None
        _lib.advantages_ref_values.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.advantages_ref.restype = None
        _lib.advantages_ref.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32] + [C.c_void_p] * 7 + \
            [C.c_float, C.c_float] + [C.c_void_p] * 3
    return _lib


def critic_size(kind, hidden):
    d = DIMS[kind][0]
    return d + 1 if hidden == 0 else hidden * (d + 2) + 1


def make_critics(kind, hidden, n_critics, seed):
    """seeded normals, f32, scaled as closed_loop_ref.make_weights scales a policy"""
    d = DIMS[kind][0]
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n_critics):
        if hidden == 0:
            parts = [rng.standard_normal(d), rng.standard_normal(1)]
        else:
            parts = [rng.standard_normal(hidden * d) / np.sqrt(d), rng.standard_normal(hidden) / np.sqrt(d),
                     rng.standard_normal(hidden) / np.sqrt(hidden), rng.standard_normal(1) / np.sqrt(hidden)]
        out.append(np.concatenate(parts).astype(np.float32))
    w = np.stack(out)
    assert w.shape == (n_critics, critic_size(kind, hidden))
    return w


def critic_value(kind, hidden, w, x):
    """V(x) under ONE critic, by the C reference"""
    w = np.ascontiguousarray(w, np.float32)
    x = np.ascontiguousarray(x, np.float32)
    assert w.size == critic_size(kind, hidden) and x.size == DIMS[kind][0]
    return np.float32(lib().advantages_ref_critic(DIMS[kind][0], hidden, w.ctypes.data, x.ctypes.data))


def values(c, x):
    """V of every column of x [D][n] under the case's critic set (zeros without a critic)"""
    x = np.ascontiguousarray(x, np.float32)
    v = np.empty(c.n, np.float32)
    w = np.ascontiguousarray(c.weights, np.float32) if c.critic else None
    lib().advantages_ref_values(DIMS[c.kind][0], c.hidden, c.n_critics, c.lanes_per_critic, c.gid0, c.n, w.ctypes.data if c.critic else None,
                                x.ctypes.data, v.ctypes.data)
    return v


def reference(c, obs=None, reward=None, done=None, truncated=None, final_obs=None, start_obs=None):
    """(advantages, returns, values), each [K][n] f32, of the case's record (or of the arrays given in its place) by the C reference"""
    pick = lambda given, own: own if given is None else given  # noqa: E731
    obs, reward, done = (np.ascontiguousarray(pick(a, b), t) for a, b, t in
                         ((obs, c.obs, np.float32), (reward, c.reward, np.float32), (done, c.done, np.uint8)))
    start_obs = np.ascontiguousarray(pick(start_obs, c.start_obs), np.float32)
    truncated = pick(truncated, c.truncated)
    final_obs = pick(final_obs, c.final_obs)
    truncated = None if truncated is None else np.ascontiguousarray(truncated, np.uint8)
    final_obs = None if final_obs is None else np.ascontiguousarray(final_obs, np.float32)
    k, d = c.steps, DIMS[c.kind][0]
    assert obs.shape == (k, d, c.n) and reward.shape == done.shape == (k, c.n) and start_obs.shape == (d, c.n)
    w = np.ascontiguousarray(c.weights, np.float32) if c.critic else None
    adv, ret, val = (np.empty((k, c.n), np.float32) for _ in range(3))
    lib().advantages_ref(d, c.hidden, c.n_critics, c.lanes_per_critic, c.gid0, c.n, k, w.ctypes.data if c.critic else None, obs.ctypes.data,
                         reward.ctypes.data, done.ctypes.data, truncated.ctypes.data if truncated is not None else None,
                         final_obs.ctypes.data if final_obs is not None else None, start_obs.ctypes.data, c.gamma, c.lam, adv.ctypes.data,
                         ret.ctypes.data, val.ctypes.data)
    return adv, ret, val


def critic_index(c):
    return np.array([((c.gid0 + i) // c.lanes_per_critic) % c.n_critics for i in range(c.n)], np.int64)  # python ints: ids go beyond 2^32


def values64(c, x):
    """The f64 restatement of the critic on the columns of x [D][n]"""
    if not c.critic:
        return np.zeros(c.n)
    d, h = DIMS[c.kind][0], c.hidden
    w = np.asarray(c.weights, np.float64)[critic_index(c)]
    x = np.asarray(x, np.float64)
    if h == 0:
        return w[:, d] + (w[:, :d] * x.T).sum(axis=1)
    w1, b1, w2, b2 = w[:, :h * d].reshape(c.n, h, d), w[:, h * d:h * d + h], w[:, h * d + h:h * d + 2 * h], w[:, -1]
    z = b1 + np.einsum("nhd,dn->nh", w1, x)
    return b2 + (w2 * np.where(z > 0, z, 0.0)).sum(axis=1)


def reference64(c):
    """(advantages, returns, values) in f64 by the same formulas, vectorised over the lanes"""
    k = c.steps
    gamma, gl = float(np.float32(c.gamma)), float(np.float32(c.gamma)) * float(np.float32(c.lam))
    adv, ret, val = (np.zeros((k, c.n)) for _ in range(3))
    nxt = np.zeros(c.n)
    for t in range(k - 1, -1, -1):
        done = c.done[t] != 0
        ended = done | ((c.truncated[t] != 0) if c.truncated is not None else False)
        v_obs = values64(c, c.obs[t])
        v_fin = values64(c, np.where(ended, c.final_obs[t], 0.0)) if c.final_obs is not None else v_obs
        v_next = np.where(done, 0.0, np.where(ended, v_fin, v_obs))
        v_cur = values64(c, c.start_obs if t == 0 else c.obs[t - 1])
        delta = gamma * v_next + c.reward[t] - v_cur
        adv[t] = gl * np.where(ended, 0.0, nxt) + delta
        ret[t] = adv[t] + v_cur
        val[t] = v_cur
        nxt = adv[t]
    return adv, ret, val


# ---- the synthetic cases of tests/test_gpu_advantages.py ------------------------------------------------------------------------------
def synthetic(kind, shape, steps, hidden, critic=True, final=True, trunc=True, gamma=0.97, lam=0.9, seed=None, specials=True):
    """A record of `steps` rows over the lanes of SHAPES[shape] with flags drawn at P_DONE / P_TRUNC per lane-step, independently (so
    both are set on about one step in a hundred).  CartPole pays 0 or 1, MountainCar -1.  final_obs holds normal draws on ended
    lane-steps and the NaN sentinel everywhere else (None without `final`); on truncated-only steps it is drawn again until the
    critic tells it from the recorded observation.  With `specials`, observations of steps that went on hold
    some NaN, +-inf and 1e30, and (with final_obs) the last row's observation of every done lane is NaN: by the rule none of the
    latter reaches an output."""
    n, gid0, lpc, n_critics = SHAPES[shape]
    d = DIMS[kind][0]
    seed = SEEDS.get((kind, shape, steps), 1) if seed is None else seed
    rng = np.random.default_rng([seed, kind, shape, steps])
    obs = rng.standard_normal((steps, d, n)).astype(np.float32)
    start_obs = rng.standard_normal((d, n)).astype(np.float32)
    done = (rng.random((steps, n)) < P_DONE).astype(np.uint8)
    truncated = (rng.random((steps, n)) < P_TRUNC).astype(np.uint8) if trunc else None
    ended = (done != 0) | ((truncated != 0) if trunc else False)
    reward = (rng.random((steps, n)) < 0.8).astype(np.float32) if kind == 0 else np.full((steps, n), -1.0, np.float32)
    final_obs = None
    if final:
        final_obs = np.full((steps, d, n), SENTINEL, np.uint32).view(np.float32)
        draws = rng.standard_normal((steps, d, n)).astype(np.float32)
        final_obs = np.where(ended[:, None, :], draws, final_obs)
    if specials:
        for value in (np.nan, np.inf, -np.inf, 1e30):
            at = (rng.random((steps, d, n)) < 0.004) & ~ended[:, None, :]
            obs[at] = np.float32(value)
        if final:
            obs[-1][:, done[-1] != 0] = np.nan
    c = SimpleNamespace(kind=kind, shape=shape, n=n, gid0=gid0, lanes_per_critic=lpc, n_critics=n_critics, steps=steps, hidden=hidden,
                        critic=critic, gamma=float(np.float32(gamma)), lam=float(np.float32(lam)), obs=obs, start_obs=start_obs, reward=reward,
                        done=done, truncated=truncated, final_obs=final_obs, ended=ended,
                        weights=make_critics(kind, hidden, n_critics, 100 + 10 * kind + hidden),
                        classes=cl.wave_classes(n, 4, gid0, n_critics if critic else 1, lpc))
    if critic and final and trunc:
        # a hidden layer whose units are all off gives b2 for any observation: where that makes V(final_obs) == V(obs) on a
        # truncated-only step, the step would not show which of the two the kernel read, so its final observation is drawn again
        for _ in range(50):
            again = np.zeros((steps, n), bool)
            for k in range(steps):
                only = (truncated[k] != 0) & (done[k] == 0)
                if only.any():
                    fin = np.where(only, final_obs[k], 0.0).astype(np.float32)
                    again[k] = (bits(values(c, fin)) == bits(values(c, obs[k]))) & only
            if not again.any():
                break
            final_obs[np.broadcast_to(again[:, None, :], final_obs.shape)] = rng.standard_normal((int(again.sum()) * d)).astype(np.float32)
    return c


def matrix():
    """[(kind, shape, K, hidden, critic, final, trunc, returns, values, (gamma, lambda))]: every shape with every K for both envs, the
    other axes taking turns (tests/test_advantages_ref.py asserts that each value of each meets both envs); then the two large shapes
    at K = 17 with every hidden width and everything switched on"""
    out = []
    for shape in range(len(SHAPES)):
        for kind in (0, 1):
            for ki, steps in enumerate(STEPS):
                i = len(out)
                out.append((kind, shape, steps, HIDDEN[(shape + kind + ki) % 3], (shape + 2 * kind + ki) % 4 != 0, (shape + kind + 2 * ki) % 3 != 1,
                            i % 5 != 4, (shape + ki) % 2 == 0, (shape + kind + ki // 2) % 2 == 0, GAMMA_LAMBDA[(shape + kind + ki) % 4]))
    for shape in (3, 4):
        for kind in (0, 1):
            for hidden in HIDDEN:
                out.append((kind, shape, 17, hidden, True, True, True, True, True, GAMMA_LAMBDA[(shape + kind + hidden) % 4]))
    return list(dict.fromkeys(out))


def coverage():
    """{(kind, critic): lanes per kernel copy (in COPIES order), summed over the matrix}: one entry per advantages_kernel.  With a
    critic no cell may be zero; without one every wave is uniform."""
    out = {}
    for kind, shape, steps, hidden, critic, *_ in matrix():
        n, gid0, lpc, n_critics = SHAPES[shape]
        row = out.setdefault((kind, critic), np.zeros(4, np.int64))
        row += np.bincount(cl.wave_classes(n, 4, gid0, n_critics if critic else 1, lpc), minlength=4)
    return out


def worth_comparing(c, per_copy=True):
    """What is missing for the case to show anything (empty: nothing), inside the lanes of every kernel copy present where `per_copy`:
    a step that is done only, one that is truncated only, one with both, a lane with two ends in the window, an end at k = 0, an end
    at k = K-1, a lane with no end; on every truncated-only step V(final_obs) and V(obs) differ in bits; critics of neighbouring
    blocks give different values.  A condition a shape cannot meet is not asked of it: two ends need K >= 2, the flag conditions need
    the truncated row, and a copy of fewer than 64 lanes (n = 1, n = 5, the one-lane ragged wave of n = 257) is asked for nothing
    but the value conditions -- a handful of lane-steps cannot hold seven kinds of lane at once."""
    missing = []
    done = c.done != 0
    trunc = (c.truncated != 0) if c.truncated is not None else np.zeros_like(done)
    ended = done | trunc
    groups = [(COPIES[k], c.classes == k) for k in np.unique(c.classes)] if per_copy else [("all", np.ones(c.n, bool))]
    for name, m in groups:
        if m.sum() < 64:
            continue
        want = [("done only", (done & ~trunc)[:, m].any()), ("an end at k = 0", ended[0, m].any()), ("an end at k = K-1", ended[-1, m].any()),
                ("a lane with no end", (~ended[:, m].any(axis=0)).any())]
        if c.truncated is not None:
            want += [("truncated only", (trunc & ~done)[:, m].any()), ("both flags", (trunc & done)[:, m].any())]
        if c.steps >= 2:
            want.append(("a lane with two ends", (ended[:, m].sum(axis=0) >= 2).any()))
        missing += [f"{name}: no {what}" for what, ok in want if not ok]
    if c.critic:
        if c.final_obs is not None:
            for k in range(c.steps):
                only = trunc[k] & ~done[k]
                if only.any():
                    fin = np.where(only, c.final_obs[k], 0.0).astype(np.float32)
                    same = (bits(values(c, fin)) == bits(values(c, c.obs[k]))) & only
                    if same.any():
                        missing.append(f"step {k}: V(final_obs) equals V(obs) on a truncated-only step")
        if c.n_critics > 1:
            idx = critic_index(c)
            v = values(c, c.start_obs)
            for i in np.flatnonzero(idx[1:] != idx[:-1])[:4] + 1:
                x = np.ascontiguousarray(c.start_obs[:, i])
                if bits(critic_value(c.kind, c.hidden, c.weights[idx[i - 1]], x)) == bits(v[i]):
                    missing.append(f"lane {i}: the critics of two neighbouring blocks agree")
    return missing
