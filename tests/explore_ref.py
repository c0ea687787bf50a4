"""An epsilon-greedy closed-loop rollout (include/gymrs_amd.h, "exploration") computed on the CPU alone.

The draw is restated here from the header's text: a Philox4x32-10 in numpy / Python integers (pinned by Random123's known answers
and by the oracle's draws in tests/test_explore_ref.py), the counter layout of the reset and action streams on stream 2, word
(g & 3) of block (g >> 2, tick), the low half against the threshold, the high half scaled to an action.  The loop is the one of
closed_loop_ref / closed_loop_table_ref -- lane_params_ref.TableReference (one f32 twin per row; a single row is an engine without
a table) stepped with the actions of closed_loop_ref.policy_ref (tests/cpp/policy_ref.c) -- with the action replaced per the
definition.  This module never imports the library: what it returns is the yardstick of tests/test_gpu_explore.py, and
tests/test_explore_ref.py shows without a GPU that its cases are worth comparing with.

A plain module like closed_loop_ref.py, imported by test files; no fixtures, no pytest hooks."""
from types import SimpleNamespace

import closed_loop_ref as cl
import lane_params_ref as lp
import numpy as np
import policy_fitness_ref as pf
from closed_loop_ref import A, COPIES, DIMS, F, FLAG_SETS, S, T, bits  # noqa: F401  (re-exported to the test files)

M32 = 0xFFFFFFFF
PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57  # Salmon et al., SC'11: the multipliers and the Weyl key increments
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
STREAM_RESET, STREAM_ACTION, STREAM_EXPLORE = 0, 1, 2
EXPLORE_ONE = 65536  # the threshold that explores on every step


def philox4x32_10(ctr, key):
    """Philox4x32-10 of the counter words ctr[0..4) and key words key[0..2): Python ints or integer arrays (broadcast against each
    other); returns four uint32 arrays of the broadcast shape."""
    c = [np.asarray(x, dtype=np.uint64) & np.uint64(M32) for x in ctr]
    k = [np.asarray(x, dtype=np.uint64) & np.uint64(M32) for x in key]
    shape = np.broadcast(*c, *k).shape
    c0, c1, c2, c3 = (np.broadcast_to(x, shape).copy() for x in c)
    k0, k1 = (np.broadcast_to(x, shape).copy() for x in k)
    mask, sh = np.uint64(M32), np.uint64(32)
    for _ in range(10):
        p0 = np.uint64(PHILOX_M0) * c0  # 32 x 32 -> 64 bits: no overflow in uint64
        p1 = np.uint64(PHILOX_M1) * c2
        c0, c1, c2, c3 = (p1 >> sh) ^ c1 ^ k0, p1 & mask, (p0 >> sh) ^ c3 ^ k1, p0 & mask
        k0 = (k0 + np.uint64(PHILOX_W0)) & mask
        k1 = (k1 + np.uint64(PHILOX_W1)) & mask
    return tuple(x.astype(np.uint32) for x in (c0, c1, c2, c3))


def as_u64(x):
    """A Python int (up to 2^64 - 1), a flat list of them, or an integer array -> a uint64 array"""
    if isinstance(x, np.ndarray):
        return x.astype(np.uint64)
    if isinstance(x, (list, tuple)):
        return np.array([int(v) for v in x], dtype=np.uint64)
    return np.array(int(x), dtype=np.uint64)


def draw4(seed, gid, tick, stream):
    """The block of (seed, gid, tick, stream): key = (seed lo, seed hi), counter = (gid lo, gid hi, tick lo, (tick hi & 0xffff) |
    stream << 16)"""
    seed, gid, tick = int(seed) & (2**64 - 1), as_u64(gid), as_u64(tick)
    sh = np.uint64(32)
    return philox4x32_10((gid, gid >> sh, tick, ((tick >> sh) & np.uint64(0xFFFF)) | np.uint64(stream << 16)), (seed & M32, seed >> 32))


def stream_word(seed, gid, tick, stream):
    """word (gid & 3) of block (gid >> 2, tick): how the action and exploration streams hand one block to four lanes"""
    gid = as_u64(gid)
    b = draw4(seed, gid >> np.uint64(2), tick, stream)
    j = np.broadcast_to((gid & np.uint64(3)).astype(np.int64), b[0].shape)
    return np.choose(j, b)


def draw(seed, threshold, n_actions, gid, tick):
    """(explored: bool array, random: uint8 array) of the step that takes lane `gid` (global id) from engine tick `tick` to
    tick + 1; gid and tick broadcast"""
    assert 0 <= threshold <= EXPLORE_ONE
    w = stream_word(seed, gid, tick, STREAM_EXPLORE).astype(np.uint64)
    explored = (w & np.uint64(0xFFFF)) < np.uint64(threshold)
    random = (((w >> np.uint64(16)) * np.uint64(n_actions)) >> np.uint64(16)).astype(np.uint8)
    return explored, random


def random_policy_actions(seed, n_actions, gid, t):
    """gymrs_fill_actions for a Discrete(n) env (stream 1): slot t >> 1, the 16-bit half (t & 1) of the word"""
    w = stream_word(seed, gid, int(t) >> 1, STREAM_ACTION).astype(np.uint64)
    half = (w >> np.uint64((int(t) & 1) * 16)) & np.uint64(0xFFFF)
    return ((half * np.uint64(n_actions)) >> np.uint64(16)).astype(np.uint8)


# ---- the cases of tests/test_gpu_explore.py (checked without a GPU by tests/test_explore_ref.py) ---------------------------------
N = 1300  # at 4 lanes per work-item five full waves and a ragged one of 20 lanes, at 8 two full waves and a ragged one of 276
OFFSETS = (0, 6, (1 << 32) + 4)  # aligned; the per-lane block path (a Philox block shared across work-items); beyond 2^32
POLICY_SETS = ((1, 1), (3, 512), (3, 1))  # (n_policies, lanes_per_policy): one policy; whole waves uniform; gathered
HIDDEN = (0, 8)
STEPS = 40
SPLITS = ((40,), (1, 7, 32))
THRESHOLD = 16384
SEED = 0xC0FFEE0123456789  # of the exploration stream
TABLE_ROWS = 3
MAX_EPISODE_STEPS = 17
RESET_SEED = 3
WEIGHTS_SEED = 5  # of closed_loop_ref.make_weights; tests/test_explore_ref.py shows that the cases it gives are worth comparing with


def axes(i):
    """The lighter axes are not crossed with (kind, flag set, table): case number i takes combination i of offset x policy set x
    hidden x split, 36 in all: -> (offset, (n_policies, lanes_per_policy), hidden, split)"""
    return OFFSETS[i % 3], POLICY_SETS[(i // 3) % 3], HIDDEN[(i // 9) % 2], SPLITS[(i // 18) % 2]


def matrix():
    """[(kind, flag set, table, case number)]: 2 envs x 10 flag sets x with / without a table"""
    out = []
    for kind in (0, 1):
        for flags in FLAG_SETS:
            for table in (False, True):
                out.append((kind, flags, table, len(out)))
    return out


def case(kind, flags, table, gid0=0, policy_set=(3, 512), hidden=0, schedule=SPLITS[0], n=N, threshold=THRESHOLD, seed=SEED, bounds=None):
    n_policies, lpp = policy_set
    k = TABLE_ROWS if table else 1
    rows = lp.make_rows(kind, k, lp.ROWS_SEED + kind, MAX_EPISODE_STEPS) if table else [lp.default_row(kind, MAX_EPISODE_STEPS)]
    index = lp.make_index(n, k, lp.INDEX_SEED + kind) if table else np.zeros(n, np.uint16)
    w = cl.make_weights(kind, hidden, n_policies, WEIGHTS_SEED)
    prepare = (lambda state: cl.mountain_car_prepare(state, 0)) if kind == 1 else None
    return SimpleNamespace(kind=kind, n=n, gid0=gid0, flags=flags, table=table, rows=rows, index=index, weights=w, hidden=hidden,
                           n_policies=n_policies, lanes_per_policy=lpp, reset_seed=RESET_SEED, schedule=tuple(schedule), prepare=prepare, bounds=bounds,
                           seed=seed, threshold=threshold, policies=pf.policies_of(n, gid0, lpp, n_policies),
                           classes={vec: cl.wave_classes(n, vec, gid0, n_policies, lpp) for vec in (4, 8)})


def matrix_case(kind, flags, table, i):
    gid0, policy_set, hidden, schedule = axes(i)
    return case(kind, flags, table, gid0, policy_set, hidden, schedule)


class Run:
    """The reference of a case, launch by launch.  launch(steps, explore) advances it -- explore = (seed, threshold): every step
    plays the epsilon-greedy action under these settings; None: the greedy action (a launch without GYMRS_CLOSED_LOOP_EXPLORE) -- and
    returns a SimpleNamespace of what an engine holds afterwards: state, obs, reward, done, truncated, final, stats, tick as the
    getters return them; rec_obs [steps][D][n], rec_actions (the action TAKEN), rec_reward, rec_done, rec_truncated [steps][n], the
    rows a recording launch keeps; fitness (n_policies, 4) int64, the records accumulated over the launches counted so far
    (`count=False` leaves a launch out); and, for tests/test_explore_ref.py, explored [steps][n] (bool) and greedy [steps][n]
    (the policy's action; 255 where the policy was not consulted)."""

    def __init__(self, c, prepare=None, weights=None, tick0=1):
        self.c = c
        self.tick0 = tick0  # the engine tick the first step starts from (1: right after a reset; else tests/time_shift.py)
        self.weights = c.weights if weights is None else weights
        self.explore = None
        self.fitness = np.zeros((c.n_policies, 4), np.int64)
        self.gids = as_u64([c.gid0 + i for i in range(c.n)])
        self._explored, self._greedy = [], []
        self.ref = lp.TableReference(c.kind, c.n, c.gid0, c.rows, c.index, c.flags, c.reset_seed, actions=self._actions,
                                     prepare=prepare if prepare is not None else c.prepare, tick0=tick0,
                                     bounds=getattr(c, "bounds", None))
        self.start_state = self.ref.state.copy()

    def _actions(self, t, obs):
        c = self.c
        tick = self.ref.tick  # the engine tick this step starts from: the reset took it to 1
        assert tick == self.tick0 + t
        seed, threshold = self.explore if self.explore is not None else (0, 0)
        if threshold < EXPLORE_ONE:
            greedy = cl.policy_ref(c.kind, c.hidden, self.weights, c.lanes_per_policy, c.gid0, obs)
        else:  # every draw is below the threshold: the policy is not asked
            greedy = np.full(c.n, 255, np.uint8)
        explored, random = draw(seed, threshold, DIMS[c.kind][1], self.gids, tick)
        self._explored.append(explored)
        self._greedy.append(greedy)
        return np.where(explored, random, greedy).astype(np.uint8)

    def launch(self, steps, explore=None, count=True):
        r = self.ref
        self.explore = explore
        first = len(r.records)
        r.step(steps)
        rec = r.records[first:]
        rows = {f: np.stack([getattr(x, f) for x in rec]) for f in ("obs", "actions", "reward", "done", "truncated")}
        if count:
            self.fitness = self.fitness + pf.fold_rows(self.c.policies, self.c.n_policies, rows["reward"], rows["done"], rows["truncated"])
        return SimpleNamespace(state=r.state, obs=r.obs, reward=r.reward, done=r.done, truncated=r.truncated, final=r.final.copy(),
                               stats=r.stats.copy(), tick=r.tick, index=r.index.copy(), flags=r.flags, rec_obs=rows["obs"],
                               rec_actions=rows["actions"], rec_reward=rows["reward"], rec_done=rows["done"],
                               rec_truncated=rows["truncated"], fitness=self.fitness.copy(),
                               explored=np.stack(self._explored[first:]), greedy=np.stack(self._greedy[first:]))


def run_case(c, prepare=None, weights=None, tick0=1):
    """One SimpleNamespace per launch of c.schedule, every launch exploring under (c.seed, c.threshold); the first also has
    start_state"""
    run = Run(c, prepare, weights, tick0)
    out = [run.launch(steps, (c.seed, c.threshold)) for steps in c.schedule]
    out[0].start_state = run.start_state
    return out


def whole(out):
    """The rows of all launches of a run_case result, stacked: explored, greedy, actions, ended [steps][n]"""
    cat = lambda f: np.concatenate([getattr(x, f) for x in out])  # noqa: E731
    return SimpleNamespace(explored=cat("explored"), greedy=cat("greedy"), actions=cat("rec_actions"),
                           ended=(cat("rec_done") | cat("rec_truncated")) != 0)
