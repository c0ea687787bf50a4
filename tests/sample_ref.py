"""A closed-loop rollout with softmax action sampling (include/gymrs_amd.h, "sampling") computed on the CPU alone.

The rule is restated in tests/cpp/sample_ref.c from the header's text (plain C, libm's fmaf / floorf / ldexpf, gcc -O2
-ffp-contract=off; the logits in the order of tests/cpp/policy_ref.c); the word of every draw comes from the numpy Philox of
tests/explore_ref.py on stream 3.  The loop is explore_ref.Run's -- lane_params_ref.TableReference stepped with these actions -- and
the transitions loop is transitions_ref's, one step at a time.  This module never imports the library: what it returns is the
yardstick of tests/test_gpu_sample.py, and tests/test_sample_ref.py shows without a GPU that its cases are worth comparing with.

A plain module like explore_ref.py, imported by test files; no fixtures, no pytest hooks."""
import ctypes as C
import math
import tempfile
from pathlib import Path

import closed_loop_ref as cl
import explore_ref as ex
import numpy as np
import spawn_server
from closed_loop_ref import A, COPIES, DIMS, F, FLAG_SETS, S, T, bits  # noqa: F401  (re-exported to the test files)
from explore_ref import HIDDEN, N, OFFSETS, POLICY_SETS, SPLITS, STEPS, axes, matrix  # noqa: F401

STREAM_SAMPLE = 3
LOG2E = math.log2(math.e)
TEMPERATURE = 8.0  # CartPole's affine logits grow with the state: at temperature 1 some cases hardly ever leave the argmax
SCALE = float(np.float32(LOG2E / TEMPERATURE))
SEED = 0x5A3B1E0FEEDC0DE5  # of the sampling stream
WEIGHTS_SEED = ex.WEIGHTS_SEED  # tests/test_sample_ref.py shows that the cases it gives are worth comparing with

_lib = None
_dir = None


def lib():
    global _lib, _dir
    if _lib is None:
        _dir = tempfile.TemporaryDirectory(prefix="sample_ref")  # removed when the interpreter exits
        out = Path(_dir.name) / "libsample_ref.so"
        src = Path(__file__).resolve().parent / "cpp" / "sample_ref.c"
        spawn_server.run(["gcc", "-O2", "-ffp-contract=off", "-shared", "-fPIC", str(src), "-o", str(out), "-lm"], check=True)
        _lib = C.CDLL(str(out))
        _lib.sample_ref_poly.restype = C.c_float
        _lib.sample_ref_poly.argtypes = [C.c_float]
        _lib.sample_ref_weight.restype = C.c_float
        _lib.sample_ref_weight.argtypes = [C.c_float]
        _lib.sample_ref_draw.restype = C.c_int
        _lib.sample_ref_draw.argtypes = [C.c_int, C.c_void_p, C.c_float, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.sample_ref_draw_many.restype = None
        _lib.sample_ref_draw_many.argtypes = [C.c_int, C.c_uint64, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.sample_ref.restype = None
        _lib.sample_ref.argtypes = [C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_float,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.sample_ref_poly_max_rel_err.restype = C.c_double
        _lib.sample_ref_poly_max_rel_err.argtypes = []
    return _lib


def words(seed, gid, tick):
    """word (gid & 3) of the stream-3 block (gid >> 2, tick): uint32, gid and tick broadcast"""
    return np.ascontiguousarray(ex.stream_word(seed, gid, tick, STREAM_SAMPLE), dtype=np.uint32)


def draw_many(logits, scale, w):
    """One draw per row of `logits` ([n][A] f32) with the words w [n]: (action, greedy: uint8 [n]; probs: f32 [n][A])"""
    y = np.ascontiguousarray(logits, np.float32)
    n, a = y.shape
    w = np.ascontiguousarray(w, np.uint32)
    assert w.shape == (n,)
    act, greedy, probs = np.empty(n, np.uint8), np.empty(n, np.uint8), np.empty((n, a), np.float32)
    lib().sample_ref_draw_many(a, n, y.ctypes.data, scale, w.ctypes.data, act.ctypes.data, greedy.ctypes.data, probs.ctypes.data)
    return act, greedy, probs


def sample_actions(kind, hidden, weights, lanes_per_policy, gid0, obs, seed, scale, tick):
    """The sampled step of every column of obs (lane gid0 + i) at engine tick `tick`: (action, greedy, prob of the action, logits
    [A][n])"""
    d, a, w, obs = cl._args(kind, hidden, weights, obs)
    n = obs.shape[1]
    wd = words(seed, ex.as_u64([gid0 + i for i in range(n)]), tick)
    act, greedy, prob, y = np.empty(n, np.uint8), np.empty(n, np.uint8), np.empty(n, np.float32), np.empty((a, n), np.float32)
    lib().sample_ref(d, a, hidden, w.size // cl.size_of(kind, hidden), lanes_per_policy, gid0, n, w.ctypes.data, obs.ctypes.data, scale,
                     wd.ctypes.data, act.ctypes.data, greedy.ctypes.data, prob.ctypes.data, y.ctypes.data)
    return act, greedy, prob, y


# ---- the cases of tests/test_gpu_sample.py: explore_ref's shapes, axes and matrix ---------------------------------------------------
def case(kind, flags, table, gid0=0, policy_set=(3, 512), hidden=0, schedule=SPLITS[0], n=N, scale=SCALE, seed=SEED, weights=None, bounds=None):
    c = ex.case(kind, flags, table, gid0, policy_set, hidden, schedule, n, seed=seed, bounds=bounds)
    c.scale = float(np.float32(scale))
    del c.threshold
    if weights is not None:
        c.weights = weights
    return c


def matrix_case(kind, flags, table, i):
    gid0, policy_set, hidden, schedule = axes(i)
    return case(kind, flags, table, gid0, policy_set, hidden, schedule)


class Run(ex.Run):
    """explore_ref.Run with the sampled action.  launch(steps, sample) -- sample = (seed, scale), or None for the greedy launch --
    returns what explore_ref.Run.launch returns (explored = the action taken is not the greedy one) and prob [steps][n]: the
    probability of the action taken (1 in a greedy launch)."""

    def __init__(self, c, prepare=None, weights=None, tick0=1):
        self._prob = []
        super().__init__(c, prepare, weights, tick0)

    def _actions(self, t, obs):
        c = self.c
        tick = self.ref.tick  # the engine tick this step starts from: the reset took it to 1
        assert tick == self.tick0 + t
        if self.explore is None:
            greedy = cl.policy_ref(c.kind, c.hidden, self.weights, c.lanes_per_policy, c.gid0, obs)
            act, prob = greedy, np.ones(c.n, np.float32)
        else:
            seed, scale = self.explore
            act, greedy, prob, _ = sample_actions(c.kind, c.hidden, self.weights, c.lanes_per_policy, c.gid0, obs, seed, scale, tick)
        self._explored.append(act != greedy)
        self._greedy.append(greedy)
        self._prob.append(prob)
        return act

    def launch(self, steps, sample=None, count=True):
        first = len(self._prob)
        out = super().launch(steps, sample, count)
        out.prob = np.stack(self._prob[first:])
        return out


def run_case(c, prepare=None, weights=None, tick0=1):
    """One SimpleNamespace per launch of c.schedule, every launch sampling under (c.seed, c.scale); the first also has start_state"""
    run = Run(c, prepare, weights, tick0)
    out = [run.launch(steps, (c.seed, c.scale)) for steps in c.schedule]
    out[0].start_state = run.start_state
    return out


whole = ex.whole


class TransitionsRun:
    """transitions_ref.Run over the sampling Run: launch(steps) also returns final_obs [steps][D][n] (valid where ended), ended
    [steps][n] and start_obs [D][n]."""

    def __init__(self, c, tick0=1):
        self.c = c
        self.run = Run(c, tick0=tick0)
        self.start_state = self.run.start_state

    def launch(self, steps, sample=None):
        sample = (self.c.seed, self.c.scale) if sample is None else sample
        start = self.run.ref.obs.copy()
        parts, finals = [], []
        for _ in range(steps):
            parts.append(self.run.launch(1, sample))
            finals.append(parts[-1].final)  # TableReference has just written the ended lanes of THIS step
        last = parts[-1]
        for f in ("rec_obs", "rec_actions", "rec_reward", "rec_done", "rec_truncated", "prob"):
            setattr(last, f, np.concatenate([getattr(p, f) for p in parts]))
        last.ended = (last.rec_done | last.rec_truncated) != 0
        last.final_obs = np.stack(finals)
        last.start_obs = start
        return last


def softmax64(logits, scale):
    """The f64 softmax the rule approximates: exp2((y - max) * scale), normalised"""
    y = np.asarray(logits, np.float64)
    w = np.exp2((y - y.max()) * float(scale))
    return w / w.sum()
