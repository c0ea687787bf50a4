"""Custom reset boxes (`options` of reset: state_dim lows then state_dim highs, f32) and the cases that run under them.

gymrs_reset(bounds) replaces the engine's sampling box, and every later GYMRS_AUTO_RESET re-arm draws from it.  The default boxes
hide a wrong read of the box: CartPole's is +-0.05 in all four components, MountainCar samples one component.  The boxes here do not:

  CartPole     DISTINCT  four disjoint intervals of four different widths: a permutation of the components, or of the three rows of
                         the kernel's SampleBox (lo, scale24, hi_prev), puts a re-armed lane outside its interval
               TERMINAL  x in [2, 3), across x_threshold = 2.4: more than half of the re-armed lanes end again on their next step
               FAR       theta in [-0.7, 400): across the fast path's range |theta| <= pi / 4 (Env::kRangeMax in
                         gym-rs_amd/csrc/gymrs_tile.h; lane_params_ref.beyond_range restates it) and across the f32 Cody-Waite range
                         of 200; a wave of 256 re-armed lanes holds about one lane inside the range
  MountainCar  GOAL      position in [0.3, 0.6), across goal_position = 0.5; the velocity bounds are a visible [0.03, 0.06), but the
                         velocity is not sampled: it is 0 after the reset and after every re-arm
               WALL      position in [-1.3, -1.1), across min_position = -1.2
               FAR       position in [60, 80), across |3 * position| = 200
  Pendulum     DISTINCT  (= FAR) theta in [190, 210), across 200; theta_dot in [7, 9), across max_speed = 8

EDGES are boxes at the corners of make_sample_box / uniform_in_box (gym-rs_amd/csrc/gymrs_philox.h), REFUSED the ones gymrs_reset
must not accept.  Both vary component 0 and leave the rest at the default.

The module also holds the closed-loop cases of tests/test_gpu_reset_box.py and the figures that show, from the references alone, that
they reach what they are for; tests/test_reset_box_ref.py asserts them without a GPU.  It never imports the library.

A plain module like closed_loop_ref.py, imported by test files; no fixtures, no pytest hooks."""
from functools import lru_cache
from types import SimpleNamespace

import closed_loop_ref as cl
import explore_ref as ex
import lane_params_ref as lp
import numpy as np
import sample_ref as sr
from closed_loop_ref import A, COPIES, F, S, T  # noqa: F401  (re-exported to the test files)

STATE_DIM = {0: 4, 1: 2, 2: 2}
SAMPLED = {0: 4, 1: 1, 2: 2}  # MountainCar's velocity is not sampled
PI_F32 = float(np.float32(np.pi))
DEFAULT = {0: ([-0.05] * 4, [0.05] * 4), 1: ([-0.6, 0.0], [-0.4, 0.0]), 2: ([-PI_F32, -1.0], [PI_F32, 1.0])}  # what the engine and the twin start with


def box(kind, lows=None, highs=None, **components):
    """lows then highs as f32: the default box of `kind` with the given components replaced (c0=(low, high), ...)"""
    lo, hi = (list(x) for x in DEFAULT[kind])
    if lows is not None:
        lo, hi = list(lows), list(highs)
    for name, (low, high) in components.items():
        lo[int(name[1:])], hi[int(name[1:])] = low, high
    return np.array(lo + hi, np.float32)


NAMED = {0: {"DISTINCT": box(0, (-2.0, 0.5, 0.05, -1.0), (-1.5, 1.0, 0.15, -0.5)),
             "TERMINAL": box(0, c0=(2.0, 3.0)),
             "FAR": box(0, c2=(-0.7, 400.0))},
         1: {"GOAL": box(1, (0.3, 0.03), (0.6, 0.06)),
             "WALL": box(1, c0=(-1.3, -1.1)),
             "FAR": box(1, c0=(60.0, 80.0))},
         2: {"DISTINCT": box(2, (190.0, 7.0), (210.0, 9.0))}}
FIRST = {0: "DISTINCT", 1: "GOAL", 2: "DISTINCT"}  # the box of the runs that take one per env
ENDS_TWICE = {(0, "TERMINAL"), (1, "GOAL")}  # lanes re-armed into a state that is already terminal
LEAVES_RANGE = {(0, "FAR"), (1, "FAR"), (2, "DISTINCT")}  # lanes re-armed into the general physics path
EDGES = {"[-1, 0)": (-1.0, 0.0),  # hi_prev is the negative subnormal
         "[-1, -0)": (-1.0, -0.0),  # the same from the other zero
         "[1, nextafter 1)": (1.0, float(np.nextafter(np.float32(1.0), np.float32(2.0)))),  # hi_prev == lo: every draw is 1
         "[1e5, 1e5 + 1)": (1.0e5, 1.0e5 + 1.0),  # an ulp of 2^-7: 128 values, and the clamp to hi_prev is reached
         "[0, 2^24)": (0.0, 16777216.0),  # scale24 = 1: the draw is the 24-bit integer itself
         "[-1.5e38, 1.5e38)": (-1.5e38, 1.5e38)}  # the widest width an f32 holds: 3e38 < FLT_MAX
REFUSED = {"[-3e38, 3e38)": (-3.0e38, 3.0e38), "[-2e38, 2e38)": (-2.0e38, 2.0e38),  # an infinite f32 width
           "[0, 1e-45)": (0.0, 1.0e-45), "[-1e-40, 1e-40)": (-1.0e-40, 1.0e-40)}  # (high - low) * 2^-24 is zero / subnormal


def edge(kind, name):
    return box(kind, c0=EDGES[name])


def refused(kind, name):
    return box(kind, c0=REFUSED[name])


def named(kind):
    return list(NAMED[kind])


def oracle_bounds(kind, bounds):
    """The same box as Oracle.reset_batch takes it (f64; MountainCar: {low, high} of the position)"""
    b = np.asarray(bounds, np.float32).astype(np.float64)
    return [b[0], b[2]] if kind == 1 else list(b)


def tolerance(kind, bounds):
    """tol_j = 2^-23 * (|hi_j - lo_j| + max(|lo_j|, |hi_j|)) per state component (0 where the component is not sampled): what an f32
    draw may differ by from the f64 draw of the same random word.  fl32(hi - lo) carries a relative error of 2^-24, spread over at most
    2^24 steps of the draw: 2^-24 * |hi - lo|; the fma rounds its result once: 2^-24 * max(|lo|, |hi|); the clamp stays within one ulp
    of hi.  Their sum, doubled for slack."""
    d = STATE_DIM[kind]
    b = np.asarray(bounds, np.float32).astype(np.float64)
    lo, hi = b[:d], b[d:]
    tol = 2.0 ** -23 * (np.abs(hi - lo) + np.maximum(np.abs(lo), np.abs(hi)))
    tol[SAMPLED[kind]:] = 0.0
    return tol


def inside(kind, bounds, state):
    """lo_j <= v < hi_j for every sampled component of every lane (and 0 for MountainCar's velocity)"""
    d = STATE_DIM[kind]
    b = np.asarray(bounds, np.float32)
    ok = all(((state[j] >= b[j]) & (state[j] < b[d + j])).all() for j in range(SAMPLED[kind]))
    return ok and all((state[j] == 0).all() for j in range(SAMPLED[kind], d))


def swapped(kind, bounds, i, j):
    """The box with components i and j transposed"""
    d = STATE_DIM[kind]
    b = np.array(bounds, np.float32)
    b[[i, j]] = b[[j, i]]
    b[[d + i, d + j]] = b[[d + j, d + i]]
    return b


# ---- the closed-loop cases of tests/test_gpu_reset_box.py --------------------------------------------------------------------------
FULL = A | S | T | F
SCHEDULE = (40, 40)
# (hidden, global offset, (n_policies, lanes_per_policy)): gathered weights on the per-lane block path; whole waves uniform
POLICIES = {"gathered": (8, 6, (3, 1)), "uniform": (0, 0, (3, 512))}
SOURCES = ("greedy", "explore", "sample")


def closed_loop_cases():
    """[(kind, policy set name, box name, table)]"""
    return [(kind, ps, name, table) for kind in (0, 1) for ps in POLICIES for name in NAMED[kind] for table in (False, True)]


def closed_loop_case(kind, ps, name, table, source, default_box=False):
    hidden, gid0, policy_set = POLICIES[ps]
    bounds = None if default_box else NAMED[kind][name]
    if source == "sample":
        return sr.case(kind, FULL, table, gid0, policy_set, hidden, SCHEDULE, bounds=bounds)
    return ex.case(kind, FULL, table, gid0, policy_set, hidden, SCHEDULE, bounds=bounds)


def settings(c, source):
    """The second argument of Run.launch"""
    return {"greedy": None, "explore": (c.seed, getattr(c, "threshold", None)), "sample": (c.seed, getattr(c, "scale", None))}[source]


@lru_cache(maxsize=None)
def closed_loop_run(kind, ps, name, table, source, default_box=False):
    """(case, [one launch record per launch of SCHEDULE]) of explore_ref.Run / sample_ref.Run; the first record also has start_state.
    Computed once and shared: nobody writes to it."""
    c = closed_loop_case(kind, ps, name, table, source, default_box)
    run = (sr.Run if source == "sample" else ex.Run)(c)
    out = [run.launch(steps, settings(c, source)) for steps in c.schedule]
    out[0].start_state = run.start_state
    return c, out


@lru_cache(maxsize=None)
def transitions_run(kind, ps, name, table):
    """(case, launches) of sample_ref.TransitionsRun: the sampling run with final_obs, ended and start_obs"""
    c = closed_loop_case(kind, ps, name, table, "sample")
    run = sr.TransitionsRun(c)
    return c, [run.launch(steps) for steps in c.schedule]


def findings(c, launches):
    """What a run shows, per lanes-per-work-item value and kernel copy:
      launches_with_rearms   in how many launches of the schedule a lane of the copy ended an episode (and was re-armed)
      twice                  lane-steps that end an episode right after a step that ended one
      beyond                 re-armed lanes whose next step starts outside the fast range
      mixed                  (full copies) wave-steps with re-armed lanes outside the range AND lanes inside it"""
    out = {}
    ended = [(x.rec_done | x.rec_truncated) != 0 for x in launches]
    all_ended = np.concatenate(ended)  # [steps][n]
    after = np.concatenate([x.rec_obs for x in launches])  # the state every step leaves, re-armed lanes included
    beyond = lp.beyond_range(c.kind, after.transpose(1, 0, 2))  # [steps][n]
    rearmed_beyond = beyond[:-1] & all_ended[:-1]  # the step after starts there
    for vec in (4, 8):
        classes = c.classes[vec]
        per_wave = 64 * vec
        for copy in np.unique(classes):
            m = classes == copy
            f = SimpleNamespace(launches_with_rearms=sum(bool(e[:, m].any()) for e in ended),
                                twice=int((all_ended[1:, m] & all_ended[:-1, m]).sum()), beyond=int(rearmed_beyond[:, m].sum()), mixed=None)
            if copy < 2:
                f.mixed = 0
                for first in range(0, c.n - per_wave + 1, per_wave):
                    if m[first]:
                        w = slice(first, first + per_wave)
                        f.mixed += int((rearmed_beyond[:, w].any(axis=1) & ~beyond[:-1, w].all(axis=1)).sum())
            out[vec, COPIES[copy]] = f
    return out


def missing(kind, name, c, launches):
    """The conditions a case has to meet; returns what is missing (empty: all met)"""
    out = []
    for (vec, copy), f in findings(c, launches).items():
        at = f"{copy} at {vec} lanes per work-item"
        if f.launches_with_rearms < 2:
            out.append(f"{at}: re-arms in {f.launches_with_rearms} launches")
        if (kind, name) in ENDS_TWICE and f.twice < 1:
            out.append(f"{at}: no lane ends on two consecutive steps")
        if (kind, name) in LEAVES_RANGE:
            if f.beyond < 1:
                out.append(f"{at}: no re-armed lane starts outside the fast range")
            if f.mixed is not None and f.mixed < 1:
                out.append(f"{at}: no wave holds re-armed lanes outside the range and lanes inside it")
    return out
