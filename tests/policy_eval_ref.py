"""gymrs_evaluate_policy (include/gymrs_amd.h, "episodic policy evaluation") computed on the CPU alone: start states from the f32
twin's reset (oracle.bindings.TwinEngine), steps on a flags = 0 twin, actions from tests/cpp/policy_ref.c through
closed_loop_ref.policy_ref, every lane stopped at its first done or at M; the records are summed with Python ints.  Like
closed_loop_ref this module never imports the library: what it returns is the yardstick of tests/test_gpu_policy_eval.py, and
tests/test_policy_eval_ref.py shows without a GPU that its cases are worth comparing with.

A plain module, imported by test files; no fixtures, no pytest hooks."""
from types import SimpleNamespace

import closed_loop_ref as ref
import numpy as np
import policy_fitness_ref as fit

from oracle.bindings import Twin, TwinEngine

FIELDS = ("return_sum", "return_sq_sum", "episodes", "done", "truncated", "steps", "return_min", "return_max")  # gymrs_policy_eval order
INT64_MAX, INT64_MIN = 2**63 - 1, -2**63
IDENTITY = (0, 0, 0, 0, 0, 0, INT64_MAX, INT64_MIN)
SIGN = {0: 1, 1: -1}  # the reward per step: CartPole +1, MountainCar -1
DONE_BIT = 0x80000000
MASK64 = 2**64 - 1

_twin = None


def _the_twin():
    global _twin
    if _twin is None:
        _twin = Twin()
    return _twin


def identity(n_policies):
    return np.array([IDENTITY] * n_policies, np.int64).reshape(n_policies, 8)


def _wrap(v):
    """an integer modulo 2^64 as the int64 with the same bits"""
    v &= MASK64
    return v - 2**64 if v >= 2**63 else v


def start_states(kind, n, gid0, params, seed, episodes, lanes_per_policy, common):
    """[E] arrays (D, n): where episode e of every lane starts: reset(seed + e) of the lane's global id, or with `common` of lane
    g % lanes_per_policy of an engine at offset 0"""
    out = []
    for e in range(episodes):
        s = (seed + e) & MASK64
        if common:
            tw = TwinEngine(_the_twin(), kind, lanes_per_policy, params, flags=0, gid0=0)
            tw.reset(s)
            idx = np.array([(gid0 + i) % lanes_per_policy for i in range(n)], np.int64)
            out.append(np.ascontiguousarray(tw.get_state()[:, idx]))
        else:
            tw = TwinEngine(_the_twin(), kind, n, params, flags=0, gid0=gid0)
            tw.reset(s)
            out.append(tw.get_state().copy())
    return out


def play(kind, n, gid0, params, weights, hidden, lanes_per_policy, starts, max_steps):
    """(length [E][n] int64, done [E][n] bool): every lane stepped from starts[e] until its first done or max_steps"""
    w = np.ascontiguousarray(weights, np.float32).reshape(-1, ref.size_of(kind, hidden))
    tw = TwinEngine(_the_twin(), kind, n, params, flags=0, gid0=gid0)
    length = np.zeros((len(starts), n), np.int64)
    done = np.zeros((len(starts), n), bool)
    for e, st in enumerate(starts):
        tw.reset(0)  # (clears steps_beyond_terminated; the state is replaced)
        tw.set_state(st)
        playing = np.ones(n, bool)
        for k in range(1, max_steps + 1):
            act = ref.policy_ref(kind, hidden, w, lanes_per_policy, gid0, tw.get_obs())
            tw.step(act)
            _, dn, _ = tw.get_result()
            dn = np.asarray(dn) != 0
            ends = playing & (dn | (k == max_steps))
            length[e, ends] = k
            done[e, ends] = dn[ends]
            playing &= ~ends
            if not playing.any():
                break
        assert not playing.any()
    return length, done


def records(kind, length, done, pol, n_policies, max_steps):
    """(n_policies, 8) int64 in FIELDS order from the episodes [E][n] of lanes whose policies are pol [n]"""
    out = identity(n_policies)
    for p in range(n_policies):
        m = pol == p
        if not m.any():
            continue
        ls = [int(x) for x in length[:, m].ravel()]
        rets = [SIGN[kind] * x for x in ls]
        out[p] = (_wrap(sum(rets)), _wrap(sum(r * r for r in rets)), len(ls), int(done[:, m].sum()), sum(x == max_steps for x in ls),
                  _wrap(sum(ls)), min(rets), max(rets))
    return out


def merge(parts):
    """The records of several engines that cut one batch: sums added (modulo 2^64), min of mins, max of maxes"""
    parts = [np.asarray(p, np.int64) for p in parts]
    out = identity(len(parts[0]))
    for p in range(len(out)):
        for c in range(6):
            out[p, c] = _wrap(sum(int(x[p, c]) for x in parts))
        out[p, 6] = min(int(x[p, 6]) for x in parts)
        out[p, 7] = max(int(x[p, 7]) for x in parts)
    return out


def packed(length, done):
    """the `lengths` buffer: uint32 [E][n], L | done << 31"""
    return (length.astype(np.uint32) | np.where(done, np.uint32(DONE_BIT), np.uint32(0))).astype(np.uint32)


def reference(kind, n, gid0, params, weights, hidden, lanes_per_policy, n_policies, seed, episodes, max_steps, common=False):
    """What gymrs_evaluate_policy leaves: .records (n_policies, 8) int64, .lengths uint32 [E][n], and .length / .done / .pol"""
    starts = start_states(kind, n, gid0, params, seed, episodes, lanes_per_policy, common)
    length, done = play(kind, n, gid0, params, weights, hidden, lanes_per_policy, starts, max_steps)
    pol = fit.policies_of(n, gid0, lanes_per_policy, n_policies)
    return SimpleNamespace(records=records(kind, length, done, pol, n_policies, max_steps), lengths=packed(length, done), length=length,
                           done=done, pol=pol, starts=starts)


# ---- the cases of tests/test_gpu_policy_eval.py (checked without a GPU by tests/test_policy_eval_ref.py) -----------------------
EPISODES, MAX_STEPS, N_POLICIES, SEED = 3, 17, 3, 11
HIDDEN = ref.HIDDEN
SHAPES = [s for s in ref.SHAPES if s[1] == 4][:2]  # (4200, 4, 2^40 + 12345, 1000) and (5000, 4, 12345, 1024): the evaluator runs at 4 lanes per work-item
assert [(s[0], s[2], s[3]) for s in SHAPES] == [(4200, (1 << 40) + 12345, 1000), (5000, 12345, 1024)]
# Seed of closed_loop_ref.make_weights per (kind, hidden, index into SHAPES), common starts off and on alike: a seed, searched with
# this module alone, that meets worth_comparing in the lanes of every copy.  tests/test_policy_eval_ref.py asserts they do.
WEIGHT_SEEDS = {(0, 0, 0): 21, (0, 0, 1): 21, (0, 7, 0): 18, (0, 7, 1): 18, (0, 8, 0): 11, (0, 8, 1): 11,
                (1, 0, 0): 20, (1, 0, 1): 20, (1, 7, 0): 55, (1, 7, 1): 55, (1, 8, 0): 2, (1, 8, 1): 2}


def mountain_car_params(params):
    """MountainCar from its reset box ends no episode in 17 steps: the goal moves into the box (and needs no speed), so lanes that
    start near it reach it and the others run into the limit"""
    params.goal_position = -0.45
    params.goal_velocity = 0.0
    return params


def cases():
    return [(kind, shape, hidden, common) for kind in (0, 1) for shape in range(len(SHAPES)) for hidden in HIDDEN for common in (False, True)]


def case(kind, shape, hidden, common, params, weight_seed=None):
    """The arguments of `reference` for one case; `params` = the engine's default parameters of `kind` (edited here)."""
    n, vec, gid0, lpp = SHAPES[shape]
    if kind == 1:
        mountain_car_params(params)
    seed = WEIGHT_SEEDS[kind, hidden, shape] if weight_seed is None else weight_seed
    return SimpleNamespace(kind=kind, n=n, gid0=gid0, params=params, weights=ref.make_weights(kind, hidden, N_POLICIES, seed), hidden=hidden,
                           lanes_per_policy=lpp, common=common, classes=ref.wave_classes(n, 4, gid0, N_POLICIES, lpp))


def run_case(c):
    return reference(c.kind, c.n, c.gid0, c.params, c.weights, c.hidden, c.lanes_per_policy, N_POLICIES, SEED, EPISODES, MAX_STEPS, c.common)


def worth_comparing(c, r):
    """What a case must show to be worth a GPU comparison; returns a list of what is missing (empty: all met)."""
    missing = []
    total = r.length.sum(axis=0)
    for copy in np.unique(c.classes):
        m = c.classes == copy
        name = ref.COPIES[copy]
        by_done = r.done[:, m] & (r.length[:, m] < MAX_STEPS)
        if not by_done.any():
            missing.append(f"{name}: no episode ends by done before the limit")
        if not (r.length[:, m] == MAX_STEPS).any():
            missing.append(f"{name}: no episode runs into the limit")
        waves = [total[f:f + 256] for f in range(0, c.n, 256) if m[f]]  # (a wave's lanes all belong to one copy)
        if not any(t.min() != t.max() for t in waves):  # some lanes of a wave park while others still play
            missing.append(f"{name}: in every wave all lanes take the same number of steps")
    rec = r.records
    if not any((rec[p] != rec[q]).any() for p in range(len(rec)) for q in range(p)):
        missing.append("the records of all policies are equal")
    if not (rec[:, 6] != rec[:, 7]).any():
        missing.append("return_min == return_max in every record")
    return missing
