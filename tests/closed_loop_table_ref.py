"""A closed-loop rollout under a per-lane parameter table computed on the CPU alone: lane_params_ref.TableReference (one f32 twin
per row, lane i read from twin index[i]) stepped with the actions of closed_loop_ref.policy_ref (tests/cpp/policy_ref.c, plain C).
Neither shares code with the library's kernels and this module never imports the library: what it returns is the yardstick of
tests/test_gpu_closed_loop_table.py (gymrs_rollout_closed_loop with GYMRS_CLOSED_LOOP_LANE_PARAMS), and
tests/test_closed_loop_table_ref.py shows without a GPU that its cases are worth comparing with.

The case table is closed_loop_ref's (SHAPES, HIDDEN, FLAG_SETS, N_POLICIES, the 17-step limit, mountain_car_prepare, reset seed 3) on
lane_params_ref's five rows, with a launch schedule of its own.

A plain module like closed_loop_ref.py, imported by test files; no fixtures, no pytest hooks."""
from types import SimpleNamespace

import closed_loop_ref as cl
import lane_params_ref as lp
import numpy as np
import policy_fitness_ref as pf
from closed_loop_ref import A, COPIES, DIMS, F, FLAG_SETS, S, T, bits  # noqa: F401  (re-exported to the test files)

K = lp.K  # rows of the table
N_POLICIES = cl.N_POLICIES
MAX_EPISODE_STEPS = cl.MAX_EPISODE_STEPS
RESET_SEED = cl.RESET_SEED
# Steps per launch.  Not closed_loop_ref.SCHEDULE: its total of 51 is a multiple of the 17-step limit, and right after a limit
# nearly every MountainCar lane holds a fresh reset draw, the same under every row: a wrong row would not show.  The totals
# compared here are 1, 8, 48 and 52.
SCHEDULE = (1, 7, 40, 4)
SHAPES = cl.SHAPES
HIDDEN = cl.HIDDEN
RECORD_HIDDEN = cl.RECORD_HIDDEN
TOLD_APART = lp.TOLD_APART
# Seed of make_weights per (kind, hidden, index into SHAPES): closed_loop_ref.SEEDS unless an entry here replaces it -- the next
# seed for which, under the table, every condition of worth_comparing holds under every flag set
# (tests/test_closed_loop_table_ref.py asserts that the seeds in use meet them).
SEEDS = {}


def seed_of(kind, hidden, shape):
    return SEEDS.get((kind, hidden, shape), cl.SEEDS[kind, hidden, shape])


def cases(record=False):
    """(kind, index into SHAPES, flag set, hidden) of every case of the matrix; record: the recording kernel's (4 lanes per
    work-item only, hidden in RECORD_HIDDEN)"""
    return [(kind, shape, flags, hidden) for kind in (0, 1) for shape, s in enumerate(SHAPES) if not record or s[1] == 4
            for flags in FLAG_SETS for hidden in (RECORD_HIDDEN if record else HIDDEN)]


def records_too(shape, hidden):
    """Whether the case is also one of the recording kernel's"""
    return SHAPES[shape][1] == 4 and hidden in RECORD_HIDDEN


def neighbour(index):
    """The row next to every lane's own: what a kernel that gathered the wrong row would have stepped with"""
    return (np.asarray(index, np.int64) + 1) % K


def case(kind, shape, flags, hidden, integrator=0):
    n, vec, gid0, lpp = SHAPES[shape]
    rows = lp.make_rows(kind, K, lp.ROWS_SEED + kind, MAX_EPISODE_STEPS, integrator)
    index = lp.make_index(n, K, lp.INDEX_SEED + kind)
    w = cl.make_weights(kind, hidden, N_POLICIES, seed_of(kind, hidden, shape))
    prepare = (lambda state: cl.mountain_car_prepare(state, 0)) if kind == 1 else None
    return SimpleNamespace(kind=kind, n=n, vec=vec, gid0=gid0, flags=flags, rows=rows, index=index, weights=w, hidden=hidden,
                           lanes_per_policy=lpp, reset_seed=RESET_SEED, schedule=SCHEDULE, prepare=prepare,
                           classes=cl.wave_classes(n, vec, gid0, N_POLICIES, lpp),
                           policies=pf.policies_of(n, gid0, lpp, N_POLICIES))


class Run:
    """The reference of a case, launch by launch.  launch(steps) advances it and returns a SimpleNamespace of what an engine holds
    afterwards -- state, obs, reward, done, truncated, final, stats, tick as the getters return them; rec_obs [steps][D][n],
    rec_actions, rec_reward, rec_done, rec_truncated [steps][n], the rows a recording launch keeps; fitness (n_policies, 4) int64,
    the per-policy records accumulated over the launches so far -- and of what shows that a comparison there means something:
    episodes [n] ended so far, actions_seen [A][n], disagree [n] (two policies of the set, asked alone, chose differently),
    told_apart = the fraction of lanes whose state would differ had they been stepped with their neighbour's row.
    set_index(index): the index rewritten between two launches (TableReference.set_index)."""

    def __init__(self, c, prepare=None):
        self.c = c
        n_act = DIMS[c.kind][1]
        self.seen = np.zeros((n_act, c.n), bool)
        self.disagree = np.zeros(c.n, bool)
        self.episodes = np.zeros(c.n, np.int64)
        self.fitness = np.zeros((N_POLICIES, 4), np.int64)
        self.ref = lp.TableReference(c.kind, c.n, c.gid0, c.rows, c.index, c.flags, c.reset_seed, actions=self._actions,
                                     prepare=prepare if prepare is not None else c.prepare)
        self.start_state = self.ref.state.copy()

    def _actions(self, t, obs):
        c = self.c
        act = cl.policy_ref(c.kind, c.hidden, c.weights, c.lanes_per_policy, c.gid0, obs)
        self.seen[act, np.arange(c.n)] = True
        alone = [cl.policy_ref(c.kind, c.hidden, c.weights[i:i + 1], 1, 0, obs) for i in range(len(c.weights))]
        for x in alone[1:]:
            self.disagree |= x != alone[0]
        return act

    def set_index(self, index):
        self.ref.set_index(index)

    def launch(self, steps):
        r = self.ref
        first = len(r.records)
        r.step(steps)
        rec = r.records[first:]
        rows = {f: np.stack([getattr(x, f) for x in rec]) for f in ("obs", "actions", "reward", "done", "truncated")}
        self.episodes = self.episodes + ((rows["done"] | rows["truncated"]) != 0).sum(axis=0)
        self.fitness = self.fitness + pf.fold_rows(self.c.policies, N_POLICIES, rows["reward"], rows["done"], rows["truncated"])
        return SimpleNamespace(state=r.state, obs=r.obs, reward=r.reward, done=r.done, truncated=r.truncated, final=r.final.copy(),
                               stats=r.stats.copy(), tick=r.tick, index=r.index.copy(), flags=r.flags, rec_obs=rows["obs"],
                               rec_actions=rows["actions"], rec_reward=rows["reward"], rec_done=rows["done"],
                               rec_truncated=rows["truncated"], fitness=self.fitness.copy(), episodes=self.episodes.copy(),
                               actions_seen=self.seen.copy(), disagree=self.disagree.copy(), told_apart=r.told_apart(neighbour(r.index)))


def run_case(c, prepare=None):
    """One SimpleNamespace per launch of c.schedule (Run.launch); the first also has start_state"""
    run = Run(c, prepare)
    out = [run.launch(steps) for steps in c.schedule]
    out[0].start_state = run.start_state
    return out


def worth_comparing(c, out):
    """What a case must show before a comparison with it means anything; returns a list of what is missing (empty: all met).
    Per copy of the kernel with lanes in the case: an episode ended (flag sets with A or T), two different actions occurred, two
    policies disagreed.  After every launch: a lane stepped with its neighbour's row would differ in at least TOLD_APART of them."""
    last = out[-1]
    missing = []
    for copy in np.unique(c.classes):
        m = c.classes == copy
        name = COPIES[copy]
        if c.flags & (A | T) and not last.episodes[m].any():
            missing.append(f"{name}: no episode ended")
        if (last.actions_seen[:, m].any(axis=1)).sum() < 2:
            missing.append(f"{name}: one action only")
        if not last.disagree[m].any():
            missing.append(f"{name}: the policies never disagree")
    for k, launch in enumerate(out):
        if not launch.told_apart >= TOLD_APART:
            missing.append(f"launch {k}: a neighbouring row shows in {launch.told_apart:.3f} of the lanes only")
    return missing


def coverage():
    """{(kind, vec, flag set, mode): lanes stepped per copy (in COPIES order), summed over the matrix's cases}, mode in ("fused",
    "fitness", "record"): one entry per instantiation of the two TableT kernel families.  No cell may be zero."""
    out = {}
    for kind, shape, flags, hidden in cases():
        n, vec, gid0, lpp = SHAPES[shape]
        lanes = np.bincount(cl.wave_classes(n, vec, gid0, N_POLICIES, lpp), minlength=4)
        for mode in ("fused", "fitness") + (("record",) if records_too(shape, hidden) else ()):
            row = out.setdefault((kind, vec, flags, mode), np.zeros(4, np.int64))
            row += lanes
    return out
