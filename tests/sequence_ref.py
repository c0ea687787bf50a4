"""One engine under a SEQUENCE of calls, computed on the CPU alone: a model of what the getters of one engine return after any
accepted call of the single-engine stepping surface (include/gymrs_amd.h), a deterministic generator of call sequences over that
surface, and the committed list tests/test_gpu_sequences.py replays on the device, comparing after every call.

Nothing new computes physics.  `Model` stands on lane_params_ref.TableReference (one f32 twin per parameter row, lane i read from
twin index[i], final observations by the flags = 0 twin, statistics rebuilt from the flags); a uniform engine is a table whose K
rows are all the same and whose index is zero, so switching a table on or off, gymrs_set_params and an index rewrite are all "other
rows, other index" -- TableReference.set_rows / set_index, which carry every lane's episode clock and steps_beyond_terminated from
twin to twin (TwinEngine.get_clocks), so they hold under every flag set.  The action sources are the existing references:
TwinEngine.fill_actions (the random policy of step, step_host, step_many's ring, rollout and rollout_record),
closed_loop_ref.policy_ref (greedy), explore_ref.draw (exploring), sample_ref.sample_actions (sampling), and
policy_fitness_ref.fold_rows folds the per-policy records.

A sequence is data: (Config, [op, ...]), every op a tuple whose first element names the call (OPS below lists them).  The
generator emits accepted calls only, apart from ("refused", name): one call the header says returns GYMRS_EINVAL in that
configuration, after which everything must still compare equal.

What the header (include/gymrs_amd.h) says and a sequence trips over:
  clone and snapshot carry table, index, box, final observations, tick and statistics -- not the policy, exploration, sampling,
  fitness or evaluation records (the replay sets the sources again, the fitness records read zero); gymrs_set_params switches a
  table off; a reset without bounds drops the box; gymrs_set_state touches only the state; gymrs_stats_clear is a baseline (open
  episodes go on); gymrs_reset keeps the table, the sources and the fitness records.

Undefined, not generated (the header is silent about the pair; candidates for it to define):
  - gymrs_set_state on Pendulum, then gymrs_get_obs before the next step: whether the (cos, sin) rows follow the new state.  The
    model marks the observation as not comparable until the next step or reset.
  - gymrs_set_param_table on an engine whose table was switched off before: whether the index starts at 0 again or is the one
    kept from the earlier table.  Every ("table", True, seed) sets the index right after the table.
  - gymrs_set_param_table with another K while a table is on: what becomes of an index >= the new K.  Tables here have K = 3.
  - gymrs_set_tuning between gymrs_explore_actions / gymrs_sample_actions / gymrs_policy_actions and the gymrs_step that plays
    the buffer: the pair is always emitted as one op.
  - gymrs_snapshot_load into an engine with another lanes_per_thread or memory hint than the source: whether the tuning is the
    blob's or the engine's.  The replay gives the second engine the first one's tuning before the load.
  - gymrs_evaluate_policy after gymrs_reset(bounds): whether evaluation episodes start from the box.  Its records are not compared.
  - a graph replay (use_graph) whose ring pointer, stride or buffer count differs from the captured one: one ring per sequence.

A plain module like lane_params_ref.py: it never imports the library; no fixtures, no pytest hooks."""
import functools
import random
from collections import namedtuple
from types import SimpleNamespace

import closed_loop_ref as cl
import elided_stores_ref as es
import explore_ref as ex
import lane_params_ref as lp
import numpy as np
import policy_fitness_ref as pf
import reset_box_ref as rb
import sample_ref as sr
from closed_loop_ref import A, COPIES, F, FLAG_SETS, S, T, bits  # noqa: F401  (re-exported to the test files)

K = 3  # rows of a table
LANES = (1, 3, 64, 65, 257, 1024, 1300, 4200)
BIG_OFFSET, BIG_LPP = cl.SHAPES[0][2], cl.SHAPES[0][3]  # 4200 lanes come with this offset and lanes_per_policy
OFFSETS = (0, 12345, 4096, 1 << 33)
CAPS = (5, 17, es.CARTPOLE_LIMIT)
HIDDEN = (0, 1, 7, 8, 64)
LPP = (1, 100, 512, 1000)
N_POLICIES = 3
ROWS_SEED, OTHER_SEED, OTHER_ACTION_SEED = 41, 99, 7
RING_HIP, RING_GRAPH = 5, 32  # buffers of a step_many call: eager launches wrap the ring, a graph walks 32 once and the rest eagerly
EVAL_EPISODES, EVAL_CAP = 2, 17
SENTINEL = 0x7FC0BEEF  # the NaN bit pattern record buffers are pre-filled with
FAULTS = ("clone-box", "fused-final", "set-params-table", "stats-clear-open", "record8-shift", "restore-truncated")

Config = namedtuple("Config", "kind n gid0 flags cap hidden lpp")

# the classes of stepping path (op_class), the events and the calls that change nothing (op_kind)
CLASSES = ("per-step", "many-hip", "many-graph", "random-fused", "cl-plain", "cl-fitness", "recording", "transitions")
EVENTS = ("reset", "reset-box", "set_state", "set_params", "table-on", "table-off", "set_index", "tune", "stats_clear", "fitness_clear",
          "clone", "restore", "set_policy", "set_exploration", "set_sampling")
QUIET = ("evaluate", "sync", "stats", "refused")
GROUPS = {"per-step": "per-step", "many-hip": "step_many", "many-graph": "step_many"}  # every other class: "fused"
OPS = """
  ("reset", seed, box)                    gymrs_reset; box: None or a name of reset_box_ref.NAMED[kind]
  ("step", how, seed, t)                  how "step" | "step_host": the actions fill_actions(seed, t); "policy" | "explore" | "sample":
                                          gymrs_policy_actions / _explore_actions / _sample_actions into a buffer, then gymrs_step
  ("many", form, steps, seed)             gymrs_step_many; form "hip" (RING_HIP buffers) | "graph" (use_graph, RING_GRAPH buffers);
                                          buffer b holds fill_actions(seed, b)
  ("rollout", steps, seed, t0)            gymrs_rollout            ("rollout_record", steps, seed, t0)   gymrs_rollout_record
  ("policy", mode, steps)                 gymrs_rollout_policy (mode "plain"), _record ("record"), _fitness ("fitness")
  ("closed", source, mode, steps, lp)     gymrs_rollout_closed_loop; source "greedy" | "explore" | "sample"; lp: LANE_PARAMS
  ("transitions", source, steps, lp)      gymrs_rollout_transitions with final_obs and start_obs
  ("set_state", count)                    lanes [0, count) take new_state()
  ("set_params", cap, gravity)            gymrs_set_params: max_episode_steps = cap, gravity (Pendulum: g) scaled by `gravity`
  ("table", on, seed)                     gymrs_set_param_table: K rows of make_rows and the index make_index(n, K, seed), or None
  ("set_index", seed)                     gymrs_set_param_index
  ("tune", vec, hint)  ("stats_clear",)  ("fitness_clear",)
  ("clone",)                              the clone takes over; policy, exploration and sampling are set again
  ("restore",)                            a snapshot loaded into a second engine that has stepped twice; it takes over likewise
  ("set_policy", hidden, lpp, seed)  ("set_exploration", seed, threshold)  ("set_sampling", seed, scale)
  ("evaluate",)  ("sync",)  ("stats",)    change nothing
  ("refused", name)                       a call of REFUSALS: GYMRS_EINVAL, changes nothing"""


def op_kind(op):
    """the name an op counts under in the coverage table"""
    if op[0] == "reset":
        return "reset-box" if op[2] else "reset"
    if op[0] == "step":
        return {"step": "step", "step_host": "step_host"}.get(op[1], op[1] + "+step")
    if op[0] == "many":
        return "many-" + op[1]
    if op[0] == "policy":
        return {"plain": "rollout_policy", "record": "rollout_policy_record", "fitness": "rollout_policy_fitness"}[op[1]]
    if op[0] == "closed":
        return f"closed-{op[1]}-{op[2]}" + ("-lp" if op[4] else "")
    if op[0] == "transitions":
        return f"transitions-{op[1]}" + ("-lp" if op[3] else "")
    if op[0] == "table":
        return "table-on" if op[1] else "table-off"
    return op[0]


def op_class(op):
    """the class of stepping path of an op, or None for an op that takes no step"""
    if op[0] == "step":
        return "per-step"
    if op[0] == "many":
        return "many-" + op[1]
    if op[0] == "rollout":
        return "random-fused"
    if op[0] == "rollout_record":
        return "recording"
    if op[0] in ("policy", "closed"):
        mode = op[1] if op[0] == "policy" else op[2]
        return {"plain": "cl-plain", "fitness": "cl-fitness", "record": "recording"}[mode]
    if op[0] == "transitions":
        return "transitions"
    return None


def op_group(op):
    c = op_class(op)
    return None if c is None else GROUPS.get(c, "fused")


def is_closed_loop(op):
    return op[0] in ("policy", "closed", "transitions")


def fmt(op):
    return " ".join(str(x) for x in op)


def stride_of(n):
    """lane stride of record buffers and action rings: n rounded up to 16 lanes"""
    return (n + 15) // 16 * 16


def uniform_row(kind, cap, gravity=1.0):
    if kind == 2:
        row = es.pendulum_row(cap)
        row.g *= gravity
        return row
    row = lp.default_row(kind, cap)
    row.gravity *= gravity
    return row


def table_rows(kind, cap):
    return lp.make_rows(kind, K, ROWS_SEED + kind, cap)


def new_state(kind, state, count):
    """The set_state event: lanes [0, count) take the state of the lane seven to their left (within the prefix); every fifth of
    them is put one step before the end of an episode (CartPole: the pole at 0.2 rad falling at 1 rad/s, MountainCar: at 0.49
    moving towards the goal at 0.04), so that episodes end on engines without a time limit too."""
    new = np.ascontiguousarray(np.roll(state[:, :count], 7, axis=1))
    if kind == 0:
        new[2, ::5], new[3, ::5] = 0.2, 1.0
    elif kind == 1:
        new[0, ::5], new[1, ::5] = 0.49, 0.04
    return new


# ---- refused calls: name -> (applies(config, table on), what) -----------------------------------------------------------------------
REFUSALS = {
    "fitness-with-record": (lambda c, table: c.kind != 2, "rollout_closed_loop with GYMRS_CLOSED_LOOP_FITNESS and a record"),
    "explore-with-sample": (lambda c, table: c.kind != 2, "rollout_closed_loop with EXPLORE and SAMPLE"),
    "transitions-no-auto-reset": (lambda c, table: c.kind != 2 and not c.flags & A, "rollout_transitions on an engine without AUTO_RESET"),
    "policy-under-table": (lambda c, table: table, "rollout_policy while a table is active"),
    "closed-under-table": (lambda c, table: table, "rollout_closed_loop without LANE_PARAMS while a table is active"),
    "graph-pendulum-limit": (lambda c, table: c.kind == 2 and bool(c.flags & T), "step_many use_graph on Pendulum with the time limit"),
    "table-pendulum": (lambda c, table: c.kind == 2, "set_param_table on Pendulum"),
    "final-obs-without-flag": (lambda c, table: not c.flags & F, "get_final_obs on an engine without FINAL_OBS"),
}


# ---- the model ------------------------------------------------------------------------------------------------------------------
class Model:
    """What the getters of one engine of Config `c` return after every op applied so far.  The engine starts with the policy
    make_weights(kind, c.hidden, N_POLICIES, seed 5) at c.lpp lanes per policy, exploration (ex.SEED, ex.THRESHOLD) and sampling
    (sr.SEED, sr.SCALE) (CartPole, MountainCar), at 4 lanes per work-item, hint 0, and must be reset first.

    After apply(op):
      state, obs, reward, done, truncated   as the last step left them (obs_valid False: the header does not say what obs holds)
      final, stats, tick, fitness           final observations, [sum_return, sum_length, n_episodes, steps], the engine tick, the
                                            per-policy records (None without a policy)
      record                                None, or the rows of the op's recording launch: obs [steps][D][n], actions, reward, done,
                                            truncated [steps][n]; transitions also final_obs [steps][D][n], ended, start_obs [D][n]
      table, index, box, vec, hint, policy, explore, sample
    and, for tests/test_sequence_ref.py: seen_actions (set), rearmed, truncations, finals_kept (counts since the first reset).
    `off`: planted faults, names of FAULTS."""

    def __init__(self, c, off=()):
        assert set(off) <= set(FAULTS)
        self.c, self.off = c, frozenset(off)
        self.kind, self.n, self.gid0, self.flags = c.kind, c.n, c.gid0, c.flags
        self.row = uniform_row(c.kind, c.cap)
        self.rows, self.table = [self.row] * K, False
        self.index = np.zeros(c.n, np.int64)
        self.box = None
        self.vec, self.hint = 4, 0
        self.policy = self.explore = self.sample = self.fitness = None
        if c.kind != 2:
            self.set_policy(c.hidden, c.lpp, 5)
            self.explore, self.sample = (ex.SEED, ex.THRESHOLD), (sr.SEED, sr.SCALE)
        self.gids = ex.as_u64([c.gid0 + i for i in range(c.n)])
        self.ref = None
        self.record = None
        self.obs_valid = True
        self._next = None
        self.seen_actions, self.rearmed, self.truncations, self.finals_kept = set(), 0, 0, 0

    # -- what the getters return
    state = property(lambda self: self.ref.state)
    obs = property(lambda self: self.ref.obs)
    reward = property(lambda self: self.ref.reward)
    done = property(lambda self: self.ref.done)
    final = property(lambda self: self.ref.final)
    stats = property(lambda self: self.ref.stats)
    tick = property(lambda self: self.ref.tick)

    @property
    def truncated(self):
        return self._truncated if self._truncated is not None else self.ref.truncated

    # -- sources
    def set_policy(self, hidden, lpp, seed):
        self.policy = SimpleNamespace(weights=cl.make_weights(self.kind, hidden, N_POLICIES, seed), hidden=hidden, lpp=lpp,
                                      of_lane=pf.policies_of(self.n, self.gid0, lpp, N_POLICIES))
        self.fitness = np.zeros((N_POLICIES, 4), np.int64)  # every gymrs_set_policy discards the records

    def _source(self, how, seed=None, t=None):
        """-> f(obs, k): the actions of step k of a call"""
        p = self.policy
        if how == "fill":
            return lambda obs, k: self.ref.tws[0].fill_actions(seed, t + k)
        if how in ("greedy", "policy"):
            return lambda obs, k: cl.policy_ref(self.kind, p.hidden, p.weights, p.lpp, self.gid0, obs)
        if how == "explore":
            def explore(obs, k):
                greedy = cl.policy_ref(self.kind, p.hidden, p.weights, p.lpp, self.gid0, obs)
                explored, rand = ex.draw(self.explore[0], self.explore[1], cl.DIMS[self.kind][1], self.gids, self.ref.tick)
                return np.where(explored, rand, greedy).astype(np.uint8)
            return explore
        assert how == "sample", how
        return lambda obs, k: sr.sample_actions(self.kind, p.hidden, p.weights, p.lpp, self.gid0, obs, self.sample[0], self.sample[1],
                                                self.ref.tick)[0]

    def _actions(self, t, obs):
        f, k = self._next
        self._next = (f, k + 1)
        return f(obs, k)

    def _steps(self, count, source, fused=False, closed=False):
        """`count` steps with the actions of `source`; returns the rows a recording launch keeps (and final_obs, ended, start_obs)"""
        r = self.ref
        self._next = (source, 0)
        start = r.obs.copy()
        kept = r.final.copy()
        finals = []
        r.records.clear()
        for _ in range(count):
            r.step(1)
            finals.append(r.final.copy())  # (the ended lanes of THIS step have just been written)
        rows = {f: np.stack([getattr(x, f) for x in r.records]) for f in ("obs", "actions", "reward", "done", "truncated")}
        r.records.clear()
        rows["ended"] = (rows["done"] | rows["truncated"]) != 0
        rows["final_obs"], rows["start_obs"] = np.stack(finals), start
        if fused and "fused-final" in self.off:
            r.final = kept
        if self.kind != 2 and closed:
            self.seen_actions |= set(np.unique(rows["actions"]).tolist())
        if self.flags & A:
            self.rearmed += int(rows["ended"].sum())
            differs = (bits(rows["final_obs"]) != bits(rows["obs"])).any(axis=1) & rows["ended"]
            self.finals_kept += int(differs.sum())
        self.truncations += int(rows["truncated"].sum())
        self._truncated = None
        self.obs_valid = True
        return rows

    def _keep(self, rows, transitions=False):
        names = ("obs", "actions", "reward", "done", "truncated") + (("final_obs", "ended", "start_obs") if transitions else ())
        self.record = {f: rows[f] for f in names}
        if self.vec == 8 and "record8-shift" in self.off:
            self.record = {f: (x if f == "start_obs" else np.roll(x, 1, axis=-1)) for f, x in self.record.items()}

    def _fold(self, rows):
        self.fitness = self.fitness + pf.fold_rows(self.policy.of_lane, N_POLICIES, rows["reward"], rows["done"], rows["truncated"])

    def _reset(self, seed, box):
        self.box = None if box is None else rb.NAMED[self.kind][box]
        self.ref = lp.TableReference(self.kind, self.n, self.gid0, self.rows, self.index, self.flags, seed, actions=self._actions, bounds=self.box)
        self._truncated = None
        self.obs_valid = True

    def _takes_over(self):
        """clone / restore: the sources are set again by the caller; the fitness records are not carried"""
        if self.policy is not None:
            self.fitness = np.zeros((N_POLICIES, 4), np.int64)

    def told_apart(self):
        """of the lanes of a table engine: the fraction whose state differs from what the neighbouring row would have made of it"""
        return self.ref.told_apart((self.ref.index + 1) % K)

    def apply(self, op):
        name, r = op[0], self.ref
        self.record = None
        if name == "reset":
            self._reset(op[1], op[2])
        elif name == "step":
            how = op[1]
            self._steps(1, self._source("fill", op[2], op[3]) if how in ("step", "step_host") else self._source(how), closed=how not in ("step", "step_host"))
        elif name == "many":
            ring = [r.tws[0].fill_actions(op[3], b) for b in range(RING_GRAPH if op[1] == "graph" else min(RING_HIP, op[2]))]
            self._steps(op[2], lambda obs, k: ring[k % len(ring)])
        elif name == "rollout":
            self._steps(op[1], self._source("fill", op[2], op[3]), fused=True)
        elif name == "rollout_record":
            self._keep(self._steps(op[1], self._source("fill", op[2], op[3]), fused=True))
        elif name in ("policy", "closed"):
            source, mode, steps = ("greedy", op[1], op[2]) if name == "policy" else op[1:4]
            assert not self.table or (name == "closed" and op[4])
            rows = self._steps(steps, self._source(source), fused=True, closed=True)
            if mode == "fitness":
                self._fold(rows)
            elif mode == "record":
                self._keep(rows)
        elif name == "transitions":
            assert self.flags & A and (not self.table or op[3])
            self._keep(self._steps(op[2], self._source(op[1]), fused=True, closed=True), transitions=True)
        elif name == "set_state":
            state = r.state.copy()
            state[:, :op[1]] = new_state(self.kind, r.state, op[1])
            r.set_state(state)
            self.obs_valid = self.kind != 2
        elif name == "set_params":
            if self.table and "set-params-table" in self.off:
                return
            self.row = uniform_row(self.kind, op[1], op[2])
            self.rows, self.table, self.index = [self.row] * K, False, np.zeros(self.n, np.int64)
            r.set_rows(self.rows, self.index)
        elif name == "table":
            if op[1]:
                self.rows, self.index = table_rows(self.kind, self.row.max_episode_steps), lp.make_index(self.n, K, op[2]).astype(np.int64)
            else:  # every lane uses row 0 again
                self.row = self.rows[0]
                self.rows, self.index = [self.row] * K, np.zeros(self.n, np.int64)
            self.table = bool(op[1])
            r.set_rows(self.rows, self.index)
        elif name == "set_index":
            assert self.table
            self.index = lp.make_index(self.n, K, op[1]).astype(np.int64)
            r.set_index(self.index)
        elif name == "tune":
            self.vec, self.hint = op[1], op[2]
        elif name == "stats_clear":
            r.stats_clear()
            if "stats-clear-open" in self.off:
                r.ep_start[:] = r.tick
        elif name == "fitness_clear":
            self.fitness = np.zeros((N_POLICIES, 4), np.int64)
        elif name == "clone":
            self._takes_over()
            if "clone-box" in self.off and self.box is not None and self.kind != 2:
                r.rebox(None)
        elif name == "restore":
            self._takes_over()
            if "restore-truncated" in self.off:  # the array the second engine held after its own two steps
                self._truncated = other_truncated(self.c)
        elif name == "set_policy":
            self.set_policy(*op[1:])
        elif name == "set_exploration":
            self.explore = (op[1], op[2])
        elif name == "set_sampling":
            self.sample = (op[1], op[2])
        else:
            assert name in QUIET, op


def other_truncated(c):
    """`truncated` of the second engine of a restore right before the load: reset(OTHER_SEED), two random steps"""
    tw = lp.TwinEngine(lp.twin(), c.kind, c.n, uniform_row(c.kind, c.cap), flags=c.flags & ~F, gid0=c.gid0)
    tw.reset(OTHER_SEED)
    for t in range(2):
        tw.step(tw.fill_actions(OTHER_ACTION_SEED, t))
    return tw.get_result()[2]


def run(c, ops, off=(), upto=None):
    """The model after ops[:upto]"""
    m = Model(c, off)
    for op in ops[:upto]:
        m.apply(op)
    return m


def worth_comparing(c, ops):
    """What a sequence must show before a comparison with it means anything; returns what is missing (empty: all met).  With
    auto-reset an episode ends and a lane is re-armed (Pendulum never terminates: without the time limit it is exempt); with the time
    limit a lane is truncated; with FINAL_OBS a final observation is kept and differs from the lane's fresh state; under a policy two
    different actions occur; every table is stepped under before it goes, and after the LAST launch under a table nearly every
    lane would differ had it stepped with the neighbouring row."""
    m, periods = Model(c), []  # per stretch with a table on: told_apart after its last launch (None: no launch under it)
    for op in ops:
        was_on = m.table
        m.apply(op)
        if m.table and not was_on:
            periods.append(None)
        if m.table and op_class(op):
            periods[-1] = m.told_apart()
    ends = not (c.kind == 2 and not c.flags & T)
    missing = []
    if c.flags & A and ends and not m.rearmed:
        missing.append("no episode ended")
    if c.flags & T and not m.truncations:
        missing.append("no lane was truncated")
    if c.flags & F and ends and not m.finals_kept:
        missing.append("no final observation differs from the fresh state")
    if any(is_closed_loop(op) or (op[0] == "step" and op[1] in ("policy", "explore", "sample")) for op in ops) and len(m.seen_actions) < 2:
        missing.append(f"one action only: {sorted(m.seen_actions)}")
    if None in periods:
        missing.append("a table went without a launch under it")
    missing += [f"a neighbouring row shows in {apart:.2f} of the lanes only" for apart in periods if apart is not None and apart < 0.9]
    return missing


def snapshot(m):
    """what a comparison after an op looks at, as {name: array} (record rows as record.<row>)"""
    out = {"state": m.state, "reward": m.reward, "done": m.done, "tick": np.array([m.tick])}
    if m.obs_valid:
        out["obs"] = m.obs
    if m.flags & T:
        out["truncated"] = m.truncated
    if m.flags & F:
        out["final"] = m.final
    if m.flags & A and m.flags & S:
        out["stats"] = m.stats
    if m.fitness is not None:
        out["fitness"] = m.fitness
    for f, x in (m.record or {}).items():
        if f == "truncated" and not m.flags & T:
            continue
        if f == "final_obs":  # (valid where the lane-step ended an episode)
            x = np.where(m.record["ended"][:, None, :], x, np.float32(0))
        out["record." + f] = x
    return {k: np.array(v) for k, v in out.items()}


def first_difference(c, ops, off):
    """(position, op, names) of the first op after which the model with the faults `off` differs from the intact one, or None"""
    good, bad = Model(c), Model(c, off)
    for k, op in enumerate(ops):
        good.apply(op)
        bad.apply(op)
        a, b = snapshot(good), snapshot(bad)
        names = [f for f in a if a[f].shape != b[f].shape or not np.array_equal(a[f].view(np.uint8), b[f].view(np.uint8))]
        if names:
            return k, op, names
    return None


# ---- the generator --------------------------------------------------------------------------------------------------------------
# Coverage holds by construction; worth_comparing (an episode ends, two actions occur, ..) depends on the draws as well: this seed's
# list meets both, and tests/test_sequence_ref.py asserts it.
GENERATOR_SEED = 20260131
MIN_SEQUENCES, MAX_SEQUENCES = 40, 64
MIN_OPS, MAX_OPS = 12, 16
MAX_STEPS = 40
MAX_REFUSALS = 1  # per sequence: at most one op in eight (MIN_OPS = 12)
WIDE = 257  # lanes from which 8 lanes per work-item is a shape of its own: 257 lanes are all ragged there, 1024 two full waves
# what has to run at 8 lanes per work-item on a wide engine of either Discrete kind, and on one of 257 lanes
AT_EIGHT = ("closed-loop", "recording", "transitions", "many-graph", "clone", "restore")

# Openings that put something within reach by construction: (kind, flags, cap, lanes or None for the turn's, ops after the first reset)
OPENINGS = (
    # the box travels with a clone: re-arms after it draw from the box (CartPole TERMINAL: most re-armed lanes end again at once)
    (0, A | S | F, 17, None, [("reset", 21, "TERMINAL"), ("many", "hip", 12, 3), ("clone",), ("rollout", 9, 4, 100), ("step", "step", 4, 7)]),
    # a fused launch writes the final observations
    (1, A | S | T | F, 5, None, [("rollout", 7, 4, 0), ("closed", "greedy", "plain", 6, False), ("step", "step", 4, 50)]),
    # gymrs_set_params switches the table off
    (0, A | T, 17, None, [("table", True, 61), ("many", "hip", 4, 3), ("set_params", 17, 1.5), ("many", "hip", 6, 5), ("rollout", 5, 4, 20)]),
    # gymrs_stats_clear leaves open episodes alone
    (0, A | S | T, 17, None, [("many", "hip", 9, 3), ("stats_clear",), ("many", "hip", 12, 5), ("stats",)]),
    # recording launches run at 4 lanes per work-item whatever the tuning
    (1, A | S | T, 5, None, [("tune", 8, 0), ("step", "step", 4, 0), ("closed", "sample", "record", 7, False), ("rollout_record", 6, 4, 30)]),
    # a snapshot load rewrites `truncated`: without auto-reset every step from the limit on truncates every lane
    (0, T, 5, None, [("many", "hip", 7, 3), ("restore",), ("sync",), ("step", "step", 4, 9)]),
    # Pendulum: its uniform truncated value across a restore and a clone
    (2, A | S | T, 5, None, [("many", "hip", 5, 3), ("restore",), ("step", "step", 4, 9), ("many", "hip", 4, 3), ("clone",), ("rollout", 3, 4, 10)]),
    # 257 lanes, all ragged at 8 lanes per work-item: a snapshot loaded into an engine tuned to 8, a graph replay, then fused
    # closed-loop, transitions and recording launches, a clone in between
    (0, A | S | T | F, 17, 257, [("tune", 8, 0), ("many", "hip", 5, 3), ("restore",), ("many", "graph", 33, 5), ("closed", "greedy", "plain", 9, False),
                                 ("closed", "explore", "fitness", 5, False), ("transitions", "sample", 6, True), ("clone",),
                                 ("closed", "greedy", "record", 7, False)]),
    # the same walk on MountainCar, two full waves and a ragged one at 8
    (1, A | S | T | F, 17, 1300, [("tune", 8, 2), ("step", "step", 4, 0), ("restore",), ("many", "graph", 32, 5), ("closed", "sample", "fitness", 9, False),
                                  ("transitions", "greedy", 6, False), ("clone",), ("policy", "record", 5), ("closed", "explore", "plain", 4, True)]),
    # CartPole with all three flags and the long limit: launches that cannot reach it, the refresh, launches that can
    (0, A | S | T, es.CARTPOLE_LIMIT, 1024, [("many", "hip", 40, 3), ("many", "graph", 36, 5), ("rollout", 21, 4, 100), ("stats",)]),
    # an index rewritten under the time limit after episodes have ended: the lanes take their episode clocks to their new rows
    (0, A | T, 17, 1300, [("table", True, 61), ("many", "hip", 21, 3), ("set_index", 77), ("many", "hip", 8, 5), ("set_index", 78),
                          ("closed", "greedy", "plain", 9, True)]),
)


def steps_of(op):
    """the steps an op takes"""
    at = {"step": None, "many": 2, "rollout": 1, "rollout_record": 1, "policy": 2, "closed": 3, "transitions": 2}
    if op[0] not in at:
        return 0
    return 1 if op[0] == "step" else op[at[op[0]]]


class Track:
    """What the generator and the coverage know of an engine without running the model: whether a table is on and how many steps
    were taken under it, whether a box is set, the tuning, the limit and the steps since the last reset (`reached`: a lane that
    lives on can have reached the time limit)"""

    def __init__(self, cap):
        self.table = self.box = self.reached = False
        self.under = self.run = 0
        self.vec, self.hint, self.cap = 4, 0, cap

    def note(self, op):
        if op[0] == "table":
            self.table, self.under = bool(op[1]), 0
        elif op[0] == "set_params":
            self.table, self.cap = False, op[1]
        elif op[0] == "reset":
            self.box, self.run = op[2] is not None, 0
        elif op[0] == "tune":
            self.vec, self.hint = op[1], op[2]
        steps = steps_of(op)
        self.run += steps
        self.under += steps if self.table else 0
        self.reached |= steps > 0 and self.run >= self.cap
        return self


def tracked(c, ops):
    """the Track of config c after ops"""
    t = Track(c.cap)
    for op in ops:
        t.note(op)
    return t


def at_eight(op):
    """the name of AT_EIGHT an op counts under when it runs at 8 lanes per work-item, or None"""
    if op[0] in ("clone", "restore"):
        return op[0]
    return {"cl-plain": "closed-loop", "cl-fitness": "closed-loop", "recording": "recording", "transitions": "transitions",
            "many-graph": "many-graph"}.get(op_class(op))


class Coverage:
    """The conditions of tests/test_sequence_ref.py, as sets of what is still missing"""

    def __init__(self):
        self.kinds = {}
        self.pairs = {(k, a, b) for k in (0, 1) for a in CLASSES for b in CLASSES}
        self.follows = {(e, g) for e in EVENTS for g in ("per-step", "step_many", "fused")}
        self.lanes = {n: 0 for n in LANES}
        self.lanes_closed = set(LANES)
        self.flag_kinds = {(f, k) for f in FLAG_SETS for k in (0, 1)}
        self.tunings = {("vec", 4), ("vec", 8)} | {("hint", h) for h in range(4)}  # closed by a STEP under the tuning
        self.carried = {(e, w) for e in ("clone", "restore") for w in ("table", "box", "final")}
        self.eight = {(k, w) for k in (0, 1, WIDE) for w in AT_EIGHT}  # kind k on WIDE lanes or more; WIDE: on exactly WIDE lanes
        self.refusals = set(REFUSALS)
        self.special = {"CartPole A|S|T at limit 45 on 1024 lanes or more", "set_index on CartPole with A|T after episodes have ended"}

    def _eight(self, c, op, t):
        """the conditions of `eight` that op closes on an engine of config c in state t"""
        w = at_eight(op)
        if w is None or t.vec != 8 or c.kind == 2 or c.n < WIDE:
            return set()
        return {(c.kind, w)} | ({(WIDE, w)} if c.n == WIDE else set())

    def wanted(self, c, prev, op, t):
        """how many open conditions `op` would close after `prev` on an engine of config c in state t (a Track)"""
        score = 0
        kind = op_kind(op)
        score += 2 if self.kinds.get(kind, 0) < 3 else 0
        if prev is not None:
            a, b = op_class(prev), op_class(op)
            if a and b and (c.kind, a, b) in self.pairs:
                score += 3
            if op_kind(prev) in EVENTS and op_group(op) and (op_kind(prev), op_group(op)) in self.follows:
                score += 3
        if kind in EVENTS and any(e == kind for e, _ in self.follows):  # an event whose followers are not all seen yet
            score += 2.5
        if is_closed_loop(op) and c.n in self.lanes_closed:
            score += 3
        if op[0] == "tune":
            score += 2 if ("vec", op[1]) in self.tunings or ("hint", op[2]) in self.tunings else 0
            wide = c.kind != 2 and c.n >= WIDE and any(k == c.kind or (k == WIDE and c.n == WIDE) for k, _ in self.eight)
            score += 4 if op[1] == 8 and t.vec != 8 and wide else (-4 if op[1] == 4 and t.vec == 8 and wide else 0)
        score += 4 * len(self._eight(c, op, t) & self.eight)
        if op[0] == "refused" and op[1] in self.refusals:
            score += 4
        if op[0] in ("clone", "restore"):
            score += 2 * sum((op[0], w) in self.carried for w, on in (("table", t.table), ("box", t.box), ("final", c.flags & F)) if on)
        return score

    def begin(self, c):
        self.lanes[c.n] += 1
        self.flag_kinds.discard((c.flags, c.kind))
        if c.kind == 0 and c.flags & (A | S | T) == A | S | T and c.cap == es.CARTPOLE_LIMIT and c.n >= 1024:
            self.special.discard("CartPole A|S|T at limit 45 on 1024 lanes or more")

    def note(self, c, ops):
        """take the last op of `ops` into account, given the ops before it"""
        t = tracked(c, ops[:-1])
        prev, op = (ops[-2] if len(ops) > 1 else None), ops[-1]
        self.kinds[op_kind(op)] = self.kinds.get(op_kind(op), 0) + 1
        if prev is not None:
            if op_class(prev) and op_class(op):
                self.pairs.discard((c.kind, op_class(prev), op_class(op)))
            if op_kind(prev) in EVENTS and op_group(op):
                self.follows.discard((op_kind(prev), op_group(op)))
        if is_closed_loop(op):
            self.lanes_closed.discard(c.n)
        if op_class(op):  # a tuning counts once a launch has run under it
            self.tunings -= {("vec", t.vec), ("hint", t.hint)}
        self.eight -= self._eight(c, op, t)
        if op[0] == "refused":
            self.refusals.discard(op[1])
        if op[0] == "set_index" and c.kind == 0 and c.flags & A and c.flags & T and t.under >= t.cap:
            self.special.discard("set_index on CartPole with A|T after episodes have ended")
        t.note(op)
        if op[0] in ("clone", "restore"):
            self.carried -= {(op[0], w) for w, on in (("table", t.table), ("box", t.box), ("final", c.flags & F)) if on}

    def add(self, c, ops):
        self.begin(c)
        for k in range(len(ops)):
            self.note(c, ops[:k + 1])

    def missing(self, all_kinds):
        out = [f"op kind {k}: {self.kinds.get(k, 0)} times" for k in all_kinds if self.kinds.get(k, 0) < 3]
        out += [f"{('CartPole', 'MountainCar')[k]}: {a} then {b}" for k, a, b in sorted(self.pairs)]
        out += [f"{e} followed by {g}" for e, g in sorted(self.follows)]
        out += [f"{n} lanes used {k} times" for n, k in self.lanes.items() if k < 2]
        out += [f"{n} lanes without a fused closed-loop launch" for n in sorted(self.lanes_closed)]
        out += [f"flag set {f} not met by kind {k}" for f, k in sorted(self.flag_kinds)]
        out += [f"no launch under tuning {t}" for t in sorted(self.tunings)] + [f"{e} with {w}" for e, w in sorted(self.carried)]
        out += [f"8 lanes per work-item, {'257 lanes' if k == WIDE else ('CartPole', 'MountainCar')[k] + ' on 257 lanes or more'}: no {w}"
                for k, w in sorted(self.eight)]
        out += [f"refusal {name} never drawn" for name in sorted(self.refusals)] + sorted(self.special)
        return out


def candidates(c, rng, table, refusals, t):
    """every op the engine accepts now, with drawn arguments; t: a counter that keeps action slots apart"""
    steps = rng.choice((1, 2, 3, 5, 8, 13, 21, MAX_STEPS))
    seed = rng.randrange(1, 100)
    out = [("step", "step", seed, t), ("step", "step_host", seed, t), ("many", "hip", steps, seed), ("rollout", steps, seed, 10 * t),
           ("rollout_record", min(steps, 13), seed, 10 * t), ("reset", rng.randrange(1 << 30), None),
           ("reset", rng.randrange(1 << 30), rng.choice(rb.named(c.kind))), ("set_state", rng.choice((1, c.n, max(1, c.n // 2), min(c.n, 300)))),
           ("set_params", rng.choice(CAPS), rng.choice((0.8, 1.25))), ("tune", rng.choice((4, 8)), rng.randrange(4)), ("stats_clear",),
           ("clone",), ("restore",), ("sync",), ("stats",)]
    if not (c.kind == 2 and c.flags & T):
        out.append(("many", "graph", rng.randrange(32, MAX_STEPS + 1), seed))
    if c.kind != 2:
        out += [("step", how, 0, t) for how in ("policy", "explore", "sample")]
        source = rng.choice(("greedy", "explore", "sample"))
        for mode in ("plain", "fitness", "record"):
            out.append(("closed", source, mode, min(steps, 13) if mode == "record" else steps, table or rng.random() < 0.5))
            if not table:
                out.append(("policy", mode, min(steps, 13) if mode == "record" else steps))
        if c.flags & A:
            out.append(("transitions", source, min(steps, 13), table or rng.random() < 0.5))
        out += [("table", not table, rng.randrange(50, 99)), ("fitness_clear",), ("evaluate",),
                ("set_policy", rng.choice(HIDDEN), BIG_LPP if c.n == 4200 else rng.choice(LPP), rng.randrange(1, 30)),
                ("set_exploration", rng.randrange(1 << 62), rng.choice((8192, 16384, 40000))),
                ("set_sampling", rng.randrange(1 << 62), float(np.float32(sr.LOG2E / rng.choice((1.0, 4.0, 8.0)))))]
        if table:
            out.append(("set_index", rng.randrange(50, 99)))
    if refusals < MAX_REFUSALS:
        out += [("refused", name) for name, (applies, _) in REFUSALS.items() if applies(c, table)]
    return out


def configs(rng, count):
    """`count` configurations, stratified: the lane counts, the flag sets and the kinds each take turns; the Discrete kinds meet
    every flag set (2 x 10 combinations after the openings), Pendulum every fifth configuration after that"""
    out = []
    combos = [(k, f) for f in FLAG_SETS for k in (0, 1)]
    for i in range(count):
        n = LANES[(i * 3 + 6) % len(LANES)]
        if i < len(OPENINGS):
            kind, flags, cap = OPENINGS[i][:3]
            n = OPENINGS[i][3] or n
        elif i % 5 == 4:
            kind, flags, cap = 2, FLAG_SETS[(i // 5) % len(FLAG_SETS)], CAPS[i % 2]
        else:
            kind, flags = combos[(i * 7) % len(combos)] if i >= 2 * len(combos) else combos[i % len(combos)]
            cap = CAPS[i % 3]
        if kind == 0 and i >= len(OPENINGS):  # a CartPole lane has to live up to the limit for it to show: few do for 45 steps
            cap = 5 if n <= 3 else (17 if n < 1024 and cap > 17 else cap)
        gid0, lpp = (BIG_OFFSET, BIG_LPP) if n == 4200 else (OFFSETS[i % 4], LPP[i % 3])
        out.append(Config(kind, n, gid0, flags, cap, HIDDEN[i % len(HIDDEN)], lpp))
    return out


def generate(seed, count=None):
    """[(Config, ops)]: `count` sequences, or (None) as many as the conditions of Coverage need, between MIN_SEQUENCES and
    MAX_SEQUENCES.  Stratified: the next op is drawn among the accepted ones that close the most open conditions."""
    rng = random.Random(seed)
    cov = Coverage()
    out = []
    for i, c in enumerate(configs(rng, MAX_SEQUENCES if count is None else count)):
        if count is None and i >= MIN_SEQUENCES and not cov.missing(()):
            break
        ops = list(OPENINGS[i][4]) if i < len(OPENINGS) else []
        if not ops or ops[0][0] != "reset":
            ops.insert(0, ("reset", rng.randrange(1 << 30), None))
        if c.kind != 2 and c.flags & A and not c.flags & T and i >= len(OPENINGS):
            ops.append(("set_state", c.n))  # without a limit few episodes end by themselves (MountainCar: none): lanes next to their end
        if c.kind != 2 and c.n <= 3 and i >= len(OPENINGS):  # three lanes may well agree on one action: explore on most steps
            ops += [("set_exploration", rng.randrange(1 << 62), 40000), ("closed", "explore", "plain", 21, False)]
        cov.begin(c)
        for k in range(len(ops)):
            cov.note(c, ops[:k + 1])
        t = tracked(c, ops)
        refusals = 0
        length = max(rng.randrange(MIN_OPS, MAX_OPS + 1), len(ops) + 2)
        while len(ops) < length:
            cands = candidates(c, rng, t.table, refusals, len(ops))
            if not any(op_class(o) for o in ops[-2:]) or ops[-1][0] == "tune":  # no three ops in a row without a step; a launch under every tuning
                cands = [o for o in cands if op_class(o)]
            if len(ops) == length - 1:  # the last op takes a step: whatever came before shows in the arrays
                cands = [o for o in cands if op_class(o)]
            if t.table and not t.under:  # a table is stepped under before it goes
                cands = [o for o in cands if o[0] not in ("table", "set_params")]
            if c.flags & T and not t.reached and length - len(ops) <= 4:  # a lane has to reach the limit: long launches, no reset
                cands = [o for o in cands if op_class(o) and steps_of(o) >= min(13, t.cap - t.run)] or [("many", "hip", MAX_STEPS, 3)]
            scored = [(cov.wanted(c, ops[-1], o, t) + rng.random(), k) for k, o in enumerate(cands)]
            op = cands[max(scored)[1]]
            ops.append(op)
            refusals += op[0] == "refused"
            cov.note(c, ops)
            t.note(op)
        out.append((c, ops))
    return out


@functools.lru_cache(maxsize=None)
def sequences():
    """The committed list: deterministic from the constants of this module"""
    return tuple(generate(GENERATOR_SEED))


def sequence_id(k, c):
    flags = "".join(ch for ch, b in zip("ASTF", (A, S, T, F)) if c.flags & b) or "0"
    return f"{k:02d}-{('cp', 'mc', 'pd')[c.kind]}-{flags}-n{c.n}-cap{c.cap}"
