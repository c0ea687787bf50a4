"""The stores a step may skip because "the array already holds the right value", computed on the CPU alone: the cases of
tests/test_gpu_elided_stores.py and what every call of a case must leave in the engine's arrays.

Three protocols keep knowledge about an array outside that array (gym-rs_amd/csrc/gymrs_step_impl.h, gymrs_engine.hip):
  1. the constant reward (MountainCar under auto-reset always, CartPole under auto-reset from 2^22 lanes on or with
     GYMRS_DEV_ELIDE_REWARD=1): one `wave_clean` word per wavefront on the device, `clean_shape` on the host;
  2. Pendulum's uniform `truncated` value (host `trunc_held`);
  3. CartPole A | S | T launches that drop the time limit and do not write `truncated` (host `trunc_zero`).
A skipped store is only seen to be wrong while the array is dirty, so a case here is a SCRIPT of calls that leaves an array dirty
across the call that has to invalidate the bookkeeping: reset, two valid steps (the words get set), a dirtying call (an invalid
action or a parameter index outside the table: the documented, recoverable GYMRS_EACTION report), the report consumed, an event,
one repairing step, two more steps.  Nothing ever writes into the engine's views.

Nothing new computes physics: the expected arrays come from the f32 twin stepped with the same actions (TwinTable
below: one twin per row as in lane_params_ref.py, a uniform engine being a table of one row).  The twin leaves a lane with an invalid action alone
and pays it 0; a lane whose parameter index is outside the table is documented to be treated the same way, so the reference hands
the twins an invalid action for such a lane.

RewardProtocol is a model of protocol 1 -- the words, clean_shape and the clearing points -- in which every clearing point can be
switched off: tests/test_elided_stores_ref.py shows with it that a case would notice the missing invalidation.

A plain module like lane_params_ref.py: it never imports the library; no fixtures, no pytest hooks."""
import ctypes as C
import functools
from collections import namedtuple
from types import SimpleNamespace

import lane_params_ref as lp
import numpy as np
from lane_params_ref import A, S, T

from oracle.bindings import Oracle, TwinEngine

N = 1300  # 4 lanes per work-item: five full wavefronts of 256 lanes and one of 20; 8 lanes: two of 512 and one of 276
SHAPES = (4, 8)
DIRTY = (300, 1234, 1299)  # wavefront slots 1, 4, 5 at 4 lanes per work-item and 0, 2, 2 at 8; lane 1299 is in the ragged wave
BAD_ACTION = 7
K = 2  # rows of the table engines
BAD_INDEX = (K, 65535, K)  # the parameter index of the DIRTY lanes in the index cases
RESET_SEED, OTHER_SEED, ACTION_SEED, RING_SEED, ROWS_SEED, INDEX_SEED = 11, 99, 6, 7, 41, 42
RING = 32  # action buffers of a step_many call; a call walks each buffer once
MANY = {"hip": 8, "graph": 32, "aql": 8}  # steps of a step_many call per form: a chain needs 8 launches, a graph replay 32
CONST = {0: 1.0, 1: -1.0}  # the constant reward
CARTPOLE_LIMIT = 45
# name -> (kind, flags, max_episode_steps); CartPole engines are created with the reward elision forced on
ENGINES = {"mc-A": (1, A, 200), "mc-AST": (1, A | S | T, 200), "cp-A": (0, A, CARTPOLE_LIMIT), "cp-AS": (0, A | S, CARTPOLE_LIMIT),
           "cp-AST": (0, A | S | T, CARTPOLE_LIMIT)}

FUSED = ("rollout", "record", "cl-greedy", "cl-explore", "cl-sample", "cl-fitness", "cl-record", "transitions")
FUSED_STEPS = {"rollout": 3, "record": 3}  # the closed-loop launches take one step: its actions are the action kernel's at that tick
UNIFORM_SOURCES = ("step", "step_host") + tuple(f"many-{form}-{where}" for form in MANY for where in ("last", "mid"))
TABLE_SOURCES = ("index-step",) + FUSED
EVENTS = ("none", "tune-other", "tune-hint", "restore", "clone", "record8", "stats-clear", "set-params", "table-off-on", "set-state")
REPAIRS = ("step", "step_host", "many-hip", "many-graph", "many-aql")
# event -> the clearing point it relies on.  (record8 changes the shape twice, but its fused launch stores every reward -- all of
# them the constant -- so the array is clean before the repairing step looks at a word: that event checks the arrays and the
# statistics around two shape changes, it cannot show a stale reward.)
CLEARED_BY = {"tune-other": "shape", "restore": "load"}
HINT_NONE = 2  # gymrs_set_tuning's memory_hint "none": at this size the automatic choice is "every access non-temporal"

Case = namedtuple("Case", "engine shape source event repair")


def slot(lane, vec):
    """the wavefront (= index of its wave_clean word) that steps `lane` at `vec` lanes per work-item"""
    return lane // (64 * vec)


def needs_table(c):
    return c.source in TABLE_SOURCES or c.event == "table-off-on"


def case_id(c):
    return "-".join((c.engine, str(c.shape), c.source, c.event, c.repair))


def scripts():
    """(source, event, repair) of every script, the same for every engine and shape: every dirty source with no event and `step`
    as the repair, every event with the `step` invalid action as the source across all repair paths, every fused source with
    step_many as the repair"""
    out = [(s, "none", "step") for s in UNIFORM_SOURCES + TABLE_SOURCES]
    out += [("step", e, r) for e in EVENTS for r in REPAIRS if (e, r) != ("none", "step")]
    out += [(s, "none", r) for s in FUSED for r in REPAIRS if r.startswith("many-")]
    return out


def reward_cases():
    return [Case(e, shape, *s) for e in ENGINES for shape in SHAPES for s in scripts()]


def rows_of(engine, table):
    kind, _, limit = ENGINES[engine]
    return lp.make_rows(kind, K, ROWS_SEED + kind, limit) if table else [lp.default_row(kind, limit)]


def index_of(engine, table):
    return lp.make_index(N, K, INDEX_SEED + ENGINES[engine][0]) if table else np.zeros(N, np.uint16)


def changed_row(kind, row):
    """the set-params event: another gravity"""
    new = type(row).from_buffer_copy(bytes(row))
    new.gravity = row.gravity * 1.25
    return new


@functools.lru_cache(maxsize=None)
def _fill(kind, seed, t):
    a = lp.fill_actions(kind, N, 0, seed, t)
    a.setflags(write=False)
    return a


def calls_of(c):
    """The script of a case: a list of calls (tuples, the first element names the call) and the positions of the dirtying call
    and of the repairing step in it.

      ("reset",)                    reset(RESET_SEED)
      ("step", path, bad)           path "step" | "step_host"; bad: the DIRTY lanes get BAD_ACTION
      ("many", form, bad_at)        one step_many call of MANY[form] steps over as many buffers, form "hip" (HIP launches) | "graph"
                                    (use_graph) | "aql" (under GYMRS_AQL=1); bad_at: the buffer whose DIRTY lanes get BAD_ACTION
      ("index", bad)                set_param_index: the DIRTY lanes get BAD_INDEX, or the whole index is put back
      ("fused", which)              one fused launch, `which` of FUSED
      ("consume",)                  sync() raises InvalidActionError
      ("tune", vec, hint)           set_tuning
      ("restore",)                  a snapshot of the engine loaded into a second engine that has stepped twice; the script goes on there
      ("clone",)                    the script goes on on the engine and on its clone
      ("stats-clear",) ("set-params",) ("set-state",)
      ("table", on)                 set_param_table(None), or the rows and the index again"""
    table = needs_table(c)
    calls = [("reset",), ("step", "step", False), ("step", "step", False)]
    dirty_at = len(calls)
    if c.source in ("step", "step_host"):
        calls.append(("step", c.source, True))
    elif c.source.startswith("many-"):
        _, form, where = c.source.split("-")
        if form == "graph":  # a valid call first, so that the dirtying one replays the CACHED graph (the ring is rewritten in place)
            calls.append(("many", "graph", None))
            dirty_at = len(calls)
        calls.append(("many", form, MANY[form] - 1 if where == "last" else MANY[form] // 2 - 1))
    else:
        calls.append(("index", True))
        dirty_at = len(calls)
        calls.append(("step", "step", False) if c.source == "index-step" else ("fused", c.source))
    calls.append(("consume",))
    if c.source in TABLE_SOURCES:
        calls.append(("index", False))
    other = 8 if c.shape == 4 else 4
    calls += {"none": [], "tune-other": [("tune", other, 0)], "tune-hint": [("tune", c.shape, HINT_NONE)], "restore": [("restore",)],
              "clone": [("clone",)], "record8": [("tune", 8, 0), ("fused", "record")], "stats-clear": [("stats-clear",)],
              "set-params": [("set-params",)], "table-off-on": [("table", False), ("table", True)], "set-state": [("set-state",)]}[c.event]
    repair_at = len(calls)
    calls.append(("many", c.repair.split("-")[1], None) if c.repair.startswith("many-") else ("step", c.repair, False))
    calls += [("step", "step", False), ("step", "step", False)]
    assert table or not any(call[0] in ("index", "table") for call in calls)
    return calls, dirty_at, repair_at


class TwinTable:
    """lane_params_ref.TableReference without what these scripts never read (final observations, records): one f32 twin per
    row, every twin stepped with the same actions, lane i read from twin index[i].  One row: the twin's own statistics; more: the
    statistics rebuilt from the flags of the chosen lanes, as TableReference does.  tests/test_elided_stores_ref.py holds the two
    against each other."""

    def __init__(self, kind, flags, rows, index):
        self.kind, self.flags = kind, flags
        self.tws = [TwinEngine(lp.twin(), kind, N, row, flags=flags) for row in rows]
        self.masks = [np.asarray(index) == r for r in range(len(rows))]
        for tw in self.tws:
            tw.reset(RESET_SEED)
        self.state = self.tws[0].get_state()  # (the reset draws do not depend on the physics)
        self.reward, self.done, self.truncated = self.tws[0].get_result()
        self.stats = np.zeros(4)
        self.tick, self.t = 1, 0
        self.ep_start = np.full(N, 1, np.int64)

    def _pick(self, per_twin):
        out = per_twin[0]
        for m, x in zip(self.masks[1:], per_twin[1:]):
            out[..., m] = x[..., m]
        return out

    def step(self, act):
        for tw in self.tws:
            tw.step(act)
        results = [tw.get_result() for tw in self.tws]
        self.state = self._pick([tw.get_state() for tw in self.tws])
        self.reward, self.done, self.truncated = (self._pick([res[j] for res in results]) for j in range(3))
        self.tick += 1
        self.t += 1
        if len(self.tws) == 1:
            self.stats = self.tws[0].stats()
            return
        self.stats[3] += N
        if (self.flags & A) and (self.flags & S):
            ended = (self.done | self.truncated) != 0
            length = (self.tick - self.ep_start[ended]).sum()
            self.stats[0] += length if self.kind == 0 else -length
            self.stats[1] += length
            self.stats[2] += ended.sum()
            self.ep_start[ended] = self.tick

    def stats_clear(self):
        for tw in self.tws:
            tw.stats_clear()
        self.stats = np.zeros(4)

    def set_state(self, st):
        for tw in self.tws:
            tw.set_state(st)
        self.state = st


class Reference:
    """What the engine of a case holds after each call of its script.  actions(call) gives what the engine is to be fed for a
    "step" (one array) or a "many" call (one array per buffer); apply(call) advances the reference and returns the expected
    state, reward, done, truncated, stats, tick -- and `launches`, one (kind, lanes per work-item, paid) per kernel launch of
    the call, paid[i] = lane i was stepped and paid the constant (RewardProtocol's input)."""

    def __init__(self, c):
        self.c = c
        self.kind, self.flags, _ = ENGINES[c.engine]
        self.table = needs_table(c)
        self.rows, self.index = rows_of(c.engine, self.table), index_of(c.engine, self.table)
        self.vec = c.shape
        self.rejected = ()
        self.r = None

    def _reset(self):
        self.r = TwinTable(self.kind, self.flags, self.rows, self.index)

    def actions(self, call):
        if call[0] == "step":
            a = _fill(self.kind, ACTION_SEED, self.r.t).copy()
            if call[2]:
                a[list(DIRTY)] = BAD_ACTION
            return a
        assert call[0] == "many"
        ring = np.stack([_fill(self.kind, RING_SEED, b) for b in range(MANY[call[1]])])
        if call[2] is not None:
            ring[call[2], list(DIRTY)] = BAD_ACTION
        return ring

    def fused_actions(self, which):
        """the random policy's actions of a fused launch that draws them itself (action_seed = ACTION_SEED, action_t0 = r.t)"""
        return np.stack([_fill(self.kind, ACTION_SEED, self.r.t + j) for j in range(FUSED_STEPS.get(which, 1))])

    def _step(self, act, kind, vec, launches):
        act = np.array(act, np.uint8)
        act[list(self.rejected)] = BAD_ACTION  # a lane whose index is outside the table is treated like one with an invalid action
        self.r.step(act)
        launches.append((kind, vec, act < (2 if self.kind == 0 else 3)))

    def apply(self, call, actions=None):
        """actions: for a closed-loop "fused" call, the actions its policy takes ([steps][N]); default: the random policy's"""
        name, launches = call[0], []
        if name == "reset":
            self._reset()
        elif name == "step":
            self._step(self.actions(call), "step", self.vec, launches)
        elif name == "many":
            for act in self.actions(call):
                self._step(act, "step", self.vec, launches)
        elif name == "index":
            self.rejected = DIRTY if call[1] else ()
        elif name == "fused":
            vec = 4 if call[1] in ("record", "cl-record", "transitions") else self.vec  # a recording kernel exists at 4 lanes only
            for act in (self.fused_actions(call[1]) if actions is None else actions):
                self._step(act, "fused", vec, launches)
        elif name == "tune":
            self.vec = call[1]
        elif name == "stats-clear":
            self.r.stats_clear()
        elif name == "set-params":
            for tw, row in zip(self.r.tws, self.rows):
                tw.set_params(changed_row(self.kind, row))
        elif name == "set-state":
            self.r.set_state(self.new_state())
        else:
            assert name in ("consume", "restore", "clone", "table"), call
        r = self.r
        return SimpleNamespace(state=r.state, reward=r.reward, done=r.done, truncated=r.truncated, stats=r.stats.copy(), tick=r.tick,
                               launches=launches)

    def new_state(self):
        """the set-state event: every lane takes the state of the lane seven to its left"""
        return np.ascontiguousarray(np.roll(self.r.state, 7, axis=1))


@functools.lru_cache(maxsize=None)
def expected(c):
    """[what Reference.apply returned after each call of the case's script], computed once (closed-loop launches with the random
    policy's actions: which valid action a lane takes does not matter to its reward)"""
    ref = Reference(c)
    return [ref.apply(call) for call in calls_of(c)[0]]


# ---- the reward protocol ----------------------------------------------------------------------------------------------------------
class RewardProtocol:
    """Which lanes of `reward` hold the constant, by the protocol of step_block_loaded and the host: a word per wavefront
    ("this wave's part holds the constant"), the launch shape the words were written with, and four clearing points -- "reset"
    (gymrs_reset), "load" (gymrs_snapshot_load), "shape" (prepare_wave_flags on a launch of another shape) and "fused" (a fused
    launch under a table, which stores every reward and may have paid 0).  `off` names the clearing points to leave out."""
    POINTS = ("reset", "load", "shape", "fused")

    def __init__(self, n, off=()):
        assert set(off) <= set(self.POINTS)
        self.n, self.off, self.words, self.shape, self.holds = n, frozenset(off), set(), 0, np.zeros(n, bool)

    def _clear(self, point):
        if point not in self.off:
            self.words = set()
        if point != "shape":
            self.shape = 0

    def reset(self):
        self.holds = np.zeros(self.n, bool)  # reset_kernel writes 0.0
        self._clear("reset")

    def load(self, blob):
        self.holds = blob.holds.copy()
        self._clear("load")

    def clone(self):
        new = RewardProtocol(self.n, self.off)  # a fresh engine: its words are clear
        new.holds = self.holds.copy()
        return new

    def _launch_shape(self, vec):
        if self.shape != vec:
            if self.shape != 0:
                self._clear("shape")
            self.shape = vec

    def step(self, vec, paid):
        self._launch_shape(vec)
        for w, first in enumerate(range(0, self.n, 64 * vec)):
            lanes = slice(first, first + 64 * vec)
            const = bool(paid[lanes].all())
            if not (w in self.words and const):
                self.holds[lanes] = paid[lanes]
            (self.words.add if const else self.words.discard)(w)

    def fused(self, vec, paid, table):
        self._launch_shape(vec)
        self.holds = paid.copy()
        if table:
            self._clear("fused")


def predicted_rewards(c, off=()):
    """The reward array RewardProtocol predicts after each call of the case's script ([calls][N] f32)"""
    table = needs_table(c)
    models = [RewardProtocol(N, off)]
    out = []
    for call, exp in zip(calls_of(c)[0], expected(c)):
        if call[0] == "reset":
            for m in models:
                m.reset()
        elif call[0] == "restore":
            other = RewardProtocol(N, off)
            other.reset()
            for _ in range(2):
                other.step(c.shape, np.ones(N, bool))
            other.load(models[0])
            models = [other]
        elif call[0] == "clone":
            models.append(models[0].clone())
        for kind, vec, paid in exp.launches:
            for m in models:
                m.step(vec, paid) if kind == "step" else m.fused(vec, paid, table)
        assert all(np.array_equal(m.holds, models[0].holds) for m in models)
        out.append(np.where(models[0].holds, np.float32(CONST[ENGINES[c.engine][0]]), np.float32(0)))
    return out


# ---- Pendulum's uniform `truncated` value ----------------------------------------------------------------------------------------
class PendulumRow(C.Structure):
    """gymrs_pendulum_params (include/gymrs_amd.h), restated; tests/test_gpu_elided_stores.py pins it against the library's"""
    _fields_ = [(f, C.c_double) for f in ("max_speed", "max_torque", "dt", "g", "m", "l")] + [("max_episode_steps", C.c_uint32), ("_pad", C.c_uint32)]


def pendulum_row(limit):
    src = Oracle().pendulum_params()
    row = PendulumRow()
    for f, _ in type(src)._fields_:
        setattr(row, f, getattr(src, f))
    row.max_episode_steps = limit
    return row


P_LIMIT, P_NEW_LIMIT, P_STEPS = 3, 5, 12
P_FLAGS = (T, A | T, A | S | T)
P_MANY = {"hip": 4, "aql": 8}  # (use_graph is refused for Pendulum with the time limit)
P_EVENTS = ("tune", "clone", "restore", "rollout-1", "rollout-2", "rollout-3", "many-hip", "many-aql", "set-limit")
PCase = namedtuple("PCase", "flags shape event after")  # after: the event sits "after" a truncating step or "before" one


def pendulum_cases():
    return [PCase(f, shape, e, after) for f in P_FLAGS for shape in SHAPES for e in P_EVENTS for after in (True, False)]


def pendulum_id(c):
    return "-".join(("pd", "".join(n for n, b in (("A", A), ("S", S), ("T", T)) if c.flags & b), str(c.shape), c.event,
                     "after" if c.after else "before"))


def pendulum_calls(c):
    """reset, steps up to the event, the event, steps on until P_STEPS steps are taken and three follow the event.  With
    auto-reset the episodes of limit 3 end at steps 3, 6, 9, ..: the event sits after step 3 (the array holds 1) or after step 5
    (it holds 0 and step 6 truncates).  Without auto-reset nothing re-arms the clock, every step from the third on truncates:
    after step 3, or after step 2.  Returns (calls, position of the event)."""
    at = 3 if c.after else (5 if c.flags & A else 2)
    calls = [("reset",)] + [("step",)] * at
    event_at = len(calls)
    if c.event == "tune":
        calls.append(("tune", 8 if c.shape == 4 else 4))
    elif c.event.startswith("rollout-"):
        calls.append(("rollout", int(c.event[-1])))
    elif c.event.startswith("many-"):
        calls.append(("many", c.event[5:]))
    else:
        calls.append((c.event,))
    taken = at + {"rollout": lambda: calls[-1][1], "many": lambda: P_MANY[calls[-1][1]]}.get(calls[-1][0], lambda: 0)()
    calls += [("step",)] * max(3, P_STEPS - taken)
    return calls, event_at


def other_steps_before_restore(c):
    """How many steps the engine a snapshot is loaded into takes first, so that ITS `truncated` array holds the opposite uniform
    value from the blob's: the blob's holds 1 after a truncating step (one step leaves 0), else 0 (three steps leave 1)."""
    return 1 if c.after else P_LIMIT


class PendulumReference:
    """One f32 twin; actions(call) gives the f32 actions of a "step" ([N]) or "many" ([steps][N]) call, apply(call) the expected
    arrays after it and `truncated_steps`, the uniform truncated value of every step the call took."""

    def __init__(self, c):
        self.c, self.t = c, 0
        self.tw = TwinEngine(lp.twin(), 2, N, pendulum_row(P_LIMIT), flags=c.flags)

    def _fill(self, seed, t):
        return self.tw.fill_actions(seed, t)

    def actions(self, call):
        if call[0] == "step":
            return self._fill(ACTION_SEED, self.t)
        return np.stack([self._fill(RING_SEED, b) for b in range(P_MANY[call[1]])])

    def apply(self, call):
        took = []
        if call[0] == "reset":
            self.tw.reset(RESET_SEED)
            self.t = 0
        elif call[0] in ("step", "many"):
            acts = self.actions(call)
            took = [acts] if call[0] == "step" else list(acts)
        elif call[0] == "rollout":  # the fused launch draws fill_actions(ACTION_SEED, action_t0 + j) itself
            took = [self._fill(ACTION_SEED, self.t + j) for j in range(call[1])]
        elif call[0] == "set-limit":
            self.tw.set_params(pendulum_row(P_NEW_LIMIT))
        else:
            assert call[0] in ("tune", "clone", "restore"), call
        flags = []
        for a in took:
            self.tw.step(a)
            self.t += 1
            tr = self.tw.get_result()[2]
            assert (tr == tr[0]).all()  # one shared episode clock
            flags.append(int(tr[0]))
        reward, done, trunc = self.tw.get_result()
        return SimpleNamespace(state=self.tw.get_state(), obs=self.tw.get_obs(), reward=reward, done=done, truncated=trunc, stats=self.tw.stats(),
                               tick=self.tw.tick(), truncated_steps=flags)


def truncating_steps(c, total):
    """Written down independently of the twin: the 1-based steps of a case that truncate.  The clock starts at step 1 and, with
    auto-reset, again after every truncating step; set-limit changes the limit from the step after the event on."""
    calls, event_at = pendulum_calls(c)
    change = sum(1 for call in calls[:event_at] if call[0] == "step") if c.event == "set-limit" else None
    out, start = [], 1
    for s in range(1, total + 1):
        limit = P_NEW_LIMIT if change is not None and s > change else P_LIMIT
        if s - start + 1 >= limit:
            out.append(s)
            if c.flags & A:
                start = s + 1
    return out
