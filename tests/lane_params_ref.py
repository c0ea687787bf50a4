"""An engine with a per-lane parameter table (gymrs_set_param_table) computed on the CPU alone.

Lanes are independent: the reset draws and the random-policy actions are keyed by global lane id and tick, never by the physics.
So lane i of a table engine is lane i of a uniform engine whose params are rows[index[i]].  The reference keeps one f32 twin
(oracle.bindings.TwinEngine) per row, all of them over the same n lanes, steps every one of them with the same actions, and
reads lane i from twin index[i].  The statistics are not the twins' (each twin counts lanes of every row): they are rebuilt from
the done | truncated flags of the chosen lanes with a per-lane episode start, the return being +length (CartPole) or -length
(MountainCar), as the constant rewards give.

This module never imports the library: what it returns is the yardstick of tests/test_gpu_lane_params_paths.py, and
tests/test_lane_params_ref.py shows without a GPU that the yardstick is sound and that its cases are worth comparing with.

A plain module like closed_loop_ref.py, imported by test files; no fixtures, no pytest hooks."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
from closed_loop_ref import A, DIMS, F, FLAG_SETS, S, T, bits, final_obs_after  # noqa: F401  (re-exported to the test files)

from oracle.bindings import Oracle, Twin, TwinEngine

_twin = None
_oracle = None


def twin():
    global _twin
    if _twin is None:
        _twin = Twin()
    return _twin


# ---- parameter rows -------------------------------------------------------------------------------------------------------------
# The layout of gymrs_cartpole_params / gymrs_mountain_car_params (include/gymrs_amd.h), restated: the twin reads a row through
# a pointer, and a test hands the same bytes to the engine (rows_for).  tests/test_lane_params_ref.py pins the layout and the
# defaults against the library's own default_params.
class CartPoleRow(C.Structure):
    _fields_ = [(f, C.c_double) for f in ("gravity", "masscart", "masspole", "length", "force_mag", "tau", "theta_threshold_radians",
                                          "x_threshold")] + [("kinematics_integrator", C.c_int32), ("max_episode_steps", C.c_uint32)]


class MountainCarRow(C.Structure):
    _fields_ = [(f, C.c_double) for f in ("min_position", "max_position", "max_speed", "goal_position", "goal_velocity", "force",
                                          "gravity")] + [("max_episode_steps", C.c_uint32), ("_pad", C.c_uint32)]


ROW = {0: CartPoleRow, 1: MountainCarRow}
SCALED = {0: ("gravity", "masscart", "masspole", "length", "force_mag", "tau", "theta_threshold_radians", "x_threshold"),
          1: ("force", "gravity", "max_speed", "goal_position")}
LOW_GOAL = -0.45  # MountainCar resets into [-0.6, -0.4]: a random policy reaches this goal, never the default one


def default_row(kind, max_steps, integrator=0):
    """The reference's default constants (from the f64 oracle's restatement of them) as a row"""
    global _oracle
    if _oracle is None:
        _oracle = Oracle()
    src = _oracle.cartpole_params() if kind == 0 else _oracle.mountain_car_params()
    row = ROW[kind]()
    for f, t in type(src)._fields_:
        if t is C.c_double:
            setattr(row, f, getattr(src, f))
    row.max_episode_steps = max_steps
    if kind == 0:
        row.kinematics_integrator = integrator
    return row


def make_rows(kind, k, seed, max_steps, integrator=0):
    """k rows, seeded.  CartPole: the eight physics fields scaled by uniform(0.5, 1.5).  MountainCar: force, gravity, max_speed and
    goal_position scaled likewise; every other row (1, 3, ...) has goal_position = LOW_GOAL, rows 2, 3 of every four
    goal_velocity = -1.0 (else 0), rows 1 of every three min_position = -0.9 (else -1.2) and rows 2 of every three
    max_position = 0.3 (else 0.6): five rows vary all seven fields.  max_episode_steps and kinematics_integrator are shared."""
    rng = np.random.default_rng(seed)
    rows = []
    for r in range(k):
        row = default_row(kind, max_steps, integrator)
        for f in SCALED[kind]:
            setattr(row, f, getattr(row, f) * float(rng.uniform(0.5, 1.5)))
        if kind == 1:
            if r % 2 == 1:
                row.goal_position = LOW_GOAL
            row.goal_velocity = -1.0 if r % 4 >= 2 else 0.0
            row.min_position = -0.9 if r % 3 == 1 else -1.2
            row.max_position = 0.3 if r % 3 == 2 else 0.6
        rows.append(row)
    return rows


def low_goal_rows(kind, rows):
    """MountainCar: the rows whose goal a random policy reaches"""
    return [r for r, row in enumerate(rows) if kind == 1 and row.goal_position == LOW_GOAL]


def rows_for(params_type, rows):
    """The same bytes as the library's own params type (set_param_table insists on it)"""
    return [params_type.from_buffer_copy(bytes(r)) for r in rows]


def make_index(n, k, seed):
    return np.random.default_rng(seed).integers(0, k, n).astype(np.uint16)


def fill_actions(kind, n, gid0, seed, t):
    """gymrs_fill_actions(seed, t) for lanes gid0 .. gid0 + n of the batch"""
    return TwinEngine(twin(), kind, n, default_row(kind, 0), gid0=gid0).fill_actions(seed, t)


# ---- the reference ----------------------------------------------------------------------------------------------------------------
class TableReference:
    """n lanes at global offset gid0, lane i with rows[index[i]], after reset(reset_seed).

    actions(t, obs) -> uint8[n] gives the actions of step t (counted from 0 since the reset) for the current observations
    `obs`; the default is the random policy fill_actions(action_seed, t).  prepare(state) (optional) returns the start state to
    use in place of the reset state; the caller applies the same function to the engine.  tick0 (default 1: the tick a reset
    leaves) is the engine tick the first step starts from: tick0 - 1 is the shift of tests/time_shift.py.  bounds (default None: the
    env's own box) is the `options` of the reset, lows then highs: every re-arm draws from it too.

    After any number of step() calls the attributes are what the engine's getters return:
      state, obs, reward, done, truncated, tick (counts the reset and every step)
      stats     [sum_return, sum_length, n_episodes, steps], counted with A | S only (steps always), as the twin and the engine do
      final     the final-observation rows: zero after reset; with auto-reset a lane whose step ended an episode takes the
                observation a flags = 0 twin with its row shows after the same step from the same state (the rule
                closed_loop_ref.reference documents)
    records [steps] keeps obs, actions, reward, done, truncated of every step (what a recording rollout writes) and
    ended_by[2][K] counts per row the lanes that terminated / were truncated."""

    def __init__(self, kind, n, gid0, rows, index, flags, reset_seed, action_seed=0, actions=None, prepare=None, tick0=1, bounds=None):
        assert len(rows) >= 1 and all(r.max_episode_steps == rows[0].max_episode_steps for r in rows)
        self.kind, self.n, self.gid0, self.rows, self.flags = kind, n, gid0, list(rows), flags
        self.index = np.array(index, np.int64)
        assert self.index.shape == (n,) and self.index.min() >= 0 and self.index.max() < len(rows)
        self.actions = actions if actions is not None else (lambda t, obs: self.tws[0].fill_actions(action_seed, t))
        self.tws = [TwinEngine(twin(), kind, n, row, flags=flags & ~F, gid0=gid0) for row in rows]
        self.tws0 = [TwinEngine(twin(), kind, n, row, flags=0) for row in rows]
        for tw in self.tws:
            tw.reset(reset_seed, bounds)
        if prepare is not None:
            start = prepare(self.tws[0].get_state())
            for tw in self.tws:
                tw.set_state(start)
        if tick0 != 1:  # the batch as time_shift.shift_engine(eng, tick0 - 1) leaves an engine right after its reset
            for tw in self.tws:
                tw.shift_time(tick0 - 1)
        d = TwinEngine._OBS_DIM[kind]  # (Pendulum, which takes no table, runs here as one row: its observation is not its state)
        self.reset_seed, self.bounds = reset_seed, bounds
        self.state = self.tws[0].get_state()  # (the reset draws do not depend on the physics: every twin holds the same)
        self.obs = self.tws[0].get_obs()
        self.reward = np.zeros(n, np.float32)
        self.done = np.zeros(n, np.uint8)
        self.truncated = np.zeros(n, np.uint8)
        self.final = np.zeros((d, n), np.float32)
        self.stats = np.zeros(4)
        if tick0 != 1 and (flags & A) and (flags & S):  # every lane's finished history grew by the shift
            self.stats[1] = n * (tick0 - 1)
            self.stats[0] = self.stats[1] if kind == 0 else -self.stats[1]
        self.tick = tick0
        self.t = 0
        self.ep_start = np.full(n, tick0, np.int64)
        self.records = []
        self.ended_by = np.zeros((2, len(rows)), np.int64)

    def _gather(self, per_twin, index=None):
        """lane i from per_twin[index[i]]"""
        index = self.index if index is None else index
        out = np.empty_like(per_twin[0])
        for r, x in enumerate(per_twin):
            m = index == r
            out[..., m] = x[..., m]
        return out

    def state_under(self, row_of_lane):
        """The state every lane would have now had it stepped with row row_of_lane[i] all along (the twins are all there)"""
        return self._gather([tw.get_state() for tw in self.tws], np.asarray(row_of_lane, np.int64))

    def rehome(self):
        """Every twin takes every lane as its own twin (index[i]) holds it: state, episode clock and CartPole's
        steps_beyond_terminated (TwinEngine.get_clocks).  After it a lane may go on under any row."""
        clocks = [tw.get_clocks() for tw in self.tws]
        start, beyond = (self._gather([c[j] for c in clocks]) for j in range(2))
        for tw in self.tws:
            tw.set_state(self.state)
            tw.set_clocks(start, beyond)

    def set_index(self, index):
        """The index rewritten between two steps: every lane goes on from its own state, episode clock and
        steps_beyond_terminated with its new row (under every flag set: rehome)."""
        self.rehome()
        self.index = np.array(index, np.int64)
        assert self.index.shape == (self.n,) and self.index.min() >= 0 and self.index.max() < len(self.rows)

    def set_rows(self, rows, index=None):
        """As many other rows (gymrs_set_params / gymrs_set_param_table between two steps: only the constants change), and
        optionally another index with them"""
        assert len(rows) == len(self.rows) and all(r.max_episode_steps == rows[0].max_episode_steps for r in rows)
        self.set_index(self.index if index is None else index)
        self.rows = list(rows)
        for tw, tw0, row in zip(self.tws, self.tws0, self.rows):
            tw.set_params(row)
            tw0.set_params(row)

    def set_state(self, state):
        """gymrs_set_state of every lane: the state and nothing else (clocks, flags and final observations stay)"""
        for tw in self.tws:
            tw.set_state(state)
        self.state = self.tws[0].get_state()
        self.obs = self.tws[0].get_obs()

    def stats_clear(self):
        """gymrs_stats_clear: the totals so far become the baseline; open episodes go on and count in full when they end"""
        for tw in self.tws:
            tw.stats_clear()
        self.stats = np.zeros(4)

    def rebox(self, bounds):
        """The same engine with another box for its coming re-arms (what a clone that lost the box would be): twins reset with
        the box and put back to this tick, these states and these clocks.  CartPole / MountainCar (Pendulum's twin keeps a
        return per lane that cannot be put back)."""
        assert self.kind != 2
        self.rehome()
        clocks = self.tws[0].get_clocks()
        for tw in self.tws:
            tw.reset(self.reset_seed, bounds)
            if self.tick != 1:
                tw.shift_time(self.tick - 1)
            tw.set_state(self.state)
            tw.set_clocks(*clocks)
        self.bounds = bounds

    def step(self, count=1):
        for _ in range(count):
            act = np.ascontiguousarray(self.actions(self.t, self.obs), np.float32 if self.kind == 2 else np.uint8)
            assert act.shape == (self.n,)
            finals = []
            results = []
            for tw, tw0 in zip(self.tws, self.tws0):
                if self.flags & A:  # (the engine keeps final observations only with auto-reset)
                    finals.append(final_obs_after(tw0, tw.get_state(), act))
                tw.step(act)
                results.append(tw.get_result())
            self.state = self._gather([tw.get_state() for tw in self.tws])
            self.obs = self._gather([tw.get_obs() for tw in self.tws])
            self.reward, self.done, self.truncated = (self._gather([res[j] for res in results]) for j in range(3))
            self.tick += 1
            self.t += 1
            ended = (self.done | self.truncated) != 0
            if self.flags & A:
                self.final[:, ended] = self._gather(finals)[:, ended]
            self.stats[3] += self.n
            if self.kind == 2:  # one row: the twin's own statistics (a float sum of rewards, not a length)
                self.stats = self.tws[0].stats()
            elif (self.flags & A) and (self.flags & S):
                length = (self.tick - self.ep_start[ended]).sum()
                self.stats[0] += length if self.kind == 0 else -length
                self.stats[1] += length
                self.stats[2] += ended.sum()
            if self.flags & A:
                self.ep_start[ended] = self.tick
            self.ended_by[0] += np.bincount(self.index[self.done != 0], minlength=len(self.rows))
            self.ended_by[1] += np.bincount(self.index[self.truncated != 0], minlength=len(self.rows))
            self.records.append(SimpleNamespace(obs=self.obs, actions=act, reward=self.reward, done=self.done, truncated=self.truncated))
        return self

    def told_apart(self, other_row):
        """Of the lanes whose row is not other_row[i]: the fraction whose state now differs bitwise from the state they would
        have under other_row[i].  Near 1: a kernel that stepped lanes with that other row could not pass a comparison here."""
        other_row = np.asarray(other_row, np.int64)
        m = self.index != other_row
        differs = (bits(self.state) != bits(self.state_under(other_row))).any(axis=0)
        return differs[m].mean() if m.any() else 1.0


# ---- the cases of tests/test_gpu_lane_params_paths.py (checked without a GPU by tests/test_lane_params_ref.py) --------------------
N, K, MAX_EPISODE_STEPS = 3001, 5, 17
OFFSETS = (12345, 4096)  # not a multiple of 4: the rollout evaluates every lane's own action block; a multiple: one block per four lanes
ROWS_SEED, INDEX_SEED, RESET_SEED, ACTION_SEED, RING_SEED = 31, 32, 3, 6, 7
RING = 4  # action buffers of step_many
# The stages one engine of the path matrix runs in order, (name, steps): compared after each.  step_many walks its ring of RING
# buffers from buffer 0 in every call; five steps wrap it.  The totals compared at (3, 4, 9, 14, 19, 26, 38, 39) avoid the
# multiples of MAX_EPISODE_STEPS: right after a limit every lane that just reached it holds a fresh reset draw, the same under
# every row, and a wrong row would show in fewer lanes.
STAGES = (("step", 3), ("step_host", 1), ("step_many", 5), ("step_many graph", 5), ("step_many graph", 5), ("rollout", 7),
          ("rollout", 12), ("step", 1))
INTEGRATOR_1_FLAGS = (A | S | T, A | S | T | F)  # CartPole, kinematics_integrator = 1
TOLD_APART = 0.9  # the least fraction of lanes a wrong row must show in, at every compared point


RECORD_STAGES = (("step", 3), ("rollout_record", 23))  # the recording kernel (4 lanes per work-item only)


def matrix_actions(kind, n, gid0, stages=STAGES):
    """The action stream of a run through `stages`: step t of a step_many stage takes ring buffer (steps into the stage) % RING,
    every other step the random policy's fill_actions(ACTION_SEED, t) (which the fused rollout generates itself from
    action_t0 = t).  Returns (callback for TableReference, ring [RING][n])."""
    ring = np.stack([fill_actions(kind, n, gid0, RING_SEED, b) for b in range(RING)])
    source = []
    for name, steps in stages:
        source += [k % RING if name.startswith("step_many") else None for k in range(steps)]

    def actions(t, obs):
        return fill_actions(kind, n, gid0, ACTION_SEED, t) if t >= len(source) or source[t] is None else ring[source[t]]
    return actions, ring


def matrix_case(kind, flags, gid0, integrator=0, stages=STAGES, max_steps=MAX_EPISODE_STEPS):
    rows = make_rows(kind, K, ROWS_SEED + kind, max_steps, integrator)
    index = make_index(N, K, INDEX_SEED + kind)
    actions, ring = matrix_actions(kind, N, gid0, stages)
    return SimpleNamespace(kind=kind, n=N, gid0=gid0, flags=flags, rows=rows, index=index, actions=actions, ring=ring, stages=stages)


def matrix_reference(c, prepare=None):
    return TableReference(c.kind, c.n, c.gid0, c.rows, c.index, c.flags, RESET_SEED, actions=c.actions, prepare=prepare)


# The cases beside the matrix
ELISION_LIMIT, ELISION_STEPS = 23, 70  # CartPole, A | S | T: launches that cannot reach the limit, then launches that can
REWRITE_STEPS, REWRITE_FLAGS = (9, 11), (A | S, A | S | F)  # rollout, index rewritten, rollout
POLICY = SimpleNamespace(seed=5, n_policies=2, lanes_per_policy=100, steps=20, flags=A | S | T | F)  # policy_actions + step


def elision_case():
    return matrix_case(0, A | S | T, OFFSETS[0], stages=(("step", ELISION_STEPS),), max_steps=ELISION_LIMIT)


def rewritten_index(kind):
    return make_index(N, K, INDEX_SEED + 10 + kind)


def policy_reference(kind):
    """(reference, weights) of the policy x table case: the actions are closed_loop_ref.policy_ref's (plain C), affine policies"""
    import closed_loop_ref
    w = closed_loop_ref.make_weights(kind, 0, POLICY.n_policies, seed=POLICY.seed)
    c = matrix_case(kind, POLICY.flags, OFFSETS[0], stages=())
    r = TableReference(kind, c.n, c.gid0, c.rows, c.index, c.flags, RESET_SEED,
                       actions=lambda t, obs: closed_loop_ref.policy_ref(kind, 0, w, POLICY.lanes_per_policy, c.gid0, obs))
    return c, r, w


# Slow-path start states: every 7th lane (of every row, the index being random) leaves the straight-line code.  CartPole: the
# angles and non-finite states of tests/test_gpu_slowpaths.py (f32 and f64 Cody-Waite, Payne-Hanek, NaN, inf); MountainCar: its
# long reductions, non-finite states and the walls of both settings of min_position / max_position.
CARTPOLE_SLOW = [(2, 1.0), (2, -3.0), (2, 199.0), (2, -201.0), (2, 1e4), (2, -4e8), (2, 1e30), (0, np.nan), (2, np.nan), (0, np.inf),
                 (0, -np.inf), (2, np.inf), (2, -np.inf), (1, np.nan), (3, np.inf)]
MOUNTAIN_CAR_SLOW = [(0, 70.0), (0, -1e6), (0, 4e8), (0, np.nan), (1, np.nan), (0, np.inf), (0, -np.inf), (1, np.inf), (1, -np.inf),
                     (0, -1.2), (0, -0.9), (0, 0.6), (0, 0.3), (0, -0.9000001), (0, 0.29999998)]


def slow_prepare(kind):
    special = CARTPOLE_SLOW if kind == 0 else MOUNTAIN_CAR_SLOW

    def prepare(state):
        state = state.copy()
        for j, lane in enumerate(range(3, state.shape[1], 7)):
            comp, value = special[j % len(special)]
            state[comp, lane] = value
        return state
    return prepare


def beyond_range(kind, state):
    """The lanes whose state is outside the fast path's range (Env::kRangeMax in gym-rs_amd/csrc/gymrs_tile.h: CartPole
    |theta| <= fl32(pi / 4), MountainCar |3 * position| <= 200; a NaN is outside)"""
    with np.errstate(invalid="ignore"):
        if kind == 0:
            return ~(np.abs(state[2]) <= np.float32(0.7853982))
        return ~(np.abs(np.float32(3.0) * state[0]) <= np.float32(200.0))
