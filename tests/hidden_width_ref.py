"""Hidden widths 1, 7 and 64 in every stochastic and recording kernel: the cases of tests/test_gpu_hidden_widths.py, CPU only.

The hidden layer of a policy is evaluated four units per trip (one per trip in the gathered copies) with a remainder loop, in every
kernel that inlines it, and twice in the text: policy_eval (argmax) and policy_logits (sampling).  The other case tables meet the
exploring, sampling, recording and transitions kernels with H = 0 and 8 only.  This one puts H = 1 (no full trip), 7 (one trip and
a remainder of three) and 64 (sixteen trips, the widest set, the largest stride into the weight table) on every family instance --
(family, env, with or without a parameter table, lanes per work-item) -- and keeps, per case, a seed of
closed_loop_ref.make_weights (and a temperature) for which the case would notice a kernel that dropped the last units:
worth_comparing says what that takes, tests/test_hidden_width_ref.py asserts it without a GPU.

Nothing new computes an answer here: the references are explore_ref.Run, sample_ref.Run, transitions_ref.Run,
sample_ref.TransitionsRun, sample_ref.sample_actions, closed_loop_ref.policy_ref and policy_eval_ref / policy_eval_table_ref, which
are generic in H.  This module never loads the library.

A plain module like explore_ref.py, imported by test files; no fixtures, no pytest hooks."""
from types import SimpleNamespace

import closed_loop_ref as cl
import closed_loop_table_ref as clt
import explore_ref as ex
import lane_params_ref as lp
import numpy as np
import policy_eval_ref as ev
import policy_eval_table_ref as tb
import policy_fitness_ref as pf
import sample_ref as sr
import transitions_ref as tr
from closed_loop_ref import A, COPIES, DIMS, F, FLAG_SETS, T, bits

WIDTHS = (1, 7, 64)
EVAL_WIDTHS = (1, 64)  # policy_eval_ref.HIDDEN has 7
# group -> its families.  A flag set belongs to an engine, and a test runs its instance's widths on one engine, so a family of four or
# eight instances cannot meet all ten sets.  The sets rotate with the instance number inside a group: every flag set meets every
# width in every group; a closed family misses two sets; the recording and transitions families take every third set, so each of them
# meets sets with and without the time limit, the statistics and the final observations, and sample_transitions takes the four
# sets that transitions_policy leaves.
GROUPS = {"closed": ("explore", "explore_fitness", "sample", "sample_fitness"),  # explore_ref.N lanes, 4 and 8 lanes per work-item
          "record": ("record_policy", "record_explore", "record_sample"),  # rollout_closed_loop with a record: transitions_ref.SHAPES
          "transitions": ("transitions_policy", "transitions_explore", "sample_transitions"),  # rollout_transitions: the same shapes
          "step": ("explore_actions", "sample_actions"),  # one per-step call, no table
          "eval": ("evaluate_policy",)}  # policy_eval_ref's shapes, widths 1 and 64
SOURCE = {"explore": "explore", "explore_fitness": "explore", "sample": "sample", "sample_fitness": "sample", "record_policy": "policy",
          "record_explore": "explore", "record_sample": "sample", "transitions_policy": "policy", "transitions_explore": "explore",
          "sample_transitions": "sample", "explore_actions": "explore", "sample_actions": "sample", "evaluate_policy": "policy"}
MAX_EPISODE_STEPS = cl.MAX_EPISODE_STEPS
RESET_SEED = cl.RESET_SEED
N_POLICIES = cl.N_POLICIES
SPECIAL_SEED = 5  # of the special-value observations, as tests/test_gpu_policy.py draws them
ENV = ("cartpole", "mountain_car")


def instances(group):
    """The family instances of a group, numbered inside it: SimpleNamespace(group, family, kind, table, vec, number, flags and
    gid0 (closed, step) or shape (record, transitions: an index into transitions_ref.SHAPES; eval: into policy_eval_ref.SHAPES))."""
    out = []
    for f, family in enumerate(GROUPS[group]):
        if group == "closed":
            axes = [(kind, table, vec) for kind in (0, 1) for table in (False, True) for vec in (4, 8)]
        elif group == "step":
            axes = [(kind, False, vec) for kind in (0, 1) for vec in (4, 8)]
        else:
            axes = [(kind, table, 4) for kind in (0, 1) for table in (False, True)]
        if group == "eval":
            axes = [a + (shape,) for a in axes for shape in (0, 1)]
        for a in axes:
            kind, table, vec = a[:3]
            i = len(out)
            inst = SimpleNamespace(group=group, family=family, kind=kind, table=table, vec=vec, number=i, source=SOURCE[family])
            if group in ("closed", "step"):
                inst.flags, inst.gid0, inst.key = FLAG_SETS[i % len(FLAG_SETS)], ex.OFFSETS[i % 3], (family, kind, int(table), vec)
            elif group == "record":
                inst.flags, inst.shape, inst.key = FLAG_SETS[3 * i % len(FLAG_SETS)], (f + kind + table) % 2, (family, kind, int(table), 4)
            elif group == "transitions":  # the eight sets with auto-reset
                inst.flags, inst.shape, inst.key = tr.FLAG_SETS[(3 * i + 4 * (f // 2)) % 8], (f + kind + table) % 2, (family, kind, int(table), 4)
            else:  # the evaluator reads no flag
                inst.flags, inst.shape, inst.key = 0, a[3], (family, kind, int(table), a[3])
            inst.id = "-".join([family, ENV[kind], "table" if table else "plain"] + ([f"shape{inst.shape}"] if group == "eval" else [f"vec{vec}"]))
            out.append(inst)
    return out


def widths_of(inst):
    return EVAL_WIDTHS if inst.group == "eval" else WIDTHS


def remainder_zeroed(kind, hidden, weights):
    """The policy set without the units the four-unit loop leaves to its remainder: the last H % 4 (H = 64: the last trip's four)
    have their b1 entries and W2 columns zeroed, so they add +0 to every logit"""
    d, a = DIMS[kind]
    r = hidden % 4 or 4
    w = np.array(weights, np.float32).reshape(-1, cl.size_of(kind, hidden))
    b1, w2 = hidden * d, hidden * (d + 1)
    w[:, b1 + hidden - r:b1 + hidden] = 0
    for j in range(a):
        w[:, w2 + j * hidden + hidden - r:w2 + (j + 1) * hidden] = 0
    return w


def special_values(state):
    """tests/test_gpu_policy.py's non-finite observations: three elements in ten replaced by NaN, infinities, huge, zero and denormal values"""
    rng = np.random.default_rng(SPECIAL_SEED)
    st = state.copy()
    special = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, 0.0, -0.0, 1e-40], np.float32)
    mask = rng.random(st.shape) < 0.3
    st[mask] = rng.choice(special, size=int(mask.sum()))
    return st


def case(inst, hidden, seed=None, temperature=None):
    """The case of instance `inst` at width `hidden`; seed and temperature default to the SEEDS entry (the search passes its own)"""
    k = widths_of(inst).index(hidden)
    if seed is None:
        seeds, temperature = SEEDS[inst.key]
        seed = seeds[k]
    kind, table, i = inst.kind, inst.table, inst.number
    if inst.group == "eval":
        common = bool((i + k) % 2)
        if table:
            c = tb.case(kind, inst.shape, hidden, common, weight_seed=seed)
        else:
            row = lp.default_row(kind, ev.MAX_STEPS)
            c = ev.case(kind, inst.shape, hidden, common, ev.mountain_car_params(row) if kind == 1 else row, weight_seed=seed)
            c.rows, c.index = [c.params], np.zeros(c.n, np.uint16)
        c.n_policies, c.vec, c.flags, c.table = ev.N_POLICIES, 4, 0, table
        c.classes = {4: c.classes}
    else:
        if inst.group in ("closed", "step"):
            n, gid0 = ex.N, inst.gid0
            n_policies, lpp = ex.POLICY_SETS[(i + k) % 3]
            schedule, n_rows = ex.SPLITS[(i + k) % 2], ex.TABLE_ROWS
        else:
            n, _, gid0, lpp = tr.SHAPES[inst.shape]
            n_policies, schedule, n_rows = N_POLICIES, clt.SCHEDULE, tr.K
        rows = lp.make_rows(kind, n_rows, lp.ROWS_SEED + kind, MAX_EPISODE_STEPS) if table else [lp.default_row(kind, MAX_EPISODE_STEPS)]
        index = lp.make_index(n, n_rows, lp.INDEX_SEED + kind) if table else np.zeros(n, np.uint16)
        c = SimpleNamespace(kind=kind, n=n, vec=inst.vec, gid0=gid0, flags=inst.flags, table=table, rows=rows, index=index, hidden=hidden,
                            weights=cl.make_weights(kind, hidden, n_policies, seed), n_policies=n_policies, lanes_per_policy=lpp,
                            reset_seed=RESET_SEED, schedule=tuple(schedule), policies=pf.policies_of(n, gid0, lpp, n_policies),
                            prepare=(lambda state: cl.mountain_car_prepare(state, 0)) if kind == 1 else None,
                            classes={vec: cl.wave_classes(n, vec, gid0, n_policies, lpp) for vec in (4, 8)})
        if inst.source == "sample":
            c.seed, c.scale = sr.SEED, float(np.float32(sr.LOG2E / temperature))
        else:
            c.seed, c.threshold = ex.SEED, ex.THRESHOLD
        c.explore = inst.source == "explore"
    c.inst, c.group, c.family, c.source, c.weights_seed, c.temperature = inst, inst.group, inst.family, inst.source, seed, temperature
    # the copies the case's launches pick from.  The per-step calls pick as at 4 lanes per work-item whatever the engine's setting
    c.copies = c.classes[4 if inst.group == "step" else c.vec]
    return c


def without_remainder(c):
    """The same case under remainder_zeroed weights"""
    return SimpleNamespace(**{**vars(c), "weights": remainder_zeroed(c.kind, c.hidden, c.weights)})


# ---- the references -------------------------------------------------------------------------------------------------------------------
def run_rollout(c):
    """A closed, record or transitions case, launch by launch: SimpleNamespace(out = what the borrowed Run's launch returns per launch
    of c.schedule (out[0] also has start_state), and over all steps actions, greedy, explored, ended [steps][n] and before
    [steps][D][n], the observations every step's action was chosen from)"""
    if c.group == "transitions":
        run = sr.TransitionsRun(c) if c.source == "sample" else tr.Run(c)
        out = [run.launch(steps) for steps in c.schedule]
        base = run.run
    else:
        run = base = sr.Run(c) if c.source == "sample" else ex.Run(c)
        how = {"sample": lambda: (c.seed, c.scale), "explore": lambda: (c.seed, c.threshold), "policy": lambda: None}[c.source]()
        out = [run.launch(steps, how) for steps in c.schedule]
    out[0].start_state = run.start_state
    cat = lambda f: np.concatenate([getattr(x, f) for x in out])  # noqa: E731
    after = cat("rec_obs")
    return SimpleNamespace(out=out, actions=cat("rec_actions"), ended=(cat("rec_done") | cat("rec_truncated")) != 0,
                           explored=np.stack(base._explored), greedy=np.stack(base._greedy),
                           before=np.concatenate([run.start_state[None], after[:-1]]))


def run_step(c):
    """A per-step case: one call on the reset (and prepared) observations, one on special_values of them, at the tick a reset leaves:
    [SimpleNamespace(obs, actions, greedy, explored, prob (sampling) or None)]"""
    start = ex.Run(c).start_state
    gids = ex.as_u64([c.gid0 + i for i in range(c.n)])
    calls = []
    for obs in (start, special_values(start)):
        if c.source == "sample":
            act, greedy, prob, _ = sr.sample_actions(c.kind, c.hidden, c.weights, c.lanes_per_policy, c.gid0, obs, c.seed, c.scale, 1)
            explored = act != greedy
        else:
            greedy = cl.policy_ref(c.kind, c.hidden, c.weights, c.lanes_per_policy, c.gid0, obs)
            explored, random = ex.draw(c.seed, c.threshold, DIMS[c.kind][1], gids, 1)
            act, prob = np.where(explored, random, greedy).astype(np.uint8), None
        calls.append(SimpleNamespace(obs=obs, actions=act, greedy=greedy, explored=explored, prob=prob))
    return calls


def run_eval(c, index=None):
    """An evaluation case: what policy_eval_ref.reference / policy_eval_table_ref.reference return"""
    if c.table:
        return tb.run_case(c, index)
    return ev.run_case(c)


def run_case(c):
    return {"step": run_step, "eval": run_eval}.get(c.group, run_rollout)(c)


def disagree(c, obs):
    """Per lane: whether two policies of the set, each asked alone about the observations obs [..][D][n], ever choose differently"""
    d = DIMS[c.kind][0]
    flat = np.ascontiguousarray(np.moveaxis(obs.reshape(-1, d, c.n), 1, 0).reshape(d, -1))
    alone = [cl.policy_ref(c.kind, c.hidden, c.weights[p:p + 1], 1, 0, flat).reshape(-1, c.n) for p in range(c.n_policies)]
    return np.any([(x != alone[0]).any(axis=0) for x in alone[1:]], axis=0) if c.n_policies > 1 else np.zeros(c.n, bool)


def remainder_shows(c, ref, zeroed):
    """{copy: how many entries differ between ref = run_case(c) and zeroed = run_case(without_remainder(c))}: recorded actions of a
    rollout (lane-steps), actions of explore_actions, `prob` words of sample_actions (the call on the reset observations), lengths
    of an evaluation.  No entry may be zero: a kernel that dropped the last units would compute `zeroed` and still pass."""
    if c.group == "eval":
        changed = ref.lengths != zeroed.lengths
    elif c.group == "step":
        changed = (ref[0].actions != zeroed[0].actions) if c.source == "explore" else (bits(ref[0].prob) != bits(zeroed[0].prob))
    else:
        changed = ref.actions != zeroed.actions
    return {COPIES[k]: int(changed[..., c.copies == k].sum()) for k in np.unique(c.copies)}


def worth_comparing(c, ref, zeroed):
    """What is missing for case c to notice a kernel that mistreats the last units (empty: nothing); ref = run_case(c), zeroed =
    run_case(without_remainder(c)).  Inside the lanes of every copy of the kernel the case's launches pick from:
      rollouts   an episode ends (flag sets with A or T), two different actions occur, two policies of the set disagree, a final
                 observation is kept (F), and THE REMAINDER MATTERS: without the last units at least one recorded action changes;
                 sampling: the greedy and a non-greedy action are both taken; exploring: explored and unexplored lane-steps both
                 occur; the transitions families: all of transitions_ref.worth_comparing as well
      per-step   the same on the call with the reset observations, where for sample_actions the remainder must change a `prob` word
      evaluate   policy_eval_ref's (under a table policy_eval_table_ref's) conditions, and without the last units a length changes"""
    missing = [f"{name}: nothing changes without the last units" for name, count in remainder_shows(c, ref, zeroed).items() if not count]
    if c.group == "eval":
        return missing + (tb.worth_comparing(_plain(c), ref, run_eval(c, np.zeros(c.n, np.int64))) if c.table else ev.worth_comparing(_plain(c), ref))
    if c.group == "step":
        actions, explored, ended, apart = ref[0].actions[None], ref[0].explored[None], None, disagree(c, ref[0].obs)
    else:
        actions, explored, ended, apart = ref.actions, ref.explored, ref.ended, disagree(c, ref.before)
    for name, m in [(COPIES[k], c.copies == k) for k in np.unique(c.copies)]:
        if ended is not None and c.flags & (A | T) and not ended[:, m].any():
            missing.append(f"{name}: no episode ended")
        if len(np.unique(actions[:, m])) < 2:
            missing.append(f"{name}: one action only")
        if c.n_policies > 1 and not apart[m].any():
            missing.append(f"{name}: the policies never disagree")
        if ended is not None and c.flags & F and not ref.out[-1].final[:, m].any():
            missing.append(f"{name}: no final observation")
        if c.source != "policy" and not (explored[:, m].any() and not explored[:, m].all()):
            both = "greedy and non-greedy actions" if c.source == "sample" else "explored and unexplored steps"
            missing.append(f"{name}: {both} do not both occur")
    if c.group == "transitions":
        missing += tr.worth_comparing(c, ref.out)
    return missing


def _plain(c):
    """policy_eval_ref.worth_comparing reads c.classes as an array"""
    return SimpleNamespace(**{**vars(c), "classes": c.classes[4]})


def last_policy_in_a_gathered_wave(c):
    """Whether a lane of a gathered wave uses the set's last policy (a read past its set would then leave the table)"""
    gathered = (c.copies == 1) | (c.copies == 3)
    policies = pf.policies_of(c.n, c.gid0, c.lanes_per_policy, c.n_policies)
    return bool((policies[gathered] == c.n_policies - 1).any())


def search(inst, hidden, seeds=range(1, 200), temperatures=(sr.TEMPERATURE, 4.0, 16.0, 2.0)):
    """How SEEDS was filled: the first (seed, temperature) that meets worth_comparing; None if there is none"""
    for temperature in temperatures if inst.source == "sample" else (None,):
        for seed in seeds:
            c = case(inst, hidden, seed, temperature)
            if not worth_comparing(c, run_case(c), run_case(without_remainder(c))):
                return seed, temperature
    return None


# (family, env, table, lanes per work-item -- evaluate_policy: index of the shape) -> ((seed of make_weights per width, in the order
# of widths_of), temperature of the sampling families): per case the first seed below 200 that `search` finds.  sample_ref's
# temperature of 8 serves every width: make_weights scales the output layer by 1 / sqrt(H), so 64 units give logits no larger than 8 do.
SEEDS = {('explore', 0, 0, 4): ((8, 2, 1), None), ('explore', 0, 0, 8): ((6, 1, 1), None), ('explore', 0, 1, 4): ((6, 1, 1), None),
         ('explore', 0, 1, 8): ((8, 1, 1), None), ('explore', 1, 0, 4): ((8, 1, 5), None), ('explore', 1, 0, 8): ((8, 3, 5), None),
         ('explore', 1, 1, 4): ((4, 1, 1), None), ('explore', 1, 1, 8): ((8, 1, 3), None), ('explore_fitness', 0, 0, 4): ((6, 1, 1), None),
         ('explore_fitness', 0, 0, 8): ((9, 2, 1), None), ('explore_fitness', 0, 1, 4): ((5, 1, 1), None),
         ('explore_fitness', 0, 1, 8): ((2, 1, 1), None), ('explore_fitness', 1, 0, 4): ((4, 1, 1), None),
         ('explore_fitness', 1, 0, 8): ((8, 1, 3), None), ('explore_fitness', 1, 1, 4): ((8, 3, 5), None),
         ('explore_fitness', 1, 1, 8): ((4, 5, 1), None), ('sample', 0, 0, 4): ((1, 1, 1), 8.0), ('sample', 0, 0, 8): ((1, 1, 1), 8.0),
         ('sample', 0, 1, 4): ((1, 1, 1), 8.0), ('sample', 0, 1, 8): ((1, 1, 1), 8.0), ('sample', 1, 0, 4): ((1, 1, 1), 8.0),
         ('sample', 1, 0, 8): ((1, 1, 1), 8.0), ('sample', 1, 1, 4): ((1, 1, 1), 8.0), ('sample', 1, 1, 8): ((1, 1, 1), 8.0),
         ('sample_fitness', 0, 0, 4): ((1, 1, 1), 8.0), ('sample_fitness', 0, 0, 8): ((1, 1, 1), 8.0),
         ('sample_fitness', 0, 1, 4): ((1, 1, 1), 8.0), ('sample_fitness', 0, 1, 8): ((1, 1, 1), 8.0),
         ('sample_fitness', 1, 0, 4): ((1, 1, 1), 8.0), ('sample_fitness', 1, 0, 8): ((1, 1, 1), 8.0),
         ('sample_fitness', 1, 1, 4): ((1, 1, 1), 8.0), ('sample_fitness', 1, 1, 8): ((1, 1, 1), 8.0),
         ('record_policy', 0, 0, 4): ((11, 1, 2), None), ('record_policy', 0, 1, 4): ((1, 1, 2), None),
         ('record_policy', 1, 0, 4): ((9, 1, 6), None), ('record_policy', 1, 1, 4): ((9, 5, 6), None),
         ('record_explore', 0, 0, 4): ((19, 1, 1), None), ('record_explore', 0, 1, 4): ((1, 1, 1), None),
         ('record_explore', 1, 0, 4): ((9, 5, 5), None), ('record_explore', 1, 1, 4): ((9, 1, 3), None),
         ('record_sample', 0, 0, 4): ((1, 1, 1), 8.0), ('record_sample', 0, 1, 4): ((1, 1, 1), 8.0),
         ('record_sample', 1, 0, 4): ((1, 1, 1), 8.0), ('record_sample', 1, 1, 4): ((1, 1, 1), 8.0),
         ('transitions_policy', 0, 0, 4): ((26, 21, 2), None), ('transitions_policy', 0, 1, 4): ((38, 2, 3), None),
         ('transitions_policy', 1, 0, 4): ((9, 5, 6), None), ('transitions_policy', 1, 1, 4): ((9, 1, 3), None),
         ('transitions_explore', 0, 0, 4): ((19, 1, 1), None), ('transitions_explore', 0, 1, 4): ((1, 1, 1), None),
         ('transitions_explore', 1, 0, 4): ((9, 5, 5), None), ('transitions_explore', 1, 1, 4): ((9, 1, 3), None),
         ('sample_transitions', 0, 0, 4): ((1, 1, 1), 8.0), ('sample_transitions', 0, 1, 4): ((1, 1, 1), 8.0),
         ('sample_transitions', 1, 0, 4): ((1, 1, 1), 8.0), ('sample_transitions', 1, 1, 4): ((1, 1, 1), 8.0),
         ('explore_actions', 0, 0, 4): ((13, 7, 1), None), ('explore_actions', 0, 0, 8): ((69, 3, 23), None),
         ('explore_actions', 1, 0, 4): ((8, 3, 5), None), ('explore_actions', 1, 0, 8): ((4, 1, 2), None),
         ('sample_actions', 0, 0, 4): ((2, 1, 1), 8.0), ('sample_actions', 0, 0, 8): ((2, 1, 1), 8.0),
         ('sample_actions', 1, 0, 4): ((1, 1, 1), 8.0), ('sample_actions', 1, 0, 8): ((1, 1, 1), 8.0),
         ('evaluate_policy', 0, 0, 0): ((38, 3), None), ('evaluate_policy', 0, 0, 1): ((38, 3), None),
         ('evaluate_policy', 0, 1, 0): ((38, 3), None), ('evaluate_policy', 0, 1, 1): ((38, 3), None),
         ('evaluate_policy', 1, 0, 0): ((70, 42), None), ('evaluate_policy', 1, 0, 1): ((70, 42), None),
         ('evaluate_policy', 1, 1, 0): ((9, 5), None), ('evaluate_policy', 1, 1, 1): ((9, 5), None)}
