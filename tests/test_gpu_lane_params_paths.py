"""Multi-row parameter tables on every stepping path against the CPU reference of tests/lane_params_ref.py (one f32 twin per row,
lane i read from twin index[i]; it shares no code with the table kernels and never loads the library).

The TableT kernels (gym-rs_amd/csrc/gymrs_table_<env>.hip) are built per flag set (10), lanes per work-item (4, 8) and recording
mode, and carry code no uniform kernel has: the per-lane row gather (with its own branch in the fused rollout), advance_fast_rows
for both integrators, the per-lane slow path and the index check.  Here every one of them steps lanes of five different rows in
full and ragged waves (n = 3001: at 4 lanes per work-item 11 full waves and one of 185 lanes, at 8 five full waves and one of 441).
tests/test_lane_params_ref.py shows on the CPU that at every point compared here a lane stepped with another row would differ.

Every comparison is bit for bit (uint32 views of floats, equal integers, statistics with ==), no lane left out.  Two exceptions,
both stated where they apply: the slow-path cases treat any NaN as equal to any NaN, as tests/test_gpu_slowpaths.py does (sign
and payload of a generated NaN are not specified), and the f64 oracle test has the project's per-step bound of 1e-6."""
import json
import os

import lane_params_ref as ref
import numpy as np
import pytest
import torch
from lane_params_ref import A, F, S, T

from oracle import bindings as orc_bindings
from oracle.bindings import Oracle

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
INVALID_ACTION = 5  # GYMRS_EACTION


def wave_report(lanes, n, vec):
    """For a failure message: how many of `lanes` lie in full waves and in the ragged one at `vec` lanes per work-item"""
    full = n // (64 * vec) * (64 * vec)
    return {"full waves": int((lanes < full).sum()), "ragged wave": int((lanes >= full).sum()), "first": lanes[:8].tolist()}


def same(what, got, want, at, vec=4, index=None, nan_equal=False):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, at, got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype == np.float32:
        bad = got.view(np.uint32) != want.view(np.uint32)
        if nan_equal:
            bad &= ~(np.isnan(got) & np.isnan(want))
    else:
        bad = got != want
    if bad.any():
        lanes = np.flatnonzero(bad.reshape(-1, bad.shape[-1]).any(axis=0))
        rows = None if index is None else np.bincount(np.asarray(index)[lanes], minlength=ref.K).tolist()
        raise AssertionError((what, at, f"{len(lanes)} lanes differ", wave_report(lanes, bad.shape[-1], vec), {"per row": rows}))


def compare(eng, r, at, vec=4, nan_equal=False, stats=True, lanes=None):
    """The engine's getters == the reference's attributes (`lanes`: a boolean mask of the lanes to look at, default all)"""
    pick = (lambda x: x) if lanes is None else (lambda x: x[..., lanes])
    kw = dict(vec=vec, index=pick(r.index), nan_equal=nan_equal)
    same("state", pick(eng.get_state()), pick(r.state), at, **kw)
    same("obs", pick(eng.get_obs()), pick(r.obs), at, **kw)
    reward, done, trunc = eng.get_step_result()
    same("reward", pick(reward), pick(r.reward), at, **kw)
    same("done", pick(done), pick(r.done), at, **kw)
    if r.flags & T:
        same("truncated", pick(trunc), pick(r.truncated), at, **kw)
    if r.flags & F:
        same("final_obs", pick(eng.get_final_obs()), pick(r.final), at, **kw)
    if stats:
        assert np.array_equal(eng.stats(), r.stats), ("stats", at, eng.stats(), r.stats)
    assert eng.tick()[0] == r.tick, ("tick", at, eng.tick(), r.tick)


def device(a):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    torch.cuda.synchronize()  # torch copied on its stream; the engine reads on its own
    return t


def table_engine(gymrs, c, vec=4, prepare=None, first=0, count=None):
    """An engine for lanes [first, first + count) of case c, with c's table and index, reset and prepared"""
    count = c.n - first if count is None else count
    rows = ref.rows_for(type(gymrs.engine.default_params(c.kind)), c.rows)
    eng = gymrs.BatchedEngine(c.kind, count, global_env_offset=c.gid0 + first, flags=c.flags, params=rows[0], lanes_per_thread=vec)
    eng.set_param_table(rows)
    eng.set_param_index(c.index[first:first + count])
    eng.reset(seed=ref.RESET_SEED)
    if prepare is not None:
        eng.set_state(prepare(eng.get_state()))
    return eng


def launched(eng):
    return json.loads(eng.env_json(0))["gymrs"]


def assert_table_launch(eng, kind, vec, at):
    name = "CartPoleT" if kind == 0 else "MountainCarT"
    assert launched(eng)["last_launch"].startswith(f"HIP launch: gymrs::step_kernel<TableT<{name}>, {vec}, "), (at, launched(eng)["last_launch"])


def run_stages(eng, r, c, vec, nan_equal=False):
    """c.stages on the engine with the reference advanced alongside, compared after each stage"""
    n = c.n
    padded = (n + 15) // 16 * 16
    ring_tight = device(c.ring)  # stride n: the buffers behind the first are not aligned for the vector load (every wave takes the guarded code)
    ring_padded = torch.zeros((ref.RING, padded), dtype=torch.uint8, device=DEV)
    ring_padded[:, :n] = ring_tight
    torch.cuda.synchronize()
    keep = []
    same("start state", eng.get_state(), r.state, "reset", vec, r.index, nan_equal)
    for number, (name, steps) in enumerate(c.stages):
        at = (number, name, f"steps {r.t} .. {r.t + steps}")
        if name == "step":
            for _ in range(steps):
                keep.append(device(c.actions(r.t, None)))
                eng.step(keep[-1].data_ptr())
                r.step()
        elif name == "step_host":
            for _ in range(steps):
                eng.step_host(c.actions(r.t, None))
                r.step()
        elif name == "step_many":
            eng.step_many(ring_tight.data_ptr(), n, ref.RING, steps)
            r.step(steps)
        elif name == "step_many graph":
            eng.step_many(ring_padded.data_ptr(), padded, ref.RING, steps, use_graph=True)
            r.step(steps)
        elif name == "rollout":
            eng.rollout(steps, action_seed=ref.ACTION_SEED, action_t0=r.t)
            r.step(steps)
        else:
            raise AssertionError(name)
        eng.sync()
        compare(eng, r, at, vec, nan_equal)
        if name != "rollout":  # (last_launch names the most recent per-step launch)
            assert_table_launch(eng, c.kind, vec, at)
        assert launched(eng)["param_table_rows"] == ref.K
    del keep


# ---- the path matrix ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gid0", ref.OFFSETS)
@pytest.mark.parametrize("vec", [4, 8])
@pytest.mark.parametrize("flags", ref.FLAG_SETS)
@pytest.mark.parametrize("kind", [0, 1])
def test_every_path_equals_the_cpu_reference(gymrs, kind, flags, vec, gid0):
    """step, step_host, step_many (eager, captured graph twice), rollout twice, step: one engine, compared after each stage"""
    c = ref.matrix_case(kind, flags, gid0)
    eng = table_engine(gymrs, c, vec)
    run_stages(eng, ref.matrix_reference(c), c, vec)
    eng.close()


@pytest.mark.parametrize("vec", [4, 8])
@pytest.mark.parametrize("flags", ref.INTEGRATOR_1_FLAGS)
def test_kinematics_integrator_1(gymrs, flags, vec):
    """advance_fast_rows<.., 1>: CartPole's other integrator with per-lane rows, on every path"""
    c = ref.matrix_case(0, flags, ref.OFFSETS[0], integrator=1)
    r = ref.matrix_reference(c)
    assert all(row.kinematics_integrator == 1 for row in c.rows)
    eng = table_engine(gymrs, c, vec)
    run_stages(eng, r, c, vec)
    assert eng.get_params().kinematics_integrator == 1
    eng.close()


# ---- the recording kernel ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", ref.FLAG_SETS)
@pytest.mark.parametrize("kind", [0, 1])
def test_rollout_record_rows_equal_the_reference_step_by_step(gymrs, kind, flags):
    c = ref.matrix_case(kind, flags, ref.OFFSETS[0], stages=ref.RECORD_STAGES)
    r = ref.matrix_reference(c)
    eng = table_engine(gymrs, c)
    (_, warm), (_, steps) = c.stages
    assert steps >= 20
    n, d = c.n, ref.DIMS[kind][0]
    stride = (n + 15) // 16 * 16 + 16  # > n: rows have padding columns
    keep = []
    for _ in range(warm):
        keep.append(device(c.actions(r.t, None)))
        eng.step(keep[-1].data_ptr())
        r.step()
    obs = torch.full((steps, d, stride), float("nan"), dtype=torch.float32, device=DEV)
    act = torch.full((steps, stride), 9, dtype=torch.uint8, device=DEV)
    rew = torch.full((steps, stride), float("nan"), dtype=torch.float32, device=DEV)
    done = torch.full((steps, stride), 9, dtype=torch.uint8, device=DEV)
    trunc = torch.full((steps, stride), 9, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()  # torch filled these on its stream; the engine writes them on its own
    eng.rollout_record(steps, ref.ACTION_SEED, r.t, obs=obs.data_ptr(), actions=act.data_ptr(), reward=rew.data_ptr(), done=done.data_ptr(),
                       truncated=trunc.data_ptr(), lane_stride=stride)
    eng.sync()
    r.step(steps)
    obs_h, act_h, rew_h, done_h, trunc_h = (x.cpu().numpy() for x in (obs, act, rew, done, trunc))
    for t, row in enumerate(r.records[warm:]):
        same("recorded obs", obs_h[t, :, :n], row.obs, t, index=r.index)
        same("recorded actions", act_h[t, :n], row.actions, t, index=r.index)
        same("recorded reward", rew_h[t, :n], row.reward, t, index=r.index)
        same("recorded done", done_h[t, :n], row.done, t, index=r.index)
        if flags & T:
            same("recorded truncated", trunc_h[t, :n], row.truncated, t, index=r.index)
    # the padding of a row is never written (nor `truncated` without the time limit)
    assert np.isnan(obs_h[:, :, n:]).all() and np.isnan(rew_h[:, n:]).all()
    assert (act_h[:, n:] == 9).all() and (done_h[:, n:] == 9).all() and (trunc_h[:, n:] == 9).all()
    if not flags & T:
        assert (trunc_h == 9).all()
    compare(eng, r, "after the recording")
    eng.close()


# ---- the slow path with per-lane constants -------------------------------------------------------------------------------------
@pytest.mark.parametrize("vec", [4, 8])
@pytest.mark.parametrize("flags", [0, T, A | S, A | S | T | F])
@pytest.mark.parametrize("kind", [0, 1])
def test_slow_path_lanes_step_with_their_own_rows(gymrs, kind, flags, vec):
    """Every 7th lane starts beyond the fast path's range (angles up to 1e30, NaN, inf: lane_params_ref.slow_prepare), in lanes of
    every row: their waves take Env::advance(lc[k], ..) for all their lanes.  With flags 0 and T nobody re-arms these lanes: they
    keep being stepped, CartPole's through steps_beyond_terminated.  Any NaN equals any NaN here, everything else bit for bit."""
    c = ref.matrix_case(kind, flags, ref.OFFSETS[0])
    prepare = ref.slow_prepare(kind)
    r = ref.matrix_reference(c, prepare)
    assert len(set(r.index[ref.beyond_range(kind, r.state)])) >= 3
    eng = table_engine(gymrs, c, vec, prepare)
    run_stages(eng, r, c, vec, nan_equal=True)
    if not flags & A and kind == 0:
        assert np.isnan(r.state).any() and (r.reward == 0).any()  # still stepped at the end, and past the one-off warning reward
    eng.close()


# ---- time-limit elision -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vec", [4, 8])
def test_time_limit_elision_on_a_table(gymrs, vec):
    """CartPole with A | S | T runs a launch without the limit (the reset-logged TableT kernel) while the host can prove that no lane
    reaches it, as tests/test_gpu_time_limit_elision.py says.  Limit 23: the first launches after the reset cannot reach it, later
    ones can, and launches with and without the limit alternate; flags after every step, state and statistics at the end."""
    steps = ref.ELISION_STEPS
    c = ref.elision_case()
    r = ref.matrix_reference(c)
    eng = table_engine(gymrs, c, vec)
    keep = []
    seen = set()
    for t in range(steps):
        keep.append(device(c.actions(t, None)))
        eng.step(keep[-1].data_ptr())
        r.step()
        reward, done, trunc = eng.get_step_result()
        same("done", done, r.done, t, vec, r.index)
        same("truncated", trunc, r.truncated, t, vec, r.index)
        same("reward", reward, r.reward, t, vec, r.index)
        seen.add(launched(eng)["last_launch"].split("flags ")[1].split(" ")[0])
        assert_table_launch(eng, 0, vec, t)
    compare(eng, r, "the end", vec)
    assert 0 < launched(eng)["time_limit_elided_launches"] < steps, launched(eng)
    assert seen == {"3", "7"}, seen  # launches of both kernels: without and with the limit
    assert (r.ended_by > 0).all()  # every row terminated and was truncated
    eng.close()


# ---- the index rewritten between fused launches ----------------------------------------------------------------------------------
class DeviceColumn:
    """A zero-copy torch view of an engine's device array"""

    def __init__(self, ptr, n, typestr):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (ptr, False), "version": 3}


@pytest.mark.parametrize("vec", [4, 8])
@pytest.mark.parametrize("flags", ref.REWRITE_FLAGS)
@pytest.mark.parametrize("kind", [0, 1])
def test_index_rewritten_between_rollouts(gymrs, kind, flags, vec):
    """A write through param_index_ptr on the engine's stream takes effect in the next fused launch: every lane goes on from its own
    state with its new row.  (Flag sets without the time limit; tests/test_gpu_sequences.py rewrites the index under the others.)"""
    c = ref.matrix_case(kind, flags, ref.OFFSETS[0], stages=())
    r = ref.matrix_reference(c)
    eng = table_engine(gymrs, c, vec)
    new = ref.rewritten_index(kind)
    first, second = ref.REWRITE_STEPS
    new_dev = device(new.view(np.int16))
    view = torch.as_tensor(DeviceColumn(eng.param_index_ptr(), c.n, "<i2"), device=DEV)
    eng.rollout(first, action_seed=ref.ACTION_SEED, action_t0=0)  # enqueued before the rewrite: the old index
    with torch.cuda.stream(torch.cuda.ExternalStream(eng.stream, device=DEV)):
        view.copy_(new_dev)
    eng.rollout(second, action_seed=ref.ACTION_SEED, action_t0=first)
    eng.sync()
    r.step(first)
    r.set_index(new)
    r.step(second)
    assert r.told_apart(c.index) >= ref.TOLD_APART  # the old index would be noticed
    compare(eng, r, "after the rewrite", vec)
    assert np.array_equal(eng.get_param_index(), new)
    keep = device(c.actions(r.t, None))
    eng.step(keep.data_ptr())
    eng.sync()
    r.step()
    compare(eng, r, "a step after the rewrite", vec)
    eng.close()


# ---- an index outside the table inside a fused rollout ----------------------------------------------------------------------------
@pytest.mark.parametrize("vec", [4, 8])
@pytest.mark.parametrize("kind", [0, 1])
def test_out_of_range_index_in_a_rollout_is_reported_and_not_stepped(gymrs, kind, vec):
    """Two lanes with index K and 65535, rollout(6): the documented GYMRS_EACTION report naming the lowest lane; those lanes keep
    their state, every other lane (their neighbours in the work-item and wave, on the per-lane path, included) equals the reference."""
    c = ref.matrix_case(kind, A, ref.OFFSETS[0], stages=())
    bad_lanes = [777, 2999]  # a full wave and the ragged one, at both widths
    r = ref.matrix_reference(c)  # (lanes are independent: the reference's own row for the two lanes does not matter)
    eng = table_engine(gymrs, c, vec)
    index = c.index.copy()
    index[bad_lanes] = [ref.K, 65535]
    eng.set_param_index(index)
    before = eng.get_state()
    eng.rollout(6, action_seed=ref.ACTION_SEED, action_t0=0)
    with pytest.raises(gymrs.InvalidActionError) as ei:
        eng.sync()
    assert ei.value.status == INVALID_ACTION and f"lane {bad_lanes[0]} " in str(ei.value) and "parameter index" in str(ei.value)
    r.step(6)
    ok = np.ones(c.n, bool)
    ok[bad_lanes] = False
    same("state of the rejected lanes", eng.get_state()[:, ~ok], before[:, ~ok], "rollout", vec)
    compare(eng, r, "the other lanes", vec, stats=False, lanes=ok)
    eng.sync()  # the report was consumed
    eng.close()


# ---- GYMRS_AQL=1 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1])
def test_step_many_with_the_chain_opt_in_still_goes_out_as_hip_launches(gymrs, kind):
    c = ref.matrix_case(kind, A | S | T, ref.OFFSETS[0], stages=(("step_many", 10),))
    r = ref.matrix_reference(c)
    eng = table_engine(gymrs, c)
    ring = device(c.ring)
    before = os.environ.get("GYMRS_AQL")
    os.environ["GYMRS_AQL"] = "1"
    try:
        eng.step_many(ring.data_ptr(), c.n, ref.RING, 10)
        eng.sync()
    finally:
        os.environ.pop("GYMRS_AQL", None)
        if before is not None:
            os.environ["GYMRS_AQL"] = before
    r.step(10)
    compare(eng, r, "step_many under GYMRS_AQL=1")
    g = launched(eng)
    assert g["aql_launches"] == 0 and g["aql_chains"] == 0 and "parameter table" in g["aql"]
    assert_table_launch(eng, kind, 4, "GYMRS_AQL=1")
    eng.close()


# ---- the native sharder -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1])
def test_sharded_engine_with_per_shard_tables(gymrs, kind):
    """3 blocks on device 0, each with the table and its slice of the index: 12 steps and a rollout against the ONE reference"""
    flags = A | S | T | F
    c = ref.matrix_case(kind, flags, ref.OFFSETS[0], stages=())
    r = ref.matrix_reference(c)
    rows = ref.rows_for(type(gymrs.engine.default_params(kind)), c.rows)
    sh = gymrs.ShardedEngine(kind, c.n, [0, 0, 0], global_env_offset=c.gid0, flags=flags, params=rows[0])
    assert [s.first_lane for s in sh.shards] == [0, 1001, 2001]
    for s in sh.shards:
        s.set_param_table(rows)
        s.set_param_index(c.index[s.first_lane:s.first_lane + s.n_envs])
    sh.reset(seed=ref.RESET_SEED)

    def check(at):
        sh.sync()
        same("state", sh.get_state(), r.state, at, index=r.index)
        reward, done, trunc = sh.get_step_result()
        same("reward", reward, r.reward, at, index=r.index)
        same("done", done, r.done, at, index=r.index)
        same("truncated", trunc, r.truncated, at, index=r.index)
        same("final_obs", sh.get_final_obs(), r.final, at, index=r.index)
        assert np.array_equal(sh.stats(), r.stats), (at, sh.stats(), r.stats)
        assert all(s.tick()[0] == r.tick for s in sh.shards)

    keep = []
    for t in range(12):
        keep.append(device(c.actions(t, None)))
        sh.step([keep[-1].data_ptr() + s.first_lane for s in sh.shards])
        r.step()
        if t in (0, 11):
            check(t)
    sh.rollout(9, action_seed=ref.ACTION_SEED, action_t0=12)
    r.step(9)
    check("rollout")
    assert all("TableT<" in launched(s)["last_launch"] for s in sh.shards)
    sh.close()


# ---- policy x table, per step -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1])
def test_policy_actions_plus_step_on_a_table(gymrs, kind):
    """gymrs_rollout_policy refuses a table and points here: policy_actions + step.  The actions and the step's result against the
    reference driven by closed_loop_ref.policy_ref (plain C): affine, 2 policies, 100 lanes per policy."""
    c, r, w = ref.policy_reference(kind)
    eng = table_engine(gymrs, c)
    eng.set_policy(w, hidden=0, lanes_per_policy=ref.POLICY.lanes_per_policy)
    with pytest.raises(gymrs.GymrsError, match="parameter table"):
        eng.rollout_policy(3)
    buf = torch.full((c.n,), 9, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    taken = set()
    for t in range(ref.POLICY.steps):
        eng.policy_actions(buf.data_ptr())
        eng.step(buf.data_ptr())
        eng.sync()
        r.step()
        same("actions", buf.cpu().numpy(), r.records[-1].actions, t, index=r.index)
        compare(eng, r, t)
        taken |= set(r.records[-1].actions.tolist())
    assert len(taken) >= 2 and r.stats[2] > 0
    assert_table_launch(eng, kind, 4, "policy")
    eng.close()


# ---- MountainCar, one step against the f64 oracle ---------------------------------------------------------------------------------
@pytest.mark.parametrize("vec", [4, 8])
def test_mountain_car_rows_one_step_against_the_f64_oracle(gymrs, vec):
    """64 rows that vary all seven physics fields (both walls, the goal and its velocity among them), states spread over and beyond
    both walls: the project's per-step bound |got - ref| <= 1e-6 * max(|ref|, 1) and equal done flags, row by row."""
    kind, k, per = 1, 64, 47
    n = k * per
    rows = ref.make_rows(kind, k, 64, 200)
    for f in ("min_position", "max_position", "max_speed", "goal_position", "goal_velocity", "force", "gravity"):
        assert len({getattr(row, f) for row in rows}) >= 2, f
    rng = np.random.default_rng(64)
    st0 = np.stack([rng.uniform(-1.3, 0.7, n), rng.uniform(-0.08, 0.08, n)]).astype(np.float32)
    st0[:, :k] = np.array([[-0.9], [-0.01]], np.float32)  # on the raised wall, moving into it (the wall rule), under every row
    act = rng.integers(0, 3, n).astype(np.uint8)
    index = np.tile(np.arange(k, dtype=np.uint16), per)
    mine = ref.rows_for(type(gymrs.engine.default_params(kind)), rows)
    eng = gymrs.BatchedEngine(kind, n, params=mine[0], lanes_per_thread=vec)
    eng.set_param_table(mine)
    eng.set_param_index(index)
    eng.reset(seed=8)
    eng.set_state(st0)
    eng.step_host(act)
    got, done = eng.get_state().astype(np.float64), eng.get_step_result()[1]
    assert "TableT<MountainCarT>" in launched(eng)["last_launch"]
    eng.close()
    orc = Oracle()
    P = orc_bindings.MountainCarParams
    n_done = clipped = 0
    for r in range(k):
        ln = np.flatnonzero(index == r)
        p = P(**{f: getattr(rows[r], f) for f, _ in P._fields_})
        want = np.ascontiguousarray(st0[:, ln].astype(np.float64))
        _, d, bad = orc.mountain_car_step_batch(want, act[ln], params=p)
        assert bad == 0 and np.array_equal(d, done[ln]), (r, np.flatnonzero(d != done[ln]))
        err = np.abs(got[:, ln] - want) / np.maximum(np.abs(want), 1.0)
        assert err.max() <= 1e-6, (r, err.max())
        n_done += int(d.sum())
        clipped += int(((want[0] == p.min_position) | (want[0] == p.max_position)).sum())
    assert n_done > 100 and clipped > 100  # goals were reached and walls were hit
