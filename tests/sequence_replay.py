"""A sequence of tests/sequence_ref.py replayed on the library and on the model, compared after every call: the body of
tests/test_gpu_sequences.py and of tools/fuzz_sequences.py.  A plain module (it imports torch and takes the loaded package as an
argument); no fixtures, no pytest hooks.

Nothing writes into the engine's views.  Every buffer a launch reads is filled on the engine's own stream (gymrs_fill_actions, the
action kernels), so nothing here waits for another stream; buffers torch fills (the sentinel) are synchronised before use."""
import closed_loop_ref as cl
import lane_params_ref as lp
import numpy as np
import reset_box_ref as rb
import sequence_ref as sq
import torch
from sequence_ref import A, F, S, T

DEV = "cuda:0"
EINVAL = 1
PAD_BYTE = 0xEE  # what u8 record rows are pre-filled with


class Mismatch(AssertionError):
    pass


class DeviceColumn:
    """A zero-copy torch view of an engine's device array"""

    def __init__(self, ptr, n, typestr):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (ptr, False), "version": 3}


def equal_bits(got, want):
    """lane-wise (last axis): equal bit for bit, a NaN equal to any NaN -> bool array over the last axis"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype == np.float32:
        ok = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
    else:
        ok = got == want
    if ok.size == 0:  # (no padding lanes: the stride is the lane count)
        return np.ones(ok.shape[-1] if ok.ndim else 1, bool)
    return ok.reshape(-1, ok.shape[-1]).all(axis=0) if ok.ndim else ok.reshape(1)


class Replay:
    def __init__(self, gymrs, c, ops, off=()):
        """off: faults planted in the MODEL (sequence_ref.FAULTS), to see that the comparison notices them"""
        self.gymrs, self.c, self.ops = gymrs, c, list(ops)
        self.P = type(gymrs.engine.default_params(c.kind))
        self.model = sq.Model(c, off)
        self.eng = self._create()
        self.log = [f"{sq.Config.__name__}{tuple(c)}"]
        self.stride = sq.stride_of(c.n)
        dt = torch.float32 if c.kind == 2 else torch.uint8
        self.ring = torch.zeros((sq.RING_GRAPH, self.stride), dtype=dt, device=DEV)
        self.act = torch.zeros(self.stride, dtype=dt, device=DEV)
        self.act2 = torch.zeros(self.stride, dtype=dt, device=DEV)
        steps = max([sq.steps_of(op) for op in ops if sq.op_class(op) in ("recording", "transitions")] + [1])
        d = lp.TwinEngine._OBS_DIM[c.kind]
        f32 = dict(dtype=torch.int32, device=DEV)  # (f32 rows are held as their bits: the sentinel is a NaN pattern)
        self.rec = dict(obs=torch.zeros((steps, d, self.stride), **f32), actions=torch.zeros((steps, self.stride), dtype=torch.int32 if c.kind == 2 else torch.uint8, device=DEV),
                        reward=torch.zeros((steps, self.stride), **f32), done=torch.zeros((steps, self.stride), dtype=torch.uint8, device=DEV),
                        truncated=torch.zeros((steps, self.stride), dtype=torch.uint8, device=DEV),
                        final_obs=torch.zeros((steps, d, self.stride), **f32), start_obs=torch.zeros((d, self.stride), **f32))
        torch.cuda.synchronize()
        self._sources()

    def params(self, row):
        return self.P.from_buffer_copy(bytes(row))

    def _create(self):
        c = self.c
        return self.gymrs.BatchedEngine(c.kind, c.n, global_env_offset=c.gid0, flags=c.flags, params=self.params(sq.uniform_row(c.kind, c.cap)))

    def _sources(self):
        """policy, exploration and sampling as the model holds them: at the start, and again on a clone or a restored engine"""
        m = self.model
        if m.policy is not None:
            self.eng.set_policy(m.policy.weights, hidden=m.policy.hidden, lanes_per_policy=m.policy.lpp)
            self.eng.set_exploration(m.explore[0], threshold=m.explore[1])
            self.eng.set_sampling(m.sample[0], scale=m.sample[1])

    def close(self):
        self.eng.close()

    # -- record buffers
    def _record(self):
        for name, t in self.rec.items():
            t.fill_(PAD_BYTE if t.dtype == torch.uint8 else sq.SENTINEL)
        torch.cuda.synchronize()  # torch filled them on its stream; the engine writes them on its own
        return dict({k: self.rec[k].data_ptr() for k in ("obs", "actions", "reward", "done", "truncated")}, lane_stride=self.stride)

    def _rows(self, name, steps):
        t = self.rec[name]
        a = (t if name == "start_obs" else t[:steps]).cpu().numpy()
        if t.dtype == torch.int32 and not (name == "actions" and self.c.kind != 2):
            a = a.view(np.float32)
        return a

    # -- one op on the engine (the model has NOT applied it yet)
    def _play(self, op):
        gymrs, eng, m, c = self.gymrs, self.eng, self.model, self.c
        name = op[0]
        if name == "reset":
            eng.reset(seed=op[1], options=None if op[2] is None else rb.NAMED[c.kind][op[2]])
        elif name == "step":
            if op[1] == "step":
                eng.fill_actions(self.act.data_ptr(), seed=op[2], t=op[3])
                eng.step(self.act.data_ptr())
            elif op[1] == "step_host":
                eng.step_host(m.ref.tws[0].fill_actions(op[2], op[3]))
            else:
                {"policy": eng.policy_actions, "explore": eng.explore_actions, "sample": eng.sample_actions}[op[1]](self.act.data_ptr())
                eng.step(self.act.data_ptr())
        elif name == "many":
            nbuf = sq.RING_GRAPH if op[1] == "graph" else min(sq.RING_HIP, op[2])
            for b in range(nbuf):
                eng.fill_actions(self.ring[b].data_ptr(), seed=op[3], t=b)
            eng.step_many(self.ring.data_ptr(), self.stride * self.ring.element_size(), nbuf, op[2], use_graph=op[1] == "graph")
        elif name == "rollout":
            eng.rollout(op[1], action_seed=op[2], action_t0=op[3])
        elif name == "rollout_record":
            rec = self._record()
            eng.rollout_record(op[1], op[2], op[3], **rec)
        elif name == "policy":
            if op[1] == "plain":
                eng.rollout_policy(op[2])
            elif op[1] == "fitness":
                eng.rollout_policy_fitness(op[2])
            else:
                eng.rollout_policy_record(op[2], **self._record())
        elif name == "closed":
            eng.rollout_closed_loop(op[3], lane_params=op[4], fitness=op[2] == "fitness", record=self._record() if op[2] == "record" else None,
                                    explore=op[1] == "explore", sample=op[1] == "sample")
        elif name == "transitions":
            eng.rollout_transitions(op[2], record=self._record(), final_obs=self.rec["final_obs"].data_ptr(), start_obs=self.rec["start_obs"].data_ptr(),
                                    lane_params=op[3], explore=op[1] == "explore", sample=op[1] == "sample")
        elif name == "set_state":
            eng.set_state(sq.new_state(c.kind, m.state, op[1]), first=0)
        elif name == "set_params":
            eng.set_params(self.params(sq.uniform_row(c.kind, op[1], op[2])))
        elif name == "table":
            if op[1]:
                eng.set_param_table(lp.rows_for(self.P, sq.table_rows(c.kind, m.row.max_episode_steps)))
                eng.set_param_index(lp.make_index(c.n, sq.K, op[2]))
            else:
                eng.set_param_table(None)
        elif name == "set_index":
            eng.set_param_index(lp.make_index(c.n, sq.K, op[1]))
        elif name == "tune":
            eng.set_tuning(op[1], op[2])
        elif name == "stats_clear":
            eng.stats_clear()
        elif name == "fitness_clear":
            eng.policy_fitness_clear()
        elif name == "clone":
            new = eng.clone()
            eng.close()
            self.eng = new
            self._sources()
        elif name == "restore":
            other = self._create()
            other.set_tuning(m.vec, m.hint)
            other.reset(seed=sq.OTHER_SEED)
            for t in range(2):  # a used engine: its own flags, clocks and bookkeeping are set
                other.fill_actions(self.act2.data_ptr(), seed=sq.OTHER_ACTION_SEED, t=t)
                other.step(self.act2.data_ptr())
            other.sync()
            other.restore(eng.snapshot())
            eng.close()
            self.eng = other
            self._sources()
        elif name == "set_policy":
            eng.set_policy(cl.make_weights(c.kind, op[1], sq.N_POLICIES, op[3]), hidden=op[1], lanes_per_policy=op[2])
        elif name == "set_exploration":
            eng.set_exploration(op[1], threshold=op[2])
        elif name == "set_sampling":
            eng.set_sampling(op[1], scale=op[2])
        elif name == "evaluate":
            eng.evaluate_policy(sq.EVAL_EPISODES, sq.EVAL_CAP, seed=3, lane_params=m.table)
            assert eng.policy_eval()[:, 2].sum() == sq.EVAL_EPISODES * c.n
        elif name == "sync":
            eng.sync()
        elif name == "stats":
            eng.stats()
        elif name == "refused":
            try:
                self._refused(op[1])
            except gymrs.GymrsError as e:
                assert e.status == EINVAL, (op, e.status, str(e))
            else:
                raise Mismatch(f"{sq.fmt(op)}: the call was accepted ({sq.REFUSALS[op[1]][1]})")
        else:
            raise AssertionError(op)

    def _refused(self, name):
        eng = self.eng
        if name == "fitness-with-record":
            eng.rollout_closed_loop(1, lane_params=True, fitness=True, record=self._record())
        elif name == "explore-with-sample":
            eng.rollout_closed_loop(1, lane_params=True, explore=True, sample=True)
        elif name == "transitions-no-auto-reset":
            eng.rollout_transitions(1, record=self._record(), final_obs=self.rec["final_obs"].data_ptr(), lane_params=True)
        elif name == "policy-under-table":
            eng.rollout_policy(1)
        elif name == "closed-under-table":
            eng.rollout_closed_loop(1)
        elif name == "graph-pendulum-limit":
            eng.step_many(self.ring.data_ptr(), self.stride * 4, sq.RING_GRAPH, sq.RING_GRAPH, use_graph=True)
        elif name == "table-pendulum":
            eng.set_param_table([self.params(sq.uniform_row(2, 5))] * 2)
        elif name == "final-obs-without-flag":
            eng.get_final_obs()
        else:
            raise AssertionError(name)

    # -- comparison
    def _fail(self, what, k, lanes=None, got=None, want=None):
        c, m = self.c, self.model
        lines = self.log[:k + 2] + [f"MISMATCH after op {k} ({sq.fmt(self.ops[k])}): {what}"]
        if lanes is not None and len(lanes):
            lpp = m.policy.lpp if m.policy is not None else 1
            classes = cl.wave_classes(c.n, m.vec, c.gid0, sq.N_POLICIES, lpp)
            lines.append(f"  {len(lanes)} lanes differ at {m.vec} lanes per work-item, hint {m.hint}; the first:")
            for lane in lanes[:6]:
                lines.append(f"    lane {lane} (wave {lane // (64 * m.vec)}, {cl.COPIES[classes[lane]]}): got {np.asarray(got)[..., lane].tolist()} want {np.asarray(want)[..., lane].tolist()}")
        raise Mismatch("\n".join(lines))

    def _same(self, what, k, got, want):
        bad = np.flatnonzero(~equal_bits(got, want))
        if len(bad):
            self._fail(what, k, bad, got, want)

    def _compare(self, k, op):
        eng, m, c = self.eng, self.model, self.c
        reward, done, trunc = eng.get_step_result()
        self._same("state", k, eng.get_state(), m.state)
        if m.obs_valid:
            self._same("obs", k, eng.get_obs(), m.obs)
        self._same("reward", k, reward, m.reward)
        self._same("done", k, done, m.done)
        if c.flags & T:
            self._same("truncated", k, trunc, m.truncated)
        if c.flags & F:
            self._same("final_obs", k, eng.get_final_obs(), m.final)
        if eng.tick()[0] != m.tick:
            self._fail(f"tick {eng.tick()[0]}, want {m.tick}", k)
        if c.flags & A and c.flags & S:
            got, want = eng.stats(), m.stats
            ok = np.array_equal(got[1:], want[1:]) and (np.allclose(got[0], want[0], rtol=1e-5) if c.kind == 2 else got[0] == want[0])
            if not ok:
                self._fail(f"stats {got.tolist()}, want {want.tolist()}", k)
        if m.fitness is not None:
            got = eng.policy_fitness()
            if not np.array_equal(got, m.fitness):
                self._fail(f"policy_fitness {got.tolist()}, want {m.fitness.tolist()}", k)
        if m.record is not None:
            self._compare_record(k, sq.steps_of(op))

    def _compare_record(self, k, steps):
        m, n = self.model, self.c.n
        self.eng.sync()
        pad32 = np.array([sq.SENTINEL], np.int32).view(np.float32)[0]
        for name, want in m.record.items():
            if name == "ended":
                continue
            got = self._rows(name, steps)
            pad = PAD_BYTE if got.dtype == np.uint8 else pad32
            sentinel = np.full_like(got, pad)
            if name == "truncated" and not self.c.flags & T:  # written with the time limit only
                want = sentinel[..., :n]
            elif name == "final_obs":  # written where the lane-step ended an episode, nowhere else
                want = np.where(m.record["ended"][:, None, :], want, sentinel[..., :n])
            self._same("record." + name, k, got[..., :n], np.ascontiguousarray(want, got.dtype))
            if not equal_bits(got[..., n:], sentinel[..., n:]).all():
                self._fail(f"record.{name}: a padding lane was written", k)

    def views(self):
        """The zero-copy views, read on the engine's stream, against the host copies: byte for byte"""
        eng, c = self.eng, self.c
        eng.sync()
        stats = eng.stats_device()
        reward, done, trunc = eng.get_step_result()
        host = {"state": eng.get_state(), "obs": eng.get_obs(), "reward": reward[None], "done": done[None], "truncated": trunc[None],
                "stats": eng.stats()[None]}
        ptrs = {"state": (eng.state_ptrs(), "<f4"), "obs": (eng.obs_ptrs(), "<f4"), "reward": ([eng.reward_ptr], "<f4"), "done": ([eng.done_ptr], "|u1"),
                "truncated": ([eng.truncated_ptr], "|u1")}
        if c.flags & F:
            host["final"], ptrs["final"] = eng.get_final_obs(), (eng.final_obs_ptrs(), "<f4")
        got = {}
        with torch.cuda.stream(torch.cuda.ExternalStream(eng.stream, device=DEV)):
            for name, (addresses, typestr) in ptrs.items():
                got[name] = np.stack([torch.as_tensor(DeviceColumn(p, c.n, typestr), device=DEV).cpu().numpy() for p in addresses])
            got["stats"] = torch.as_tensor(DeviceColumn(stats, 4, "<f8"), device=DEV).cpu().numpy()[None]
        eng.sync()
        for name, want in host.items():
            assert got[name].shape == want.shape and got[name].tobytes() == np.ascontiguousarray(want).tobytes(), ("view", name, self.log[0])

    def run(self, views=True):
        try:
            for k, op in enumerate(self.ops):
                self.log.append(f"  {k:2d}  {sq.fmt(op)}")
                self._play(op)
                self.model.apply(op)
                self._compare(k, op)
            if views:
                self.views()
            self.eng.sync()
        finally:
            self.close()


def replay(gymrs, c, ops, views=True):
    Replay(gymrs, c, ops).run(views)
