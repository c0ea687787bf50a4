"""gymrs_entropy_gradient on the device against gymrs_entropy_lane (host only; tests/test_entropy_host.py holds it to the numpy restatement
of the rule) summed in Python integers: grad, excluded, sums and counts bit for bit.  The records are real: a sampled
rollout_transitions, old_prob from a policy_gradient launch, then the weights are perturbed so that the ratios differ from 1.  Rows are
wider than n_envs with NaN in the padding lanes, and every table starts from non-zero words (the call ADDS)."""
import closed_loop_ref as cl
import numpy as np
import pytest
import torch
from advantages_ref import SENTINEL
from entropy_ref import DIMS, size_of
from test_gpu_advantages import stride_of

pytestmark = pytest.mark.gpu
DEV, EINVAL = "cuda:0", 1
A, S, T = 1, 2, 4
GID0 = 5 * 256  # nonzero, and a multiple of 256: with lanes_per_policy = 256 every full wave has one set and neighbours differ
COEF, FILL = 0.01, 5
# (n_envs, lanes_per_policy): one lane; one ragged wave; a full 256-lane wave plus a ragged one; a second workgroup -- each with
# uniform sets (n_envs; at GID0 one wave straddles two sets), uniform waves of different sets (256) and gathered weights (3)
SHAPES = [(1, 1), (255, 255), (255, 3), (260, 260), (260, 256), (260, 3), (1028, 1028), (1028, 256), (1028, 3)]


class Record:
    """K sampled steps of an engine of n lanes at GID0, old_prob under the weights it was drawn with, then perturbed weights"""

    def __init__(self, gymrs, kind, hidden, n, lpp, steps):
        self.kind, self.hidden, self.n, self.lpp, self.steps, self.d = kind, hidden, n, lpp, steps, DIMS[kind][0]
        self.stride = s = stride_of(n)
        params = gymrs.engine.default_params(kind)
        params.max_episode_steps = cl.MAX_EPISODE_STEPS
        self.eng = eng = gymrs.BatchedEngine(kind, n, global_env_offset=GID0, flags=A | S | T, params=params)
        eng.reset(seed=cl.RESET_SEED)
        eng.set_policy(cl.make_weights(kind, hidden, cl.N_POLICIES, 11), hidden=hidden, lanes_per_policy=lpp)
        eng.set_sampling(0x5A3B1E0FEEDC0DE5, temperature=1.0)
        f32 = lambda *shape: torch.full(shape, SENTINEL, dtype=torch.int32, device=DEV)  # noqa: E731
        u8 = lambda *shape: torch.full(shape, 9, dtype=torch.uint8, device=DEV)  # noqa: E731
        self.obs, self.fin, self.start, self.old = f32(steps, self.d, s), f32(steps, self.d, s), f32(self.d, s), f32(steps, s)
        self.act, self.rew, self.done, self.trunc = u8(steps, s), f32(steps, s), u8(steps, s), u8(steps, s)
        zero, scrap = torch.zeros((steps, s), dtype=torch.float32, device=DEV), self.tables()  # a zero coefficient row: only prob is wanted
        torch.cuda.synchronize()
        eng.rollout_transitions(steps, record=self.record(), final_obs=self.fin.data_ptr(), start_obs=self.start.data_ptr(), sample=True)
        eng.policy_gradient(steps, record=self.record(), start_obs=self.start.data_ptr(), coef=zero.data_ptr(), grad=scrap[0].data_ptr(),
                            excluded=scrap[1].data_ptr(), prob=self.old.data_ptr(), temperature=1.0)
        eng.sync()
        rng = np.random.default_rng([kind, hidden, n, lpp])
        drawn = eng.get_policy()[0]
        self.weights = (drawn + 0.3 * rng.standard_normal(drawn.shape)).astype(np.float32)
        eng.set_policy(self.weights, hidden=hidden, lanes_per_policy=lpp)

    def record(self, lane=0):
        return dict(obs=self.obs.data_ptr() + 4 * lane, actions=self.act.data_ptr() + lane, reward=self.rew.data_ptr() + 4 * lane,
                    done=self.done.data_ptr() + lane, truncated=self.trunc.data_ptr() + lane, lane_stride=self.stride)

    def tables(self):
        n_sets, size = cl.N_POLICIES, size_of(self.kind, self.hidden)
        return [torch.full(shape, FILL, dtype=torch.int64, device=DEV) for shape in ((n_sets, size), (n_sets,), (n_sets, 2), (n_sets, 2))]

    def launch(self, eng, tables, kl, lane=0):
        grad, excluded, sums, counts = tables
        torch.cuda.synchronize()
        eng.entropy_gradient(self.steps, record=self.record(lane), start_obs=self.start.data_ptr() + 4 * lane, grad=grad.data_ptr(),
                             excluded=excluded.data_ptr(), sums=sums.data_ptr(), counts=counts.data_ptr(), coef=COEF, temperature=1.0,
                             old_prob=self.old.data_ptr() + 4 * lane if kl else None)
        eng.sync()

    def want(self, gymrs, kl):
        """the tables by gymrs_entropy_lane, lane after lane, in Python integers"""
        n, host = self.n, lambda t: t.cpu().numpy()[..., :self.n]  # noqa: E731
        obs, start, old, act = host(self.obs).view(np.float32), host(self.start).view(np.float32), host(self.old).view(np.float32), host(self.act)
        assert (act < DIMS[self.kind][1]).all() and (old > 0).all()
        x = np.concatenate([start[None], obs[:self.steps - 1]])  # [K][D][n]
        n_sets, size = cl.N_POLICIES, size_of(self.kind, self.hidden)
        grad, excluded = [[0] * size for _ in range(n_sets)], [0] * n_sets
        sums, counts = [[0, 0] for _ in range(n_sets)], [[0, 0] for _ in range(n_sets)]
        for i in range(n):
            m = ((GID0 + i) // self.lpp) % n_sets
            q, ex, sm, ct = gymrs.entropy_lane(self.kind, self.hidden, self.weights[m], x[:, :, i], act[:, i] if kl else None, old[:, i] if kl else None,
                                               coef=COEF, temperature=1.0)
            grad[m] = [g + int(v) for g, v in zip(grad[m], q)]
            excluded[m] += ex
            sums[m] = [int(sums[m][j]) + int(sm[j]) for j in range(2)]
            counts[m] = [counts[m][j] + int(ct[j]) for j in range(2)]
        return grad, excluded, sums, counts

    def check(self, gymrs, tables, kl, at):
        want = self.want(gymrs, kl)
        for t, w, name in zip(tables, want, ("grad", "excluded", "sums", "counts")):
            got = (t.cpu().numpy().astype(object) - FILL)
            assert np.array_equal(got, np.array(w, dtype=object)), (name, at)
        assert np.array(want[0], dtype=object).any() and sum(c[0] for c in want[3]) == self.n * self.steps
        if kl:
            assert sum(c[1] for c in want[3]) == self.n * self.steps and (self.n == 1 or any(s[1] for s in want[2]))  # (one lane's kl can round to 0)
        for t in (self.obs, self.start, self.old):
            assert (t.cpu().numpy().view(np.uint32)[..., self.n:] == SENTINEL).all(), "a padding lane was written"


@pytest.mark.parametrize("n,lpp", SHAPES)
@pytest.mark.parametrize("hidden", [0, 1, 7, 64])  # affine; one ragged chunk; two chunks, the last ragged; all chunks
@pytest.mark.parametrize("kind", [0, 1])
def test_the_tables_equal_the_host_lane_summed(gymrs, kind, hidden, n, lpp):
    for steps in (1, 3):  # no prefetch; prefetch with the last row
        rec = Record(gymrs, kind, hidden, n, lpp, steps)
        for kl in (False, True):
            tables = rec.tables()
            rec.launch(rec.eng, tables, kl)
            rec.check(gymrs, tables, kl, (kind, hidden, n, lpp, steps, kl))
        rec.eng.close()


@pytest.mark.parametrize("kind,hidden,lpp", [(0, 7, 3), (1, 0, 256)])
def test_two_engines_that_cut_one_batch_add_up_to_one(gymrs, kind, hidden, lpp):
    n, cut = 1028, 528  # the second block's rows start 16-byte aligned inside the first one's
    rec = Record(gymrs, kind, hidden, n, lpp, 3)
    tables = rec.tables()
    parts = []
    for lane, lanes in ((0, cut), (cut, n - cut)):
        eng = gymrs.BatchedEngine(kind, lanes, global_env_offset=GID0 + lane, flags=A | S | T)
        eng.reset(seed=3)
        eng.set_policy(rec.weights, hidden=hidden, lanes_per_policy=lpp)
        rec.launch(eng, tables, True, lane)
        parts.append(eng)
    rec.check(gymrs, tables, True, "two engines")
    for eng in parts + [rec.eng]:
        eng.close()


def test_refusals_and_no_steps(gymrs):
    rec = Record(gymrs, 0, 0, 260, 3, 3)
    eng, tables = rec.eng, rec.tables()
    good = dict(record=rec.record(), start_obs=rec.start.data_ptr(), grad=tables[0].data_ptr(), excluded=tables[1].data_ptr(), sums=tables[2].data_ptr(),
                counts=tables[3].data_ptr(), old_prob=rec.old.data_ptr(), coef=COEF, scale=1.0)
    no_actions = dict(rec.record(), actions=0)
    nan, inf = float("nan"), float("inf")
    cases = [("flag", dict(flags=1)), ("scale", dict(scale=nan)), ("scale", dict(scale=-1.0)), ("coef", dict(coef=nan)), ("coef", dict(coef=inf)),
             ("record.obs", dict(record=dict(rec.record(), obs=0))), ("record.actions", dict(record=no_actions)), ("start_obs", dict(start_obs=0)),
             ("grad is NULL", dict(grad=0)), ("excluded is NULL", dict(excluded=0)), ("sums is NULL", dict(sums=0)),
             ("16-byte aligned", dict(old_prob=rec.old.data_ptr() + 4)), ("16-byte aligned", dict(start_obs=rec.start.data_ptr() + 8)),
             ("8-byte aligned", dict(sums=tables[2].data_ptr() + 4)), ("8-byte aligned", dict(counts=tables[3].data_ptr() + 4)),
             ("lane_stride", dict(record=dict(rec.record(), lane_stride=256))), ("lane_stride", dict(record=dict(rec.record(), lane_stride=rec.stride + 8)))]
    for word, change in cases:
        with pytest.raises(gymrs.GymrsError, match=word) as err:
            eng.entropy_gradient(3, **dict(good, **change))
        assert err.value.status == EINVAL and "gymrs_entropy_gradient" in str(err.value), word
    eng.entropy_gradient(3, **dict(good, record=no_actions, old_prob=None))  # actions may be NULL when old_prob is
    eng.sync()
    first = [t.clone() for t in tables]
    assert (first[0] != FILL).any()
    eng.entropy_gradient(0, **good)  # a no-op after the checks
    eng.sync()
    assert all(torch.equal(a, b) for a, b in zip(first, tables))
    eng.set_policy(None)
    with pytest.raises(gymrs.GymrsError, match="gymrs_set_policy"):
        eng.entropy_gradient(3, **good)
    eng.close()
    pend = gymrs.BatchedEngine(gymrs.PENDULUM, 256, flags=A | T)
    pend.reset(seed=1)
    with pytest.raises(gymrs.GymrsError, match="Pendulum"):
        pend.entropy_gradient(3, **good)
    pend.close()
