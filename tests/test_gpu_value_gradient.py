"""gymrs_value_gradient on the device against gymrs_value_lane (host only; tests/test_value_host.py holds it to the numpy restatement of
the rule) summed in Python integers: grad, excluded, sums, counts and values bit for bit.  Rows are wider than n_envs with NaN in the
padding lanes, every table starts from non-zero words (the call ADDS), and `values` keeps the bytes of its padding."""
import advantages_ref as adv
import numpy as np
import pytest
import torch
import value_ref as vr
from advantages_ref import SENTINEL

pytestmark = pytest.mark.gpu
DEV, EINVAL, FILL, CLIP, GID0 = "cuda:0", 1, 5, 0.2, 7
F = np.float32


class Case:
    def __init__(self, gymrs, kind, hidden, n, gathered, steps):
        self.kind, self.hidden, self.n, self.steps = kind, hidden, n, steps
        self.n_sets, self.lpp = (2, 3) if gathered else (1, n)
        self.stride = s = (n + 15) // 16 * 16 + 16  # > n_envs
        self.w = adv.make_critics(kind, hidden, self.n_sets, 60 + hidden)
        self.x, rn, on = vr.draw(kind, hidden, n, steps, 2)
        self.set = [((GID0 + i) // self.lpp) % self.n_sets for i in range(n)]
        v = np.stack([gymrs.value_lane(kind, hidden, self.w[self.set[i]], self.x[:, :, i], np.zeros(steps, F))[4] for i in range(n)], axis=1)
        self.R, self.vo = (v + rn).astype(F), (v + on).astype(F)
        self.R[0, n // 2] = np.nan  # one lane that is excluded
        self.vo[0, 0] = np.nan  # compares false both ways: neither clipped nor cut (an even lane-step, which value_ref.draw never cuts)
        pad = lambda a: torch.from_numpy(np.concatenate([a, np.full(a.shape[:-1] + (s - n,), np.nan, F)], axis=-1)).to(DEV)  # noqa: E731
        self.start, self.obs, self.dR, self.dvo = pad(self.x[0]), pad(np.concatenate([self.x[1:], self.x[:1]])), pad(self.R), pad(self.vo)
        self.eng = gymrs.BatchedEngine(kind, n, global_env_offset=GID0, flags=1)
        self.eng.reset(seed=1)
        self.eng.set_critic(self.w, hidden=hidden, lanes_per_critic=self.lpp)

    def run(self, gymrs, clipped, with_values=True):
        size = self.w.shape[1]
        grad, excluded, sums, counts = (torch.full(shape, FILL, dtype=torch.int64, device=DEV) for shape in ((self.n_sets, size), (self.n_sets,), (self.n_sets, 2), (self.n_sets, 2)))
        values = torch.full((self.steps, self.stride), SENTINEL, dtype=torch.int32, device=DEV)
        torch.cuda.synchronize()
        self.eng.value_gradient(self.steps, record=dict(obs=self.obs.data_ptr(), truncated=0, lane_stride=self.stride), start_obs=self.start.data_ptr(),
                                returns=self.dR.data_ptr(), old_values=self.dvo.data_ptr() if clipped else None, clip=CLIP if clipped else None,
                                values=values.data_ptr() if with_values else None, grad=grad.data_ptr(), excluded=excluded.data_ptr(),
                                sums=sums.data_ptr(), counts=counts.data_ptr())
        self.eng.sync()
        want = [[[0] * size for _ in range(self.n_sets)], [0] * self.n_sets, [[0, 0] for _ in range(self.n_sets)], [[0, 0] for _ in range(self.n_sets)]]
        wv = np.empty((self.steps, self.n), F)
        for i, m in enumerate(self.set):
            q, ex, sm, ct, wv[:, i] = gymrs.value_lane(self.kind, self.hidden, self.w[m], self.x[:, :, i], self.R[:, i], self.vo[:, i] if clipped else None, clip=CLIP)
            want[0][m] = [a + int(b) for a, b in zip(want[0][m], q)]
            want[1][m] += ex
            want[2][m] = [a + int(b) for a, b in zip(want[2][m], sm)]
            want[3][m] = [a + int(b) for a, b in zip(want[3][m], ct)]
        for t, w, name in zip((grad, excluded, sums, counts), want, ("grad", "excluded", "sums", "counts")):
            assert np.array_equal(t.cpu().numpy().astype(object) - FILL, np.array(w, dtype=object)), (name, clipped, with_values)
        got = values.cpu().numpy().view(np.uint32)
        if with_values:
            assert np.array_equal(got[:, :self.n], wv.view(np.uint32)) and (got[:, self.n:] == SENTINEL).all(), "values"
        else:
            assert (got == SENTINEL).all()
        seen, cut = sum(c[0] for c in want[3]), sum(c[1] for c in want[3])
        assert seen == self.n * self.steps and sum(want[1]) > 0 and np.array(want[0], dtype=object).any()
        assert (0.25 * seen <= cut < seen) if clipped else cut == 0, (cut, seen)  # at least a quarter, not all, of the lane-steps are cut


@pytest.mark.parametrize("gathered", [False, True])
@pytest.mark.parametrize("hidden", [0, 1, 7, 64])  # affine; one ragged chunk; two chunks, the last ragged; all chunks
@pytest.mark.parametrize("n", [5, 256, 259])  # a ragged wave only; exactly one full wave of 4-lane items; full plus ragged
@pytest.mark.parametrize("kind", [0, 1])
def test_the_tables_equal_the_host_lane_summed(gymrs, kind, n, hidden, gathered):
    for steps in (1, 3):  # no prefetch; prefetch with the last row
        case = Case(gymrs, kind, hidden, n, gathered, steps)
        for clipped in (False, True):
            case.run(gymrs, clipped)
        if hidden and steps == 3:
            case.run(gymrs, True, with_values=False)  # the v row is the engine's scratch
        case.eng.close()


def test_refusals_and_no_steps(gymrs):
    case = Case(gymrs, 0, 7, 259, True, 3)
    eng, tab = case.eng, torch.zeros((2, 64), dtype=torch.int64, device=DEV)
    rec = dict(obs=case.obs.data_ptr(), truncated=0, lane_stride=case.stride)
    good = dict(record=rec, start_obs=case.start.data_ptr(), returns=case.dR.data_ptr(), old_values=case.dvo.data_ptr(), clip=CLIP, grad=tab.data_ptr(),
                excluded=tab[1].data_ptr(), sums=tab[1, 8:].data_ptr(), counts=tab[1, 16:].data_ptr())
    nan, inf = float("nan"), float("inf")
    cases = [("flag", dict(flags=2)), ("clip", dict(clip=nan)), ("clip", dict(clip=inf)), ("clip", dict(clip=0.0)), ("old_values is NULL", dict(old_values=None)),
             ("old_values without", dict(flags=0)), ("record.obs", dict(record=dict(rec, obs=0))), ("start_obs", dict(start_obs=0)), ("returns is NULL", dict(returns=0)),
             ("grad is NULL", dict(grad=0)), ("excluded is NULL", dict(excluded=0)), ("alias", dict(values=case.dR.data_ptr())), ("alias", dict(values=case.dvo.data_ptr())),
             ("16-byte aligned", dict(returns=case.dR.data_ptr() + 4)), ("8-byte aligned", dict(sums=tab.data_ptr() + 4)),
             ("lane_stride", dict(record=dict(rec, lane_stride=256))), ("lane_stride", dict(record=dict(rec, lane_stride=case.stride + 8)))]
    for word, change in cases:
        with pytest.raises(gymrs.GymrsError, match=word) as err:
            eng.value_gradient(3, **dict(good, **change))
        assert err.value.status == EINVAL and "gymrs_value_gradient" in str(err.value), word
    eng.value_gradient(0, **good)  # a no-op after the checks
    eng.sync()
    assert not tab.any()
    eng.set_critic(None)
    with pytest.raises(gymrs.GymrsError, match="gymrs_set_critic"):
        eng.value_gradient(3, **good)
    eng.close()
    pend = gymrs.BatchedEngine(gymrs.PENDULUM, 256, flags=5)
    pend.reset(seed=1)
    with pytest.raises(gymrs.GymrsError, match="Pendulum"):
        pend.value_gradient(3, **good)
    pend.close()
