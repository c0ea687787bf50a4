"""gymrs_vtrace on the device against gymrs_vtrace_lane per lane, bit for bit; padding lanes keep a sentinel, counts start non-zero, ends sit on pass edges."""
import re
from pathlib import Path

import advantages_ref as adv
import closed_loop_ref as cl
import numpy as np
import pytest
import torch
import vtrace_ref as vt
from advantages_ref import SENTINEL

pytestmark = pytest.mark.gpu
DEV, EINVAL, FILL, GID0, INF, F = "cuda:0", 1, 5, 7, float("inf"), np.float32
GAMMA, LAM, SCALE, BARS = 0.97, 0.9, float(F(1.4426950408889634 / 4.0)), (1.0, 2.0, 0.5)
R = int(re.search(r"kVtraceRows = (\d+)", (Path(__file__).resolve().parent.parent / "gym-rs_amd" / "csrc" / "gymrs_kernels.h").read_text()).group(1))
# (policy sets, lanes), (critic sets, lanes), widths: one set; every tile gathers; blocks wider than a tile: uniform tiles with n_policies > 1 beside gathering ones
SETS = {"one": ((1, 1 << 20), (1, 1 << 20), None), "gathered": ((3, 7), (2, 5), None), "blocks": ((2, 96), (2, 128), (7, 64))}


class Case:
    def __init__(self, gymrs, kind, n, steps, sets, specials=True):
        self.kind, self.n, self.steps, self.A = kind, n, steps, cl.DIMS[kind][1]
        (self.np_, self.lpp), (self.nc, self.lpc), widths = SETS[sets]
        self.hp, self.hc = widths or ((0, 7) if (kind + (sets == "one")) % 2 else (64, 0))  # every code copy meets an affine and a hidden network
        self.wp, self.wc = cl.make_weights(kind, self.hp, self.np_, 40 + self.hp), adv.make_critics(kind, self.hc, self.nc, 50 + self.hc)
        self.stride = s = (n + 15) // 16 * 16 + 16  # > n_envs
        self.r = r = vt.record(kind, n, steps, 5, end_rows=[k for k in (0, steps - 1, steps - R, steps - R - 1) if k >= 0])
        self.po = (0.1 + 0.9 * np.random.default_rng(steps).random((steps, n))).astype(F)  # ratios on both sides of every bar
        if specials:
            self.po[steps // 2, 2], r["actions"][0, 3] = np.nan, self.A  # one NaN ratio; one action that is none of the A
        pad = lambda a, fill=np.nan: torch.from_numpy(np.concatenate([a, np.full(a.shape[:-1] + (s - n,), fill, a.dtype)], axis=-1)).to(DEV)  # noqa: E731
        self.dev = {k: pad(r[k]) for k in ("obs", "start_obs", "final_obs", "reward")}
        self.dev.update({k: pad(r[k], 9) for k in ("actions", "done", "truncated")}, old_prob=pad(self.po))
        self.outs = {k: torch.full((steps, s), SENTINEL, dtype=torch.int32, device=DEV) for k in ("vs", "pg_advantages", "values", "prob")}
        self.counts = torch.full((self.np_, 3), FILL, dtype=torch.int64, device=DEV)
        torch.cuda.synchronize()  # the engines run on streams of their own

    def engine(self, gymrs, first=0, count=None):
        eng = gymrs.BatchedEngine(self.kind, count or self.n, global_env_offset=GID0 + first, flags=1)
        eng.reset(seed=1)
        eng.set_policy(self.wp, hidden=self.hp, lanes_per_policy=self.lpp)
        eng.set_critic(self.wc, hidden=self.hc, lanes_per_critic=self.lpc)
        return eng

    def args(self, first=0, final=True, bars=BARS):
        at = lambda t: t.data_ptr() + 4 * first if t.element_size() == 4 else t.data_ptr() + first  # noqa: E731  (a later engine's lanes start here)
        rec = dict({k: at(self.dev[k]) for k in ("obs", "actions", "reward", "done", "truncated")}, lane_stride=self.stride)
        return dict(record=rec, start_obs=at(self.dev["start_obs"]), final_obs=at(self.dev["final_obs"]) if final else None, old_prob=at(self.dev["old_prob"]),
                    counts=self.counts.data_ptr(), gamma=GAMMA, lam=LAM, scale=SCALE, rho_bar=bars[0], c_bar=bars[1], pg_rho_bar=bars[2],
                    **{k: at(t) for k, t in self.outs.items()})

    def check(self, gymrs, final=True, bars=BARS):
        want_counts = np.zeros((self.np_, 3), np.int64)
        for i in range(self.n):
            p, c = ((GID0 + i) // self.lpp) % self.np_, ((GID0 + i) // self.lpc) % self.nc
            got = gymrs.vtrace_lane(self.kind, self.hp, self.hc, self.wp[p], self.wc[c], *vt.lane_inputs(self.r, i, final), self.po[:, i], gamma=GAMMA, lam=LAM,
                                    scale=SCALE, rho_bar=bars[0], c_bar=bars[1], pg_rho_bar=bars[2])
            for name, w in zip(("vs", "pg_advantages", "values", "prob"), got):
                assert np.array_equal(self.outs[name][:, i].cpu().numpy().view(np.uint32), w.view(np.uint32)), (name, i)
            want_counts[p] += got[4].astype(np.int64)
        assert all((t[:, self.n:] == SENTINEL).all() for t in self.outs.values()), "padding"
        assert np.array_equal(self.counts.cpu().numpy() - FILL, want_counts), "counts"


@pytest.mark.parametrize("sets", list(SETS))
@pytest.mark.parametrize("steps", [1, R - 1, R, R + 1, 2 * R + 1])
@pytest.mark.parametrize("n", [5, 64, 259])  # a ragged tile; one full tile; full tiles plus a ragged one
@pytest.mark.parametrize("kind", [0, 1])
def test_rows_and_counts_equal_the_host_lane(gymrs, kind, n, steps, sets):
    case = Case(gymrs, kind, n, steps, sets)
    eng = case.engine(gymrs)
    eng.vtrace(steps, **case.args())
    eng.sync()
    case.check(gymrs)
    eng.close()


@pytest.mark.parametrize("kind", [0, 1])
def test_equal_probabilities_give_gae_on_the_device(gymrs, kind):
    """old_prob = the prob row of a first call, bars >= 1: vs, values = gymrs_advantages' returns, values (here without final observations)"""
    case = Case(gymrs, kind, 259, 2 * R + 1, "gathered", specials=False)
    eng = case.engine(gymrs)
    a = case.args(final=False, bars=(1.0, INF, 2.0))
    eng.vtrace(case.steps, **a)
    eng.sync()
    case.dev["old_prob"].copy_(case.outs["prob"].view(torch.float32))
    case.counts.fill_(FILL)
    torch.cuda.synchronize()
    eng.vtrace(case.steps, **a)
    ret, val = (torch.zeros((case.steps, case.stride), dtype=torch.float32, device=DEV) for _ in range(2))
    eng.advantages(case.steps, record=a["record"], start_obs=a["start_obs"], advantages=case.outs["pg_advantages"].data_ptr(), returns=ret.data_ptr(),
                   values=val.data_ptr(), gamma=GAMMA, lam=LAM, critic=True)
    eng.sync()
    assert all(torch.equal(case.outs[name][:, :259], t.view(torch.int32)[:, :259]) for name, t in (("vs", ret), ("values", val)))
    assert (case.counts[:, 1:] == FILL).all()  # no ratio above 1
    eng.close()


def test_two_engines_cut_the_batch(gymrs):
    case = Case(gymrs, 0, 259, R + 1, "gathered")
    one, two = case.engine(gymrs, 0, 96), case.engine(gymrs, 96, 163)  # (byte rows stay 16-byte aligned at lane 96)
    one.vtrace(case.steps, **case.args(0)), two.vtrace(case.steps, **case.args(96)), one.sync(), two.sync()
    case.check(gymrs)  # the same rows, and counts that add up to one engine's
    one.close(), two.close()


def test_refusals_and_no_steps(gymrs):
    case = Case(gymrs, 0, 259, 3, "gathered")
    eng, good, nan = case.engine(gymrs), case.args(), float("nan")
    rec = good["record"]
    cases = [("flags", dict(flags=1)), ("gamma", dict(gamma=1.5)), ("lambda", dict(lam=-0.5)), ("scale", dict(scale=INF)),
             ("rho_bar", dict(rho_bar=0.0)), ("c_bar", dict(c_bar=nan)), ("pg_rho_bar", dict(pg_rho_bar=-1.0)), ("record.obs", dict(record=dict(rec, obs=0))),
             ("record.actions", dict(record=dict(rec, actions=0))), ("record.reward", dict(record=dict(rec, reward=0))), ("record.done", dict(record=dict(rec, done=0))),
             ("start_obs", dict(start_obs=0)), ("old_prob is NULL", dict(old_prob=0)), ("vs is NULL", dict(vs=0)), ("pg_advantages is NULL", dict(pg_advantages=0)),
             ("alias", dict(prob=good["old_prob"])), ("16-byte aligned", dict(vs=good["vs"] + 4)), ("8-byte aligned", dict(counts=good["counts"] + 4)),
             ("lane_stride", dict(record=dict(rec, lane_stride=256))), ("lane_stride", dict(record=dict(rec, lane_stride=case.stride + 8)))]
    for word, change in cases:
        with pytest.raises(gymrs.GymrsError, match=word) as err:
            eng.vtrace(3, **dict(good, **change))
        assert err.value.status == EINVAL and "gymrs_vtrace" in str(err.value), word
    eng.vtrace(3, **dict(good, rho_bar=INF, values=None, prob=None, counts=None))  # +inf is no clipping; three outputs are optional
    eng.vtrace(0, **dict(good, vs=case.outs["values"].data_ptr()))  # a no-op after the checks
    eng.sync()
    assert (case.outs["values"] == SENTINEL).all() and (case.counts == FILL).all() and (case.outs["vs"][:, :259] != SENTINEL).any()
    eng.set_critic(None)
    bare, pend = gymrs.BatchedEngine(0, 259, flags=1), gymrs.BatchedEngine(gymrs.PENDULUM, 256, flags=5)
    for e, word in ((eng, "gymrs_set_critic"), (bare, "gymrs_set_policy"), (pend, "Pendulum")):
        e.reset(seed=1)
        with pytest.raises(gymrs.GymrsError, match=word):
            e.vtrace(3, **good)
        e.close()
