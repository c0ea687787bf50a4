"""gymrs_vtrace_lane without a GPU: the f32 restatement bit for bit, the f64 textbook form within a measured tolerance, GAE, refusals, symbols."""
import ctypes as C
import re
from importlib import import_module
from pathlib import Path

import advantages_ref as adv
import closed_loop_ref as cl
import numpy as np
import pytest
import vtrace_ref as vt
from closed_loop_ref import bits

ROOT = Path(__file__).resolve().parent.parent
F, EINVAL, INF = np.float32, 1, float("inf")
GAMMA, LAM, SCALE, STEPS = 0.97, 0.9, float(F(1.4426950408889634 / 4.0)), 12
WIDTHS = [(0, 0), (7, 64), (64, 7)]
BARS = [(1.0, 1.0, 1.0), (INF, INF, INF), (0.5, 2.0, 1.0)]


def lane_case(gymrs, kind, hp, hc, specials):
    r = vt.record(kind, 4, STEPS, 3, end_rows=(0, STEPS - 1, 5))
    wp, wc = cl.make_weights(kind, hp, 1, 40 + hp)[0], adv.make_critics(kind, hc, 1, 50 + hc)[0]
    ins = vt.lane_inputs(r, 1 if specials else 2)
    pa = gymrs.vtrace_lane(kind, hp, hc, wp, wc, *ins, np.ones(STEPS, F), gamma=GAMMA, lam=LAM, scale=SCALE)[3]
    po = (pa * np.resize(np.array([1.0, 0.3, 2.5, 0.7, 4.0], F), STEPS)).astype(F)  # every bar clips some steps and spares others
    if specials:
        po[3], ins[2][7] = np.nan, cl.DIMS[kind][1]  # a NaN ratio; an action that is none of the A
    return wp, wc, ins, po


@pytest.mark.parametrize("bars", BARS)
@pytest.mark.parametrize("hp,hc", WIDTHS)
@pytest.mark.parametrize("kind", [0, 1])
def test_lane_equals_the_f32_restatement_and_meets_the_textbook_form(gymrs, kind, hp, hc, bars):
    for specials in (True, False):
        wp, wc, ins, po = lane_case(gymrs, kind, hp, hc, specials)
        got = gymrs.vtrace_lane(kind, hp, hc, wp, wc, *ins, po, gamma=GAMMA, lam=LAM, scale=SCALE, rho_bar=bars[0], c_bar=bars[1], pg_rho_bar=bars[2])
        want = vt.lane32(kind, hp, hc, wp, wc, *ins, po, GAMMA, LAM, SCALE, bars)
        assert [np.array_equal(bits(g), bits(w)) for g, w in zip(got[:4], want[:4])] == [True] * 4, specials  # vs, pg, values, prob
        assert got[4].tolist() == want[4] and 0 < want[4][0] and (want[4][1] > 0) == (bars[0] < INF)
    vs64, pg64 = vt.lane64(kind, hp, hc, wp, wc, *ins, po, GAMMA, LAM, SCALE, bars)
    err = max(np.abs(got[0] - vs64).max(), np.abs(got[1] - pg64).max()) / max(1.0, np.abs(vs64).max(), np.abs(pg64).max())
    # the f32 restatement's largest distance from the f64 form over these 18 cases, relative to the largest target: 1.75e-7; times 4 for
    # the different rounding order
    assert err <= 4 * 1.75e-7, err


@pytest.mark.parametrize("kind", [0, 1])
def test_equal_probabilities_give_gae(gymrs, kind):
    """old_prob == pa and bars >= 1: ratio == 1.0f, and vs / values are the returns / values of the advantages reference"""
    c = adv.synthetic(kind, 1, 17, 7, specials=False)  # 5 lanes, 3 critics, flags and final observations drawn
    _, ret, val = adv.reference(c)
    r = dict(start_obs=c.start_obs, obs=c.obs, final_obs=c.final_obs, ended=c.ended.astype(np.uint8), reward=c.reward, done=c.done,
             actions=np.resize(np.arange(cl.DIMS[kind][1], dtype=np.uint8), (17, c.n)))
    wp = cl.make_weights(kind, 7, 1, 4)[0]
    for i, m in enumerate(adv.critic_index(c)):
        ins = vt.lane_inputs(r, i)
        pa = gymrs.vtrace_lane(kind, 7, 7, wp, c.weights[m], *ins, np.ones(17, F), gamma=GAMMA, lam=LAM, scale=SCALE)[3]
        vs, _, values, _, counts = gymrs.vtrace_lane(kind, 7, 7, wp, c.weights[m], *ins, pa, gamma=GAMMA, lam=LAM, scale=SCALE, rho_bar=1.0, c_bar=2.0)
        assert np.array_equal(bits(vs), bits(ret[:, i])) and np.array_equal(bits(values), bits(val[:, i])) and counts.tolist() == [17, 0, 0]


def test_refusals(gymrs):
    lib = gymrs.load_library()
    wp, wc, x, f1, b1 = (C.c_float * 10)(), (C.c_float * 5)(), (C.c_float * 4)(), (C.c_float * 1)(0.5), (C.c_uint8 * 1)()
    ok = [0, 0, 0, wp, wc, 1, x, x, b1, f1, b1, b1, f1, 0.9, 0.9, 1.0, 1.0, 1.0, 1.0, *[(C.c_float * 1)() for _ in range(4)], (C.c_uint64 * 3)()]
    assert lib.gymrs_vtrace_lane(*ok) == 0
    changes = [(0, 2, b"Pendulum"), (1, 65, b"hidden"), (2, 65, b"hidden"), (13, float("nan"), b"gamma"), (13, 1.5, b"gamma"), (14, -0.1, b"lambda"), (15, INF, b"scale"),
               (15, -1.0, b"scale"), (16, 0.0, b"rho_bar"), (17, float("nan"), b"c_bar"), (18, -1.0, b"pg_rho_bar"), (22, f1, b"alias")]
    changes += [(at, None, b"NULL") for at in (3, 4, 6, 7, 8, 9, 10, 11, 12, 19, 20)]
    for at, value, word in changes:
        args = list(ok)
        args[at] = value
        assert lib.gymrs_vtrace_lane(*args) == EINVAL and word in lib.gymrs_last_error() and b"gymrs_vtrace_lane" in lib.gymrs_last_error(), (at, value)
    for at, value in ((16, INF), (21, None), (22, None), (23, None)):  # +inf does not clip; values, prob and counts are optional
        args = list(ok)
        args[at] = value
        assert lib.gymrs_vtrace_lane(*args) == 0, at
    assert lib.gymrs_vtrace(None, C.byref(gymrs.VtraceDesc())) == EINVAL and b"gymrs_vtrace" in lib.gymrs_last_error()


def test_symbols_signatures_and_mirrors(gymrs):
    text = (ROOT / "include" / "gymrs_amd.h").read_text()
    assert re.search(r"#define GYMRS_ABI_VERSION 3\b", text) and re.search(r"\} gymrs_vtrace_desc;\s*/\* 152 bytes \*/", text)
    assert re.search(r"^gymrs_status gymrs_vtrace\(gymrs_engine\* e, const gymrs_vtrace_desc\* d\);$", text, flags=re.M)
    lib, sigs = gymrs.load_library(), import_module("gym-rs_amd._lib").SIGNATURES
    assert hasattr(lib, "gymrs_vtrace") and hasattr(lib, "gymrs_vtrace_lane") and sigs["gymrs_vtrace"] == (C.c_int, [C.c_void_p, C.c_void_p])
    assert len(sigs["gymrs_vtrace_lane"][1]) == 24 and sigs["gymrs_vtrace_lane"][1][13:19] == [C.c_float] * 6
    assert C.sizeof(gymrs.VtraceDesc) == 152 and [getattr(gymrs.VtraceDesc, f).offset for f in ("record", "final_obs", "vs", "counts", "reserved")] == [32, 80, 104, 136, 144]
    assert "gymrs_vtrace_desc" in (ROOT / "include" / "gymrs_env.hpp").read_text() and callable(gymrs.BatchedEngine.vtrace)
