"""gymrs_replay_priority and gymrs_replay_draw (host only, no GPU) against tests/replay_ref.py, bit for bit; every sample in its
stratum; the refusals that need no engine."""
import ctypes as C

import numpy as np
import pytest
import replay_ref as ref

NAN, INF = float("nan"), float("inf")
EPS, CAP = 1e-3, 4.0
COUNTS = (5, 4096, 4100, 3 * 4096 + 1)


@pytest.mark.parametrize("alpha", [0.0, 0.6, 1.0])
def test_priority_equals_the_restatement(gymrs, alpha):
    above = float(np.nextafter(np.float32(CAP), np.float32(INF)))
    td = [0.0, -0.0, 1e-45, -1e-40, EPS, -EPS, CAP, above, CAP - EPS, 1e30, INF, -INF, NAN, -NAN, -0.37, 2.5] + np.geomspace(1e-6, 8.0, 40).tolist()
    got = np.array([gymrs.replay_priority(t, alpha=alpha, eps=EPS, cap=CAP) for t in td], np.uint32)
    want = ref.priority(td, alpha, EPS, CAP)
    assert np.array_equal(got, want), np.argwhere(got != want)[:4]
    assert got.min() >= 1 and got.max() == ref.MAX_P and (got[[6, 7, 10, 11, 12, 13]] == ref.MAX_P).all()  # cap, above it, inf, NaN
    if alpha == 0.0:
        assert (got == ref.MAX_P).all()  # uniform replay
    else:
        assert got[0] < got[15] < got[6] and got[14] == gymrs.replay_priority(0.37, alpha=alpha, eps=EPS, cap=CAP)
    assert gymrs.replay_priority(0.0, alpha=1.0, eps=2.0**-126, cap=3e38) == 1  # the far tail weighs nothing: clamped to 1


@pytest.mark.parametrize("count", COUNTS)
def test_draw_equals_the_restatement_and_stays_in_its_stratum(gymrs, count):
    for name, prio in ref.patterns(count).items():
        prefix = np.concatenate([[0], np.cumsum(prio.astype(np.uint64))]).astype(np.uint64)
        for n_samples in (1, 7, count, 3 * count):
            idx, total = gymrs.replay_draw(prio, n_samples, seed=0xFEEDFACE12345678, draw=(1 << 33) + 5)
            want, want_total = ref.draw(prio, n_samples, 0xFEEDFACE12345678, (1 << 33) + 5)
            assert total == want_total == int(prefix[-1]) and np.array_equal(idx, want), (name, n_samples, np.argwhere(idx != want)[:4])
            if total == 0:
                assert (idx == ref.NONE).all()
                continue
            assert (prio[idx] > 0).all() and (np.diff(idx.astype(np.int64)) >= 0).all()
            for j, (lo, w) in enumerate(ref.strata(total, n_samples)):  # the entry's mass meets the stratum (an empty one: the last mass)
                a, b = int(prefix[idx[j]]), int(prefix[idx[j] + 1])
                assert (a < lo + w and b > lo) if w else b == total, (name, n_samples, j)


def test_refusals(gymrs):
    lib, out, idx, total = gymrs.load_library(), C.c_uint32(), (C.c_uint32 * 4)(), C.c_uint64()
    for alpha, eps, cap in ((-0.1, EPS, CAP), (1.5, EPS, CAP), (NAN, EPS, CAP), (0.6, 0.0, CAP), (0.6, 2.0**-127, CAP), (0.6, 5.0, CAP), (0.6, EPS, INF),
                            (0.6, NAN, CAP), (0.6, EPS, NAN)):
        assert lib.gymrs_replay_priority(1.0, alpha, eps, cap, C.byref(out)) == 1 and b"gymrs_replay_priority" in lib.gymrs_last_error()
    assert lib.gymrs_replay_priority(1.0, 0.6, EPS, CAP, None) == 1
    prio = (C.c_uint32 * 4)(1, 2, 3, 4)
    for args in ((None, 4, 4, 0, 0, idx, C.byref(total)), (prio, 4, 4, 0, 0, None, C.byref(total)), (prio, 0, 4, 0, 0, idx, C.byref(total)),
                 (prio, (1 << 26) + 1, 4, 0, 0, idx, C.byref(total)), (prio, 4, 0, 0, 0, idx, C.byref(total)),
                 (prio, 4, (1 << 24) + 1, 0, 0, idx, C.byref(total))):
        assert lib.gymrs_replay_draw(*args) == 1 and b"gymrs_replay_draw" in lib.gymrs_last_error()
    assert lib.gymrs_replay_draw(prio, 4, 4, 0, 0, idx, None) == 0  # total is optional on the host
    desc = gymrs.ReplayUpdateDesc()
    for name in ("gymrs_replay_push", "gymrs_replay_sample", "gymrs_replay_update"):
        assert getattr(lib, name)(None, C.byref(desc)) == 1 and name.encode() in lib.gymrs_last_error()
    assert (C.sizeof(gymrs.Replay), C.sizeof(gymrs.ReplayPushDesc), C.sizeof(gymrs.ReplaySampleDesc), C.sizeof(gymrs.ReplayUpdateDesc)) == (56, 152, 176, 104)
