"""gymrs_es_rank_utilities (host only; include/gymrs_amd.h, "Evolution strategies", centred ranks) against numpy, bit for bit: the rule
is integers up to one f64 division and one cast, so nothing here has a tolerance.  `ranks` and `records_for` are what
tests/test_gpu_es_ranks.py checks the device against as well."""
import ctypes as C

import numpy as np
import pytest

INVALID = 0xFFFFFFFF
PATTERNS = ["equal", "distinct", "ties", "half invalid", "one valid", "none valid", "negative", "huge"]


def ranks(records):
    """(u f32 [P], rank2 uint32 [P]) from int64 records [P][8] (return_sum, return_sq_sum, episodes, ...)"""
    valid = records[:, 2] > 0
    with np.errstate(all="ignore"):
        F = records[:, 0].astype(np.float64) / records[:, 2].astype(np.float64)  # the rule's one IEEE division
    ordered, n = np.sort(F[valid]), int(valid.sum())
    rank2 = np.searchsorted(ordered, F, "left") + np.searchsorted(ordered, F, "right") - 1  # 2 * less + equal - 1
    with np.errstate(all="ignore"):
        u = ((rank2 - (n - 1)).astype(np.float64) / np.float64(2 * (n - 1))).astype(np.float32)
    return np.where(valid & (n > 1), u, np.float32(0)), np.where(valid, rank2, INVALID).astype(np.uint32)


def records_for(pattern, P, seed=7):
    rng = np.random.default_rng([seed, P])
    rec = np.zeros((P, 8), np.int64)
    rec[:, 2] = rng.integers(1, 4, P)
    if pattern == "equal":
        rec[:, 0] = 17 * rec[:, 2]
    elif pattern == "distinct":
        rec[:, 0], rec[:, 2] = rng.permutation(P) - P // 2, 1
    elif pattern == "negative":
        rec[:, 0] = -rng.integers(0, 600, P)  # (0 among them: +0.0 and no -0.0)
    elif pattern == "huge":  # distinct rationals near +-2^62 that round to equal doubles: they tie by the rule
        rec[:, 2] = np.where(rng.random(P) < 0.5, 1, 3)
        rec[:, 0] = rng.choice([-1, 1], P) * (2**62 - rng.integers(0, 4, P))
    else:
        rec[:, 0] = rng.choice([-200, 9, 10, 57, 500], P) * rec[:, 2]  # returns drawn from 5 values
    if pattern == "half invalid":
        rec[rng.permutation(P)[:(P + 1) // 2], 2] = 0
    elif pattern in ("one valid", "none valid"):
        rec[:, 2] = 0
        rec[P // 2, 2] = pattern == "one valid"
    return rec


@pytest.mark.parametrize("P", [1, 2, 3, 64])
@pytest.mark.parametrize("pattern", PATTERNS)
def test_rank_utilities_equal_numpy(gymrs, pattern, P):
    rec = records_for(pattern, P)
    (u, rank2), (want_u, want_rank2) = gymrs.es_rank_utilities(rec), ranks(rec)
    assert np.array_equal(u.view(np.uint32), want_u.view(np.uint32)) and np.array_equal(rank2, want_rank2)
    valid = rec[:, 2] > 0
    n = int(valid.sum())
    assert (rank2[valid].astype(np.int64) - (n - 1)).sum() == 0 and (np.abs(u) <= 0.5).all() and not u.view(np.uint32)[~valid].any()
    if pattern == "huge" and P == 64:
        assert len(np.unique(rec[:, 0])) > len(np.unique(rank2))  # sums that differ share a rank
    if pattern == "distinct":
        assert len(np.unique(rank2)) == P


def test_refusals(gymrs):
    lib, rec, u = gymrs.load_library(), records_for("ties", 4), np.empty(4, np.float32)
    rp, up = rec.ctypes.data_as(C.c_void_p), u.ctypes.data_as(C.POINTER(C.c_float))
    assert lib.gymrs_es_rank_utilities(rp, 4, up, None) == 0  # rank2_out may be NULL
    assert np.array_equal(u.view(np.uint32), ranks(rec)[0].view(np.uint32))
    for args in [(None, 4, up, None), (rp, 4, None, None), (rp, 0, up, None), (rp, gymrs.ES_MAX_POLICIES + 1, up, None)]:
        assert lib.gymrs_es_rank_utilities(*args) == 1 and b"gymrs_es_rank_utilities" in lib.gymrs_last_error()
