"""gymrs_q_lane (host only, no GPU) against the f64 calculus of tests/q_ref.py: the TD errors and the summed table lie within the
reference's own error bound, the planted lanes land in `excluded`, and the host-side refusals."""
import ctypes as C

import numpy as np
import pytest
import q_ref as ref

INF = float("inf")


def lanes(gymrs, c):
    """q [n][S], excluded [n], td [K][n], counts [n][2] of every lane of the case by gymrs_q_lane"""
    idx = ref.set_index(c)
    x, xn = ref.transitions(c)
    out = [gymrs.q_lane(c.kind, c.hidden, c.weights[idx[i]], c.target[idx[i]], x[:, :, i], xn[:, :, i], c.actions[:, i], c.reward[:, i], c.done[:, i],
                        gamma=c.gamma, kappa=c.kappa, flags=c.flags) for i in range(c.n)]
    return (np.stack([o[0] for o in out]), np.array([o[1] for o in out], np.uint64), np.stack([o[2] for o in out], axis=1),
            np.stack([o[3] for o in out]))


def check_against_calculus(c, q, excluded, td, counts):
    """q [n_sets][S] int64 summed per set, excluded [n_sets], td [K][n], counts [n_sets][2]"""
    r = ref.reference(c)
    grad, bound, want_excluded, want_counts = ref.table(c, r)
    finite = np.isfinite(r.td)
    assert (np.abs(td[finite].astype(np.float64) - r.td[finite]) <= 2.0**-22 * r.err[finite]).all() and not np.isfinite(td[~finite]).any()
    assert (np.abs(q * 2.0**-24 - grad) <= ref.tolerance(c, bound)).all() and grad.any()
    assert np.array_equal(excluded, want_excluded) and np.array_equal(counts, want_counts)


@pytest.mark.parametrize("gamma,kappa", [(0.97, 1.0), (1.0, INF)])
@pytest.mark.parametrize("flags", [0, ref.DOUBLE])
@pytest.mark.parametrize("hidden", [0, 5, 64])
@pytest.mark.parametrize("kind", [0, 1])
def test_the_lane_equals_the_calculus(gymrs, kind, hidden, flags, gamma, kappa):
    c = ref.synthetic(kind, 4, 7, hidden, flags, gamma, kappa)
    q, excluded, td, counts = lanes(gymrs, c)
    check_against_calculus(c, q.sum(axis=0)[None], excluded.sum()[None], td, counts.sum(axis=0)[None])
    p = c.planted
    assert excluded[p["nan"]] > 0 and (kappa != INF or (excluded[p["inf"]] > 0 and excluded[p["big"]] > 0))


def test_refusals(gymrs):
    lib = gymrs.load_library()
    f, b = (C.c_float * 10)(), (C.c_uint8 * 1)()
    q, ex = (C.c_int64 * 10)(), C.c_uint64()
    good = [0, 0, 0, 0.9, 1.0, f, f, 1, f, f, b, f, b, q, C.pointer(ex), None, None]  # kind, hidden, flags, gamma, kappa, then the arrays
    assert lib.gymrs_q_lane(*good) == 0  # td and counts are optional
    nan = float("nan")
    bad = [(0, 2, b"Pendulum"), (1, 65, b"hidden"), (2, 2, b"flag"), (3, 1.5, b"gamma"), (3, nan, b"gamma"), (3, -0.1, b"gamma"), (4, 0.0, b"kappa"),
           (4, -1.0, b"kappa"), (4, nan, b"kappa")] + [(i, None, b"NULL") for i in (5, 6, 8, 9, 10, 11, 12, 13, 14)]
    for i, value, word in bad:
        args = list(good)
        args[i] = value
        assert lib.gymrs_q_lane(*args) == 1 and b"gymrs_q_lane" in lib.gymrs_last_error() and word in lib.gymrs_last_error(), (i, value)
