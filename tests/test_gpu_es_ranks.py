"""gymrs_es_ranks on the device against the numpy restatement of tests/test_es_ranks_host.py, bit for bit on u and on rank2: the rule is
exact, so nothing here has a tolerance.  The records are written straight into the evaluation table through its zero-copy view, after one
tiny evaluate_policy that brings the table into being.  P meets every path of the kernels: 1, 2, 63, 65 (networks of 2 .. 128 keys, a
ragged wave), 4095 / 4096 (one full tile, still the single launch), 4097 (the first two-launch case: a tile with one policy),
2 * 4096 + 5 and 5 * 4096 - 1 (an odd number of tiles through the double buffer)."""
import ctypes as C

import numpy as np
import pytest
import torch
from test_es_ranks_host import INVALID, ranks, records_for

pytestmark = pytest.mark.gpu
DEV, EINVAL, T, PAD, SENTINEL = "cuda:0", 1, 4096, 3, 0x5A5A5A5A
CASES = [(1, "ties"), (2, "distinct"), (63, "half invalid"), (63, "equal"), (65, "ties"), (65, "negative"), (4095, "ties"), (4096, "distinct"),
         (4096, "none valid"), (4097, "ties"), (4097, "half invalid"), (2 * T + 5, "same tiles"), (2 * T + 5, "huge"), (5 * T - 1, "invalid tile"),
         (5 * T - 1, "distinct"), (5 * T - 1, "one valid")]


class Column:
    """A zero-copy torch view of an engine's device array"""

    def __init__(self, ptr, n, typestr):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (ptr, False), "version": 3}


def case_records(pattern, P):
    if pattern == "same tiles":  # every full tile holds the same multiset: less and equal must add across tiles
        return records_for("ties", T)[np.arange(P) % T]
    rec = records_for("ties" if pattern == "invalid tile" else pattern, P)
    if pattern == "invalid tile":  # all the invalid policies in one tile
        rec[T:2 * T, 2] = 0
    return rec


@pytest.fixture(scope="module")
def eng(gymrs):
    e = gymrs.BatchedEngine(gymrs.CARTPOLE, 64, flags=7)
    e.reset(seed=1)
    yield e
    e.close()


def table_with(eng, rec):
    """The evaluation table of a fresh set of len(rec) policies, holding rec"""
    eng.set_policy(np.zeros((len(rec), 10), np.float32))
    eng.evaluate_policy(1, max_episode_steps=1)
    eng.sync()
    ptr, n = eng.policy_eval_ptr()
    assert n == len(rec)
    table = torch.as_tensor(Column(ptr, n * 8, "<i8"), device=DEV)
    table.copy_(torch.from_numpy(rec.reshape(-1)))
    torch.cuda.synchronize()  # torch copied on its stream; the engine reads on its own
    return table


def device_ranks(eng, P, with_rank2=True):
    """(u bits, rank2) as uint32 [P + PAD] rows the call wrote into sentinel-filled buffers"""
    out = torch.full((2, P + PAD), SENTINEL, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    eng.es_ranks(out[0].data_ptr(), out[1].data_ptr() if with_rank2 else 0)
    eng.sync()
    return out.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("P,pattern", CASES)
def test_device_equals_numpy(gymrs, eng, P, pattern):
    rec = case_records(pattern, P)
    table = table_with(eng, rec)
    want_u, want_rank2 = ranks(rec)
    for with_rank2 in (True, False):  # (the second call meets the scratch the first one left)
        u, rank2 = device_ranks(eng, P, with_rank2)
        bad = np.flatnonzero((u[:P] != want_u.view(np.uint32)) | (with_rank2 & (rank2[:P] != want_rank2)))
        assert bad.size == 0, (bad[:8], u[bad[:8]], want_u.view(np.uint32)[bad[:8]], rank2[bad[:8]], want_rank2[bad[:8]])
        assert (u[P:] == SENTINEL).all() and (rank2[P if with_rank2 else 0:] == SENTINEL).all()  # padding, and a rank2 that was not asked for
    assert np.array_equal(table.cpu().numpy(), rec.reshape(-1))  # the table is read only
    host_u, host_rank2 = gymrs.es_rank_utilities(rec)
    assert np.array_equal(host_u.view(np.uint32), u[:P]) and np.array_equal(host_rank2, want_rank2)
    assert pattern != "invalid tile" or (want_rank2[T:2 * T] == INVALID).all()


REFUSALS = [("NULL engine", "NULL engine"), ("NULL desc", "NULL desc"), ("pendulum", "Pendulum"), ("no policy", "gymrs_set_policy"),
            ("no table", "gymrs_evaluate_policy"), ("too many", "GYMRS_ES_MAX_POLICIES"), ("utilities NULL", "utilities is NULL"),
            ("utilities + 2", "utilities must be 4-byte aligned"), ("rank2 + 2", "rank2 must be 4-byte aligned"), ("flags", "flag"), ("reserved", "reserved")]


@pytest.mark.parametrize("case,cause", REFUSALS)
def test_refusals(gymrs, case, cause):
    e = gymrs.BatchedEngine(gymrs.PENDULUM if case == "pendulum" else gymrs.CARTPOLE, 64, flags=5 if case == "pendulum" else 7)
    e.reset(seed=1)
    if case not in ("pendulum", "no policy"):
        e.set_policy(np.zeros((gymrs.ES_MAX_POLICIES + 1 if case == "too many" else 4, 10), np.float32))
        if case not in ("no table", "too many"):
            e.evaluate_policy(1, max_episode_steps=1)
    buf = torch.full((2, 8), SENTINEL, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    u, rank2 = buf[0].data_ptr(), buf[1].data_ptr()
    desc = gymrs.EsRanksDesc(None if case == "utilities NULL" else u + 2 * (case == "utilities + 2"), rank2 + 2 * (case == "rank2 + 2"),
                             int(case == "flags"), int(case == "reserved"))
    status = e._lib.gymrs_es_ranks(None if case == "NULL engine" else e._h, None if case == "NULL desc" else C.byref(desc))
    message = e._lib.gymrs_last_error()
    assert status == EINVAL and cause.encode() in message and b"gymrs_es_ranks" in message, message
    e.sync()
    assert (buf.cpu().numpy().view(np.uint32) == SENTINEL).all()  # a refused call wrote nothing
    e.close()


def test_a_generation_shaped_by_ranks(gymrs):
    """evaluate, ranks, step with the ranks as utilities: no host round trip; the step used exactly the numpy ranks"""
    P = 64
    e = gymrs.BatchedEngine(gymrs.CARTPOLE, P, flags=7)
    e.reset(seed=3)
    e.es_init(np.linspace(-1, 1, 10, dtype=np.float32), n_policies=P, sigma=0.125, seed=11)
    u = torch.zeros(P, dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    e.evaluate_policy(1, max_episode_steps=32, seed=5)
    e.es_ranks(u.data_ptr())
    e.es_step(lr=0.05, grad_scale=2.0**-24 / (P * 0.125), utilities=u.data_ptr())
    e.sync()
    want_u, _ = ranks(e.policy_eval())
    ptr, n = e.es_utilities_ptr()
    used = torch.as_tensor(Column(ptr, n, "<f4"), device=DEV).cpu().numpy()
    assert n == P and len(np.unique(want_u)) > 2 and np.array_equal(used.view(np.uint32), want_u.view(np.uint32))
    assert np.array_equal(u.cpu().numpy().view(np.uint32), want_u.view(np.uint32)) and e.es_state(centre=False)["generation"] == 1
    e.close()
