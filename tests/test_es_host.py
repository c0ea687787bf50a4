"""The host-only definitions of include/gymrs_amd.h, "Evolution strategies" (gymrs_es_noise, gymrs_es_utilities) against their plain
numpy restatement, bit for bit.  The restatement lives here and is what tests/test_gpu_es.py feeds the optimizer's reference with: the
noise from explore_ref.draw4, the population through optimizer_ref.fmaf, the utilities and the gradient in f64 / int64 numpy.  It
never imports the library."""
from decimal import Decimal, getcontext

import explore_ref
import numpy as np
import optimizer_ref as opt
import pytest

STREAM_ES = 4
SCALE = np.float32(1.0 / np.sqrt(np.float64(2863311530.0)))  # 8 uniform 16-bit halves: variance 8 * (65536^2 - 1) / 12
F32, F64 = np.float32, np.float64


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def noise(seed, gen, pair, s):
    """eps(gen, pair, s) as f32; pair and s broadcast"""
    pair, s = np.broadcast_arrays(np.asarray(pair, np.uint64), np.asarray(s, np.uint64))
    tick = np.uint64((int(gen) & (2**39 - 1)) << 9) | s
    h = sum((w & 0xFFFF).astype(np.int64) + (w >> 16).astype(np.int64) for w in explore_ref.draw4(seed, pair, tick, STREAM_ES))
    return (h - 262140).astype(F32) * SCALE


def population(theta, sigma, seed, gen, n_policies):
    eps = noise(seed, gen, np.arange(n_policies // 2)[:, None], np.arange(len(theta))[None, :])
    w = np.empty((n_policies, len(theta)), F32)
    w[0::2], w[1::2] = opt.fmaf(F32(sigma), eps, theta[None]), opt.fmaf(-F32(sigma), eps, theta[None])
    return w


def fold(slot):
    """slot[..., 0] after slot[l] += slot[l ^ mask] for mask = 512 .. 1"""
    for mask in (512, 256, 128, 64, 32, 16, 8, 4, 2, 1):
        slot = slot + slot[..., np.arange(1024) ^ mask]
    return slot[..., 0]


def two_level(values, valid):
    chunks = -(-len(values) // 1024)
    slots, top = np.zeros(chunks * 1024, F64), np.zeros(1024, F64)
    slots[:len(values)] = np.where(valid, values, 0.0)
    top[:chunks] = fold(slots.reshape(chunks, 1024))
    return fold(top)


def utilities(records):
    """u[P] as f32 from int64 records [P][8] (return_sum, return_sq_sum, episodes, ...)"""
    valid = records[:, 2] > 0
    with np.errstate(all="ignore"):
        F = records[:, 0].astype(F64) / records[:, 2].astype(F64)
        n = two_level(valid.astype(F64), valid)
        mean = two_level(F, valid) / n
        sd = np.sqrt(two_level((F - mean) * (F - mean), valid) / n)
        u = ((F - mean) / sd).astype(F32)
    return np.where(valid & (sd > 0), u, F32(0))


def gradient(u, seed, gen, n_params):
    """(G int64 [S], excluded) from the utilities of one generation"""
    u = np.asarray(u, F32)
    with np.errstate(all="ignore"):
        t = (u[0::2] - u[1::2])[:, None] * noise(seed, gen, np.arange(len(u) // 2)[:, None], np.arange(n_params)[None, :])
        ok = np.abs(t) < F32(2.0**30)  # False for NaN and the infinities
    q = np.rint(np.where(ok, t, F32(0)).astype(F64) * 2.0**24).astype(np.int64)
    return q.sum(axis=0), int((~ok).sum())


def test_noise_scale_is_the_nearest_f32():
    getcontext().prec = 60
    exact = 1 / Decimal(2863311530).sqrt()
    others = (np.nextafter(SCALE, F32(0)), np.nextafter(SCALE, F32(1)))
    assert all(abs(Decimal(float(SCALE)) - exact) < abs(Decimal(float(o)) - exact) for o in others)
    assert float(SCALE).hex() == "0x1.3988e20000000p-16"


@pytest.mark.parametrize("gen", [0, 2**39 - 1, 2**39 + 3])  # (bit 39 and above do not enter the key)
def test_noise_corners(gymrs, gen):
    pair, s = np.array([0, 1, 2**32 + 5, 2**64 - 1], np.uint64)[:, None], np.array([0, 1, 449, 511])[None, :]
    got, want = gymrs.es_noise(0xDEADBEEF12345678, gen, pair, s), noise(0xDEADBEEF12345678, gen, pair, s)
    assert np.array_equal(bits(got), bits(want))
    assert np.array_equal(bits(want), bits(noise(0xDEADBEEF12345678, gen & (2**39 - 1), pair, s))) and len(np.unique(want)) > 8


def test_noise_moments(gymrs):
    """65 536 draws of one seed: the standard errors of the mean and of the variance are 0.0039 and 0.0055 (kurtosis 2.85)"""
    pair, s = np.arange(128)[:, None], np.arange(512)[None, :]
    eps = noise(2024, 7, pair, s).astype(F64)
    assert abs(eps.mean()) < 0.02 and abs(eps.var() - 1.0) < 0.03 and np.abs(eps).max() < 4.9
    assert np.array_equal(bits(gymrs.es_noise(2024, 7, pair[:8], s)), bits(eps[:8].astype(F32)))


def records_for(case):
    rng = np.random.default_rng(5)
    n = {"pair": 2, "ragged chunk": 1026, "no episodes": 1026, "equal": 130}[case]
    rec = np.zeros((n, 8), np.int64)
    rec[:, 2] = rng.integers(1, 4, n)
    rec[:, 0] = 17 * rec[:, 2] if case == "equal" else -rng.integers(1, 600, n)
    if case == "no episodes":
        rec[rng.random(n) < 0.3, 2] = 0
        rec[[0, 1023, 1025], 2] = 0
    return rec


@pytest.mark.parametrize("case", ["pair", "ragged chunk", "no episodes", "equal"])
def test_utilities(gymrs, case):
    rec = records_for(case)
    got, want = gymrs.es_utilities(rec), utilities(rec)
    assert np.array_equal(bits(got), bits(want))
    if case == "equal":
        assert not bits(got).any()  # sd = 0: every utility is +0.0f
    else:
        assert len(np.unique(want)) > 1 and not bits(want[rec[:, 2] == 0]).any()
