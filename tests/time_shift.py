"""Put an engine (and its CPU twin) at a high tick in milliseconds: patch a snapshot taken right after reset().

``gymrs_reset`` restarts the tick at 0, so stepping to tick 2^32 would take hours.  The snapshot blob carries the tick,
Pendulum's uniform episode clock and every lane's episode start; moving all three forward by ``delta`` (the starts mod
2^32) and leaving ``epoch`` alone gives the engine as it stands after ``delta`` real ticks in which every lane's FINISHED
history grew by ``delta`` steps while the number of finished episodes stayed what it was.  ``TwinEngine.shift_time`` applies
the same shift to the CPU twin (oracle/f32_twin.cpp, twin_shift_time).

The blob layout is ``SnapshotHeader`` + ``snapshot_segments()`` of gym-rs_amd/csrc/gymrs_engine_io.hip; the helper checks
what it relies on before it writes anything.

Ticks at or beyond 2^48 alias in the Philox counter by construction (draw4 keeps tick bits 32..47 in counter word 3):
nothing here goes there.
"""
import ctypes
import struct

SMALL = 1000               # checks the harness only: no 32-bit quantity wraps
WRAP = (1 << 32) - 30      # the tick crosses 2^32 about 30 steps into a run
HIGH = 3 * (1 << 32) + 5   # steady state with tick bits in Philox counter word 3
DELTAS = {"SMALL": SMALL, "WRAP": WRAP, "HIGH": HIGH}

HEADER_BYTES = 320
_OFF_VERSION, _OFF_KIND, _OFF_N, _OFF_FLAGS, _OFF_STATE_DIM, _OFF_EPOCH, _OFF_STAT_BLOCKS = 8, 12, 16, 32, 36, 40, 44
_OFF_TICK, _OFF_USTART = 64, 72
_STATS_BASE_WORDS = 4
_FINAL_OBS = 8
_OBS_DIM = {0: 4, 1: 2, 2: 3}
_M32 = (1 << 32) - 1


def _u32(blob, off):
    return struct.unpack_from("<I", blob, off)[0]


def _u64(blob, off):
    return struct.unpack_from("<Q", blob, off)[0]


def layout(blob, params_bytes=None):
    """-> dict(version, kind, n, flags, epoch, tick, uniform_start, ep_start_off, arrays_end, total): where things lie in
    a snapshot blob; `total` is the size the header implies (v5: needs the size of one parameter row)."""
    assert blob[:8] == b"GYMRSNAP", "not a gymrs snapshot"
    version, kind, n = _u32(blob, _OFF_VERSION), _u32(blob, _OFF_KIND), _u64(blob, _OFF_N)
    flags, state_dim, n_stat = _u32(blob, _OFF_FLAGS), _u32(blob, _OFF_STATE_DIM), _u32(blob, _OFF_STAT_BLOCKS)
    assert version in (4, 5), f"snapshot version {version}: this helper knows 4 and 5 (with a parameter table)"
    before = state_dim * n * 4 + (2 * n * 4 if kind == 2 else 0) + n * 4 + 3 * n  # state, cos / sin, reward, done, truncated, beyond
    after = n_stat * 16 + n_stat * 8 + _STATS_BASE_WORDS * 8 + 8                # episode slots, open sums, baseline, error words
    if flags & _FINAL_OBS:
        after += _OBS_DIM[kind] * n * 4
    ep_off = HEADER_BYTES + before
    end = ep_off + n * 4 + after
    total = end
    if version == 5:
        assert params_bytes, "a v5 blob: pass the size of one parameter row"
        total = end + 8 + _u64(blob, end) * params_bytes + 2 * n
    return dict(version=version, kind=kind, n=n, flags=flags, epoch=_u32(blob, _OFF_EPOCH), tick=_u64(blob, _OFF_TICK),
                uniform_start=_u64(blob, _OFF_USTART), ep_start_off=ep_off, arrays_end=end, total=total)


def shift_blob(blob, delta, params_bytes=None, expect_tick=None):
    """The blob of a freshly reset engine, moved `delta` ticks forward.  delta = 0 returns the same bytes."""
    import numpy as np

    assert 0 <= delta and delta + 1 < 1 << 48
    lay = layout(blob, params_bytes)
    assert lay["total"] == len(blob), f"segment sizes add up to {lay['total']}, the blob has {len(blob)} bytes"
    if expect_tick is not None:
        assert lay["tick"] == expect_tick, (lay["tick"], expect_tick)
    n, off = lay["n"], lay["ep_start_off"]
    starts = np.frombuffer(blob, dtype="<u4", count=n, offset=off)
    assert (starts == lay["epoch"]).all(), "not a snapshot taken right after reset(): some episode start differs from the epoch"
    out = bytearray(blob)
    struct.pack_into("<Q", out, _OFF_TICK, lay["tick"] + delta)
    struct.pack_into("<Q", out, _OFF_USTART, lay["uniform_start"] + delta)
    out[off:off + 4 * n] = ((starts.astype(np.uint64) + np.uint64(delta & _M32)) & np.uint64(_M32)).astype("<u4").tobytes()
    return bytes(out)


def shift_engine(eng, delta):
    """Call right after eng.reset(), before any step and any stats_clear.  -> the patched blob (restored into `eng`)."""
    blob = eng.snapshot()
    patched = shift_blob(blob, delta, params_bytes=ctypes.sizeof(eng.params), expect_tick=eng.tick()[0])
    eng.restore(patched)
    assert eng.tick()[0] == layout(blob, ctypes.sizeof(eng.params))["tick"] + delta
    return patched
