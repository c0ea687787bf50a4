"""The host-side decisions of the stepping path (gym-rs_amd/csrc/gymrs_step_plan.h), walked without a GPU: plain g++ compiles the
header alone and a small program prints what it decides.  The expected values are what the engine did before the decisions had a
header of their own."""
from math import gcd
from pathlib import Path

import pytest
import spawn_server

ROOT = Path(__file__).resolve().parent.parent
MIB = 1 << 20
SIZES = (48 * MIB, 48 * MIB + 1, 1024 * MIB - 1, 1024 * MIB)
ROWS = 8  # kResetLogRows
T0 = 1000  # the tick the ring walk and the clock walk start at
UNLOGGED_AT, OTHER_SHAPE_FROM, LAUNCHES = 13, 27, 41

PROGRAM = r"""
#include "gymrs_step_plan.h"
#include <cstdio>
using namespace gymrs;
int main()
{
    std::printf("rows %u\n", kResetLogRows);
    std::printf("per_lane %llu %llu %llu\n", (unsigned long long)bytes_per_step(GYMRS_CARTPOLE, 4, 1), (unsigned long long)bytes_per_step(GYMRS_MOUNTAIN_CAR, 2, 1),
                (unsigned long long)bytes_per_step(GYMRS_PENDULUM, 2, 1));
    std::printf("bytes %llu\n", (unsigned long long)bytes_per_step(GYMRS_CARTPOLE, 4, 1ull << 32));
    const uint64_t sizes[] = {48ull << 20, (48ull << 20) + 1, (1024ull << 20) - 1, 1024ull << 20};
    for (int nt_mode = 0; nt_mode < 4; ++nt_mode)
        for (uint64_t bytes : sizes)
            std::printf("hint %d %llu %u %u\n", nt_mode, (unsigned long long)bytes, hint_bits(nt_mode, bytes, false), hint_bits(nt_mode, bytes, true));
    // the ring: logged launches of 4 lanes per work-item, one unlogged launch, then launches of 8 lanes per work-item
    ResetLogRing ring{0, 0, 4};
    for (int i = 0; i < WALK_LAUNCHES; ++i) {
        const bool logged = i != WALK_UNLOGGED_AT;
        const int vec = i < WALK_OTHER_SHAPE_FROM ? 4 : 8;
        const ResetLogStep s = reset_log_step(ring, logged, WALK_T0 + i, vec);
        std::printf("ring %d %d %d %d %u %u %llu %d\n", i, (int)logged, vec, (int)s.fold_first, s.fold_step, s.after.pending,
                    (unsigned long long)s.after.first_tick, s.after.vec);
        ring = s.after;
    }
    // on an empty ring neither asks for a fold
    std::printf("empty %d %d\n", (int)reset_log_step(ResetLogRing{0, 7, 4}, false, 99, 4).fold_first, (int)reset_log_step(ResetLogRing{0, 7, 4}, true, 99, 8).fold_first);
    for (uint32_t n_buffers = 1; n_buffers <= 40; ++n_buffers)
        std::printf("graph %u %u %u\n", n_buffers, graph_steps(n_buffers, false), graph_steps(n_buffers, true));
    for (int auto_reset = 0; auto_reset < 2; ++auto_reset) {
        uint64_t start = WALK_T0;
        for (int k = 1; k <= 16; ++k) {
            const uint64_t tick = WALK_T0 + k - 1; // the k-th step runs at this tick
            const bool hit = uniform_clock_hits(tick, start, 5);
            start = uniform_clock_after(tick, start, hit, auto_reset != 0);
            std::printf("clock %d %d %d %llu\n", auto_reset, k, (int)hit, (unsigned long long)start);
        }
    }
    return 0;
}
"""


def build_walker(tmp_path, name):
    src = tmp_path / f"{name}.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / name
    spawn_server.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{ROOT / 'include'}", f"-I{ROOT / 'gym-rs_amd' / 'csrc'}",
                      f"-DWALK_T0={T0}", f"-DWALK_UNLOGGED_AT={UNLOGGED_AT}", f"-DWALK_OTHER_SHAPE_FROM={OTHER_SHAPE_FROM}", f"-DWALK_LAUNCHES={LAUNCHES}",
                      str(src), "-o", str(exe)], check=True)
    return exe


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    """{first word of a line: [the line's other words as ints, ...]}"""
    exe = build_walker(tmp_path_factory.mktemp("step_plan"), "walk")
    out = {}
    for line in spawn_server.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines():
        key, *rest = line.split()
        out.setdefault(key, []).append(tuple(int(x) for x in rest))
    assert out["rows"] == [(ROWS,)]
    return out


def test_bytes_per_step(plan):
    assert plan["per_lane"] == [(42, 26, 34)]
    assert plan["bytes"] == [(42 << 32,)]  # the largest engine: no 32-bit product on the way


def test_hints(plan):
    nt, out, loads = 0x100, 0x200, 0x400
    got = {(mode, size): (hip, chain) for mode, size, hip, chain in plan["hint"]}
    assert len(got) == 16
    for size in SIZES:
        assert got[1, size] == (nt, nt) and got[2, size] == (0, 0) and got[3, size] == (out, out)
        if size <= 48 * MIB:
            assert got[0, size] == (nt, out | loads)
        elif size >= 1024 * MIB:
            assert got[0, size] == (nt, nt)
        else:
            assert got[0, size] == (out, out)


def test_reset_log_ring(plan):
    walk = plan["ring"]
    assert len(walk) == LAUNCHES
    pending, first_tick, ring_vec, since_empty = 0, 0, 4, 0
    stand_alone = []
    for i, logged, vec, fold_first, fold_step, after_pending, after_first, after_vec in walk:
        assert logged == (i != UNLOGGED_AT) and vec == (4 if i < OTHER_SHAPE_FROM else 8)
        if fold_first:
            assert pending != 0  # only if rows are pending
            stand_alone.append(i)
            pending, since_empty = 0, 0
        if logged:
            if pending == 0:  # first_tick / vec are taken when the ring is empty
                first_tick, ring_vec = T0 + i, vec
            since_empty += 1
            assert fold_step == (1 if since_empty % ROWS == 0 else 0)  # exactly every eighth logged launch since the ring was last empty
            pending = 0 if fold_step else pending + 1
        else:
            assert fold_step == 0
        assert (after_pending, after_first, after_vec) == (pending, first_tick, ring_vec)
        assert after_pending < ROWS
        if after_pending == 0 and (fold_step or not logged):
            since_empty = 0
    assert stand_alone == [UNLOGGED_AT, OTHER_SHAPE_FROM]  # rows were pending at both: 13 % 8 = 5, (27 - 14) % 8 = 5
    assert sum(w[4] for w in walk) == 13 // 8 + (27 - 14) // 8 + (41 - 27) // 8


def test_a_fold_is_only_asked_for_when_rows_are_pending(plan):
    assert plan["empty"] == [(0, 0)]  # an unlogged launch, a launch of another shape


def test_graph_length(plan):
    assert [g[0] for g in plan["graph"]] == list(range(1, 41))
    for n_buffers, plain, logged in plan["graph"]:
        assert plain % n_buffers == 0 and plain >= 32 and plain - n_buffers < 32
        unit = n_buffers * ROWS // gcd(n_buffers, ROWS)  # lcm
        assert logged % n_buffers == 0 and logged % ROWS == 0 and logged >= 32 and logged - unit < 32


def test_pendulum_clock(plan):
    for auto_reset in (0, 1):
        rows = [r[1:] for r in plan["clock"] if r[0] == auto_reset]
        assert [k for k, *_ in rows] == list(range(1, 17))
        start = T0
        for k, hit, after in rows:
            if auto_reset:
                assert hit == (k in (5, 10, 15))
                if hit:
                    start = T0 + k  # the clock restarts: every lane's next episode starts at the next tick
            else:
                assert hit == (k >= 5)
            assert after == start
