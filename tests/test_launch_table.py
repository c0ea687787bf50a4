"""The launch table of the kernel library (gym-rs_amd/csrc/gymrs_launch.h), walked without a GPU: plain g++ compiles the header
alone and a small program prints which compile-time (flag set, lanes per work-item) pair every run-time pair reaches.  The sets it
reaches are the ones the GPU matrices iterate over (closed_loop_ref.FLAG_SETS): the two lists cannot drift apart silently."""
from pathlib import Path

import closed_loop_ref as ref
import pytest
import spawn_server
from closed_loop_ref import A, F, S, T

ROOT = Path(__file__).resolve().parent.parent

PROGRAM = r"""
#include "gymrs_launch.h"
#include <cstdio>
int main()
{
    const int lanes[] = {1, 4, 8, 16};
    for (uint32_t flags = 0; flags < 16; ++flags)
        for (int vec : lanes) {
            const int got = gymrs::dispatch_table<WALK_MINIMAL>(vec, flags | WALK_HIGH_BITS, -1, [](auto l, auto f) {
                static_assert(decltype(l)::value == 4 || decltype(l)::value == 8, "compile-time lanes");
                return (int)(decltype(f)::value * 100u) + decltype(l)::value;
            });
            std::printf("%u %d %d\n", flags, vec, got);
        }
    // the two halves on their own, and the recording rule
    std::printf("lanes %d %d\n", gymrs::dispatch_lanes(8, -1, [](auto l) { return (int)decltype(l)::value; }),
                gymrs::dispatch_lanes(2, -1, [](auto l) { return (int)decltype(l)::value; }));
    std::printf("rec %d %d %d %d\n", gymrs::dispatch_recording<4>(true, -1, [](auto r) { return (int)decltype(r)::value; }),
                gymrs::dispatch_recording<4>(false, -1, [](auto r) { return (int)decltype(r)::value; }),
                gymrs::dispatch_recording<8>(true, -1, [](auto r) { return (int)decltype(r)::value; }),
                gymrs::dispatch_recording<8>(false, -1, [](auto r) { return (int)decltype(r)::value; }));
    return 0;
}
"""


def walk(tmp_path, name, minimal=False, high_bits=0):
    """{(run-time flags, lanes): (compile-time flags, lanes) or None} and the program's other lines"""
    src = tmp_path / f"{name}.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / name
    spawn_server.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{ROOT / 'include'}", f"-I{ROOT / 'gym-rs_amd' / 'csrc'}",
                      f"-DWALK_MINIMAL={'true' if minimal else 'false'}", f"-DWALK_HIGH_BITS={high_bits}u", str(src), "-o", str(exe)], check=True)
    lines = spawn_server.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()
    table = {}
    for line in lines[:64]:
        flags, vec, got = (int(x) for x in line.split())
        table[flags, vec] = None if got < 0 else divmod(got, 100)
    assert len(table) == 64
    return table, lines[64:]


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    return walk(tmp_path_factory.mktemp("launch_table"), "walk")


def test_exactly_the_ten_flag_sets_are_reached(table):
    reached = {got[0] for got in table[0].values() if got is not None}
    assert reached == {0, A, A | S, T, A | T, A | S | T, A | F, A | S | F, A | T | F, A | S | T | F}
    assert len(ref.FLAG_SETS) == 10 and reached == set(ref.FLAG_SETS)  # the list the GPU matrices iterate over


def test_statistics_and_final_observations_need_auto_reset(table):
    for flags in range(16):
        want = flags if flags & A else flags & ~(S | F)
        for vec in (4, 8):
            assert table[0][flags, vec] == (want, vec), (flags, vec)
    assert (A, S, T, F) == (1, 2, 4, 8)


def test_only_4_and_8_lanes_per_work_item(table):
    for flags in range(16):
        assert table[0][flags, 1] is None and table[0][flags, 16] is None
        assert table[0][flags, 4] is not None and table[0][flags, 8] is not None
    assert table[1][0] == "lanes 8 -1"


def test_recording_exists_at_4_lanes_only(table):
    assert table[1][1] == "rec 1 0 -1 0"


def test_hint_and_table_bits_do_not_change_the_set(tmp_path, table):
    """the internal launch flags (0x100 .. 0x800) travel in the same word: the table looks at its four bits only"""
    assert walk(tmp_path, "high", high_bits=0xf00)[0] == table[0]


def test_developer_builds_keep_the_headline_sets_at_4_lanes(tmp_path):
    minimal = walk(tmp_path, "minimal", minimal=True)[0]
    for (flags, vec), got in minimal.items():
        want = flags if flags & A else flags & ~(S | F)
        assert got == ((want, 4) if vec == 4 and want in (A | S, A | S | T) else None), (flags, vec)
