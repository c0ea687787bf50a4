"""The launch table of the kernel library (gym-rs_amd/csrc/gymrs_launch.h), walked without a GPU: plain g++ compiles the header
alone and a small program prints which compile-time (flag set, lanes per work-item) pair every run-time pair reaches.  The sets it
reaches are the ones the GPU matrices iterate over (closed_loop_ref.FLAG_SETS): the two lists cannot drift apart silently.  A second
program walks the closed-loop routing decision (dispatch_closed_loop): which kernel family every request reaches, or that it is refused."""
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


# ---- the closed-loop route: dispatch_closed_loop, walked over every request and compared with a table written out here from the rules
# (not from the header): which of the eight kernel families a request reaches, at which lanes / flag set / REC, or none.

CLOSED_LOOP_PROGRAM = r"""
#include "gymrs_launch.h"
#include <cstdio>
int main()
{
    using namespace gymrs;
    const ClosedLoopSource sources[] = {ClosedLoopSource::policy, ClosedLoopSource::exploring, ClosedLoopSource::sampling};
    const int lanes[] = {1, 4, 8, 16};
    for (int s = 0; s < 3; ++s)
        for (int bits = 0; bits < 8; ++bits)
            for (int vec : lanes)
                for (uint32_t flags = 0; flags < 16; ++flags) {
                    const bool fitness = bits & 1, record = bits & 2, transitions = bits & 4;
                    std::printf("%d %d %d %d %d %u :", s, (int)fitness, (int)record, (int)transitions, vec, flags);
                    const int got = dispatch_closed_loop(sources[s], fitness, record, transitions, vec, flags | WALK_HIGH_BITS, -1, [](auto family, auto l, auto f, auto rec) {
                        static_assert(decltype(l)::value == 4 || decltype(l)::value == 8, "compile-time lanes");
                        std::printf(" %d %d %u %d", (int)decltype(family)::value, (int)decltype(l)::value, (unsigned)decltype(f)::value, (int)decltype(rec)::value);
                        return 0;
                    });
                    std::printf(got < 0 ? " invalid\n" : "\n");
                }
    std::printf("families %d\n", kClosedLoopFamilies);
    return 0;
}
"""

# the eight families in the order of the header's enumeration, which is the order of the issue's list of kernels
FAMILIES = ("policy", "policy_fitness", "explore", "explore_fitness", "sample", "sample_fitness", "transitions", "sample_transitions")
SOURCES = ("policy", "exploring", "sampling")


def closed_loop_rule(source, fitness, record, transitions, vec, flags):
    """(family, lanes, flag set, REC) or None, by the rules of the routing decision"""
    ten = flags if flags & A else flags & ~(S | F)  # the ten flag sets: statistics and final observations need auto-reset
    if fitness and (record or transitions):
        return None  # no recording fitness kernel
    if transitions:
        if not record or not flags & A:
            return None
        return ("sample_transitions" if source == "sampling" else "transitions", 4, flags, 1)  # 4 lanes whatever vec says; the eight sets with A
    if vec not in (4, 8):
        return None
    if fitness:
        return ({"policy": "policy_fitness", "exploring": "explore_fitness", "sampling": "sample_fitness"}[source], vec, ten, 0)
    if record and vec != 4:
        return None
    return ({"policy": "policy", "exploring": "explore", "sampling": "sample"}[source], vec, ten, int(record))


def walk_closed_loop(tmp_path, name, high_bits=0):
    src = tmp_path / f"{name}.cpp"
    src.write_text(CLOSED_LOOP_PROGRAM)
    exe = tmp_path / name
    spawn_server.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{ROOT / 'include'}", f"-I{ROOT / 'gym-rs_amd' / 'csrc'}",
                      f"-DWALK_HIGH_BITS={high_bits}u", str(src), "-o", str(exe)], check=True)
    lines = spawn_server.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()
    assert lines[-1] == f"families {len(FAMILIES)}"
    reached = {}
    for line in lines[:-1]:
        key, got = line.split(":")
        s, fitness, record, transitions, vec, flags = (int(x) for x in key.split())
        got = got.split()
        if got == ["invalid"]:
            reached[SOURCES[s], fitness, record, transitions, vec, flags] = None
        else:
            assert len(got) == 4, line  # reached exactly once, and not reported invalid after it
            reached[SOURCES[s], fitness, record, transitions, vec, flags] = (FAMILIES[int(got[0])], int(got[1]), int(got[2]), int(got[3]))
    return reached


@pytest.fixture(scope="module")
def closed_loop(tmp_path_factory):
    return walk_closed_loop(tmp_path_factory.mktemp("closed_loop_route"), "route")


def test_closed_loop_route_is_the_rules_for_every_request(closed_loop):
    assert len(closed_loop) == 3 * 2 * 2 * 2 * 4 * 16
    for key, got in closed_loop.items():
        assert got == closed_loop_rule(*key), key


def test_closed_loop_route_reaches_every_family_from_its_own_source_only(closed_loop):
    """a greedy request routed to the exploring family would give the same bits on a GPU (threshold 0): only this walk sees it"""
    sources_of = {f: set() for f in FAMILIES}
    for key, got in closed_loop.items():
        if got is not None:
            sources_of[got[0]].add(key[0])
    assert sources_of == {"policy": {"policy"}, "policy_fitness": {"policy"}, "explore": {"exploring"}, "explore_fitness": {"exploring"},
                          "sample": {"sampling"}, "sample_fitness": {"sampling"}, "transitions": {"policy", "exploring"},
                          "sample_transitions": {"sampling"}}


def test_closed_loop_route_refusals_hold_for_every_source(closed_loop):
    for (source, fitness, record, transitions, vec, flags), got in closed_loop.items():
        if fitness and (record or transitions):
            assert got is None, (source, record, transitions, vec, flags)
        if transitions and (not record or not flags & A):
            assert got is None, (source, fitness, record, vec, flags)
        if transitions and got is not None:
            assert got[1:] == (4, flags, 1) and flags & A  # 4 lanes and REC whatever vec says


def test_closed_loop_route_ignores_the_hint_and_table_bits(tmp_path, closed_loop):
    assert walk_closed_loop(tmp_path, "route_high", high_bits=0xf00) == closed_loop
