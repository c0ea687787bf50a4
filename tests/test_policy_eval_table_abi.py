"""GYMRS_EVAL_LANE_PARAMS and the sharded parameter-table calls at the C boundary, without a GPU: the constant and the four
prototypes in the header, exported by the library, bound in Python and declared in the Rust binding; a plain-C translation unit that
static-asserts the constant, the unchanged gymrs_eval_desc and the ABI version; the NULL checks; the mirrors' new members."""
import ctypes as C
import re
import spawn_server
from importlib import import_module
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
SHARDED_CALLS = ("gymrs_sharded_set_param_table", "gymrs_sharded_get_param_table", "gymrs_sharded_set_param_index", "gymrs_sharded_get_param_index")
EINVAL = 1
LINK = ["-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib"]


def test_constant_and_prototypes_in_header():
    text = (ROOT / "include" / "gymrs_amd.h").read_text()
    assert re.search(r"^#define GYMRS_EVAL_LANE_PARAMS 4u\b", text, flags=re.M)
    assert re.search(r"^#define GYMRS_EVAL_COMMON_STARTS 1u\b", text, flags=re.M)
    assert re.search(r"#define GYMRS_ABI_VERSION 3\b", text)  # additive: callers detect the feature by symbol
    protos = {"gymrs_sharded_set_param_table": r"gymrs_sharded\* h, const void\* rows[^,;\n]*, uint32_t k",
              "gymrs_sharded_get_param_table": r"gymrs_sharded\* h, void\* rows_out, uint32_t capacity, uint32_t\* k",
              "gymrs_sharded_set_param_index": r"gymrs_sharded\* h, uint64_t first, uint64_t count, const uint16_t\* index_host",
              "gymrs_sharded_get_param_index": r"gymrs_sharded\* h, uint64_t first, uint64_t count, uint16_t\* index_out"}
    assert sorted(protos) == sorted(SHARDED_CALLS)
    for name, args in protos.items():
        assert re.search(rf"^gymrs_status {name}\({args}\);$", text, flags=re.M), name
    # the rollout calls' refusal of a table is documented as not built, the evaluator's is gone from that line
    not_built = re.search(r"- Not built:(.*?)\n \*   - ", text, flags=re.S).group(1)
    assert "gymrs_rollout_policy" in not_built and "flags word" in not_built and "parameter tables," not in not_built


def test_exported_bound_and_in_rust_ffi(gymrs):
    lib = gymrs.load_library()
    sigs = import_module("gym-rs_amd._lib").SIGNATURES
    ffi = (ROOT / "bindings" / "rust" / "src" / "ffi.rs").read_text()
    for name in SHARDED_CALLS:
        assert hasattr(lib, name) and name in sigs, name
    assert sigs["gymrs_sharded_set_param_table"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32])
    assert sigs["gymrs_sharded_get_param_table"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)])
    assert sigs["gymrs_sharded_set_param_index"] == (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]) == sigs["gymrs_sharded_get_param_index"]
    assert re.search(r"pub const GYMRS_EVAL_LANE_PARAMS: u32 = 4;", ffi)
    assert re.search(r"pub fn gymrs_sharded_set_param_table\(h: \*mut GymrsSharded, rows: \*const c_void, k: u32\) -> c_int;", ffi)
    assert re.search(r"pub fn gymrs_sharded_get_param_table\(h: \*mut GymrsSharded, rows_out: \*mut c_void, capacity: u32, k: \*mut u32\) -> c_int;", ffi)
    assert re.search(r"pub fn gymrs_sharded_set_param_index\(h: \*mut GymrsSharded, first: u64, count: u64, index_host: \*const u16\) -> c_int;", ffi)
    assert re.search(r"pub fn gymrs_sharded_get_param_index\(h: \*mut GymrsSharded, first: u64, count: u64, index_out: \*mut u16\) -> c_int;", ffi)
    assert lib.gymrs_abi_version() == 3


def test_python_constant_and_desc(gymrs):
    assert gymrs.EVAL_LANE_PARAMS == 4 == gymrs.engine.EVAL_LANE_PARAMS and gymrs.EVAL_COMMON_STARTS == 1
    make = gymrs.engine._eval_desc
    assert make(3, 17, 5, False, 0, None, True).flags == 4 and make(3, 17, 5, True, 0, None, True).flags == 5
    assert make(3, 17, 5, True, 0, None).flags == 1 and make(3, 17, 5, True, 0, 6, True).flags == 6  # raw flags override both
    desc = gymrs.EvalDesc
    assert C.sizeof(desc) == 32 and [(n, getattr(desc, n).offset) for n, _ in desc._fields_] == [
        ("episodes_per_lane", 0), ("max_episode_steps", 4), ("seed", 8), ("flags", 16), ("reserved", 20), ("lengths_dev", 24)]


def test_calls_refuse_a_null_handle(gymrs):
    lib = gymrs.load_library()
    k = C.c_uint32()
    idx = (C.c_uint16 * 4)()
    row = gymrs.engine.default_params(0)
    calls = {
        "gymrs_sharded_set_param_table": lambda: lib.gymrs_sharded_set_param_table(None, C.byref(row), 1),
        "gymrs_sharded_get_param_table": lambda: lib.gymrs_sharded_get_param_table(None, None, 0, C.byref(k)),
        "gymrs_sharded_set_param_index": lambda: lib.gymrs_sharded_set_param_index(None, 0, 4, idx),
        "gymrs_sharded_get_param_index": lambda: lib.gymrs_sharded_get_param_index(None, 0, 4, idx),
    }
    assert sorted(calls) == sorted(SHARDED_CALLS)
    for name, call in calls.items():
        assert call() == EINVAL, name
        assert name in lib.gymrs_last_error().decode(), name


def test_mirrors_have_the_members(gymrs):
    import inspect
    for cls in (gymrs.BatchedEngine, gymrs.ShardedEngine):
        assert inspect.signature(cls.evaluate_policy).parameters["lane_params"].default is False, cls
    for m in ("set_param_table", "param_table", "set_param_index", "get_param_index"):
        assert callable(getattr(gymrs.ShardedEngine, m)), m
    hpp = (ROOT / "include" / "gymrs_env.hpp").read_text()
    for name in SHARDED_CALLS + ("GYMRS_EVAL_LANE_PARAMS",):
        assert name in hpp, name
    rs = ROOT / "bindings" / "rust" / "src"
    assert "GYMRS_EVAL_LANE_PARAMS" in (rs / "engine.rs").read_text()
    sharded = (rs / "sharded.rs").read_text()
    for name in SHARDED_CALLS + ("GYMRS_EVAL_LANE_PARAMS",):
        assert name in sharded, name
    for text, name in ((ROOT / "INTEGRATION.md").read_text(), "INTEGRATION.md"), ((ROOT / "README.md").read_text(), "README.md"):
        assert "GYMRS_EVAL_LANE_PARAMS" in text, name


def test_constant_layout_and_null_checks_from_c(tmp_path):
    src = tmp_path / "eval_table.c"
    src.write_text(r'''
#include "gymrs_amd.h"
#include <stddef.h>
#include <stdio.h>
#include <string.h>
_Static_assert(GYMRS_EVAL_LANE_PARAMS == 4u && GYMRS_EVAL_COMMON_STARTS == 1u, "flag bits");
_Static_assert((GYMRS_EVAL_LANE_PARAMS & GYMRS_EVAL_COMMON_STARTS) == 0u && (GYMRS_EVAL_LANE_PARAMS & 2u) == 0u, "bit 1 stays unassigned");
_Static_assert(GYMRS_ABI_VERSION == 3, "additive");
_Static_assert(sizeof(gymrs_eval_desc) == 32, "desc size");
_Static_assert(offsetof(gymrs_eval_desc, episodes_per_lane) == 0 && offsetof(gymrs_eval_desc, max_episode_steps) == 4, "desc layout");
_Static_assert(offsetof(gymrs_eval_desc, seed) == 8 && offsetof(gymrs_eval_desc, flags) == 16, "desc layout");
_Static_assert(offsetof(gymrs_eval_desc, reserved) == 20 && offsetof(gymrs_eval_desc, lengths_dev) == 24, "desc layout");
int main(void) {
    gymrs_eval_desc d = {3, 17, 5, GYMRS_EVAL_COMMON_STARTS | GYMRS_EVAL_LANE_PARAMS, 0, NULL};
    gymrs_cartpole_params row;
    uint16_t idx[4] = {0, 1, 2, 3};
    uint32_t k = 7;
    if (d.flags != 5u || gymrs_abi_version() != 3) return 1;
    if (gymrs_default_params(GYMRS_CARTPOLE, &row) != GYMRS_OK) return 2;
    if (gymrs_sharded_set_param_table(NULL, &row, 1) != GYMRS_EINVAL) return 3;
    if (gymrs_sharded_get_param_table(NULL, NULL, 0, &k) != GYMRS_EINVAL) return 4;
    if (gymrs_sharded_set_param_index(NULL, 0, 4, idx) != GYMRS_EINVAL) return 5;
    if (gymrs_sharded_get_param_index(NULL, 0, 4, idx) != GYMRS_EINVAL) return 6;
    if (gymrs_sharded_evaluate_policy(NULL, &d) != GYMRS_EINVAL) return 7;
    printf("%s\n", gymrs_last_error());
    return strstr(gymrs_last_error(), "gymrs_sharded_evaluate_policy") ? 0 : 8;
}
''')
    exe = tmp_path / "eval_table"
    lib_dir = ROOT / "gym-rs_amd"
    spawn_server.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", f"-I{ROOT / 'include'}", str(src), "-o", str(exe),
                      f"-L{lib_dir}", "-lgymrs_amd", f"-Wl,-rpath,{lib_dir}"] + LINK, check=True, capture_output=True, text=True)
    res = spawn_server.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stdout + res.stderr


def test_cpp_mirror_members_compile(tmp_path):
    """A small program of its own that names every new member of include/gymrs_env.hpp (their signatures are part of the check); it
    runs no engine: it only has to compile, link and start."""
    src = tmp_path / "eval_table_mirror.cpp"
    src.write_text(r'''
#include <cstdint>
#include <cstdio>
#include <vector>
#include "gymrs_env.hpp"
using gymrs::ShardedVecEnv;
using gymrs::VecEnv;
int main() {
    void (VecEnv::*a)(std::uint32_t, std::uint32_t, std::uint64_t, bool, std::uint32_t*, bool) = &VecEnv::evaluate_policy;
    void (VecEnv::*a5)(std::uint32_t, std::uint32_t, std::uint64_t, bool, std::uint32_t*) = &VecEnv::evaluate_policy;  // (unchanged)
    void (ShardedVecEnv::*b)(const void*, std::uint32_t) = &ShardedVecEnv::set_param_table;
    std::uint32_t (ShardedVecEnv::*c)(void*, std::uint32_t) = &ShardedVecEnv::param_table;
    void (ShardedVecEnv::*d)(std::uint64_t, std::uint64_t, const std::uint16_t*) = &ShardedVecEnv::set_param_index;
    std::vector<std::uint16_t> (ShardedVecEnv::*e)(std::uint64_t, std::uint64_t) = &ShardedVecEnv::param_index;
    static_assert(GYMRS_EVAL_LANE_PARAMS == 4u && sizeof(gymrs_eval_desc) == 32, "constant, size");
    const bool all = a && a5 && b && c && d && e;
    std::printf(all ? "EVAL_TABLE_MIRROR_OK\n" : "missing\n");
    return all ? 0 : 1;
}
''')
    exe = tmp_path / "eval_table_mirror"
    lib_dir = ROOT / "gym-rs_amd"
    spawn_server.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe), f"-L{lib_dir}", "-lgymrs_amd",
                      f"-Wl,-rpath,{lib_dir}"] + LINK, check=True, capture_output=True, text=True)
    res = spawn_server.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0 and "EVAL_TABLE_MIRROR_OK" in res.stdout, res.stdout + res.stderr
