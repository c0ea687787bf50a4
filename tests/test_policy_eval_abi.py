"""Episodic policy evaluation at the C boundary, without a GPU: the five entry points (three on an engine, two on a sharded batch)
declared, exported, bound in Python and declared in the Rust binding; the sizes and field offsets of the record and the desc as a C
compiler sees the header; the NULL checks; the C++ mirror's new methods compile in a small program of their own."""
import ctypes as C
import re
import spawn_server
from importlib import import_module
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
ENGINE_CALLS = ("gymrs_evaluate_policy", "gymrs_get_policy_eval", "gymrs_policy_eval_ptr")
SHARDED_CALLS = ("gymrs_sharded_evaluate_policy", "gymrs_sharded_get_policy_eval")
NEW = ENGINE_CALLS + SHARDED_CALLS
EINVAL = 1
LINK = ["-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib"]
RECORD = ("return_sum", "return_sq_sum", "episodes", "done", "truncated", "steps", "return_min", "return_max")


def test_prototypes_in_header():
    text = (ROOT / "include" / "gymrs_amd.h").read_text()
    for name in ENGINE_CALLS:
        assert re.search(rf"^gymrs_status {name}\(gymrs_engine\* e[^;\n]*\);$", text, flags=re.M), name
    for name in SHARDED_CALLS:
        assert re.search(rf"^gymrs_status {name}\(gymrs_sharded\* h[^;\n]*\);$", text, flags=re.M), name
    assert re.search(r"#define GYMRS_ABI_VERSION 3\b", text)  # additive: callers detect the feature by symbol
    assert re.search(r"#define GYMRS_EVAL_COMMON_STARTS 1u\b", text)
    assert re.search(r"#define GYMRS_POLICY_EVAL_MAX_STEPS 16777216u\b", text)
    assert re.search(r"\} gymrs_eval_desc;", text) and re.search(r"\} gymrs_policy_eval;", text)


def test_exported_bound_and_in_rust_ffi(gymrs):
    lib = gymrs.load_library()
    sigs = import_module("gym-rs_amd._lib").SIGNATURES
    ffi = (ROOT / "bindings" / "rust" / "src" / "ffi.rs").read_text()
    for name in NEW:
        assert hasattr(lib, name) and name in sigs, name
    for name in ENGINE_CALLS:
        assert re.search(rf"pub fn {name}\(e: \*mut GymrsEngine", ffi), name
    for name in SHARDED_CALLS:
        assert re.search(rf"pub fn {name}\(h: \*mut GymrsSharded", ffi), name
    fields = r"\s*".join(rf"pub {n}: {'i64' if n.startswith('return_') and n != 'return_sq_sum' else 'u64'}," for n in RECORD)
    assert re.search(r"pub struct GymrsPolicyEval \{\s*" + fields + r"\s*\}", ffi)
    assert re.search(r"pub struct GymrsEvalDesc \{\s*pub episodes_per_lane: u32,\s*pub max_episode_steps: u32,\s*pub seed: u64,\s*pub flags: u32,\s*"
                     r"pub reserved: u32,\s*pub lengths_dev: \*mut u32,\s*\}", ffi)
    assert lib.gymrs_abi_version() == 3
    # argtypes: (engine, desc), (engine, first, count, out), (engine, out pointer, out count)
    assert sigs["gymrs_evaluate_policy"] == (C.c_int, [C.c_void_p, C.c_void_p]) == sigs["gymrs_sharded_evaluate_policy"]
    assert sigs["gymrs_get_policy_eval"] == (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]) == sigs["gymrs_sharded_get_policy_eval"]
    assert sigs["gymrs_policy_eval_ptr"][1][0] is C.c_void_p and len(sigs["gymrs_policy_eval_ptr"][1]) == 3


def test_python_structs_are_the_c_structs(gymrs):
    rec, desc = gymrs.PolicyEval, gymrs.EvalDesc
    assert rec is gymrs.engine.PolicyEval and C.sizeof(rec) == 64 and C.sizeof(desc) == 32
    assert [(n, getattr(rec, n).offset) for n, _ in rec._fields_] == [(n, 8 * i) for i, n in enumerate(RECORD)]
    assert [t for _, t in rec._fields_] == [C.c_int64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int64, C.c_int64]
    assert [(n, getattr(desc, n).offset) for n, _ in desc._fields_] == [("episodes_per_lane", 0), ("max_episode_steps", 4), ("seed", 8),
                                                                        ("flags", 16), ("reserved", 20), ("lengths_dev", 24)]
    assert gymrs.EVAL_COMMON_STARTS == 1


def test_calls_refuse_null_engine_and_null_handle(gymrs):
    lib = gymrs.load_library()
    desc = gymrs.EvalDesc(1, 1, 0, 0, 0, None)
    ptr = C.c_void_p()
    n = C.c_uint32()
    rec = gymrs.PolicyEval()
    calls = {
        "gymrs_evaluate_policy": lambda: lib.gymrs_evaluate_policy(None, C.byref(desc)),
        "gymrs_get_policy_eval": lambda: lib.gymrs_get_policy_eval(None, 0, 1, C.byref(rec)),
        "gymrs_policy_eval_ptr": lambda: lib.gymrs_policy_eval_ptr(None, C.byref(ptr), C.byref(n)),
        "gymrs_sharded_evaluate_policy": lambda: lib.gymrs_sharded_evaluate_policy(None, C.byref(desc)),
        "gymrs_sharded_get_policy_eval": lambda: lib.gymrs_sharded_get_policy_eval(None, 0, 1, C.byref(rec)),
    }
    assert sorted(calls) == sorted(NEW)
    for name, call in calls.items():
        assert call() == EINVAL, name
        assert name in lib.gymrs_last_error().decode(), name


def test_mirrors_have_the_methods(gymrs):
    for m in ("evaluate_policy", "policy_eval", "policy_eval_ptr"):
        assert callable(getattr(gymrs.BatchedEngine, m)), m
        assert callable(getattr(gymrs.ShardedEngine, m)), m
    hpp = (ROOT / "include" / "gymrs_env.hpp").read_text()
    for name in NEW:
        assert name + "(" in hpp, name
    for src, names in (("engine.rs", ("evaluate_policy", "policy_eval", "policy_eval_ptr")), ("sharded.rs", ("evaluate_policy", "policy_eval"))):
        text = (ROOT / "bindings" / "rust" / "src" / src).read_text()
        for name in names:
            assert re.search(rf"pub fn {name}\(", text), (src, name)


def test_layouts_and_null_checks_from_c(tmp_path):
    src = tmp_path / "policy_eval.c"
    src.write_text(r'''
#include "gymrs_amd.h"
#include <stddef.h>
#include <stdio.h>
#include <string.h>
_Static_assert(sizeof(gymrs_policy_eval) == 64, "record size");
_Static_assert(sizeof(gymrs_eval_desc) == 32, "desc size");
_Static_assert(offsetof(gymrs_policy_eval, return_sum) == 0 && offsetof(gymrs_policy_eval, return_sq_sum) == 8, "record layout");
_Static_assert(offsetof(gymrs_policy_eval, episodes) == 16 && offsetof(gymrs_policy_eval, done) == 24, "record layout");
_Static_assert(offsetof(gymrs_policy_eval, truncated) == 32 && offsetof(gymrs_policy_eval, steps) == 40, "record layout");
_Static_assert(offsetof(gymrs_policy_eval, return_min) == 48 && offsetof(gymrs_policy_eval, return_max) == 56, "record layout");
_Static_assert(offsetof(gymrs_eval_desc, episodes_per_lane) == 0 && offsetof(gymrs_eval_desc, max_episode_steps) == 4, "desc layout");
_Static_assert(offsetof(gymrs_eval_desc, seed) == 8 && offsetof(gymrs_eval_desc, flags) == 16, "desc layout");
_Static_assert(offsetof(gymrs_eval_desc, reserved) == 20 && offsetof(gymrs_eval_desc, lengths_dev) == 24, "desc layout");
_Static_assert(GYMRS_EVAL_COMMON_STARTS == 1u && GYMRS_POLICY_EVAL_MAX_STEPS == 16777216u && GYMRS_ABI_VERSION == 3, "constants");
int main(void) {
    gymrs_eval_desc d = {3, 17, 5, GYMRS_EVAL_COMMON_STARTS, 0, NULL};
    gymrs_policy_eval r = {-1, 2, 3, 4, 5, 6, -7, 8};
    gymrs_policy_eval* view = NULL;
    uint32_t n = 0;
    if (r.return_sum >= 0 || r.return_min >= 0 || sizeof r.return_sq_sum != 8) return 1;
    if (gymrs_abi_version() != 3) return 2;
    if (gymrs_evaluate_policy(NULL, &d) != GYMRS_EINVAL) return 3;
    if (gymrs_get_policy_eval(NULL, 0, 1, &r) != GYMRS_EINVAL) return 4;
    if (gymrs_policy_eval_ptr(NULL, &view, &n) != GYMRS_EINVAL) return 5;
    if (gymrs_sharded_evaluate_policy(NULL, &d) != GYMRS_EINVAL) return 6;
    if (gymrs_sharded_get_policy_eval(NULL, 0, 1, &r) != GYMRS_EINVAL) return 7;
    printf("%s\n", gymrs_last_error());
    return strstr(gymrs_last_error(), "gymrs_sharded_get_policy_eval") ? 0 : 8;
}
''')
    exe = tmp_path / "policy_eval"
    lib_dir = ROOT / "gym-rs_amd"
    spawn_server.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", f"-I{ROOT / 'include'}", str(src), "-o", str(exe),
                      f"-L{lib_dir}", "-lgymrs_amd", f"-Wl,-rpath,{lib_dir}"] + LINK, check=True, capture_output=True, text=True)
    res = spawn_server.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stdout + res.stderr


def test_cpp_mirror_methods_compile(tmp_path):
    """A small program of its own that names every new method of include/gymrs_env.hpp (their signatures are part of the check);
    it runs no engine: it only has to compile, link and start."""
    src = tmp_path / "eval_mirror.cpp"
    src.write_text(r'''
#include <cstdint>
#include <cstdio>
#include <vector>
#include "gymrs_env.hpp"
using gymrs::ShardedVecEnv;
using gymrs::VecEnv;
int main() {
    void (VecEnv::*a)(const gymrs_eval_desc&) = &VecEnv::evaluate_policy;
    void (VecEnv::*b)(std::uint32_t, std::uint32_t, std::uint64_t, bool, std::uint32_t*) = &VecEnv::evaluate_policy;
    std::vector<gymrs_policy_eval> (VecEnv::*c)(std::uint32_t, std::uint32_t) = &VecEnv::policy_eval;
    gymrs_policy_eval* (VecEnv::*d)(std::uint32_t*) = &VecEnv::policy_eval_view;
    void (ShardedVecEnv::*e)(const gymrs_eval_desc&) = &ShardedVecEnv::evaluate_policy;
    std::vector<gymrs_policy_eval> (ShardedVecEnv::*f)(std::uint32_t, std::uint32_t) = &ShardedVecEnv::policy_eval;
    static_assert(sizeof(gymrs_policy_eval) == 64 && sizeof(gymrs_eval_desc) == 32, "sizes");
    const bool all = a && b && c && d && e && f;
    std::printf(all ? "EVAL_MIRROR_OK\n" : "missing\n");
    return all ? 0 : 1;
}
''')
    exe = tmp_path / "eval_mirror"
    lib_dir = ROOT / "gym-rs_amd"
    spawn_server.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe), f"-L{lib_dir}", "-lgymrs_amd",
                      f"-Wl,-rpath,{lib_dir}"] + LINK, check=True, capture_output=True, text=True)
    res = spawn_server.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0 and "EVAL_MIRROR_OK" in res.stdout, res.stdout + res.stderr
