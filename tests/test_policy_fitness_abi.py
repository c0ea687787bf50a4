"""Per-policy fitness at the C boundary, without a GPU: the nine entry points (four on an engine, five on a sharded batch) declared,
exported, bound in Python and declared in the Rust binding; the record's size and field offsets as a C compiler sees the header;
the NULL checks; the C++ mirror's new methods compile in a small program of their own."""
import ctypes as C
import re
import spawn_server
from importlib import import_module
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
ENGINE_CALLS = ("gymrs_rollout_policy_fitness", "gymrs_policy_fitness_ptr", "gymrs_get_policy_fitness", "gymrs_policy_fitness_clear")
SHARDED_CALLS = ("gymrs_sharded_set_policy", "gymrs_sharded_rollout_policy", "gymrs_sharded_rollout_policy_fitness",
                 "gymrs_sharded_get_policy_fitness", "gymrs_sharded_policy_fitness_clear")
NEW = ENGINE_CALLS + SHARDED_CALLS
OK, EINVAL = 0, 1
LINK = ["-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib"]


def test_prototypes_in_header():
    text = (ROOT / "include" / "gymrs_amd.h").read_text()
    for name in ENGINE_CALLS:
        assert re.search(rf"^gymrs_status {name}\(gymrs_engine\* e[^;\n]*\);$", text, flags=re.M), name
    for name in SHARDED_CALLS:
        assert re.search(rf"^gymrs_status {name}\(gymrs_sharded\* h[^;\n]*\);$", text, flags=re.M), name
    assert re.search(r"typedef struct \{ int64_t reward_sum; uint64_t episodes; uint64_t done; uint64_t truncated; \} gymrs_policy_fitness;", text)
    assert re.search(r"#define GYMRS_ABI_VERSION 3\b", text)  # additive: callers detect the feature by symbol
    assert re.search(r"#define GYMRS_POLICY_FITNESS_MAX_STEPS \(1u << 24\)", text)
    assert "has no policy calls yet" not in text
    assert "has no policy calls yet" not in (ROOT / "INTEGRATION.md").read_text()


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
    assert re.search(r"pub struct GymrsPolicyFitness \{\s*pub reward_sum: i64,\s*pub episodes: u64,\s*pub done: u64,\s*pub truncated: u64,\s*\}", ffi)
    assert lib.gymrs_abi_version() == 3


def test_python_record_is_the_c_record(gymrs):
    rec = gymrs.PolicyFitness
    assert rec is gymrs.engine.PolicyFitness and C.sizeof(rec) == 32
    assert [(n, getattr(rec, n).offset) for n, _ in rec._fields_] == [("reward_sum", 0), ("episodes", 8), ("done", 16), ("truncated", 24)]
    assert rec._fields_[0][1] is C.c_int64 and all(t is C.c_uint64 for _, t in rec._fields_[1:])


def test_calls_refuse_null_engine_and_null_handle(gymrs):
    lib = gymrs.load_library()
    desc = gymrs.engine.PolicyDesc(0, 1, 1)
    w = (C.c_float * 10)()
    ptr = C.c_void_p()
    n = C.c_uint32()
    rec = gymrs.PolicyFitness()
    calls = {
        "gymrs_rollout_policy_fitness": lambda: lib.gymrs_rollout_policy_fitness(None, 1),
        "gymrs_policy_fitness_ptr": lambda: lib.gymrs_policy_fitness_ptr(None, C.byref(ptr), C.byref(n)),
        "gymrs_get_policy_fitness": lambda: lib.gymrs_get_policy_fitness(None, 0, 1, C.byref(rec)),
        "gymrs_policy_fitness_clear": lambda: lib.gymrs_policy_fitness_clear(None),
        "gymrs_sharded_set_policy": lambda: lib.gymrs_sharded_set_policy(None, C.byref(desc), w),
        "gymrs_sharded_rollout_policy": lambda: lib.gymrs_sharded_rollout_policy(None, 1),
        "gymrs_sharded_rollout_policy_fitness": lambda: lib.gymrs_sharded_rollout_policy_fitness(None, 1),
        "gymrs_sharded_get_policy_fitness": lambda: lib.gymrs_sharded_get_policy_fitness(None, 0, 1, C.byref(rec)),
        "gymrs_sharded_policy_fitness_clear": lambda: lib.gymrs_sharded_policy_fitness_clear(None),
    }
    assert sorted(calls) == sorted(NEW)
    for name, call in calls.items():
        assert call() == EINVAL, name
        assert name in lib.gymrs_last_error().decode(), name


def test_python_mirror_has_the_methods(gymrs):
    for m in ("rollout_policy_fitness", "policy_fitness", "policy_fitness_ptr", "policy_fitness_clear"):
        assert callable(getattr(gymrs.BatchedEngine, m)), m
        assert callable(getattr(gymrs.ShardedEngine, m)), m
    for m in ("set_policy", "rollout_policy"):
        assert callable(getattr(gymrs.ShardedEngine, m)), m
    hpp = (ROOT / "include" / "gymrs_env.hpp").read_text()
    for name in NEW:
        assert name + "(" in hpp, name
    for src, names in (("engine.rs", ("rollout_policy_fitness", "policy_fitness", "policy_fitness_ptr", "policy_fitness_clear")),
                       ("sharded.rs", ("set_policy", "rollout_policy", "rollout_policy_fitness", "policy_fitness", "policy_fitness_clear"))):
        text = (ROOT / "bindings" / "rust" / "src" / src).read_text()
        for name in names:
            assert re.search(rf"pub fn {name}\(", text), (src, name)


def test_record_layout_and_null_checks_from_c(tmp_path):
    src = tmp_path / "fitness.c"
    src.write_text(r'''
#include "gymrs_amd.h"
#include <stddef.h>
#include <stdio.h>
#include <string.h>
int main(void) {
    gymrs_policy_desc d = {0, 1, 1};
    gymrs_policy_fitness f = {-1, 2, 3, 4};
    gymrs_policy_fitness* view = NULL;
    float w[10] = {0};
    uint32_t n = 0;
    if (sizeof(gymrs_policy_fitness) != 32) return 1;
    if (offsetof(gymrs_policy_fitness, reward_sum) != 0 || offsetof(gymrs_policy_fitness, episodes) != 8) return 2;
    if (offsetof(gymrs_policy_fitness, done) != 16 || offsetof(gymrs_policy_fitness, truncated) != 24) return 3;
    if (f.reward_sum >= 0 || sizeof f.reward_sum != 8 || sizeof f.truncated != 8) return 4;
    if (GYMRS_POLICY_FITNESS_MAX_STEPS != 16777216u || GYMRS_ABI_VERSION != 3 || gymrs_abi_version() != 3) return 5;
    if (gymrs_rollout_policy_fitness(NULL, 1) != GYMRS_EINVAL) return 6;
    if (gymrs_policy_fitness_ptr(NULL, &view, &n) != GYMRS_EINVAL) return 7;
    if (gymrs_get_policy_fitness(NULL, 0, 1, &f) != GYMRS_EINVAL) return 8;
    if (gymrs_policy_fitness_clear(NULL) != GYMRS_EINVAL) return 9;
    if (gymrs_sharded_set_policy(NULL, &d, w) != GYMRS_EINVAL) return 10;
    if (gymrs_sharded_rollout_policy(NULL, 1) != GYMRS_EINVAL) return 11;
    if (gymrs_sharded_rollout_policy_fitness(NULL, 1) != GYMRS_EINVAL) return 12;
    if (gymrs_sharded_policy_fitness_clear(NULL) != GYMRS_EINVAL) return 13;
    if (gymrs_sharded_get_policy_fitness(NULL, 0, 1, &f) != GYMRS_EINVAL) return 14;
    printf("%s\n", gymrs_last_error());
    return strstr(gymrs_last_error(), "gymrs_sharded_get_policy_fitness") ? 0 : 15;
}
''')
    exe = tmp_path / "fitness"
    lib_dir = ROOT / "gym-rs_amd"
    spawn_server.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", f"-I{ROOT / 'include'}", str(src), "-o", str(exe),
                      f"-L{lib_dir}", "-lgymrs_amd", f"-Wl,-rpath,{lib_dir}"] + LINK, check=True, capture_output=True, text=True)
    res = spawn_server.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stdout + res.stderr


def test_cpp_mirror_methods_compile(tmp_path):
    """A small program of its own that names every new method of include/gymrs_env.hpp (their signatures are part of the check);
    it runs no engine: it only has to compile, link and start."""
    src = tmp_path / "fitness_mirror.cpp"
    src.write_text(r'''
#include <cstdint>
#include <cstdio>
#include <vector>
#include "gymrs_env.hpp"
using gymrs::ShardedVecEnv;
using gymrs::VecEnv;
int main() {
    void (VecEnv::*a)(std::uint32_t) = &VecEnv::rollout_policy_fitness;
    std::vector<gymrs_policy_fitness> (VecEnv::*b)(std::uint32_t, std::uint32_t) = &VecEnv::policy_fitness;
    gymrs_policy_fitness* (VecEnv::*c)(std::uint32_t*) = &VecEnv::policy_fitness_view;
    void (VecEnv::*d)() = &VecEnv::policy_fitness_clear;
    void (ShardedVecEnv::*e)(const float*, std::uint32_t, std::uint32_t, std::uint64_t) = &ShardedVecEnv::set_policy;
    void (ShardedVecEnv::*f)() = &ShardedVecEnv::clear_policy;
    void (ShardedVecEnv::*g)(std::uint32_t) = &ShardedVecEnv::rollout_policy;
    void (ShardedVecEnv::*h)(std::uint32_t) = &ShardedVecEnv::rollout_policy_fitness;
    std::vector<gymrs_policy_fitness> (ShardedVecEnv::*i)(std::uint32_t, std::uint32_t) = &ShardedVecEnv::policy_fitness;
    void (ShardedVecEnv::*j)() = &ShardedVecEnv::policy_fitness_clear;
    static_assert(sizeof(gymrs_policy_fitness) == 32, "record size");
    const bool all = a && b && c && d && e && f && g && h && i && j;
    std::printf(all ? "FITNESS_MIRROR_OK\n" : "missing\n");
    return all ? 0 : 1;
}
''')
    exe = tmp_path / "fitness_mirror"
    lib_dir = ROOT / "gym-rs_amd"
    spawn_server.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe), f"-L{lib_dir}", "-lgymrs_amd",
                      f"-Wl,-rpath,{lib_dir}"] + LINK, check=True, capture_output=True, text=True)
    res = spawn_server.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0 and "FITNESS_MIRROR_OK" in res.stdout, res.stdout + res.stderr
