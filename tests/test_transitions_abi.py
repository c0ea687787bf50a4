"""gymrs_rollout_transitions at the C boundary, without a GPU: the descriptor and the prototype in the header, exported by the
library, bound in Python and declared in the Rust binding; a plain-C translation unit that static-asserts the descriptor's layout
and the ABI version; the NULL checks; the mirrors' new members."""
import ctypes as C
import inspect
import re
import spawn_server
from importlib import import_module
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CALL = "gymrs_rollout_transitions"
EINVAL = 1
LINK = ["-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib"]
OFFSETS = [("n_steps", 0), ("flags", 4), ("record", 8), ("final_obs", 56), ("start_obs", 64), ("reserved", 72)]


def test_struct_and_prototype_in_header():
    text = (ROOT / "include" / "gymrs_amd.h").read_text()
    assert re.search(r"#define GYMRS_ABI_VERSION 3\b", text)  # additive: callers detect the feature by symbol
    assert re.search(r"typedef struct \{\s*uint32_t n_steps;\s*uint32_t flags;[^\n]*\n\s*gymrs_trajectory record;[^\n]*\n\s*float\* final_obs;[^\n]*\n"
                     r"\s*float\* start_obs;[^\n]*\n\s*uint64_t reserved;[^\n]*\n\} gymrs_transitions_desc;\s*/\* 80 bytes \*/", text)
    assert re.search(r"^gymrs_status gymrs_rollout_transitions\(gymrs_engine\* e, const gymrs_transitions_desc\* d\);$", text, flags=re.M)
    doc = re.search(r"/\* Transitions:(.*?)\*/", text, flags=re.S).group(1)
    for word in ("if and only if", "BEFORE the re-arm", "gymrs_final_obs_ptrs", "start_obs", "ended ? final_obs[k] : obs[k]", "no sharded counterpart",
                 "GYMRS_AUTO_RESET", "GYMRS_CLOSED_LOOP_FITNESS", "n_steps == 0"):
        assert word in doc, word


def test_exported_bound_and_in_rust_ffi(gymrs):
    lib = gymrs.load_library()
    sigs = import_module("gym-rs_amd._lib").SIGNATURES
    assert hasattr(lib, CALL) and sigs[CALL] == (C.c_int, [C.c_void_p, C.c_void_p])
    ffi = (ROOT / "bindings" / "rust" / "src" / "ffi.rs").read_text()
    assert re.search(r"#\[repr\(C\)\]\s*#\[derive\([^)]*\)\]\s*pub struct GymrsTransitionsDesc \{\s*pub n_steps: u32,\s*pub flags: u32,\s*pub record: Trajectory,"
                     r"\s*pub final_obs: \*mut f32,\s*pub start_obs: \*mut f32,\s*pub reserved: u64,\s*\}", ffi)
    assert re.search(r"pub fn gymrs_rollout_transitions\(e: \*mut GymrsEngine, d: \*const GymrsTransitionsDesc\) -> c_int;", ffi)
    assert lib.gymrs_abi_version() == 3


def test_python_desc(gymrs):
    desc = gymrs.TransitionsDesc
    assert desc is gymrs.engine.TransitionsDesc
    assert C.sizeof(desc) == 80 and [(n, getattr(desc, n).offset) for n, _ in desc._fields_] == OFFSETS
    assert C.sizeof(gymrs.engine.Trajectory) == 48


def test_call_refuses_null_arguments(gymrs):
    lib = gymrs.load_library()
    desc = gymrs.TransitionsDesc(3, 0, gymrs.engine.Trajectory(16, 32, 48, 64, 80, 128), 96, None, 0)
    assert lib.gymrs_rollout_transitions(None, C.byref(desc)) == EINVAL and CALL in lib.gymrs_last_error().decode()
    assert lib.gymrs_rollout_transitions(None, None) == EINVAL


def test_mirrors_have_the_members(gymrs):
    params = inspect.signature(gymrs.BatchedEngine.rollout_transitions).parameters
    assert list(params)[:2] == ["self", "n_steps"]
    for name, default in (("start_obs", None), ("lane_params", False), ("explore", False), ("flags", None)):
        assert params[name].default is default and params[name].kind is inspect.Parameter.KEYWORD_ONLY, name
    for name in ("record", "final_obs"):
        assert params[name].default is inspect.Parameter.empty and params[name].kind is inspect.Parameter.KEYWORD_ONLY, name
    assert not hasattr(gymrs.ShardedEngine, "rollout_transitions")  # records are refused there: no sharded counterpart
    hpp = (ROOT / "include" / "gymrs_env.hpp").read_text()
    assert CALL in hpp and "gymrs_transitions_desc" in hpp
    engine = (ROOT / "bindings" / "rust" / "src" / "engine.rs").read_text()
    assert "pub unsafe fn rollout_transitions(" in engine and "GymrsTransitionsDesc" in engine
    for text, name in ((ROOT / "INTEGRATION.md").read_text(), "INTEGRATION.md"), ((ROOT / "README.md").read_text(), "README.md"):
        assert CALL in text, name


def test_layout_and_null_checks_from_c(tmp_path):
    src = tmp_path / "transitions.c"
    src.write_text(r'''
#include "gymrs_amd.h"
#include <stddef.h>
#include <stdio.h>
#include <string.h>
_Static_assert(GYMRS_ABI_VERSION == 3, "additive");
_Static_assert(sizeof(gymrs_transitions_desc) == 80 && sizeof(gymrs_trajectory) == 48, "desc size");
_Static_assert(offsetof(gymrs_transitions_desc, n_steps) == 0 && offsetof(gymrs_transitions_desc, flags) == 4, "desc layout");
_Static_assert(offsetof(gymrs_transitions_desc, record) == 8 && offsetof(gymrs_transitions_desc, final_obs) == 56, "desc layout");
_Static_assert(offsetof(gymrs_transitions_desc, start_obs) == 64 && offsetof(gymrs_transitions_desc, reserved) == 72, "desc layout");
int main(void) {
    gymrs_transitions_desc d;
    memset(&d, 0, sizeof d);
    d.n_steps = 100;
    d.flags = GYMRS_CLOSED_LOOP_LANE_PARAMS | GYMRS_CLOSED_LOOP_EXPLORE;
    if (d.flags != 20u || gymrs_abi_version() != 3) return 1;
    if (gymrs_rollout_transitions(NULL, &d) != GYMRS_EINVAL) return 2;
    if (!strstr(gymrs_last_error(), "gymrs_rollout_transitions")) return 3;
    if (gymrs_rollout_transitions(NULL, NULL) != GYMRS_EINVAL) return 4;
    printf("TRANSITIONS_ABI_OK\n");
    return 0;
}
''')
    exe = tmp_path / "transitions"
    lib_dir = ROOT / "gym-rs_amd"
    spawn_server.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", f"-I{ROOT / 'include'}", str(src), "-o", str(exe),
                      f"-L{lib_dir}", "-lgymrs_amd", f"-Wl,-rpath,{lib_dir}"] + LINK, check=True, capture_output=True, text=True)
    res = spawn_server.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0 and "TRANSITIONS_ABI_OK" in res.stdout, res.stdout + res.stderr


def test_cpp_mirror_members_compile(tmp_path):
    """A small program of its own that names the new members of include/gymrs_env.hpp (their signatures are part of the check); it
    runs no engine: it only has to compile, link and start."""
    src = tmp_path / "transitions_mirror.cpp"
    src.write_text(r'''
#include <cstdint>
#include <cstdio>
#include "gymrs_env.hpp"
using gymrs::VecEnv;
int main() {
    void (VecEnv::*a)(const gymrs_transitions_desc&) = &VecEnv::rollout_transitions;
    void (VecEnv::*b)(std::uint32_t, const gymrs_trajectory&, float*, float*, bool, bool) = &VecEnv::rollout_transitions;
    static_assert(sizeof(gymrs_transitions_desc) == 80, "size");
    const bool all = a && b;
    std::printf(all ? "TRANSITIONS_MIRROR_OK\n" : "missing\n");
    return all ? 0 : 1;
}
''')
    exe = tmp_path / "transitions_mirror"
    lib_dir = ROOT / "gym-rs_amd"
    spawn_server.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe), f"-L{lib_dir}", "-lgymrs_amd",
                      f"-Wl,-rpath,{lib_dir}"] + LINK, check=True, capture_output=True, text=True)
    res = spawn_server.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0 and "TRANSITIONS_MIRROR_OK" in res.stdout, res.stdout + res.stderr
