"""gymrs_rollout_closed_loop and its sharded counterpart at the C boundary, without a GPU: the two flag constants, the descriptor
and both prototypes in the header, exported by the library, bound in Python and declared in the Rust binding; a plain-C translation
unit that static-asserts the constants, the descriptor's layout and the ABI version; the NULL checks; the mirrors' new members."""
import ctypes as C
import inspect
import re
import spawn_server
from importlib import import_module
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CALLS = ("gymrs_rollout_closed_loop", "gymrs_sharded_rollout_closed_loop")
EINVAL = 1
LINK = ["-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib"]


def test_constants_struct_and_prototypes_in_header():
    text = (ROOT / "include" / "gymrs_amd.h").read_text()
    assert re.search(r"^#define GYMRS_CLOSED_LOOP_FITNESS 1u\b", text, flags=re.M)
    assert re.search(r"^#define GYMRS_CLOSED_LOOP_LANE_PARAMS 4u\b", text, flags=re.M)
    assert re.search(r"#define GYMRS_ABI_VERSION 3\b", text)  # additive: callers detect the feature by symbol
    assert re.search(r"^typedef struct \{ uint32_t n_steps; uint32_t flags; const gymrs_trajectory\* record; uint64_t reserved; \} "
                     r"gymrs_closed_loop_desc;", text, flags=re.M)
    assert re.search(r"^gymrs_status gymrs_rollout_closed_loop\(gymrs_engine\* e, const gymrs_closed_loop_desc\* d\);$", text, flags=re.M)
    assert re.search(r"^gymrs_status gymrs_sharded_rollout_closed_loop\(gymrs_sharded\* h, const gymrs_closed_loop_desc\* d\);$", text, flags=re.M)
    # the three older calls still refuse a table (they take no flags word); the "Not built" line now points at the call that has one
    not_built = re.search(r"- Not built:(.*?)\n \*   - ", text, flags=re.S).group(1)
    assert "gymrs_rollout_policy" in not_built and "flags word" in not_built and "gymrs_rollout_closed_loop" in not_built
    assert "GYMRS_CLOSED_LOOP_LANE_PARAMS" in not_built


def test_exported_bound_and_in_rust_ffi(gymrs):
    lib = gymrs.load_library()
    sigs = import_module("gym-rs_amd._lib").SIGNATURES
    ffi = (ROOT / "bindings" / "rust" / "src" / "ffi.rs").read_text()
    for name in CALLS:
        assert hasattr(lib, name) and name in sigs, name
        assert sigs[name] == (C.c_int, [C.c_void_p, C.c_void_p]), name
    assert re.search(r"pub const GYMRS_CLOSED_LOOP_FITNESS: u32 = 1;", ffi)
    assert re.search(r"pub const GYMRS_CLOSED_LOOP_LANE_PARAMS: u32 = 4;", ffi)
    assert re.search(r"pub struct GymrsClosedLoopDesc \{\s*pub n_steps: u32,\s*pub flags: u32,\s*pub record: \*const Trajectory,\s*pub reserved: u64,\s*\}", ffi)
    assert re.search(r"pub fn gymrs_rollout_closed_loop\(e: \*mut GymrsEngine, d: \*const GymrsClosedLoopDesc\) -> c_int;", ffi)
    assert re.search(r"pub fn gymrs_sharded_rollout_closed_loop\(h: \*mut GymrsSharded, d: \*const GymrsClosedLoopDesc\) -> c_int;", ffi)
    assert lib.gymrs_abi_version() == 3


def test_python_constants_and_desc(gymrs):
    assert gymrs.CLOSED_LOOP_FITNESS == 1 == gymrs.engine.CLOSED_LOOP_FITNESS
    assert gymrs.CLOSED_LOOP_LANE_PARAMS == 4 == gymrs.engine.CLOSED_LOOP_LANE_PARAMS == gymrs.EVAL_LANE_PARAMS
    desc = gymrs.ClosedLoopDesc
    assert C.sizeof(desc) == 24 and [(n, getattr(desc, n).offset) for n, _ in desc._fields_] == [
        ("n_steps", 0), ("flags", 4), ("record", 8), ("reserved", 16)]
    make = gymrs.engine._closed_loop_desc
    assert make(100, 7, False, False, None).flags == 0 and make(100, 7, True, False, None).flags == 4
    assert make(100, 7, True, True, None).flags == 5 and make(100, 7, False, True, None, flags=6).flags == 6  # raw flags override both
    d = make(100, 7, False, False, None)
    assert d.n_steps == 7 and not d.record and d.reserved == 0
    d = make(100, 7, True, False, dict(obs=16, actions=32, reward=48, done=64))
    t = d.record.contents
    assert (t.obs, t.actions, t.reward, t.done, t.truncated, t.lane_stride) == (16, 32, 48, 64, None, 112)
    traj = gymrs.engine.Trajectory(16, 32, 48, 64, 80, 128)
    assert make(100, 7, False, False, traj).record.contents.lane_stride == 128


def test_calls_refuse_null_arguments(gymrs):
    lib = gymrs.load_library()
    desc = gymrs.ClosedLoopDesc(3, 0, None, 0)
    for name in CALLS:
        assert getattr(lib, name)(None, C.byref(desc)) == EINVAL, name
        assert name in lib.gymrs_last_error().decode(), name
        assert getattr(lib, name)(None, None) == EINVAL, name


def test_mirrors_have_the_members(gymrs):
    for cls in (gymrs.BatchedEngine, gymrs.ShardedEngine):
        params = inspect.signature(cls.rollout_closed_loop).parameters
        assert list(params)[:2] == ["self", "n_steps"], cls
        for name, default in (("lane_params", False), ("fitness", False), ("record", None)):
            assert params[name].default is default and params[name].kind is inspect.Parameter.KEYWORD_ONLY, (cls, name)
    hpp = (ROOT / "include" / "gymrs_env.hpp").read_text()
    for name in CALLS + ("GYMRS_CLOSED_LOOP_LANE_PARAMS", "GYMRS_CLOSED_LOOP_FITNESS", "gymrs_closed_loop_desc"):
        assert name in hpp, name
    rs = ROOT / "bindings" / "rust" / "src"
    engine, sharded = (rs / "engine.rs").read_text(), (rs / "sharded.rs").read_text()
    assert "gymrs_rollout_closed_loop" in engine and "GYMRS_CLOSED_LOOP_LANE_PARAMS" in engine and "GYMRS_CLOSED_LOOP_FITNESS" in engine
    assert "gymrs_sharded_rollout_closed_loop" in sharded and "GYMRS_CLOSED_LOOP_LANE_PARAMS" in sharded
    for text, name in ((ROOT / "INTEGRATION.md").read_text(), "INTEGRATION.md"), ((ROOT / "README.md").read_text(), "README.md"):
        assert "gymrs_rollout_closed_loop" in text and "GYMRS_CLOSED_LOOP_LANE_PARAMS" in text, name


def test_constants_layout_and_null_checks_from_c(tmp_path):
    src = tmp_path / "closed_loop.c"
    src.write_text(r'''
#include "gymrs_amd.h"
#include <stddef.h>
#include <stdio.h>
#include <string.h>
_Static_assert(GYMRS_CLOSED_LOOP_FITNESS == 1u && GYMRS_CLOSED_LOOP_LANE_PARAMS == 4u, "flag bits");
_Static_assert(GYMRS_CLOSED_LOOP_LANE_PARAMS == GYMRS_EVAL_LANE_PARAMS, "the bit of the evaluator's flag");
_Static_assert(GYMRS_ABI_VERSION == 3, "additive");
_Static_assert(sizeof(gymrs_closed_loop_desc) == 24, "desc size");
_Static_assert(offsetof(gymrs_closed_loop_desc, n_steps) == 0 && offsetof(gymrs_closed_loop_desc, flags) == 4, "desc layout");
_Static_assert(offsetof(gymrs_closed_loop_desc, record) == 8 && offsetof(gymrs_closed_loop_desc, reserved) == 16, "desc layout");
int main(void) {
    gymrs_closed_loop_desc d = {100, GYMRS_CLOSED_LOOP_FITNESS | GYMRS_CLOSED_LOOP_LANE_PARAMS, NULL, 0};
    if (d.flags != 5u || gymrs_abi_version() != 3) return 1;
    if (gymrs_rollout_closed_loop(NULL, &d) != GYMRS_EINVAL) return 2;
    if (!strstr(gymrs_last_error(), "gymrs_rollout_closed_loop")) return 3;
    if (gymrs_sharded_rollout_closed_loop(NULL, &d) != GYMRS_EINVAL) return 4;
    if (!strstr(gymrs_last_error(), "gymrs_sharded_rollout_closed_loop")) return 5;
    if (gymrs_rollout_closed_loop(NULL, NULL) != GYMRS_EINVAL || gymrs_sharded_rollout_closed_loop(NULL, NULL) != GYMRS_EINVAL) return 6;
    printf("CLOSED_LOOP_ABI_OK\n");
    return 0;
}
''')
    exe = tmp_path / "closed_loop"
    lib_dir = ROOT / "gym-rs_amd"
    spawn_server.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", f"-I{ROOT / 'include'}", str(src), "-o", str(exe),
                      f"-L{lib_dir}", "-lgymrs_amd", f"-Wl,-rpath,{lib_dir}"] + LINK, check=True, capture_output=True, text=True)
    res = spawn_server.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0 and "CLOSED_LOOP_ABI_OK" in res.stdout, res.stdout + res.stderr


def test_cpp_mirror_members_compile(tmp_path):
    """A small program of its own that names the new members of include/gymrs_env.hpp (their signatures are part of the check); it
    runs no engine: it only has to compile, link and start."""
    src = tmp_path / "closed_loop_mirror.cpp"
    src.write_text(r'''
#include <cstdint>
#include <cstdio>
#include "gymrs_env.hpp"
using gymrs::ShardedVecEnv;
using gymrs::VecEnv;
int main() {
    void (VecEnv::*a)(const gymrs_closed_loop_desc&) = &VecEnv::rollout_closed_loop;
    void (VecEnv::*b)(std::uint32_t, bool, bool, const gymrs_trajectory*) = &VecEnv::rollout_closed_loop;
    void (ShardedVecEnv::*c)(const gymrs_closed_loop_desc&) = &ShardedVecEnv::rollout_closed_loop;
    void (ShardedVecEnv::*d)(std::uint32_t, bool, bool) = &ShardedVecEnv::rollout_closed_loop;
    static_assert(GYMRS_CLOSED_LOOP_LANE_PARAMS == 4u && GYMRS_CLOSED_LOOP_FITNESS == 1u && sizeof(gymrs_closed_loop_desc) == 24, "constants, size");
    const bool all = a && b && c && d;
    std::printf(all ? "CLOSED_LOOP_MIRROR_OK\n" : "missing\n");
    return all ? 0 : 1;
}
''')
    exe = tmp_path / "closed_loop_mirror"
    lib_dir = ROOT / "gym-rs_amd"
    spawn_server.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe), f"-L{lib_dir}", "-lgymrs_amd",
                      f"-Wl,-rpath,{lib_dir}"] + LINK, check=True, capture_output=True, text=True)
    res = spawn_server.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0 and "CLOSED_LOOP_MIRROR_OK" in res.stdout, res.stdout + res.stderr
